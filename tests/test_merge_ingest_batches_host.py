"""Several fused batches per call without a GPU: ct_hdr_merge_ingest_batches is declared, exported and refuses every malformed
call before any launch, with the status the single-batch entry point gives; the ops front raises what the single-batch front
raises on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, NO_GRADIENT, TOO_LARGE = 0, -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    from clair_torch_amd import build, _native
    build.build()
    return _native.load()


def _stages(*kinds):
    from clair_torch_amd import _native as nv
    arr = (nv.IngestStage * max(len(kinds), 1))()
    for k, kind in enumerate(kinds):
        arr[k].kind, arr[k].sub, arr[k].div, arr[k].mul, arr[k].add = kind, 64.0, 959.0, 1.0, 0.0
        for c in range(4):
            arr[k].lo[c], arr[k].hi[c] = 0.0, 1.0
    return arr


def _geom(c=3, h=4, w=4, layout=0, h_global=None, row_offset=0):
    from clair_torch_amd import _native as nv
    return nv.Geometry(channels=c, h_tile=h, width=w, h_global=h if h_global is None else h_global, row_offset=row_offset,
                       image_stride=c * h * w, layout=layout)


def test_ct_hdr_merge_ingest_batches_is_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ct_hdr_merge_ingest_batches\s*\(", header)
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    assert "ct_hdr_merge_ingest_batches" in nv.EXPORTS and hasattr(lib, "ct_hdr_merge_ingest_batches")
    assert "ct_merge_ingest_multi.hip" in build.SOURCES and "ct_merge_ingest_kernel.hpp" in build.HEADERS
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    declared = re.search(r"\bint\s+ct_hdr_merge_ingest_batches\s*\(([^)]*)\)", header).group(1)
    assert len(lib.ct_hdr_merge_ingest_batches.argtypes) == len(declared.split(",")) == 21


def test_ct_hdr_merge_ingest_batches_validates_before_any_launch(lib):
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    NHWC, BGR = nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    FIRST, FINAL, ONE = nv.MERGE_FIRST_BATCH, nv.MERGE_FINALIZE, nv.MERGE_REQUIRE_ONE_LAUNCH
    fake = 0x1000  # never dereferenced: validation fails first, or there is nothing to launch
    fakep = ctypes.c_void_p(fake)
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    one = _stages(nv.INGEST_AFFINE)
    data = _stages(nv.INGEST_AFFINE_DATA)

    def ptrs(values):
        return None if values is None else (ctypes.c_void_p * len(values))(*values)

    def call(frames=(None, None), sizes=(2, 2), n=None, dtype=U16, geom=None, stages=one, n_stages=1, consts=None, stds=None,
             std_mode=nv.STD_NONE, expo=None, model=linear, weight=nv.WEIGHT_GAUSS, state=(None, None, None), mean_out=fakep,
             std_out=fakep, flags=FIRST | FINAL):
        geom = _geom() if geom is None else geom
        size_arr = None if sizes is None else (ctypes.c_int32 * len(sizes))(*sizes)
        n = (0 if sizes is None else len(sizes)) if n is None else n
        return lib.ct_hdr_merge_ingest_batches(ptrs(frames), size_arr, n, dtype, ctypes.byref(geom), stages, n_stages, ptrs(consts),
                                               ptrs(stds), std_mode, 0.05, expo, ctypes.byref(model), weight, state[0], state[1],
                                               state[2], mean_out, std_out, flags, None)

    # the frames and the exposure times are NULL in every call below: whatever is documented comes before they matter
    # the number of batches and the two arrays every call needs
    assert call(sizes=(), frames=()) == INVALID and call(n=-1) == INVALID
    assert call(sizes=(1,) * 17, frames=(None,) * 17) == INVALID
    assert call(frames=None, n=2) == INVALID and call(sizes=None, n=2) == INVALID
    assert call(sizes=(0,) * 16, frames=(None,) * 16) == OK   # 16 batches are taken
    # nothing to do: CT_OK without a launch (empty batches are skipped)
    assert call(sizes=(0, 0)) == OK and call(sizes=(0, 0, 0), frames=(None,) * 3, stages=None, n_stages=0) == OK
    assert call(geom=_geom(h=0)) == OK and call(geom=_geom(w=0), dtype=U8) == OK
    assert call(sizes=(0, 0), geom=_geom(layout=BGR), std_mode=nv.STD_MULTIPLIER) == OK
    assert call(sizes=(0, 0), stages=data, consts=(fake, fake)) == OK
    # one batch is the single-batch entry point
    assert call(sizes=(0,), frames=(None,)) == OK and call(sizes=(2,), frames=(None,)) == INVALID
    assert call(sizes=(2,), frames=(None,), dtype=F32) == UNSUPPORTED and call(sizes=(-1,), frames=(None,)) == INVALID
    assert call(sizes=(2,), frames=(None,), flags=FIRST) == INVALID
    assert call(sizes=(0,), frames=(None,), flags=FIRST | FINAL | ONE) == OK
    # with something to do, the NULL frames are what is wrong -- of any batch -- then the NULL exposure times
    assert call() == INVALID and call(frames=(fake, None), expo=fakep) == INVALID and call(frames=(None, fake), expo=fakep) == INVALID
    assert call(frames=(fake, fake)) == INVALID
    assert call(frames=(fake, 0x1001), expo=fakep) == INVALID            # uint16 at an odd address
    assert call(sizes=(0, 2, 0), frames=(None, None, None)) == INVALID   # the one batch that is not empty
    # dtype, layout, geometry, batch sizes
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(dtype=F32) == UNSUPPORTED
    assert call(geom=_geom(layout=3)) == INVALID and call(geom=_geom(layout=-1)) == INVALID
    assert call(geom=_geom(c=0)) == INVALID and call(sizes=(2, -1)) == INVALID and call(sizes=(-1, 0)) == INVALID
    assert call(geom=_geom(h=4, h_global=3)) == INVALID and call(geom=_geom(h=4, h_global=6, row_offset=3)) == INVALID
    assert call(geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE
    # the stage list
    assert call(stages=_stages(*[nv.INGEST_AFFINE] * 5), n_stages=5) == INVALID
    assert call(n_stages=-1) == INVALID and call(stages=None, n_stages=1) == INVALID and call(stages=_stages(7)) == INVALID
    assert call(stages=data) == INVALID                                    # without constants
    assert call(stages=data, consts=(fake, None)) == INVALID              # ... of one batch
    assert call(sizes=(0, 0), stages=data, consts=(None, fake)) == INVALID
    assert call(stages=_stages(nv.INGEST_AFFINE_DATA, nv.INGEST_AFFINE_DATA), n_stages=2, consts=(fake, fake)) == INVALID
    assert call(sizes=(0, 0), stages=_stages(nv.INGEST_AFFINE, nv.INGEST_AFFINE_DATA), n_stages=2, consts=(fake, fake)) == OK
    assert call(consts=(fake, 0x1002)) == INVALID
    # not built: interleaved with C != 3
    assert call(geom=_geom(c=4, layout=NHWC)) == UNSUPPORTED and call(geom=_geom(c=1, layout=BGR), dtype=U8) == UNSUPPORTED
    # the flags this entry point does not take
    for flag in (nv.MERGE_F64_MOMENTS, nv.MERGE_REFERENCE_ORDER, nv.MERGE_OUT_AS_INPUT):
        assert call(flags=FIRST | FINAL | flag) == UNSUPPORTED, flag
    # ... and the modes ct_hdr_merge_batch sends to the reference-order kernel, unless the closed form is asked for
    for interp in (nv.INTERP_LOOKUP, nv.INTERP_CATMULL):
        model = nv.Icrf(lut_dev=0x2000, n_points=256, interp=interp)
        for std_mode in (nv.STD_CONSTANT, nv.STD_MULTIPLIER):
            assert call(model=model, std_mode=std_mode) == UNSUPPORTED
            assert call(sizes=(0, 0), model=model, std_mode=std_mode, flags=FIRST | FINAL | nv.MERGE_CLOSED_FORM) == OK
        assert call(sizes=(0, 0), model=model) == OK   # without uncertainties they are closed-form anyway
    # the model, the modes, the state: as ct_hdr_merge_ingest_batch
    lookup = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LOOKUP)
    assert call(model=lookup, std_mode=nv.STD_MULTIPLIER, weight=nv.WEIGHT_NONE) == NO_GRADIENT
    assert call(model=lookup, std_mode=nv.STD_MULTIPLIER, weight=nv.WEIGHT_NONE, flags=FIRST | FINAL | nv.MERGE_CLOSED_FORM) == NO_GRADIENT
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=256, interp=7)) == INVALID
    assert call(model=nv.Icrf(lut_dev=None, n_points=256, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)) == TOO_LARGE   # the LUT exceeds the LDS
    assert call(sizes=(2, 1 << 20)) == TOO_LARGE                          # one batch's exposure times exceed the LDS
    assert call(std_mode=4) == INVALID and call(std_mode=-1) == INVALID and call(weight=2) == INVALID
    assert call(flags=FIRST) == INVALID and call(flags=FINAL) == INVALID and call(flags=0) == INVALID   # several batches, no state
    assert call(sizes=(0, 0), flags=0, state=(fakep, fakep, None)) == OK
    assert call(sizes=(0, 0), flags=0, state=(fakep, fakep, None), std_mode=nv.STD_CONSTANT) == INVALID   # no variance state
    assert call(mean_out=None) == INVALID and call(std_out=None, std_mode=nv.STD_CONSTANT) == INVALID
    assert call(frames=(fake, fake), expo=fakep, std_mode=nv.STD_EXPLICIT, stds=None) == INVALID
    assert call(frames=(fake, fake), expo=fakep, std_mode=nv.STD_EXPLICIT, stds=(fake, None)) == INVALID
    assert call(frames=(fake, fake), expo=fakep, std_mode=nv.STD_EXPLICIT, stds=(fake, 0x1002)) == INVALID
    short = _geom()
    short.image_stride = 47
    assert call(geom=short) == INVALID
    # what cannot be one launch -- constants for some batches only, more exposure times than the LDS holds together -- is one
    # launch per batch, which needs a state; CT_MERGE_REQUIRE_ONE_LAUNCH refuses it instead.  (The frames are real addresses
    # nowhere: both refusals come before any launch.)
    mixed = dict(frames=(fake, fake), expo=fakep, consts=(fake, None))
    assert call(**mixed) == INVALID and call(flags=FIRST | FINAL | ONE, **mixed) == UNSUPPORTED
    assert call(flags=FIRST | FINAL | ONE, state=(fakep, fakep, None), **mixed) == UNSUPPORTED
    many = dict(frames=(fake, fake), expo=fakep, sizes=(12000, 12000))     # 96 KB of scales each, 192 KB together
    assert call(**many) == INVALID and call(flags=FIRST | FINAL | ONE, **many) == UNSUPPORTED


def test_front_end_without_a_device():
    from clair_torch_amd import ops
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)
    stages = [("affine", 0.0, 1.0, 1.0, 0.0)]
    frames = [torch.zeros((2, 3, 4, 4), dtype=torch.uint8)] * 2
    expo = [torch.tensor([1.0, 2.0])] * 2
    assert ops.MAX_MERGE_BATCHES == 16
    for k in (1, 2):   # one batch forwards to hdr_merge_ingest_batch: the same error either way
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.hdr_merge_ingest_batches(frames[:k], stages, expo[:k], lut=lut)
    with pytest.raises(ValueError, match="equal length"):
        ops.hdr_merge_ingest_batches(frames, stages, expo[:1], lut=lut)
    with pytest.raises(ValueError, match="equal length"):
        ops.hdr_merge_ingest_batches([], stages, [], lut=lut)
    with pytest.raises(ValueError, match="equal length"):
        ops.hdr_merge_ingest_batches(frames, stages, expo, lut=lut, consts=[None])
    with pytest.raises(ValueError, match="at most 16"):
        ops.hdr_merge_ingest_batches(frames * 9, stages, expo * 9, lut=lut)


def test_fallback_route_and_batch_order_statuses(lib):
    """What the walk over the batch list answers where the list cannot be one launch, without a launch: one channel and a LINEAR
    table of 20470 points leave 80 B of the LDS, so the scales of one batch of 4 fit and those of the whole list do not."""
    from clair_torch_amd import _native as nv
    from test_merge_dark_batches_host import LDS_EDGE_POINTS
    FIRST, FINAL, ONE = nv.MERGE_FIRST_BATCH, nv.MERGE_FINALIZE, nv.MERGE_REQUIRE_ONE_LAUNCH
    fake = 0x1000
    fakep = ctypes.c_void_p(fake)
    edge = nv.Icrf(lut_dev=0x2000, n_points=LDS_EDGE_POINTS, interp=nv.INTERP_LINEAR)
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    one = _stages(nv.INGEST_AFFINE)
    state = (fakep, fakep, None)   # no uncertainties: no variance state

    def call(frames=(fake,) * 16, sizes=(4,) * 16, geom=None, model=edge, state=(None, None, None), flags=FIRST | FINAL):
        geom = _geom(c=1) if geom is None else geom
        return lib.ct_hdr_merge_ingest_batches((ctypes.c_void_p * len(frames))(*frames), (ctypes.c_int32 * len(sizes))(*sizes), len(sizes),
                                               nv.DTYPE_U16, ctypes.byref(geom), one, 1, None, None, nv.STD_NONE, 0.05, fakep,
                                               ctypes.byref(model), nv.WEIGHT_GAUSS, state[0], state[1], state[2], fakep, fakep, flags, None)

    assert 8 * LDS_EDGE_POINTS + 8 * 4 <= 160 * 1024 < 8 * LDS_EDGE_POINTS + 8 * 60
    # one launch per batch: refused with the flag, and without a state
    assert call(flags=FIRST | FINAL | ONE, state=state) == UNSUPPORTED
    assert call(flags=FIRST | FINAL | ONE) == UNSUPPORTED          # the flag is looked at before the state
    assert call(flags=FIRST | FINAL) == INVALID                    # a whole merge, but every launch but the last leaves a state
    assert call(flags=0) == INVALID and call(flags=FIRST) == INVALID and call(flags=FINAL) == INVALID   # (every batch's own refusal)
    # an empty batch among batches with frames is skipped: its NULL frames are no fault, the other 15 are still too many
    holed = dict(frames=(fake,) * 7 + (None,) + (fake,) * 8, sizes=(4,) * 7 + (0,) + (4,) * 8)
    assert call(flags=FIRST | FINAL | ONE, state=state, **holed) == UNSUPPORTED and call(**holed) == INVALID
    assert call(frames=(fake,) * 7 + (None,) + (fake,) * 8, flags=FIRST | FINAL | ONE, state=state) == INVALID   # ... with frames it is one
    # every batch is judged before any pointer, the first batch's refusal before the second's
    assert call(sizes=(1 << 20, -1), frames=(fake, fake), model=linear) == TOO_LARGE
    assert call(sizes=(-1, 1 << 20), frames=(fake, fake), model=linear) == INVALID
    assert call(sizes=(1 << 20, 2), frames=(None, None), model=linear) == TOO_LARGE
