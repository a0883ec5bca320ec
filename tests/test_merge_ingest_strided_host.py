"""StridedDownscale inside the fused merge, without a GPU: ct_hdr_merge_ingest_strided_batches is declared, exported and bound,
refuses every malformed call before any launch with the documented status; the ops fronts check their arguments on CPU tensors;
``stage_images(step_in_kernel=True)`` leaves the ``DeferredIngest`` described in its docstring and without the argument returns
what it always returned."""
import ctypes
import dataclasses
import os
import re

import pytest
import torch

from clair_torch_amd import ops
from clair_torch_amd.common import transforms as T
from clair_torch_amd.inference._staging import DeferredIngest, stage_images

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


def test_the_symbol_is_declared_exported_and_bound(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    declared = re.search(r"\bint\s+ct_hdr_merge_ingest_strided_batches\s*\(([^)]*)\)", header)
    assert declared is not None
    assert "ct_hdr_merge_ingest_strided_batches" in nv.EXPORTS and hasattr(lib, "ct_hdr_merge_ingest_strided_batches")
    assert "ct_merge_ingest_strided.hip" in build.SOURCES
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    # the arguments of ct_hdr_merge_ingest_batches plus the step
    parent = re.search(r"\bint\s+ct_hdr_merge_ingest_batches\s*\(([^)]*)\)", header).group(1)
    args = [" ".join(a.split()) for a in declared.group(1).split(",")]
    assert len(lib.ct_hdr_merge_ingest_strided_batches.argtypes) == len(args) == 22
    assert "int32_t step" in args and [a for a in args if a != "int32_t step"] == [" ".join(a.split()) for a in parent.split(",")]
    assert callable(ops.hdr_merge_ingest_batches_strided) and callable(ops.hdr_merge_ingest_batch_strided)
    from clair_torch_amd import torch_ops  # noqa: F401
    assert hasattr(torch.ops.clair_hip, "hdr_merge_ingest_batches_strided") and hasattr(torch.ops.clair_hip, "hdr_merge_ingest_batch_strided")


def test_every_malformed_call_is_refused_before_any_launch(lib):
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

    def call(frames=(None, None), sizes=(2, 2), n=None, dtype=U16, geom=None, step=2, stages=one, n_stages=1, consts=None, stds=None,
             std_mode=nv.STD_NONE, expo=None, model=linear, weight=nv.WEIGHT_GAUSS, state=(None, None, None), mean_out=fakep,
             std_out=fakep, flags=FIRST | FINAL):
        geom = _geom() if geom is None else geom
        size_arr = None if sizes is None else (ctypes.c_int32 * len(sizes))(*sizes)
        n = (0 if sizes is None else len(sizes)) if n is None else n
        return lib.ct_hdr_merge_ingest_strided_batches(ptrs(frames), size_arr, n, dtype, ctypes.byref(geom), step, stages, n_stages,
                                                       ptrs(consts), ptrs(stds), std_mode, 0.05, expo, ctypes.byref(model), weight,
                                                       state[0], state[1], state[2], mean_out, std_out, flags, None)

    # the step comes first, whatever else is wrong
    for step in (0, -1, -(1 << 31)):
        assert call(step=step) == INVALID and call(step=step, sizes=(0, 0)) == INVALID and call(step=step, dtype=F32) == INVALID
    # step 1 is ct_hdr_merge_ingest_batches: a row band is taken there (nothing to do: CT_OK), and refused behind a step
    band = _geom(h=4, h_global=8, row_offset=2)
    assert call(step=1, sizes=(0, 0), geom=band) == OK
    for step in (2, 3, 1 << 30):
        assert call(step=step, sizes=(0, 0), geom=band) == INVALID
        assert call(step=step, sizes=(0, 0), geom=_geom(h=4, h_global=8)) == INVALID
        assert call(step=step, sizes=(0, 0)) == OK
    # ... behind what ct_hdr_merge_ingest_batch refuses on the source geometry, in its order
    assert call(geom=band, dtype=F32) == UNSUPPORTED and call(geom=band, dtype=7) == INVALID
    assert call(geom=_geom(h=4, h_global=3)) == INVALID
    # the list
    assert call(sizes=(), frames=()) == INVALID and call(n=-1) == INVALID
    assert call(sizes=(1,) * 17, frames=(None,) * 17) == INVALID
    assert call(frames=None, n=2) == INVALID and call(sizes=None, n=2) == INVALID
    assert call(sizes=(0,) * 16, frames=(None,) * 16) == OK
    # nothing to do: CT_OK without a launch
    assert call(sizes=(0, 0)) == OK and call(sizes=(0,), frames=(None,)) == OK
    assert call(geom=_geom(h=0)) == OK and call(geom=_geom(w=0), dtype=U8) == OK
    assert call(sizes=(0, 0), stages=data, consts=(fake, fake)) == OK
    # with something to do the NULL frames are what is wrong -- one batch or several -- then the NULL exposure times
    assert call() == INVALID and call(sizes=(2,), frames=(None,)) == INVALID
    assert call(frames=(fake, None), expo=fakep) == INVALID and call(frames=(fake, fake)) == INVALID
    assert call(frames=(fake, 0x1001), expo=fakep) == INVALID            # uint16 at an odd address
    # dtype, layout, geometry, batch sizes
    assert call(dtype=3) == INVALID and call(dtype=F32) == UNSUPPORTED and call(sizes=(2,), frames=(None,), dtype=F32) == UNSUPPORTED
    assert call(geom=_geom(layout=3)) == INVALID and call(geom=_geom(c=0)) == INVALID and call(sizes=(2, -1)) == INVALID
    assert call(geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE           # the SOURCE frames exceed 2^31 elements
    assert call(geom=_geom(c=4, layout=NHWC)) == UNSUPPORTED and call(geom=_geom(c=1, layout=BGR), dtype=U8) == UNSUPPORTED
    # the stage list
    assert call(stages=_stages(*[nv.INGEST_AFFINE] * 5), n_stages=5) == INVALID and call(stages=_stages(7)) == INVALID
    assert call(stages=data) == INVALID and call(stages=data, consts=(fake, None)) == INVALID
    # flags and modes the fused merge does not take
    for flag in (nv.MERGE_F64_MOMENTS, nv.MERGE_REFERENCE_ORDER, nv.MERGE_OUT_AS_INPUT):
        assert call(flags=FIRST | FINAL | flag) == UNSUPPORTED, flag
    for interp in (nv.INTERP_LOOKUP, nv.INTERP_CATMULL):
        model = nv.Icrf(lut_dev=0x2000, n_points=256, interp=interp)
        assert call(model=model, std_mode=nv.STD_CONSTANT) == UNSUPPORTED
        assert call(sizes=(0, 0), model=model, std_mode=nv.STD_CONSTANT, flags=FIRST | FINAL | nv.MERGE_CLOSED_FORM) == OK
    lookup = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LOOKUP)
    assert call(model=lookup, std_mode=nv.STD_MULTIPLIER, weight=nv.WEIGHT_NONE) == NO_GRADIENT
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)) == TOO_LARGE
    assert call(sizes=(2, 1 << 20)) == TOO_LARGE
    assert call(std_mode=4) == INVALID and call(weight=2) == INVALID
    # the state and the outputs
    assert call(flags=FIRST) == INVALID and call(flags=0) == INVALID and call(sizes=(2,), frames=(None,), flags=FIRST) == INVALID
    assert call(sizes=(0, 0), flags=0, state=(fakep, fakep, None)) == OK
    assert call(sizes=(0, 0), flags=0, state=(fakep, fakep, None), std_mode=nv.STD_CONSTANT) == INVALID
    assert call(mean_out=None) == INVALID and call(std_out=None, std_mode=nv.STD_CONSTANT) == INVALID
    assert call(frames=(fake, fake), expo=fakep, std_mode=nv.STD_EXPLICIT, stds=None) == INVALID
    assert call(frames=(fake, fake), expo=fakep, std_mode=nv.STD_EXPLICIT, stds=(fake, 0x1002)) == INVALID
    short = _geom()
    short.image_stride = 47   # holds the 3 x 2 x 2 selected elements, not a source frame
    assert call(geom=short) == INVALID
    # what cannot be one launch is one launch per batch, which needs a state; CT_MERGE_REQUIRE_ONE_LAUNCH refuses it instead
    mixed = dict(frames=(fake, fake), expo=fakep, consts=(fake, None))
    assert call(**mixed) == INVALID and call(flags=FIRST | FINAL | ONE, **mixed) == UNSUPPORTED
    many = dict(frames=(fake, fake), expo=fakep, sizes=(12000, 12000))     # 96 KB of scales each, 192 KB together
    assert call(**many) == INVALID and call(flags=FIRST | FINAL | ONE, **many) == UNSUPPORTED


def test_front_end_without_a_device():
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)
    stages = [("affine", 0.0, 1.0, 1.0, 0.0)]
    frames = [torch.zeros((2, 3, 4, 4), dtype=torch.uint8)] * 2
    expo = [torch.tensor([1.0, 2.0])] * 2
    for step in (0, -2, True, 2.0, "2", None):
        with pytest.raises(ValueError, match="step must be an int >= 1"):
            ops.hdr_merge_ingest_batches_strided(frames, step, stages, expo, lut=lut)
        with pytest.raises(ValueError, match="step must be an int >= 1"):
            ops.hdr_merge_ingest_batch_strided(frames[0], step, stages, expo[0], lut=lut)
    with pytest.raises(ValueError, match="tile= cannot be combined with step > 1"):
        ops.hdr_merge_ingest_batches_strided(frames, 2, stages, expo, lut=lut, tile=ops.TileGeometry(8, 0))
    for step in (1, 2):   # one batch or several, with or without a step: there is no CPU path
        for k in (1, 2):
            with pytest.raises(RuntimeError, match="no CPU path"):
                ops.hdr_merge_ingest_batches_strided(frames[:k], step, stages, expo[:k], lut=lut)
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.hdr_merge_ingest_batch_strided(frames[0], step, stages, expo[0], lut=lut)
        with pytest.raises(ValueError, match="equal length"):
            ops.hdr_merge_ingest_batches_strided(frames, step, stages, expo[:1], lut=lut)
        with pytest.raises(ValueError, match="at most 16"):
            ops.hdr_merge_ingest_batches_strided(frames * 9, step, stages, expo * 9, lut=lut)


# ---- staging -------------------------------------------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: the one device property the route choice reads."""
    is_cuda = property(lambda self: True)


@pytest.fixture
def calls(monkeypatch):
    """Recording stubs in place of the four ``ops`` calls of the staging."""
    seq = []

    def downscale(stack, step, layout="nchw", out=None):
        seq.append(f"D{step}:{layout}")
        return (stack[..., ::step, ::step] if layout == "nchw" else stack[:, ::step, ::step]).contiguous()

    def transform(stack, stages, layout="nchw", out=None, consts=None):
        seq.append(f"T{len(stages)}{'c' if consts is not None else ''}:{layout}")
        return torch.zeros(ops.ingest_shape(tuple(stack.shape), layout))

    def extrema(stack, prefix_stages=(), layout="nchw", min_val=None, max_val=None):
        seq.append(f"X{len(prefix_stages)}:{layout}{tuple(stack.shape)}")
        return torch.ones(4)

    monkeypatch.setattr(ops, "strided_downscale", downscale)
    monkeypatch.setattr(ops, "ingest_transform", transform)
    monkeypatch.setattr(ops, "ingest_extrema", extrema)
    monkeypatch.setattr(ops, "check_ingest_consts", lambda consts: seq.append("C"))
    return seq


def _lists():
    cast, cv, sd, free = T.CastTo("float32"), T.CvToTorch(), T.StridedDownscale(2), T.Normalize()
    black = T.Normalize(4095, 64)
    return {
        "sd_black": ([sd, cast, black], "planar"),
        "black_sd": ([cast, black, sd], "planar"),
        "cv_sd_black": ([cv, sd, cast, black], "raw"),
        "data_sd": ([cast, free, sd], "planar"),        # the Normalize in FRONT of the downscale: extrema of the full stack
        "cv_data_sd": ([cv, cast, free, sd], "raw"),
        "sd_data": ([sd, cast, free], "planar"),        # ... behind it: step_first
        "black": ([cast, black], "planar"),             # no downscale
        "sd_pair": ([sd, cast, T.Normalize(65535, 0)], "planar"),   # route "code"
    }


def _batch(kind):
    base = (torch.arange(2 * 3 * 6 * 10, dtype=torch.float32) * 7 % 251 + 1).to(torch.uint16)
    return (base.view(2, 3, 6, 10) if kind == "planar" else base.view(2, 6, 10, 3)).as_subclass(_OnDevice)


def test_plan_staging_says_step_in_kernel_only_when_asked():
    for name, (ts, kind) in _lists().items():
        x = _batch(kind)
        plain, asked = T.plan_staging(x, ts), T.plan_staging(x, ts, step_in_kernel=True)
        assert not plain.step_in_kernel, name
        assert asked.step_in_kernel == (plain.step > 1), name
        assert asked == (dataclasses.replace(plain, step_in_kernel=True) if plain.step > 1 else plain), name


def test_stage_images_leaves_the_step_to_the_kernel(calls):
    cpu = torch.device("cpu")
    # list -> (device calls, step of the DeferredIngest, shape of its frames, constants)
    want = {
        "sd_black": ("", 2, (2, 3, 6, 10), False),
        "black_sd": ("", 2, (2, 3, 6, 10), False),
        "cv_sd_black": ("", 2, (2, 6, 10, 3), False),
        "data_sd": ("X0:nchw(2, 3, 6, 10) C", 2, (2, 3, 6, 10), True),
        "cv_data_sd": ("X0:nhwc_bgr(2, 6, 10, 3) C", 2, (2, 6, 10, 3), True),
        "sd_data": ("D2:nchw X0:nchw(2, 3, 3, 5) C", 1, (2, 3, 3, 5), True),
        "black": ("D1:nchw", 1, (2, 3, 6, 10), False),
    }
    for name, (ts, kind) in _lists().items():
        del calls[:]
        x = _batch(kind)
        out = stage_images(x, cpu, ts, defer_ingest=True, step_in_kernel=True)
        if name == "sd_pair":   # route "code" with a downscale keeps today's route
            assert calls == ["D2:nchw"] and out[0].dtype == torch.uint16 and tuple(out[0].shape) == (2, 3, 3, 5) and out[1] == 65535.0
            continue
        d, max_code, layout = out
        seq, step, shape, has_consts = want[name]
        assert isinstance(d, DeferredIngest) and max_code is None and layout == "nchw", name
        assert " ".join(calls) == seq, name
        assert d.step == step and tuple(d.frames.shape) == shape and (d.consts is not None) == has_consts, name
        assert d.layout == ("nhwc_bgr" if kind == "raw" else "nchw"), name
        if step > 1:
            assert d.frames.data_ptr() == x.data_ptr(), name   # the raw frames themselves
        # the one helper that materialises it: the downscale where it is still owed, then the chain
        del calls[:]
        pixels = d.materialise()
        c = "c" if has_consts else ""
        assert calls == ([f"D{step}:{d.layout}"] if step > 1 else []) + [f"T{len(d.stages)}{c}:{d.layout}"], name
        assert tuple(pixels.shape) == ((2, 3, 6, 10) if name == "black" else (2, 3, 3, 5)), name


def test_stage_images_without_the_new_argument_is_unchanged(calls):
    cpu = torch.device("cpu")
    for name, (ts, kind) in _lists().items():
        x = _batch(kind)
        for defer in (False, True):
            del calls[:]
            base = stage_images(x, cpu, ts, defer_ingest=defer)
            base_calls = list(calls)
            # the flag off, and the flag on without defer_ingest (it is only read with it): the same calls, the same result
            for kw in (dict(step_in_kernel=False), dict(step_in_kernel=True)) if not defer else (dict(step_in_kernel=False),):
                del calls[:]
                again = stage_images(x, cpu, ts, defer_ingest=defer, **kw)
                assert calls == base_calls, (name, defer, kw)
                assert type(again[0]) is type(base[0]) and again[1:] == base[1:], (name, defer, kw)
            if isinstance(base[0], DeferredIngest):
                assert base[0].step == 1, name   # behind the compaction, as ever
                assert ("D2" in " ".join(base_calls)) == (name not in ("black",)), name
    assert DeferredIngest(torch.zeros(1), (), "nchw").step == 1 and DeferredIngest(torch.zeros(1), (), "nchw", None).consts is None
