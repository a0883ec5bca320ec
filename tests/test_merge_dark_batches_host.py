"""Several dark-field batches per call without a GPU: ct_hdr_merge_dark_batches is declared, exported and refuses every malformed
call before any launch, each batch with the status ct_hdr_merge_dark_batch gives it; the ops front and compute_hdr_image refuse
what they document."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, NO_GRADIENT, TOO_LARGE = -1, -2, -4, -5
# LINEAR entries are 8 B: with one channel, 20470 points are 163760 B of the 163840 B of LDS, so the 8 B per exposure of one batch
# of 4 (32 B) fit beside them and those of 16 batches of 4 (512 B) do not
LDS_EDGE_POINTS = 20470


@pytest.fixture(scope="module")
def lib():
    from clair_torch_amd import build, _native
    build.build()
    return _native.load()


def _geom(c=3, h=4, w=4, layout=0, h_global=None, row_offset=0):
    from clair_torch_amd import _native as nv
    return nv.Geometry(channels=c, h_tile=h, width=w, h_global=h if h_global is None else h_global, row_offset=row_offset,
                       image_stride=c * h * w, layout=layout)


def _pointers(values):
    return (ctypes.c_void_p * len(values))(*values)


def test_ct_hdr_merge_dark_batches_is_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ct_hdr_merge_dark_batches\s*\(([^)]*)\)", header)
    assert m, "not declared in include/clair_hip.h"
    assert "ct_hdr_merge_dark_batches" in nv.EXPORTS and hasattr(lib, "ct_hdr_merge_dark_batches")
    assert "ct_merge_dark_multi.hip" in build.SOURCES and "ct_merge_dark_kernel.hpp" in build.HEADERS
    for name in ("ct_merge_dark_multi.hip", "ct_merge_dark_kernel.hpp"):
        assert os.path.exists(os.path.join(ROOT, "clair_torch_amd", "csrc", name))
    assert len(lib.ct_hdr_merge_dark_batches.argtypes) == len(m.group(1).split(",")) == 25
    assert lib.ct_hdr_merge_dark_batches.restype is ctypes.c_int32
    # the exported ct_* set and the header stay identical
    assert set(re.findall(r"\b(ct_[a-z0-9_]+)\s*\(", header)) == set(nv.EXPORTS)
    assert "hdr_merge_dark_batches" in dir(ops)


def test_ct_hdr_merge_dark_batches_refuses_before_any_launch(lib):
    """Every call below is malformed (or, where it says so, refused for its route) and made-up pointers stand for device
    memory: a status comes back, nothing is read."""
    from clair_torch_amd import _native as nv
    FIRST, FINAL, CLOSED, ONE = nv.MERGE_FIRST_BATCH, nv.MERGE_FINALIZE, nv.MERGE_CLOSED_FORM, nv.MERGE_REQUIRE_ONE_LAUNCH
    fake = 0x1000
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    lookup = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LOOKUP)
    catmull = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_CATMULL)
    state = (ctypes.c_void_p(fake),) * 3
    missing = object()

    def call(n=2, sizes=(2, 2), stacks=missing, halos=None, stds=None, std_mode=nv.STD_MULTIPLIER, darks=missing, dark_stds=missing,
             dark_batches=missing, geom=None, model=linear, weight=nv.WEIGHT_GAUSS, state=(None, None, None), flags=FIRST | FINAL,
             dtype=nv.DTYPE_U16, expo=fake):
        k = len(sizes)
        geom = _geom() if geom is None else geom
        stacks = [fake] * k if stacks is missing else stacks
        darks = [fake] * k if darks is missing else darks
        dark_stds = [fake] * k if dark_stds is missing else dark_stds
        dark_batches = list(sizes) if dark_batches is missing else dark_batches
        opt = lambda v: None if v is None else _pointers(v)   # noqa: E731
        return lib.ct_hdr_merge_dark_batches(opt(stacks), (ctypes.c_int32 * k)(*sizes), n, dtype, 65535.0, ctypes.byref(geom), opt(halos),
                                             opt(stds), std_mode, 0.05, opt(darks), opt(dark_stds), (ctypes.c_int32 * k)(*dark_batches),
                                             0.05, 50.0, expo, ctypes.byref(model), weight, state[0], state[1], state[2],
                                             ctypes.c_void_p(fake), ctypes.c_void_p(fake), flags, None)

    # ---- the batch list itself ----
    assert call(n=0) == INVALID and call(n=-1) == INVALID
    assert call(n=17, sizes=(2,) * 17) == INVALID
    assert call(stacks=None) == INVALID and call(darks=None) == INVALID
    # a dark std for every batch or for none; halo rows for every batch or for none
    assert call(dark_stds=[fake, None]) == INVALID and call(dark_stds=[None, fake]) == INVALID
    band = _geom(h=4, h_global=12, row_offset=4)
    assert call(geom=band, halos=[fake, None]) == INVALID and call(geom=band, halos=[None, fake]) == INVALID
    assert call(halos=[fake, None]) == INVALID                                  # (also where no band needs them)
    assert call(geom=band) == INVALID                                           # a band without its halo rows
    # ---- every batch as ct_hdr_merge_dark_batch judges it, the first refusal wins ----
    assert call(stacks=[fake, None]) == INVALID and call(darks=[fake, None]) == INVALID
    assert call(sizes=(2, 0)) == INVALID
    assert call(sizes=(4, 3), dark_batches=[4, 2]) == INVALID                   # neither 1 nor B_k
    assert call(sizes=(4, 3), dark_batches=[2, 3]) == INVALID
    assert call(sizes=(4, 3), dark_batches=[4, 1]) == UNSUPPORTED               # shared dark + its std + B_k > 1
    assert call(std_mode=nv.STD_EXPLICIT) == INVALID and call(std_mode=nv.STD_EXPLICIT, stds=[fake, None]) == INVALID
    assert call(geom=_geom(layout=nv.LAYOUT_NHWC)) == UNSUPPORTED
    assert call(dtype=3) == UNSUPPORTED
    assert call(expo=None) == INVALID and call(weight=2) == INVALID
    for flags in (FIRST | FINAL, FIRST | FINAL | CLOSED):                       # LOOKUP, unit weights, a dark std
        assert call(model=lookup, weight=nv.WEIGHT_NONE, flags=flags) == NO_GRADIENT
    for flag in (nv.MERGE_REFERENCE_ORDER, nv.MERGE_OUT_AS_INPUT, nv.MERGE_F64_MOMENTS):
        assert call(flags=FIRST | FINAL | flag) == UNSUPPORTED, flag
    assert call(model=lookup) == UNSUPPORTED and call(model=catmull) == UNSUPPORTED   # reference order unless CLOSED_FORM
    # no state: the call must be a whole merge
    assert call(flags=FIRST) == INVALID and call(flags=FINAL) == INVALID and call(flags=0) == INVALID
    assert call(flags=0, state=(state[0], state[1], None)) == INVALID           # a dark std needs the variance state
    assert call(stacks=[fake, 0x1001]) == INVALID and call(darks=[fake, 0x1002]) == INVALID   # alignment, of any batch
    assert call(sizes=(2, 1 << 16), dark_batches=[2, 1 << 16]) == TOO_LARGE     # a batch that does not fit alone
    # the mixture is refused before the batches are looked at; the first batch's refusal comes before the second's
    assert call(dark_stds=[fake, None], geom=_geom(layout=nv.LAYOUT_NHWC)) == INVALID
    assert call(sizes=(4, 3), dark_batches=[1, 2]) == UNSUPPORTED
    # ---- the LDS of one launch: each batch of 4 fits beside the LUT, 16 of them do not ----
    edge = nv.Icrf(lut_dev=0x2000, n_points=LDS_EDGE_POINTS, interp=nv.INTERP_LINEAR)
    one, sixteen = dict(sizes=(4,), n=1), dict(sizes=(4,) * 16, n=16)
    assert 8 * LDS_EDGE_POINTS + 8 * 4 <= 160 * 1024 < 8 * LDS_EDGE_POINTS + 8 * 64
    assert call(geom=_geom(c=1), model=edge, flags=FIRST | FINAL | ONE, state=state, **sixteen) == UNSUPPORTED
    assert call(geom=_geom(c=1), model=edge, flags=FIRST | FINAL, **sixteen) == UNSUPPORTED   # one launch per batch needs a state
    over = nv.Icrf(lut_dev=0x2000, n_points=LDS_EDGE_POINTS + 8, interp=nv.INTERP_LINEAR)
    assert call(geom=_geom(c=1), model=over, state=state, **one) == TOO_LARGE  # the single-batch entry point's own answer
    assert call(geom=_geom(c=1), model=over, state=state, **sixteen) == TOO_LARGE


def test_front_end_refuses_what_it_documents():
    from clair_torch_amd import ops
    from clair_torch_amd.inference.dark_field import DarkField
    x = torch.zeros((2, 3, 4, 4), dtype=torch.uint8)
    dark = torch.zeros((2, 3, 4, 4))
    t = torch.tensor([1.0, 2.0])
    assert ops.MAX_MERGE_BATCHES == 16
    with pytest.raises(ValueError, match="at most 16 batches"):
        ops.hdr_merge_dark_batches([x] * 17, [t] * 17, [dark] * 17, [dark] * 17)
    with pytest.raises(ValueError, match="equal length"):
        ops.hdr_merge_dark_batches([x, x], [t], [dark, dark], [dark, dark])
    with pytest.raises(ValueError, match="equal length"):
        ops.hdr_merge_dark_batches([], [], [], [])
    with pytest.raises(ValueError, match="every batch"):
        ops.hdr_merge_dark_batches([x, x], [t, t], [dark, dark], [dark, None])
    with pytest.raises(RuntimeError, match="no CPU path"):      # as hdr_merge_dark_batch on a CPU stack
        ops.hdr_merge_dark_batches([x, x], [t, t], [dark, dark], [dark, dark], std_mode="multiplier", std_value=0.05)
    assert callable(DarkField.merge_batches)


@pytest.mark.parametrize("bad", [0, 17, True, 2.0, None])
def test_compute_hdr_image_checks_the_keyword(bad):
    import inspect
    from torch.utils.data import DataLoader
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image, hdr_merge
    p = inspect.signature(compute_hdr_image).parameters
    assert type(p["dark_batches_per_launch"].default) is int and 1 <= p["dark_batches_per_launch"].default <= 16
    assert hdr_merge.DARK_QUEUE_BYTES == 8 << 30
    loader = DataLoader(StackDataset(torch.zeros((2, 1, 4, 4)), [1.0, 2.0]), batch_size=1, shuffle=False, collate_fn=custom_collate)
    with pytest.raises(ValueError, match="dark_batches_per_launch"):
        compute_hdr_image(loader, "cpu", dark_batches_per_launch=bad)


def test_fallback_route_and_batch_order_statuses(lib):
    """What the walk over the batch list answers where the scales of all batches do not fit the LDS and those of each batch do
    (16 batches of 4, one channel, the table of LDS_EDGE_POINTS), without a launch."""
    from clair_torch_amd import _native as nv
    FIRST, FINAL, ONE = nv.MERGE_FIRST_BATCH, nv.MERGE_FINALIZE, nv.MERGE_REQUIRE_ONE_LAUNCH
    fake = 0x1000
    fakep = ctypes.c_void_p(fake)
    edge = nv.Icrf(lut_dev=0x2000, n_points=LDS_EDGE_POINTS, interp=nv.INTERP_LINEAR)
    state = (fakep,) * 3

    def call(sizes=(4,) * 16, stacks=None, dark_batches=None, state=(None, None, None), flags=FIRST | FINAL):
        k = len(sizes)
        geom = _geom(c=1)
        stacks = [fake] * k if stacks is None else stacks
        dark_batches = list(sizes) if dark_batches is None else dark_batches
        return lib.ct_hdr_merge_dark_batches(_pointers(stacks), (ctypes.c_int32 * k)(*sizes), k, nv.DTYPE_U16, 65535.0, ctypes.byref(geom),
                                             None, None, nv.STD_MULTIPLIER, 0.05, _pointers([fake] * k), _pointers([fake] * k),
                                             (ctypes.c_int32 * k)(*dark_batches), 0.05, 50.0, fakep, ctypes.byref(edge), nv.WEIGHT_GAUSS,
                                             state[0], state[1], state[2], fakep, fakep, flags, None)

    assert call(flags=FIRST | FINAL | ONE, state=state) == UNSUPPORTED
    assert call(flags=FIRST | FINAL | ONE) == UNSUPPORTED
    assert call(flags=FIRST | FINAL) == UNSUPPORTED                # a whole merge, but every launch but the last leaves a state
    assert call(flags=0) == INVALID and call(flags=FIRST) == INVALID and call(flags=FINAL) == INVALID   # (every batch's own refusal)
    # an empty batch is not skipped: the single-batch entry point refuses it
    holed = (4,) * 7 + (0,) + (4,) * 8
    assert call(sizes=holed, flags=FIRST | FINAL | ONE, state=state) == INVALID and call(sizes=holed, state=state) == INVALID
    # the first batch's refusal before the second's, either way round
    assert call(sizes=(4, 3), dark_batches=[1, 2]) == UNSUPPORTED and call(sizes=(4, 3), dark_batches=[2, 1]) == INVALID
    assert call(sizes=(1 << 16, 2), stacks=[fake, None]) == TOO_LARGE and call(sizes=(2, 1 << 16), stacks=[None, fake]) == INVALID
