"""ct_hdr_merge_dark_ingest_batches without a GPU: it is declared, exported and refuses every malformed call before any launch;
the ops front refuses what it documents; ``DarkField.fuses_with_merge_ingest`` follows its table; and ``compute_hdr_image``
sends every batch to the op its docstring names (``ops`` replaced by recorders: nothing here touches a device)."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from test_merge_dark_batches_host import LDS_EDGE_POINTS, _geom, _pointers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, NO_GRADIENT, TOO_LARGE = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    from clair_torch_amd import build, _native
    build.build()
    return _native.load()


def test_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ct_hdr_merge_dark_ingest_batches\s*\(([^)]*)\)", header)
    assert m, "not declared in include/clair_hip.h"
    assert "ct_hdr_merge_dark_ingest_batches" in nv.EXPORTS and hasattr(lib, "ct_hdr_merge_dark_ingest_batches")
    for name in ("ct_merge_dark_ingest.hip", "ct_merge_dark_ingest_packed.hip"):
        assert name in build.SOURCES and os.path.exists(os.path.join(ROOT, "clair_torch_amd", "csrc", name))
    assert "ct_merge_dark_ingest_kernel.hpp" in build.HEADERS
    assert len(lib.ct_hdr_merge_dark_ingest_batches.argtypes) == len(m.group(1).split(",")) == 27
    assert set(re.findall(r"\b(ct_[a-z0-9_]+)\s*\(", header)) == set(nv.EXPORTS)
    assert "hdr_merge_dark_ingest_batches" in dir(ops)


def test_refuses_before_any_launch(lib):
    """Every call below is malformed (or refused for its route) and made-up pointers stand for device memory: a status comes
    back, nothing is read."""
    from clair_torch_amd import _native as nv
    FIRST, FINAL, CLOSED, ONE = nv.MERGE_FIRST_BATCH, nv.MERGE_FINALIZE, nv.MERGE_CLOSED_FORM, nv.MERGE_REQUIRE_ONE_LAUNCH
    fake = 0x1000
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    lookup = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LOOKUP)
    catmull = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_CATMULL)
    state = (ctypes.c_void_p(fake),) * 3
    missing = object()
    affine = dict(kind=nv.INGEST_AFFINE, sub=64.0, div=1000.0, mul=1.0, add=0.0)
    data = dict(kind=nv.INGEST_AFFINE_DATA, mul=1.0, add=0.0)

    def call(n=2, sizes=(2, 2), frames=missing, halos=None, stds=None, std_mode=nv.STD_MULTIPLIER, darks=missing, dark_stds=missing,
             dark_batches=missing, consts=None, stages=(affine,), n_stages=None, geom=None, model=linear, weight=nv.WEIGHT_GAUSS,
             state=(None, None, None), flags=FIRST | FINAL, dtype=nv.DTYPE_U16, expo=fake):
        k = len(sizes)
        geom = _geom() if geom is None else geom
        frames = [fake] * k if frames is missing else frames
        darks = [fake] * k if darks is missing else darks
        dark_stds = [fake] * k if dark_stds is missing else dark_stds
        dark_batches = list(sizes) if dark_batches is missing else dark_batches
        opt = lambda v: None if v is None else _pointers(v)   # noqa: E731
        arr = (nv.IngestStage * max(len(stages), 1))(*[nv.IngestStage(**s) for s in stages])
        return lib.ct_hdr_merge_dark_ingest_batches(
            opt(frames), (ctypes.c_int32 * k)(*sizes), n, dtype, ctypes.byref(geom), arr, len(stages) if n_stages is None else n_stages,
            opt(consts), opt(halos), opt(stds), std_mode, 0.05, opt(darks), opt(dark_stds), (ctypes.c_int32 * k)(*dark_batches), 0.05, 50.0,
            expo, ctypes.byref(model), weight, state[0], state[1], state[2], ctypes.c_void_p(fake), ctypes.c_void_p(fake), flags, None)

    # ---- the batch list itself ----
    assert call(n=0) == INVALID and call(n=-1) == INVALID and call(n=17, sizes=(2,) * 17) == INVALID
    assert call(frames=None) == INVALID and call(darks=None) == INVALID
    # mixed NULL and non-NULL dark-std / halo / consts pointers across the batches
    assert call(dark_stds=[fake, None]) == INVALID and call(dark_stds=[None, fake]) == INVALID
    band = _geom(h=4, h_global=12, row_offset=4)
    assert call(geom=band, halos=[fake, None]) == INVALID and call(halos=[None, fake]) == INVALID
    assert call(consts=[fake, None], stages=(data,)) == INVALID and call(consts=[None, fake]) == INVALID
    assert call(geom=band) == INVALID                                           # a band without its halo rows
    # ---- the stage list: a data stage needs constants, and there is one at most ----
    assert call(stages=(data,)) == INVALID
    assert call(stages=(affine, data, data), consts=[fake, fake]) == INVALID
    assert call(stages=(affine,) * 5) == INVALID and call(n_stages=-1) == INVALID
    assert call(stages=(dict(kind=7),)) == INVALID and call(dtype=3) == INVALID
    assert call(geom=_geom(layout=5)) == INVALID
    assert call(geom=_geom(c=2, layout=nv.LAYOUT_NHWC)) == UNSUPPORTED           # interleaved frames have 3 channels
    # ---- a row band on interleaved frames ----
    assert call(geom=_geom(h=4, h_global=12, row_offset=4, layout=nv.LAYOUT_NHWC_BGR), halos=[fake, fake]) == UNSUPPORTED
    assert call(geom=_geom(h=4, h_global=12, row_offset=0, layout=nv.LAYOUT_NHWC), halos=[fake, fake]) == UNSUPPORTED
    # ---- every batch as ct_hdr_merge_dark_batch judges the float32 stack, the first refusal wins ----
    assert call(frames=[fake, None]) == INVALID and call(darks=[fake, None]) == INVALID
    assert call(sizes=(2, 0)) == INVALID
    assert call(sizes=(4, 3), dark_batches=[4, 2]) == INVALID                   # neither 1 nor B_k
    assert call(sizes=(4, 3), dark_batches=[4, 1]) == UNSUPPORTED               # shared dark + its std + B_k > 1
    assert call(std_mode=nv.STD_EXPLICIT) == INVALID and call(std_mode=nv.STD_EXPLICIT, stds=[fake, None]) == INVALID
    assert call(geom=_geom(w=1)) == INVALID and call(geom=_geom(h=1)) == INVALID  # the reflection needs two columns / rows
    assert call(geom=_geom(w=1, layout=nv.LAYOUT_NHWC)) == INVALID
    assert call(geom=_geom(h=1, h_global=12, row_offset=0), halos=[fake, fake]) == UNSUPPORTED   # a one-row band at the edge
    assert call(expo=None) == INVALID and call(weight=2) == INVALID
    for flags in (FIRST | FINAL, FIRST | FINAL | CLOSED):                       # LOOKUP, unit weights, a dark std
        assert call(model=lookup, weight=nv.WEIGHT_NONE, flags=flags) == NO_GRADIENT
    for flag in (nv.MERGE_REFERENCE_ORDER, nv.MERGE_OUT_AS_INPUT, nv.MERGE_F64_MOMENTS):
        assert call(flags=FIRST | FINAL | flag) == UNSUPPORTED, flag
    assert call(model=lookup) == UNSUPPORTED and call(model=catmull) == UNSUPPORTED   # reference order unless CLOSED_FORM
    assert call(flags=FIRST) == INVALID and call(flags=FINAL) == INVALID and call(flags=0) == INVALID   # no state: a whole merge
    assert call(flags=0, state=(state[0], state[1], None)) == INVALID           # a dark std needs the variance state
    assert call(frames=[fake, 0x1001]) == INVALID and call(darks=[fake, 0x1002]) == INVALID   # alignment, of any batch
    assert call(consts=[fake, 0x1002], stages=(data,)) == INVALID
    assert call(sizes=(2, 1 << 16), dark_batches=[2, 1 << 16]) == TOO_LARGE     # a batch that does not fit alone
    assert call(n=1, sizes=(2,), flags=FIRST) == INVALID                        # one batch is judged like any other
    # the mixture is refused before the stage list, the stage list before the batches
    assert call(dark_stds=[fake, None], stages=(data,)) == INVALID
    assert call(stages=(data,), sizes=(4, 3), dark_batches=[4, 1]) == INVALID
    # ---- the LDS of one launch: each batch of 4 fits beside the LUT, 16 of them do not ----
    edge = nv.Icrf(lut_dev=0x2000, n_points=LDS_EDGE_POINTS, interp=nv.INTERP_LINEAR)
    sixteen = dict(sizes=(4,) * 16, n=16)
    assert call(geom=_geom(c=1), model=edge, flags=FIRST | FINAL | ONE, state=state, **sixteen) == TOO_LARGE
    assert call(geom=_geom(c=1), model=edge, flags=FIRST | FINAL, **sixteen) == UNSUPPORTED   # one launch per batch needs a state
    over = nv.Icrf(lut_dev=0x2000, n_points=LDS_EDGE_POINTS + 8, interp=nv.INTERP_LINEAR)
    assert call(geom=_geom(c=1), model=over, state=state, **sixteen) == TOO_LARGE


def test_front_end_refuses_what_it_documents():
    from clair_torch_amd import ops
    call = ops.hdr_merge_dark_ingest_batches
    x = torch.zeros((2, 3, 4, 4), dtype=torch.uint8)
    dark = torch.zeros((2, 3, 4, 4))
    t = torch.tensor([1.0, 2.0])
    st = [("affine", 0.0, 255.0, 1.0, 0.0)]
    with pytest.raises(ValueError, match="at most 16 batches"):
        call([x] * 17, st, [t] * 17, [dark] * 17, [dark] * 17)
    with pytest.raises(ValueError, match="equal length"):
        call([x, x], st, [t], [dark, dark], [dark, dark])
    with pytest.raises(ValueError, match="equal length"):
        call([], st, [], [], [])
    with pytest.raises(ValueError, match="equal length"):
        call([x, x], st, [t, t], [dark, dark], [dark, dark], consts=[None])
    with pytest.raises(ValueError, match="a dark std for every batch"):
        call([x, x], st, [t, t], [dark, dark], [dark, None])
    with pytest.raises(ValueError, match="constants for every batch"):
        call([x, x], st, [t, t], [dark, dark], [dark, dark], consts=[torch.zeros(4), None])
    with pytest.raises(RuntimeError, match="no CPU path"):      # as every front on a CPU stack
        call([x, x], st, [t, t], [dark, dark], [dark, dark], std_mode="multiplier", std_value=0.05)


def test_fuses_with_merge_ingest_truth_table():
    from clair_torch_amd import ops
    from clair_torch_amd.inference._staging import DeferredIngest
    from clair_torch_amd.inference.dark_field import DarkField
    fuses = DarkField.fuses_with_merge_ingest
    st = (("affine", 0.0, 1.0, 1.0, 0.0),)
    planar = {dt: DeferredIngest(torch.zeros((2, 3, 4, 5), dtype=dt), st, "nchw") for dt in (torch.uint8, torch.uint16, torch.float32)}
    bgr = DeferredIngest(torch.zeros((2, 4, 5, 3), dtype=torch.uint16), st, "nhwc_bgr")
    whole, band = ops.TileGeometry(h_global=4, row_offset=0), ops.TileGeometry(h_global=12, row_offset=4)
    for d in list(planar.values()) + [bgr, DeferredIngest(bgr.frames, st, "nhwc")]:
        for interp in ("linear", None):
            assert fuses(d, interp, None) and fuses(d, interp, False) and not fuses(d, interp, True)
        for interp in ("lookup", "catmull"):      # a matched batch carries uncertainties: reference order unless told otherwise
            assert not fuses(d, interp, None) and fuses(d, interp, False) and not fuses(d, interp, True)
    assert fuses(planar[torch.uint16], "linear", None, band) and fuses(planar[torch.uint16], "linear", None, whole)
    assert fuses(bgr, "linear", None, whole) and not fuses(bgr, "linear", None, band)          # no bands on interleaved frames
    assert not fuses(torch.zeros((2, 3, 4, 5)), "linear", None)                               # not deferred: ``fuses_with_merge`` decides
    assert not fuses(DeferredIngest(torch.zeros((3, 4, 5)), st, "nchw"), "linear", None)
    assert not fuses(DeferredIngest(torch.zeros((2, 3, 4, 5), dtype=torch.float64), st, "nchw"), "linear", None)
    assert not fuses(DeferredIngest(torch.zeros((2, 4, 5, 4), dtype=torch.uint8), st, "nhwc"), "linear", None)
    assert callable(DarkField.merge_ingest_batches)


# ---- compute_hdr_image's routing, every op a recorder -----------------------------------------------------------------------------
class _Some:
    """A dark-field dataset with an image for the frames in ``frames`` only."""

    def __init__(self, stack, frames):
        self.stack, self.frames = stack, set(frames)

    def get_matching_artefact_images(self, names):
        if not set(names) <= self.frames:
            return None, None, None, None
        return self.stack.get_matching_artefact_images(names)


@pytest.fixture()
def routed(monkeypatch):
    """compute_hdr_image on 12 planar uint16 frames of 3x4x6 in batches of 2 behind a black level, MULTIPLIER uncertainties, with
    ``ops``, the device and the halo exchange replaced: -> run(matched frames, **keywords) = the list of calls made."""
    from clair_torch_amd import ops
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, Normalize
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import dark_field, hdr_merge
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    from torch.utils.data import DataLoader
    calls = []
    result = (torch.zeros((3, 4, 6), dtype=torch.float64), torch.zeros((3, 4, 6)))

    def recorder(name, sizes):
        def op(*args, **kw):
            calls.append((name, sizes(args), kw.get("finalize")))
            return result if kw.get("finalize", True) else None
        return op

    monkeypatch.setattr(hdr_merge, "resolve_device", lambda device: torch.device("cpu"))
    monkeypatch.setattr(ops, "MergeState", lambda shape, dev, with_variance: SimpleNamespace(shape=tuple(shape), batches=0))
    monkeypatch.setattr(ops, "hdr_merge_dark_ingest_batches", recorder("dark_ingest", lambda a: [int(f.shape[0]) for f in a[0]]))
    monkeypatch.setattr(ops, "hdr_merge_ingest_batches", recorder("ingest", lambda a: [int(f.shape[0]) for f in a[0]]))
    monkeypatch.setattr(ops, "hdr_merge_dark_batch", recorder("dark", lambda a: [int(a[0].shape[0])]))
    monkeypatch.setattr(ops, "hdr_merge_dark_batches", recorder("dark_batches", lambda a: [int(f.shape[0]) for f in a[0]]))
    monkeypatch.setattr(ops, "hdr_merge_batches", recorder("plain", lambda a: [int(f.shape[0]) for f in a[0]]))
    monkeypatch.setattr(ops, "strided_downscale", lambda images, step, layout="nchw": images)

    def ingest_transform(frames, stages, layout="nchw", out=None, consts=None):
        calls.append(("ingest_transform", [int(frames.shape[0])], None))
        return torch.zeros(ops.ingest_shape(tuple(frames.shape), layout))

    monkeypatch.setattr(ops, "ingest_transform", ingest_transform)

    def dark_field_blur(images, dark, dark_std, **kw):
        calls.append(("blur", [int(images.shape[0])], None))
        return torch.zeros(tuple(images.shape)), torch.zeros(tuple(images.shape))

    monkeypatch.setattr(ops, "dark_field_blur", dark_field_blur)

    def exchange_halo(images, tile, group=None):
        calls.append(("halo", [int(images.shape[0])], str(images.dtype)))
        return None if tile is None else torch.zeros((images.shape[0], images.shape[1], 2, images.shape[3]), dtype=images.dtype)

    monkeypatch.setattr(dark_field, "exchange_halo", exchange_halo)
    codes = torch.zeros((12, 3, 4, 6), dtype=torch.uint16)
    ds = StackDataset(codes, [0.001 * 2 ** k for k in range(12)], missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05,
                      materialize_std=False)
    art = ArtefactStack(torch.zeros((3, 4, 6)), torch.zeros((3, 4, 6)))
    model = ICRFModelDirect(icrf=torch.stack([torch.linspace(0, 1, 16)] * 3), interpolation_mode=InterpMode.LINEAR)

    def run(frames=range(12), interp=InterpMode.LINEAR, tf=(CastTo("float32"), Normalize(65535, 64)), **kw):
        del calls[:]
        model.interpolation_mode = interp
        loader = DataLoader(ds, batch_size=2, shuffle=False, collate_fn=custom_collate)
        hdr_merge.compute_hdr_image(loader, "cpu", model, weight_fn=gaussian_value_weights, gpu_transforms=list(tf),
                                    dark_field_dataset=_Some(art, [ds.files[i] for i in frames]), **kw)
        return list(calls)

    return SimpleNamespace(run=run, hdr_merge=hdr_merge)


def _ops_only(calls):
    return [(name, sizes) for name, sizes, _ in calls if name != "halo"]


def test_routing_matched_unmatched_declined(routed):
    run = routed.run
    # every batch matched: queued, flushed at k batches and at the end; one batch per launch with k = 1
    assert _ops_only(run(fused_dark_ingest=True, dark_batches_per_launch=4)) == [("dark_ingest", [2, 2, 2, 2]), ("dark_ingest", [2, 2])]
    assert _ops_only(run(fused_dark_ingest=True, dark_batches_per_launch=1)) == [("dark_ingest", [2])] * 6
    calls = run(fused_dark_ingest=True, dark_batches_per_launch=16)
    assert _ops_only(calls) == [("dark_ingest", [2] * 6)] and [c[2] for c in calls if c[0] == "dark_ingest"] == [True]
    # the halo rows are exchanged on the RAW frames when a batch is queued, in loader order, before any launch
    assert [c[0] for c in calls] == ["halo"] * 6 + ["dark_ingest"] and {c[2] for c in calls if c[0] == "halo"} == {"torch.uint16"}
    # unmatched batches take the chain + merge queue; the key changes mid-stream
    some = [2, 3, 4, 5, 10, 11]
    assert _ops_only(run(some, fused_dark_ingest=True, dark_batches_per_launch=16)) == \
        [("ingest", [2]), ("dark_ingest", [2, 2]), ("ingest", [2, 2]), ("dark_ingest", [2])]
    # declined (the reference-order kernel is not fused): materialised, then today's path
    declined = _ops_only(run(fused_dark_ingest=True, reference_order=True))
    assert declined == _ops_only(run(fused_dark_ingest=False, reference_order=True))
    assert declined == [("ingest_transform", [2]), ("blur", [2])] * 6 + [("plain", [2] * 6)]


def test_routing_off_is_todays(routed):
    run = routed.run
    today = _ops_only(run(fused_dark_ingest=False))
    assert today == [("ingest_transform", [2]), ("dark", [2])] * 6
    assert _ops_only(run()) == today or routed.hdr_merge.FUSED_DARK_INGEST_DEFAULT   # the default follows the measured rule
    assert _ops_only(run(fused_dark_ingest=True, fused_dark=False)) == _ops_only(run(fused_dark_ingest=False, fused_dark=False))
    assert all(name != "dark_ingest" for name, _ in _ops_only(run(fused_dark_ingest=True, fused_dark=False)))
    queued = _ops_only(run(fused_dark_ingest=False, dark_batches_per_launch=3))     # staged as float32, then the existing queue
    assert [c for c in queued if c[0] != "ingest_transform"] == [("dark_batches", [2, 2, 2])] * 2
    assert queued.count(("ingest_transform", [2])) == 6


def test_routing_byte_cap(routed, monkeypatch):
    one = 2 * 3 * 4 * 6 * 2 + 2 * (2 * 3 * 4 * 6 * 4)      # two uint16 frames, their dark fields and dark stds as float32
    monkeypatch.setattr(routed.hdr_merge, "DARK_QUEUE_BYTES", 2 * one - 1)
    assert _ops_only(routed.run(fused_dark_ingest=True, dark_batches_per_launch=16)) == [("dark_ingest", [2])] * 6
    monkeypatch.setattr(routed.hdr_merge, "DARK_QUEUE_BYTES", 3 * one)
    assert _ops_only(routed.run(fused_dark_ingest=True, dark_batches_per_launch=16)) == [("dark_ingest", [2, 2, 2])] * 2


def test_compute_hdr_image_has_the_keyword():
    import inspect
    from clair_torch_amd.inference import compute_hdr_image, hdr_merge
    p = inspect.signature(compute_hdr_image).parameters
    assert p["fused_dark_ingest"].default is hdr_merge.FUSED_DARK_INGEST_DEFAULT and type(hdr_merge.FUSED_DARK_INGEST_DEFAULT) is bool
