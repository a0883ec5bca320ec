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


# ---- the same routing with the keywords of every call, the MergeState and the halo exchange in one record ---------------------------
# Recorded from compute_hdr_image before its four queues became one; the literals below are the contract.
MERGE_OPS = {"hdr_merge_dark_ingest_batches": "dark_ingest", "hdr_merge_ingest_batches": "ingest", "hdr_merge_dark_batch": "dark",
             "hdr_merge_dark_batches": "dark_batches", "hdr_merge_batches": "plain"}


@pytest.fixture()
def events(routed, monkeypatch):
    """``routed`` with a second recorder around each replacement: -> run(n_frames, matched, **keywords) = the events in order,
    ("state", shape, with_variance) for a MergeState made, ("halo", frames) for an exchange, ("ingest_transform" | "blur", frames),
    and (op, batch sizes, which MergeState it got (0 = the first one made) | None, finalize, std_mode, tile, layout) for a merge.
    ``matched``: the frames a dark field matches, None = no dark-field dataset at all."""
    from clair_torch_amd import ops
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, Normalize
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import dark_field, hdr_merge
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    from torch.utils.data import DataLoader
    log, states = [], []

    def merge_op(name, inner):
        def op(*args, **kw):
            sizes = [int(args[0].shape[0])] if name == "dark" else [int(f.shape[0]) for f in args[0]]
            tile = kw.get("tile")
            log.append((name, sizes, None if kw["state"] is None else [id(s) for s in states].index(id(kw["state"])), kw["finalize"],
                        kw["std_mode"], None if tile is None else (tile.h_global, tile.row_offset), kw.get("layout")))
            return inner(*args, **kw)
        return op

    for attr, name in MERGE_OPS.items():
        monkeypatch.setattr(ops, attr, merge_op(name, getattr(ops, attr)))
    make_state = ops.MergeState

    def merge_state(shape, dev, with_variance):
        states.append(make_state(shape, dev, with_variance))
        log.append(("state", tuple(shape), with_variance))
        return states[-1]

    monkeypatch.setattr(ops, "MergeState", merge_state)

    def counted(name, inner):
        def op(images, *args, **kw):
            log.append((name, int(images.shape[0])))
            return inner(images, *args, **kw)
        return op

    monkeypatch.setattr(ops, "ingest_transform", counted("ingest_transform", ops.ingest_transform))
    monkeypatch.setattr(ops, "dark_field_blur", counted("blur", ops.dark_field_blur))
    monkeypatch.setattr(dark_field, "exchange_halo", counted("halo", dark_field.exchange_halo))
    flat = (torch.zeros((3, 4, 6), dtype=torch.float64), torch.zeros((3, 4, 6)))
    monkeypatch.setattr(hdr_merge, "_flat_field_epilogue", lambda state, *a: flat)
    art = ArtefactStack(torch.zeros((3, 4, 6)), torch.zeros((3, 4, 6)))
    model = ICRFModelDirect(icrf=torch.stack([torch.linspace(0, 1, 16)] * 3), interpolation_mode=InterpMode.LINEAR)

    def run(n_frames=12, matched=None, existing=None, **kw):
        del log[:], states[:]
        if existing is not None:            # one of the runs of the three tests above, through ``routed.run`` itself
            routed.run(*existing, **kw)
            return list(log)
        ds = StackDataset(torch.zeros((n_frames, 3, 4, 6), dtype=torch.uint16), [0.001 * 2 ** (k % 12) for k in range(n_frames)],
                          missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
        if matched is not None:
            kw["dark_field_dataset"] = _Some(art, [ds.files[i] for i in matched])
        loader = DataLoader(ds, batch_size=2, shuffle=False, collate_fn=custom_collate)
        hdr_merge.compute_hdr_image(loader, "cpu", model, weight_fn=gaussian_value_weights,
                                    gpu_transforms=[CastTo("float32"), Normalize(65535, 64)], **kw)
        return list(log)

    return SimpleNamespace(run=run, flat=art)


H, T, B, ST = ("halo", 2), ("ingest_transform", 2), ("blur", 2), ("state", (3, 4, 6), True)
SOME = [2, 3, 4, 5, 10, 11]


def _m(name, batches, state, finalize, tile=None, std_mode="multiplier"):
    """The event of a merge op on ``batches`` batches of 2 frames; the dark ops on staged images take no layout."""
    return (name, [2] * batches, state, finalize, std_mode, tile, None if name in ("dark", "dark_batches") else "nchw")


def test_routing_without_a_dark_field_dataset(events):
    run = events.run
    assert run(fused_ingest=True) == [_m("ingest", 6, None, True)]
    assert run(fused_ingest=False) == [T] * 6 + [_m("plain", 6, None, True)]
    # 18 batches: MAX_MERGE_BATCHES per call, on a MergeState made before the first launch
    assert run(36, fused_ingest=True) == [ST, _m("ingest", 16, 0, False), _m("ingest", 2, 0, True)]
    assert run(36, fused_ingest=False) == [T] * 17 + [ST, _m("plain", 16, 0, False), T, _m("plain", 2, 0, True)]


def test_routing_with_a_flat_field_dataset(events):
    """No call finalizes, one MergeState is made before the first launch and every call gets it."""
    run, flat = events.run, events.flat
    assert run(fused_ingest=True, flat_field_dataset=flat) == [ST, _m("ingest", 6, 0, False)]
    assert run(36, fused_ingest=False, flat_field_dataset=flat) == [T] * 17 + [ST, _m("plain", 16, 0, False), T, _m("plain", 2, 0, False)]
    assert run(matched=range(12), fused_dark_ingest=True, dark_batches_per_launch=4, flat_field_dataset=flat) == \
        [H] * 5 + [ST, _m("dark_ingest", 4, 0, False), H, _m("dark_ingest", 2, 0, False)]
    assert run(matched=range(12), fused_dark_ingest=False, dark_batches_per_launch=4, flat_field_dataset=flat) == \
        [T, H] * 5 + [ST, _m("dark_batches", 4, 0, False), T, H, _m("dark_batches", 2, 0, False)]
    assert run(matched=SOME, fused_dark_ingest=False, flat_field_dataset=flat) == \
        [T, T, ST, _m("plain", 1, 0, False), H, _m("dark", 1, 0, False), T, H, _m("dark", 1, 0, False), T, T, T,
         _m("plain", 2, 0, False), H, _m("dark", 1, 0, False)]


def test_routing_of_a_row_band(events):
    """Planar frames: the halo rows of a queued batch are exchanged when it is queued, in loader order, before the launch that
    consumes them; the single-batch dark path exchanges after the flush of what was queued before it."""
    from clair_torch_amd import ops
    run, band = events.run, (12, 4)
    tile = ops.TileGeometry(h_global=12, row_offset=4)
    assert run(matched=range(12), fused_dark_ingest=True, dark_batches_per_launch=4, tile=tile) == \
        [H] * 5 + [ST, _m("dark_ingest", 4, 0, False, band), H, _m("dark_ingest", 2, 0, True, band)]
    assert run(matched=range(12), fused_dark_ingest=False, dark_batches_per_launch=4, tile=tile) == \
        [T, H] * 5 + [ST, _m("dark_batches", 4, 0, False, band), T, H, _m("dark_batches", 2, 0, True, band)]
    assert run(matched=SOME, fused_dark_ingest=False, tile=tile) == \
        [T, T, ST, _m("plain", 1, 0, False, band), H, _m("dark", 1, 0, False, band), T, H, _m("dark", 1, 0, False, band), T, T, T,
         _m("plain", 2, 0, False, band), H, _m("dark", 1, 0, True, band)]
    assert run(matched=SOME, fused_dark_ingest=True, dark_batches_per_launch=16, tile=tile) == \
        [H, ST, _m("ingest", 1, 0, False, band), H, _m("dark_ingest", 2, 0, False, band), H, _m("ingest", 2, 0, False, band),
         _m("dark_ingest", 1, 0, True, band)]


def test_keywords_of_the_routed_calls(events):
    """The runs of the three routing tests above, with state=, finalize=, std_mode=, tile= and layout= of every call."""
    run = events.run
    assert run(existing=(), fused_dark_ingest=True, dark_batches_per_launch=4) == \
        [H] * 5 + [ST, _m("dark_ingest", 4, 0, False), H, _m("dark_ingest", 2, 0, True)]
    assert run(existing=(), fused_dark_ingest=True, dark_batches_per_launch=1) == \
        [H, H, ST, _m("dark_ingest", 1, 0, False)] + [H, _m("dark_ingest", 1, 0, False)] * 4 + [_m("dark_ingest", 1, 0, True)]
    assert run(existing=(), fused_dark_ingest=True, dark_batches_per_launch=16) == [H] * 6 + [_m("dark_ingest", 6, None, True)]
    assert run(existing=(SOME,), fused_dark_ingest=True, dark_batches_per_launch=16) == \
        [H, ST, _m("ingest", 1, 0, False), H, _m("dark_ingest", 2, 0, False), H, _m("ingest", 2, 0, False), _m("dark_ingest", 1, 0, True)]
    declined = [T, H, B] * 6 + [_m("plain", 6, None, True, std_mode="explicit")]
    assert run(existing=(), fused_dark_ingest=True, reference_order=True) == declined
    assert run(existing=(), fused_dark_ingest=False, reference_order=True) == declined
    assert run(existing=(), fused_dark_ingest=True, fused_dark=False) == declined
    assert run(existing=(), fused_dark_ingest=False) == \
        [T, ST, H, _m("dark", 1, 0, False)] + [T, H, _m("dark", 1, 0, False)] * 4 + [T, H, _m("dark", 1, 0, True)]
    assert run(existing=(), fused_dark_ingest=False, dark_batches_per_launch=3) == \
        [T, H] * 4 + [ST, _m("dark_batches", 3, 0, False)] + [T, H] * 2 + [_m("dark_batches", 3, 0, True)]


def test_keywords_under_the_byte_cap(events, routed, monkeypatch):
    one = 2 * 3 * 4 * 6 * 2 + 2 * (2 * 3 * 4 * 6 * 4)      # as in test_routing_byte_cap
    monkeypatch.setattr(routed.hdr_merge, "DARK_QUEUE_BYTES", 2 * one - 1)
    assert events.run(existing=(), fused_dark_ingest=True, dark_batches_per_launch=16) == \
        [H, H, ST, _m("dark_ingest", 1, 0, False)] + [H, _m("dark_ingest", 1, 0, False)] * 4 + [_m("dark_ingest", 1, 0, True)]
    monkeypatch.setattr(routed.hdr_merge, "DARK_QUEUE_BYTES", 3 * one)
    assert events.run(existing=(), fused_dark_ingest=True, dark_batches_per_launch=16) == \
        [H] * 4 + [ST, _m("dark_ingest", 3, 0, False), H, H, _m("dark_ingest", 3, 0, True)]
    # the staged-image queue counts the same bytes (float32 images: twice the frames' share)
    monkeypatch.setattr(routed.hdr_merge, "DARK_QUEUE_BYTES", 3 * (one + 2 * 3 * 4 * 6 * 2))
    assert events.run(existing=(), fused_dark_ingest=False, dark_batches_per_launch=16) == \
        [T, H] * 4 + [ST, _m("dark_batches", 3, 0, False)] + [T, H] * 2 + [_m("dark_batches", 3, 0, True)]


def test_fallback_route_and_batch_order_statuses(lib):
    """What the walk over the batch list answers where the scales of all batches do not fit the LDS and those of each batch do
    (16 batches of 4, one channel, the table of LDS_EDGE_POINTS), without a launch."""
    from clair_torch_amd import _native as nv
    FIRST, FINAL, ONE = nv.MERGE_FIRST_BATCH, nv.MERGE_FINALIZE, nv.MERGE_REQUIRE_ONE_LAUNCH
    fake = 0x1000
    fakep = ctypes.c_void_p(fake)
    edge = nv.Icrf(lut_dev=0x2000, n_points=LDS_EDGE_POINTS, interp=nv.INTERP_LINEAR)
    state = (fakep,) * 3
    stage = (nv.IngestStage * 1)(nv.IngestStage(kind=nv.INGEST_AFFINE, sub=64.0, div=1000.0, mul=1.0, add=0.0))

    def call(sizes=(4,) * 16, frames=None, dark_batches=None, state=(None, None, None), flags=FIRST | FINAL):
        k = len(sizes)
        geom = _geom(c=1)
        frames = [fake] * k if frames is None else frames
        dark_batches = list(sizes) if dark_batches is None else dark_batches
        return lib.ct_hdr_merge_dark_ingest_batches(
            _pointers(frames), (ctypes.c_int32 * k)(*sizes), k, nv.DTYPE_U16, ctypes.byref(geom), stage, 1, None, None, None,
            nv.STD_MULTIPLIER, 0.05, _pointers([fake] * k), _pointers([fake] * k), (ctypes.c_int32 * k)(*dark_batches), 0.05, 50.0, fakep,
            ctypes.byref(edge), nv.WEIGHT_GAUSS, state[0], state[1], state[2], fakep, fakep, flags, None)

    assert call(flags=FIRST | FINAL | ONE, state=state) == TOO_LARGE
    assert call(flags=FIRST | FINAL | ONE) == TOO_LARGE            # the flag is looked at before the state
    assert call(flags=FIRST | FINAL) == UNSUPPORTED                # a whole merge, but every launch but the last leaves a state
    assert call(flags=0) == INVALID and call(flags=FIRST) == INVALID and call(flags=FINAL) == INVALID   # (every batch's own refusal)
    # an empty batch is not skipped: ct_hdr_merge_dark_batch's judgement refuses it
    holed = (4,) * 7 + (0,) + (4,) * 8
    assert call(sizes=holed, flags=FIRST | FINAL | ONE, state=state) == INVALID and call(sizes=holed, state=state) == INVALID
    # the first batch's refusal before the second's, either way round
    assert call(sizes=(4, 3), dark_batches=[1, 2]) == UNSUPPORTED and call(sizes=(4, 3), dark_batches=[2, 1]) == INVALID
    assert call(sizes=(1 << 16, 2), frames=[fake, None]) == TOO_LARGE and call(sizes=(2, 1 << 16), frames=[None, fake]) == INVALID
