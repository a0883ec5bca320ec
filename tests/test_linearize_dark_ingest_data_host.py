"""The fused chain + dark-field blur + linearization with per-frame constants, without a GPU: ct_linearize_dark_ingest_data is
declared, exported and refuses every malformed call before any launch; the ops front raises where its sibling and
linearize_ingest_frames(consts=) raise; DarkField.fuses_with_linearize_ingest_data decides the route; the generator has the
keyword, off by default."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, NO_GRADIENT, TOO_LARGE = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    from clair_torch_amd import build, _native
    build.build()
    return _native.load()


def _geom(c=3, h=4, w=4, layout=0, h_global=None, row_offset=0):
    from clair_torch_amd import _native as nv
    return nv.Geometry(channels=c, h_tile=h, width=w, h_global=h if h_global is None else h_global, row_offset=row_offset,
                       image_stride=c * h * w, layout=layout)


def test_the_symbol_is_declared_and_exported_and_the_abi_stays_3(lib):
    from clair_torch_amd import _native as nv
    text = open(os.path.join(ROOT, "include", "clair_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+ct_linearize_dark_ingest_data\s*\(([^)]*)\)", header)
    assert m, "not declared in include/clair_hip.h"
    sibling = re.search(r"\bint\s+ct_linearize_dark_ingest\s*\(([^)]*)\)", header)
    assert sibling and sibling.start() < m.start(), "declared beside (behind) its sibling"
    assert "ct_linearize_dark_ingest_data" in nv.EXPORTS and hasattr(lib, "ct_linearize_dark_ingest_data")
    assert len(lib.ct_linearize_dark_ingest_data.argtypes) == len(m.group(1).split(",")) == 18
    assert lib.ct_linearize_dark_ingest_data.restype is ctypes.c_int32
    # the sibling's arguments with consts_dev in front of the stream
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    sibling_names = [a.split()[-1].lstrip("*") for a in sibling.group(1).split(",")]
    assert names == sibling_names[:-1] + ["consts_dev", "stream"]
    assert lib.ct_linearize_dark_ingest_data.argtypes[:16] == lib.ct_linearize_dark_ingest.argtypes[:16]
    assert lib.ct_abi_version() == 3 == nv.ABI_VERSION
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", text)


def test_ct_linearize_dark_ingest_data_refuses_before_any_launch(lib):
    """Every call below is malformed and made-up pointers stand for device memory: a status comes back with no GPU present,
    nothing is read (the pointer arrays and the stage list are host memory and real)."""
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    NHWC, BGR = nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    AFFINE, CLAMP, DATA = nv.INGEST_AFFINE, nv.INGEST_CLAMP, nv.INGEST_AFFINE_DATA
    fake = ctypes.c_void_p(0x1000)
    consts_ok = ctypes.c_void_p(0x4000)
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    lookup = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LOOKUP)
    missing = object()

    def ptrs(n, value=0x3000):
        return (ctypes.c_void_p * max(n, 1))(*([value] * max(n, 1)))

    def chain(*kinds, pairs=None):
        arr = (nv.IngestStage * max(len(kinds), 1))()
        for k, kind in enumerate(kinds):
            arr[k].kind, arr[k].div, arr[k].mul = kind, 1.0, 1.0
            for c in range(4):
                arr[k].lo[c], arr[k].hi[c] = (0.0, 1.0) if pairs is None else pairs[c]
        return arr, len(kinds)

    one = chain(DATA)

    def call(frames=fake, dtype=U16, n=2, geom=missing, stages=one, std=None, std_mode=nv.STD_MULTIPLIER, darks=missing,
             dark_stds=missing, model=linear, lin=fake, std_out=fake, consts=consts_ok):
        geom = _geom() if geom is missing else geom
        gp = None if geom is None else ctypes.byref(geom)
        mp = None if model is None else ctypes.byref(model)
        darks = ptrs(n) if darks is missing else darks
        dark_stds = ptrs(n) if dark_stds is missing else dark_stds
        return lib.ct_linearize_dark_ingest_data(frames, dtype, n, gp, stages[0], stages[1], std, std_mode, 0.05, darks, dark_stds,
                                                 0.05, 50.0, mp, lin, std_out, consts, None)

    # ---- the constants: NULL (then a data stage has none to read) and misaligned; two data stages; too many stages ----
    assert call(consts=None) == INVALID
    assert call(consts=ctypes.c_void_p(0x4002)) == INVALID and call(consts=ctypes.c_void_p(0x4001)) == INVALID
    assert call(consts=ctypes.c_void_p(0x4002), stages=chain(AFFINE)) == INVALID      # ... whether or not a stage reads them
    assert call(stages=chain(DATA, DATA)) == INVALID and call(stages=chain(DATA, CLAMP, DATA)) == INVALID
    assert call(stages=chain(AFFINE, DATA, CLAMP, AFFINE, CLAMP)) == INVALID          # more than CT_INGEST_MAX_STAGES
    assert call(stages=(one[0], 5)) == INVALID and call(stages=(one[0], -1)) == INVALID and call(stages=(None, 1)) == INVALID
    assert call(stages=chain(7)) == INVALID
    # ---- row bands, LOOKUP, a hole in the dark pointers, an interleaved layout with C != 3 ----
    assert call(geom=_geom(h=4, h_global=12, row_offset=4)) == UNSUPPORTED
    assert call(geom=_geom(h=4, h_global=8)) == UNSUPPORTED and call(geom=_geom(h=4, h_global=8, row_offset=4, layout=BGR)) == UNSUPPORTED
    for mode in (nv.STD_NONE, nv.STD_CONSTANT, nv.STD_MULTIPLIER):
        assert call(model=lookup, std_mode=mode) == NO_GRADIENT
    assert call(model=lookup, std_mode=nv.STD_EXPLICIT, std=fake, geom=_geom(layout=BGR)) == NO_GRADIENT
    holed = ptrs(3)
    holed[1] = None
    assert call(n=3, darks=holed) == INVALID and call(n=3, dark_stds=holed) == INVALID
    assert call(geom=_geom(c=4, layout=NHWC)) == UNSUPPORTED and call(geom=_geom(c=1, layout=BGR)) == UNSUPPORTED
    # ---- everything else its sibling refuses, in its order ----
    assert call(frames=None) == INVALID and call(geom=None) == INVALID and call(darks=None) == INVALID and call(dark_stds=None) == INVALID
    assert call(lin=None) == INVALID and call(std_out=None) == INVALID and call(n=0) == INVALID and call(n=-1) == INVALID
    assert call(geom=_geom(w=1)) == INVALID and call(geom=_geom(h=1)) == INVALID
    assert call(std_mode=4) == INVALID and call(std_mode=nv.STD_EXPLICIT, std=None) == INVALID
    assert call(dtype=3) == INVALID and call(geom=_geom(layout=3)) == INVALID
    differ = chain(CLAMP, pairs=[(0.0, 1.0), (0.1, 0.9), (0.0, 1.0), (0.0, 1.0)])
    assert call(geom=_geom(c=5), stages=differ) == UNSUPPORTED
    assert call(model=None) == INVALID and call(model=nv.Icrf(lut_dev=0x2000, n_points=1, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)) == TOO_LARGE
    assert call(geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE
    odd = ctypes.c_void_p(0x1002)
    assert call(frames=ctypes.c_void_p(0x1001)) == INVALID and call(dtype=F32, frames=odd) == INVALID
    assert call(std_mode=nv.STD_EXPLICIT, std=odd) == INVALID and call(lin=odd) == INVALID and call(std_out=odd) == INVALID
    assert call(darks=ptrs(2, 0x3002)) == INVALID and call(dark_stds=ptrs(2, 0x3002)) == INVALID
    assert call(dtype=U8, frames=ctypes.c_void_p(0x1001), darks=ptrs(2, 0x3002)) == INVALID
    # ---- the first refusal wins ----
    assert call(geom=_geom(h=4, h_global=8), stages=chain(DATA, DATA)) == UNSUPPORTED      # the band before the stage list
    assert call(geom=_geom(h=4, h_global=8), consts=None) == UNSUPPORTED
    assert call(stages=chain(DATA, DATA), model=lookup) == INVALID                         # the stage list before the model
    assert call(consts=ctypes.c_void_p(0x4002), model=lookup) == INVALID                   # ... and so the constants
    assert call(geom=_geom(c=1, layout=BGR), model=lookup) == UNSUPPORTED
    # ---- ct_linearize_dark_ingest itself still refuses the kind ----
    plain = lib.ct_linearize_dark_ingest
    g = _geom()
    for stages in (one, chain(AFFINE, DATA)):
        assert plain(fake, U16, 2, ctypes.byref(g), stages[0], stages[1], None, nv.STD_MULTIPLIER, 0.05, ptrs(2), ptrs(2), 0.05, 50.0,
                     ctypes.byref(linear), fake, fake, None) == INVALID


def test_front_end_refuses_cpu_tensors_and_malformed_constants():
    from clair_torch_amd import ops
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)
    x = torch.zeros((2, 3, 4, 4), dtype=torch.uint8)
    dark = torch.zeros((2, 3, 4, 4))
    data = [("affine_data", 1, 0)]
    K = torch.zeros((2, 4))
    call = ops.linearize_dark_ingest_frames_data
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(x, data, dark, dark, lut, consts=K, std_mode="multiplier", std_value=0.05)
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(x.permute(0, 2, 3, 1).contiguous(), data, dark, dark, lut, consts=K, layout="nhwc_bgr")
    with pytest.raises(TypeError):
        call([1, 2], data, dark, dark, lut, consts=K)
    with pytest.raises(TypeError):
        call(x, data, dark, dark, lut)                      # consts is required

    class _OnDevice(torch.Tensor):      # is_cuda is all the front asks of a tensor before the shape errors
        is_cuda = True

    xd, Kd = x.as_subclass(_OnDevice), K.as_subclass(_OnDevice)
    with pytest.raises(RuntimeError, match="consts is on cpu"):
        call(xd, data, dark, dark, lut, consts=K)
    with pytest.raises(TypeError, match="takes the \\(F, 4\\) consts"):
        call(xd, data, dark, dark, lut, consts=None)
    with pytest.raises(TypeError, match="consts must be a torch.Tensor"):
        call(xd, data, dark, dark, lut, consts=[0.0, 1.0, 0.0, 1.0])
    with pytest.raises(TypeError, match="consts must be float32"):
        call(xd, data, dark, dark, lut, consts=Kd.double())
    for bad in (Kd[0], Kd[:1], torch.zeros((3, 4)).as_subclass(_OnDevice), torch.zeros((2, 2)).as_subclass(_OnDevice),
                torch.zeros((2, 8)).as_subclass(_OnDevice)[:, ::2]):
        with pytest.raises(ValueError, match="consts must be the contiguous \\(2, 4\\) float32 tensor"):
            call(xd, data, dark, dark, lut, consts=bad)
    # the stage list: one data stage at most, and everything linearize_dark_ingest_frames refuses
    with pytest.raises(ValueError, match="one \\('affine_data', mul, add\\) stage"):
        call(xd, data * 2, dark, dark, lut, consts=Kd)
    with pytest.raises(ValueError, match="at most 4 stages"):
        call(xd, data + [("affine", 0, 255, 1, 0)] * 4, dark, dark, lut, consts=Kd)
    with pytest.raises(ValueError, match="stage 1: expected"):
        call(xd, data + [("gamma", 2.2)], dark, dark, lut, consts=Kd)
    with pytest.raises(ValueError, match="4-dimensional"):
        call(xd[0], data, dark, dark, lut, consts=Kd)
    with pytest.raises(ValueError, match="unknown layout"):
        call(xd, data, dark, dark, lut, consts=Kd, layout="chwn")
    with pytest.raises(ValueError, match="takes \\(B, H, W, 3\\) frames"):
        call(xd, data, dark, dark, lut, consts=Kd, layout="nhwc_bgr")
    with pytest.raises(ValueError, match="unknown std_mode"):
        call(xd, data, dark, dark, lut, consts=Kd, std_mode="bogus")
    with pytest.raises(ValueError, match="dark_stds is required"):
        call(xd, data, dark, None, lut, consts=Kd)
    # a new front beside linearize_dark_ingest_frames, whose signature stays what it was
    p = inspect.signature(call).parameters
    assert list(p)[:6] == ["frames", "stages", "darks", "dark_stds", "lut", "interp"] and p["interp"].default == "linear"
    assert p["consts"].kind is inspect.Parameter.KEYWORD_ONLY and p["consts"].default is inspect.Parameter.empty
    for name, default in (("std", None), ("std_mode", "none"), ("std_value", 0.0), ("layout", "nchw"), ("out", None),
                          ("threshold", 0.05), ("alpha", 50.0)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name
    assert "consts" not in inspect.signature(ops.linearize_dark_ingest_frames).parameters
    with pytest.raises(ValueError, match="stage 0: expected"):       # ... and it still takes no data stage
        ops.linearize_dark_ingest_frames(xd, data, dark, dark, lut)


def _plan(probe, transforms, **kw):
    from clair_torch_amd.common.transforms import plan_staging
    kw.setdefault("on_device", True)
    return plan_staging(probe, transforms, planar=True, **kw)


def test_dark_field_ingest_data_route_decision():
    from dataclasses import replace

    from clair_torch_amd.common.transforms import CastTo, ClampAlongDims, CvToTorch, Normalize, StridedDownscale
    from clair_torch_amd.inference.dark_field import DarkField
    fuses = DarkField.fuses_with_linearize_ingest_data
    earlier = (DarkField.fuses_with_linearize, DarkField.fuses_with_linearize_ingest)
    assert isinstance(inspect.getattr_static(DarkField, "fuses_with_linearize_ingest_data"), staticmethod)
    u16, u8, px = torch.zeros((1, 3, 6, 5), dtype=torch.uint16), torch.zeros((1, 3, 6, 5), dtype=torch.uint8), torch.zeros((1, 3, 6, 5))
    raw16, raw8 = torch.zeros((1, 6, 5, 3), dtype=torch.uint16), torch.zeros((1, 6, 5, 3), dtype=torch.uint8)
    cast, cv = CastTo("float32"), CvToTorch()
    clamp = ClampAlongDims(1, [(0.0, 1.0), (0.01, 0.95), (0.0, 0.9)])
    for interp in ("linear", "catmull"):
        for probe, chain, layout in ((u16, [cast, Normalize()], "nchw"), (u8, [cast, Normalize()], "nchw"),
                                     (raw16, [cv, cast, Normalize()], "nhwc_bgr"), (raw8, [cv, cast, Normalize()], "nhwc_bgr"),
                                     (px, [Normalize()], "nchw"),
                                     (u16, [cast, Normalize(65535, 64), Normalize()], "nchw"),          # a black level in front
                                     (raw16, [cv, cast, Normalize(65535, 64), Normalize()], "nhwc_bgr"),
                                     (u16, [cast, Normalize(None, 64)], "nchw"), (u16, [cast, Normalize(), clamp], "nchw")):
            plan = _plan(probe, chain)
            assert plan.route == "ingest_data" and plan.step == 1 and plan.source_layout == layout, (chain, plan)
            assert fuses(probe, plan, interp), chain
            for first in earlier:                          # the two decisions in front still decline these plans
                assert not first(probe, plan, interp), chain
                assert not first(probe, _plan(probe, chain, on_device=False), interp), chain
            # planned for the host, the route does not exist: declined
            assert _plan(probe, chain, on_device=False).route != "ingest_data"
            assert not fuses(probe, _plan(probe, chain, on_device=False), interp), chain
        # declined: constant chains and the code pair (the decisions in front take them)
        for probe, chain in ((u16, [cast, Normalize(65535, 64)]), (u16, [cast, Normalize(65535, 0)]), (px, []),
                             (px, [ClampAlongDims(1, (0.0, 1.0))]), (raw16, [cv, cast, Normalize(65535, 0)])):
            assert _plan(probe, chain).route != "ingest_data" and not fuses(probe, _plan(probe, chain), interp), chain
        # a StridedDownscale on either side of the data stage, with the step left to the staging or to a kernel
        for chain in ([cast, Normalize(), StridedDownscale(2)], [StridedDownscale(2), cast, Normalize()],
                      [cv, StridedDownscale(2), cast, Normalize()], [cv, cast, Normalize(), StridedDownscale(2)]):
            probe = raw16 if chain[0] is cv else u16
            plan = _plan(probe, chain)
            assert plan.route == "ingest_data" and plan.step == 2
            assert not fuses(probe, plan, interp) and not fuses(probe, _plan(probe, chain, step_in_kernel=True), interp)
        # two data-dependent stages run as torch ops; 3-D probes; float64 frames; things that are no tensors
        assert not fuses(u16, _plan(u16, [cast, Normalize(), Normalize()]), interp)
        plan = _plan(u16, [cast, Normalize()])
        assert not fuses(u16[0], _plan(u16[0], [cast, Normalize()]), interp) and not fuses(u16[0], plan, interp)
        assert not fuses(u16.to(torch.float64), plan, interp) and not fuses(object(), plan, interp)
        assert not fuses(u16.to(torch.int16), plan, interp)
    # LOOKUP: no gradient path; the frame-by-frame route raises it at the first matched frame
    assert not fuses(u16, _plan(u16, [cast, Normalize()]), "lookup") and not fuses(raw16, _plan(raw16, [cv, cast, Normalize()]), "lookup")
    assert not fuses(u16, _plan(u16, [cast, Normalize()]), None)
    # the other layouts and steps of a hand-made plan
    plan = _plan(u16, [cast, Normalize()])
    assert fuses(u16, replace(plan, source_layout="nhwc_bgr"), "linear") and not fuses(u16, replace(plan, source_layout="nhwc"), "linear")
    assert not fuses(u16, replace(plan, step=2), "linear") and not fuses(u16, replace(plan, route="ingest"), "linear")


def test_generator_has_the_keyword_off_by_default():
    from clair_torch_amd.inference import linearization, linearize_dataset_generator
    p = inspect.signature(linearize_dataset_generator).parameters
    assert "fused_dark_ingest_data" in p and p["fused_dark_ingest_data"].default is False
    assert p["fused_dark_ingest_data"].default is linearization.FUSED_DARK_INGEST_DATA_DEFAULT
    assert p["fused_dark_ingest_data"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    # the keywords in front keep their places and defaults
    assert list(p)[:10] == ["dataloader", "device", "icrf_model", "flatfield_dataset", "gpu_transforms", "dark_field_dataset",
                            "output_layout", "fused_dark", "fused_dark_ingest", "fused_flat"]
    assert p["fused_dark"].default is linearization.FUSED_DARK_DEFAULT
    assert p["fused_dark_ingest"].default is linearization.FUSED_DARK_INGEST_DEFAULT and p["fused_flat"].default is linearization.FUSED_FLAT_DEFAULT
    # a non-bool value is a TypeError before anything else is looked at, like fused_flat
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="fused_dark_ingest_data must be a bool"):
            next(linearize_dataset_generator(None, "cuda", None, fused_dark_ingest_data=bad))
    with pytest.raises(TypeError, match="fused_flat must be a bool"):
        next(linearize_dataset_generator(None, "cuda", None, fused_flat=1, fused_dark_ingest_data=1))
    # the launchers take the constants through a trailing keyword; the parameters in front keep names and defaults
    runs = inspect.signature(linearization._linearize_dark_runs).parameters
    assert list(runs)[-3:] == ["chain", "flat", "consts"] and all(runs[n].default is None for n in ("chain", "flat", "consts"))
    run = inspect.signature(linearization._linearize_run).parameters
    assert list(run)[-6:] == ["stages", "layout", "step", "consts", "pairs", "flat"] and run["consts"].default is None
    plan = inspect.signature(linearization._pipeline_plan).parameters
    assert list(plan)[-1] == "fused_dark_ingest_data" and plan["fused_dark_ingest_data"].default is False


def test_the_plan_is_asked_only_with_all_three_keywords():
    """_pipeline_plan on host probes: the "ingest_data" plan comes back only with a dark field, fused_dark, fused_dark_ingest
    and the new keyword; everything else is what it was (None: frame by frame)."""
    from clair_torch_amd.common.transforms import CastTo, CvToTorch, Normalize, StridedDownscale
    from clair_torch_amd.inference import linearization
    from clair_torch_amd.inference.dark_field import DarkField
    dark = DarkField(None, None, torch.device("cuda", 0))
    dev = torch.device("cuda", 0)
    u16, raw16 = torch.zeros((1, 3, 6, 5), dtype=torch.uint16), torch.zeros((1, 6, 5, 3), dtype=torch.uint16)
    cast = CastTo("float32")

    def plan(probe, tf, *flags, interp="linear", with_dark=True):
        return linearization._pipeline_plan(probe, False, tf, dev, interp, dark if with_dark else None, *flags)

    for probe, tf, layout in ((u16, [cast, Normalize()], "nchw"), (raw16, [CvToTorch(), cast, Normalize()], "nhwc_bgr")):
        got = plan(probe, tf, True, True, True)
        assert got is not None and got.route == "ingest_data" and got.source_layout == layout and got.step == 1
        assert got.stages[-1][0] == "affine_data" and got.prefix == ()
        assert plan(probe, tf, True, True, False) is None and plan(probe, tf, True, True) is None      # the default
        assert plan(probe, tf, True, False, True) is None and plan(probe, tf, False, True, True) is None
        assert plan(probe, tf, True, True, True, interp="lookup") is None
        # without a dark field the keyword is not read: pipeline_data_route's plan, as ever
        bare = plan(probe, tf, True, True, True, with_dark=False)
        assert bare is not None and bare == plan(probe, tf, True, True, False, with_dark=False) and bare.route == "ingest_data"
    assert plan(u16, [cast, Normalize(), StridedDownscale(2)], True, True, True) is None
    assert plan(u16, [StridedDownscale(2), cast, Normalize()], True, True, True) is None
    # constant chains keep the plan of the decisions in front, whatever the new keyword says
    black = [cast, Normalize(65535, 64)]
    assert plan(u16, black, True, True, True) == plan(u16, black, True, True, False) and plan(u16, black, True, True, True).route == "ingest"


def test_dark_runs_hand_each_run_its_rows_of_the_constants(monkeypatch):
    """_linearize_dark_runs with the group's constants: matched runs go to linearize_dark_ingest_frames_data, unmatched ones to
    linearize_ingest_frames, each with rows [a:b]; without constants the calls are what they were."""
    from types import SimpleNamespace

    from clair_torch_amd import ops
    from clair_torch_amd.inference import linearization
    group, chw = 6, (3, 4, 6)
    slot = SimpleNamespace(frames=torch.zeros((group, 4, 6, 3), dtype=torch.uint16), std=None, lin_out=torch.zeros((group,) + chw),
                           std_out=torch.zeros((group,) + chw), consts=torch.arange(group * 4, dtype=torch.float32).view(group, 4))
    stages = (("affine_data", 1.0, 0.0),)
    lut = torch.zeros(3, 16)
    pairs = [None if i in (1, 2, 5) else (torch.full(chw, float(i)), torch.full(chw, 10.0 + i)) for i in range(group)]
    calls = []

    def recorder(name):
        def front(frames, *args, **kw):
            calls.append((name, frames.storage_offset() // slot.frames[0].numel(), frames.shape[0], args, kw))
            return kw.get("out")
        return front

    for name in ("linearize_frames", "linearize_ingest_frames", "linearize_dark_frames", "linearize_dark_ingest_frames",
                 "linearize_dark_ingest_frames_data", "flatfield_correct"):
        monkeypatch.setattr(ops, name, recorder(name))
    back = linearization._linearize_dark_runs(slot, group, pairs, False, lut, "catmull", "multiplier", 0.5, None, (stages, "nhwc_bgr"),
                                              consts=slot.consts)
    assert back[0].data_ptr() == slot.lin_out.data_ptr() and back[0].shape[0] == group
    assert [(c[0], c[1], c[2]) for c in calls] == [("linearize_dark_ingest_frames_data", 0, 1), ("linearize_ingest_frames", 1, 2),
                                                   ("linearize_dark_ingest_frames_data", 3, 2), ("linearize_ingest_frames", 5, 1)]
    for name, a, n, args, kw in calls:
        assert torch.equal(kw["consts"], slot.consts[a:a + n]) and kw["consts"].data_ptr() == slot.consts[a:a + n].data_ptr()
        assert kw["layout"] == "nhwc_bgr" and kw["std"] is None and kw["std_mode"] == "multiplier" and kw["std_value"] == 0.5
        assert kw["out"][0].data_ptr() == slot.lin_out[a:a + n].data_ptr() and kw["out"][1].data_ptr() == slot.std_out[a:a + n].data_ptr()
        if name == "linearize_dark_ingest_frames_data":
            assert args[0] == stages and args[3] is lut and args[4] == "catmull"
            assert [float(d[0, 0, 0]) for d in args[1]] == [float(i) for i in range(a, a + n)]
            assert [float(d[0, 0, 0]) for d in args[2]] == [10.0 + i for i in range(a, a + n)]
        else:
            assert args == (stages, lut, "catmull") and kw["want_std"] is True
    # a flat field on this route: ct_flatfield_apply behind the launch of a matched run, as on the constant chains
    calls.clear()
    flat = (torch.ones(chw), None, torch.ones(3))
    monkeypatch.setattr(ops, "linearize_ingest_frames_flat", recorder("linearize_ingest_frames_flat"))
    linearization._linearize_dark_runs(slot, 2, pairs[:2], False, lut, "linear", "multiplier", 0.5, None, (stages, "nhwc_bgr"), flat,
                                       consts=slot.consts[:2])
    assert [c[0] for c in calls] == ["linearize_dark_ingest_frames_data", "flatfield_correct", "linearize_ingest_frames_flat"]
    assert calls[2][4]["flat"] is flat and torch.equal(calls[2][4]["consts"], slot.consts[1:2])
    # without constants: the sibling, as before
    calls.clear()
    linearization._linearize_dark_runs(slot, 2, pairs[:2], False, lut, "linear", "multiplier", 0.5, None,
                                       ((("affine", 0.0, 65535.0, 1.0, 0.0),), "nhwc_bgr"))
    assert [c[0] for c in calls] == ["linearize_dark_ingest_frames", "linearize_ingest_frames"]
    assert "consts" not in calls[0][4] and calls[1][4]["consts"] is None
