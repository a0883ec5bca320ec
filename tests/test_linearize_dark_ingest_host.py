"""The fused chain + dark-field blur + linearization without a GPU: ct_linearize_dark_ingest is declared, exported and refuses
every malformed call before any launch, in the documented order; the ops front raises where the fronts of
linearize_dark_frames and linearize_ingest_frames raise; DarkField decides the route; the generator has the keyword."""
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


def test_ct_linearize_dark_ingest_is_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    text = open(os.path.join(ROOT, "include", "clair_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+ct_linearize_dark_ingest\s*\(([^)]*)\)", header)
    assert m, "not declared in include/clair_hip.h"
    assert "ct_linearize_dark_ingest" in nv.EXPORTS and hasattr(lib, "ct_linearize_dark_ingest")
    assert "ct_linearize_dark_ingest.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "clair_torch_amd", "csrc", "ct_linearize_dark_ingest.hip"))
    assert len(lib.ct_linearize_dark_ingest.argtypes) == len(m.group(1).split(",")) == 17
    assert lib.ct_linearize_dark_ingest.restype is ctypes.c_int32
    # the argument order of ct_linearize_dark with (stages, n_stages) in place of max_code
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["frames_dev", "dtype", "n_frames", "geom", "stages", "n_stages", "std_dev", "std_mode", "std_value", "dark_devs",
                     "dark_std_devs", "threshold", "alpha", "icrf", "lin_out_dev", "std_out_dev", "stream"]


def test_ct_linearize_dark_ingest_refuses_before_any_launch(lib):
    """Every call below is malformed and made-up pointers stand for device memory: a status comes back, nothing is read (the
    pointer arrays and the stage list are host memory and real)."""
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    NHWC, BGR = nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    fake = ctypes.c_void_p(0x1000)
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

    one = chain(nv.INGEST_AFFINE)

    def call(frames=fake, dtype=U16, n=2, geom=missing, stages=one, std=None, std_mode=nv.STD_MULTIPLIER, darks=missing,
             dark_stds=missing, model=linear, lin=fake, std_out=fake):
        geom = _geom() if geom is missing else geom
        gp = None if geom is None else ctypes.byref(geom)
        mp = None if model is None else ctypes.byref(model)
        darks = ptrs(n) if darks is missing else darks
        dark_stds = ptrs(n) if dark_stds is missing else dark_stds
        return lib.ct_linearize_dark_ingest(frames, dtype, n, gp, stages[0], stages[1], std, std_mode, 0.05, darks, dark_stds, 0.05,
                                            50.0, mp, lin, std_out, None)

    # ---- 1. what ct_linearize_dark refuses first ----
    assert call(frames=None) == INVALID and call(geom=None) == INVALID and call(darks=None) == INVALID and call(dark_stds=None) == INVALID
    assert call(lin=None) == INVALID and call(std_out=None) == INVALID        # uncertainties are always propagated here
    assert call(n=0) == INVALID and call(n=-1) == INVALID
    holed = ptrs(3)
    holed[1] = None
    assert call(n=3, darks=holed) == INVALID and call(n=3, dark_stds=holed) == INVALID
    # ---- 2. the dark geometry ----
    assert call(geom=_geom(c=0)) == INVALID and call(geom=_geom(h=0)) == INVALID
    assert call(geom=_geom(w=1)) == INVALID and call(geom=_geom(h=1)) == INVALID     # the blur reflects: two columns and rows
    assert call(geom=_geom(w=1, layout=BGR)) == INVALID
    assert call(geom=_geom(h=4, h_global=3)) == INVALID and call(geom=_geom(h=4, h_global=6, row_offset=3)) == INVALID
    assert call(std_mode=4) == INVALID and call(std_mode=-1) == INVALID
    assert call(std_mode=nv.STD_EXPLICIT, std=None) == INVALID
    assert call(geom=_geom(h=4, h_global=12, row_offset=4)) == UNSUPPORTED          # a row band: no halo is built here
    assert call(geom=_geom(h=4, h_global=8)) == UNSUPPORTED and call(geom=_geom(h=4, h_global=8, row_offset=4, layout=BGR)) == UNSUPPORTED
    short = _geom()
    short.image_stride = 47
    assert call(geom=short) == INVALID
    # ---- 3. the stack and the stage list ----
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(geom=_geom(layout=3)) == INVALID and call(geom=_geom(layout=-1)) == INVALID
    assert call(stages=chain(nv.INGEST_AFFINE_DATA)) == INVALID                      # no data-dependent Normalize here
    assert call(stages=chain(nv.INGEST_AFFINE, nv.INGEST_AFFINE_DATA)) == INVALID
    assert call(stages=chain(7)) == INVALID
    assert call(stages=(one[0], 5)) == INVALID and call(stages=(one[0], -1)) == INVALID and call(stages=(None, 1)) == INVALID
    assert call(geom=_geom(c=4, layout=NHWC)) == UNSUPPORTED and call(geom=_geom(c=1, layout=BGR)) == UNSUPPORTED
    differ = chain(nv.INGEST_CLAMP, pairs=[(0.0, 1.0), (0.1, 0.9), (0.0, 1.0), (0.0, 1.0)])
    assert call(geom=_geom(c=5), stages=differ) == UNSUPPORTED
    # ---- 4. the model, LOOKUP, the LDS budget, 2^31, alignment ----
    assert call(model=None) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=256, interp=7)) == INVALID
    assert call(model=nv.Icrf(lut_dev=None, n_points=256, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1, interp=nv.INTERP_LINEAR)) == INVALID
    for mode in (nv.STD_NONE, nv.STD_CONSTANT, nv.STD_MULTIPLIER):                   # sigma_eff always has the dark term
        assert call(model=lookup, std_mode=mode) == NO_GRADIENT
    assert call(model=lookup, std_mode=nv.STD_EXPLICIT, std=fake, geom=_geom(layout=BGR)) == NO_GRADIENT
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)) == TOO_LARGE
    assert call(geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE                       # 2^31 elements per frame
    assert call(geom=_geom(c=1 << 17, h=2, w=2), model=nv.Icrf(lut_dev=None, n_points=0, interp=nv.INTERP_NONE)) == TOO_LARGE
    odd = ctypes.c_void_p(0x1002)
    assert call(frames=ctypes.c_void_p(0x1001)) == INVALID and call(dtype=F32, frames=odd) == INVALID
    assert call(dtype=U8, frames=ctypes.c_void_p(0x1001), darks=ptrs(2, 0x3002)) == INVALID
    assert call(std_mode=nv.STD_EXPLICIT, std=odd) == INVALID
    assert call(lin=odd) == INVALID and call(std_out=odd) == INVALID
    assert call(darks=ptrs(2, 0x3002)) == INVALID and call(dark_stds=ptrs(2, 0x3002)) == INVALID
    # ---- the first refusal wins ----
    assert call(geom=_geom(w=1), model=lookup) == INVALID                            # 2 before 4
    assert call(geom=_geom(h=4, h_global=8), stages=chain(nv.INGEST_AFFINE_DATA)) == UNSUPPORTED    # 2 before 3
    assert call(n=0, geom=_geom(h=4, h_global=8)) == INVALID                         # 1 before 2
    assert call(geom=_geom(c=1, layout=BGR), model=lookup) == UNSUPPORTED            # 3 before 4
    assert call(stages=chain(nv.INGEST_AFFINE_DATA), model=lookup) == INVALID
    assert call(model=lookup, geom=_geom(h=1 << 15, w=1 << 15)) == NO_GRADIENT       # LOOKUP before the 2^31 limit
    big_lut = nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)
    assert call(model=big_lut, geom=_geom(h=1 << 15, w=1 << 15), lin=odd) == TOO_LARGE


def test_front_end_refuses_cpu_tensors_and_malformed_stage_lists():
    from clair_torch_amd import ops
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)
    x = torch.zeros((2, 3, 4, 4), dtype=torch.uint8)
    dark = torch.zeros((2, 3, 4, 4))
    pair = [("affine", 0, 255, 1, 0)]
    with pytest.raises(RuntimeError, match="no CPU path"):      # as linearize_dark_frames / linearize_ingest_frames on CPU frames
        ops.linearize_dark_ingest_frames(x, pair, dark, dark, lut, std_mode="multiplier", std_value=0.05)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linearize_dark_ingest_frames(x.permute(0, 2, 3, 1).contiguous(), pair, dark, dark, lut, layout="nhwc_bgr")
    with pytest.raises(TypeError):
        ops.linearize_dark_ingest_frames([1, 2], pair, dark, dark, lut)

    class _OnDevice(torch.Tensor):      # is_cuda is all the front asks of the frames before the shape errors
        is_cuda = True

    xd = x.as_subclass(_OnDevice)
    call = ops.linearize_dark_ingest_frames
    with pytest.raises(ValueError, match="4-dimensional"):
        call(xd[0], pair, dark, dark, lut)
    with pytest.raises(TypeError, match="unsupported"):
        call(xd.double(), pair, dark, dark, lut)
    with pytest.raises(ValueError, match="unknown layout"):
        call(xd, pair, dark, dark, lut, layout="chwn")
    with pytest.raises(ValueError, match="takes \\(B, H, W, 3\\) frames"):
        call(xd, pair, dark, dark, lut, layout="nhwc_bgr")
    with pytest.raises(ValueError, match="at most 4 stages"):
        call(xd, pair * 5, dark, dark, lut)
    with pytest.raises(ValueError, match="stage 0: expected"):
        call(xd, [("affine_data", 1, 0)], dark, dark, lut)
    with pytest.raises(ValueError, match="stage 1: expected"):
        call(xd, pair + [("gamma", 2.2)], dark, dark, lut)
    with pytest.raises(ValueError, match="takes four constants"):
        call(xd, [("affine", 0, 255)], dark, dark, lut)
    with pytest.raises(ValueError, match="Normalization range is zero"):
        call(xd, [("affine", 0, 0, 1, 0)], dark, dark, lut)
    with pytest.raises(ValueError, match="min/max pairs"):
        call(xd, pair + [("clamp", [(0, 1), (0, 1)])], dark, dark, lut)
    with pytest.raises(TypeError, match="must be an int or a float"):
        call(xd, [("affine", 0, "255", 1, 0)], dark, dark, lut)
    with pytest.raises(ValueError, match="unknown std_mode"):
        call(xd, pair, dark, dark, lut, std_mode="bogus")
    with pytest.raises(ValueError, match="dark_stds is required"):
        call(xd, pair, dark, None, lut)
    with pytest.raises(ValueError, match="3 darks for 2 frames"):
        call(xd, pair, [dark[0]] * 3, [dark[0]] * 3, lut)
    p = inspect.signature(call).parameters
    assert list(p)[:6] == ["frames", "stages", "darks", "dark_stds", "lut", "interp"] and p["interp"].default == "linear"
    for name, default in (("std", None), ("std_mode", "none"), ("std_value", 0.0), ("layout", "nchw"), ("out", None),
                          ("threshold", 0.05), ("alpha", 50.0)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name


def _plan(probe, transforms, **kw):
    from clair_torch_amd.common.transforms import plan_staging
    return plan_staging(probe, transforms, planar=True, **kw)


def test_dark_field_ingest_route_decision():
    from clair_torch_amd.common.transforms import CastTo, ClampAlongDims, CvToTorch, Normalize, StridedDownscale
    from clair_torch_amd.inference.dark_field import DarkField
    fuses, first = DarkField.fuses_with_linearize_ingest, DarkField.fuses_with_linearize
    u16, u8, px = torch.zeros((1, 3, 6, 5), dtype=torch.uint16), torch.zeros((1, 3, 6, 5), dtype=torch.uint8), torch.zeros((1, 3, 6, 5))
    raw16, raw8 = torch.zeros((1, 6, 5, 3), dtype=torch.uint16), torch.zeros((1, 6, 5, 3), dtype=torch.uint8)
    cast, cv = CastTo("float32"), CvToTorch()
    black = [cast, Normalize(65535, 64)]
    for interp in ("linear", "catmull"):
        # accepted: route "ingest" without a StridedDownscale, every dtype, planar and raw BGR frames
        for probe, chain, layout in ((u16, black, "nchw"), (u8, [cast, Normalize(255, 16)], "nchw"),
                                     (u16, [cast, Normalize(65535, 0, target_range=(0.1, 0.9))], "nchw"),
                                     (u16, [cast, Normalize(65535, 0), ClampAlongDims(1, [(0.0, 1.0), (0.01, 0.95), (0.0, 0.9)])], "nchw"),
                                     (px, [Normalize(1.0, 0.25)], "nchw"), (px, [ClampAlongDims(1, (0.0, 1.0))], "nchw"),
                                     (raw16, [cv, cast, Normalize(65535, 0)], "nhwc_bgr"), (raw8, [cv, cast, Normalize(255, 0)], "nhwc_bgr"),
                                     (raw16, [cv] + black, "nhwc_bgr")):
            plan = _plan(probe, chain)
            assert plan.route == "ingest" and plan.step == 1 and plan.source_layout == layout, (chain, plan)
            assert fuses(probe, plan, interp), chain
            assert not first(probe, plan, interp), chain         # fuses_with_linearize still declines route "ingest"
        # declined: what the first decision takes, a data-dependent Normalize, a StridedDownscale, torch lists, 3-D frames
        pair16 = [cast, Normalize(65535, 0)]
        assert _plan(u16, pair16).route == "code" and not fuses(u16, _plan(u16, pair16), interp) and first(u16, _plan(u16, pair16), interp)
        assert not fuses(px, _plan(px, []), interp) and first(px, _plan(px, []), interp)
        data = [cast, Normalize()]
        assert not fuses(u16, _plan(u16, data), interp)
        assert _plan(u16, data, on_device=True).route == "ingest_data" and not fuses(u16, _plan(u16, data, on_device=True), interp)
        assert not fuses(raw16, _plan(raw16, [cv] + data, on_device=True), interp)
        for chain in (black + [StridedDownscale(2)], [StridedDownscale(2)] + black, [cv, StridedDownscale(2)] + black):
            probe = raw16 if chain[0] is cv else u16
            assert _plan(probe, chain).step == 2
            assert not fuses(probe, _plan(probe, chain), interp) and not fuses(probe, _plan(probe, chain, step_in_kernel=True), interp)
        assert not fuses(u16, _plan(u16, [cast, Normalize(65535, 64), cast, Normalize(1, 0), Normalize(1, 0), Normalize(1, 0),
                                          Normalize(1, 0)]), interp)     # five stages: torch ops run
        assert not fuses(u16[0], _plan(u16[0], black), interp) and not fuses(object(), _plan(u16, black), interp)
        assert not fuses(u16, _plan(u16, []), interp)
    # LOOKUP: no gradient path; the frame-by-frame route raises it at the first matched frame
    assert not fuses(u16, _plan(u16, black), "lookup") and not fuses(raw16, _plan(raw16, [cv] + black), "lookup")
    # the other layouts and dtypes of a hand-made plan
    plan = _plan(u16, black)
    from dataclasses import replace
    assert fuses(u16, replace(plan, source_layout="nhwc_bgr"), "linear") and not fuses(u16, replace(plan, source_layout="nhwc"), "linear")
    assert not fuses(u16.to(torch.float64), plan, "linear") and not fuses(u16, replace(plan, step=2), "linear")


def test_generator_has_the_keyword():
    from clair_torch_amd.inference import linearize_dataset_generator
    from clair_torch_amd.inference import linearization
    p = inspect.signature(linearize_dataset_generator).parameters
    assert "fused_dark_ingest" in p and isinstance(p["fused_dark_ingest"].default, bool)
    assert p["fused_dark_ingest"].default is linearization.FUSED_DARK_INGEST_DEFAULT
    assert p["fused_dark"].default is linearization.FUSED_DARK_DEFAULT
    assert inspect.signature(linearization._linearize_dark_runs).parameters["chain"].default is None
