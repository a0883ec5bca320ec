"""The fused dark-field blur + linearization without a GPU: ct_linearize_dark is declared, exported and refuses every malformed
call with the status of the pair it replaces (ct_dark_field_blur per frame, then ct_linearize_std) before any launch; the ops
front raises where the fronts of those two raise; DarkField decides the route and keys its device cache; the generator has
the keyword."""
import ctypes
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


def test_ct_linearize_dark_is_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    text = open(os.path.join(ROOT, "include", "clair_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+ct_linearize_dark\s*\(([^)]*)\)", header)
    assert m, "not declared in include/clair_hip.h"
    assert re.search(r"#define\s+CT_LINEARIZE_DARK_MAX_FRAMES\s+16\b", text) and nv.LINEARIZE_DARK_MAX_FRAMES == 16
    assert "ct_linearize_dark" in nv.EXPORTS and hasattr(lib, "ct_linearize_dark")
    assert "ct_linearize_dark.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "clair_torch_amd", "csrc", "ct_linearize_dark.hip"))
    assert len(lib.ct_linearize_dark.argtypes) == len(m.group(1).split(",")) == 16
    assert lib.ct_linearize_dark.restype is ctypes.c_int32


def test_ct_linearize_dark_refuses_before_any_launch(lib):
    """Every call below is malformed and made-up pointers stand for device memory: a status comes back, nothing is read (the
    two pointer arrays are host memory and real)."""
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    fake = ctypes.c_void_p(0x1000)
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    lookup = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LOOKUP)
    missing = object()

    def ptrs(n, value=0x3000):
        return (ctypes.c_void_p * max(n, 1))(*([value] * max(n, 1)))

    def call(frames=fake, dtype=U16, max_code=65535.0, n=2, geom=missing, std=None, std_mode=nv.STD_MULTIPLIER, darks=missing,
             dark_stds=missing, model=linear, lin=fake, std_out=fake):
        geom = _geom() if geom is missing else geom
        gp = None if geom is None else ctypes.byref(geom)
        mp = None if model is None else ctypes.byref(model)
        darks = ptrs(n) if darks is missing else darks
        dark_stds = ptrs(n) if dark_stds is missing else dark_stds
        return lib.ct_linearize_dark(frames, dtype, max_code, n, gp, std, std_mode, 0.05, darks, dark_stds, 0.05, 50.0, mp, lin,
                                     std_out, None)

    # ---- what ct_dark_field_blur refuses, with its status ----
    assert call(frames=None) == INVALID and call(geom=None) == INVALID and call(darks=None) == INVALID and call(dark_stds=None) == INVALID
    assert call(lin=None) == INVALID and call(std_out=None) == INVALID        # uncertainties are always propagated here
    assert call(n=0) == INVALID and call(n=-1) == INVALID
    holed = ptrs(3)
    holed[1] = None
    assert call(n=3, darks=holed) == INVALID and call(n=3, dark_stds=holed) == INVALID   # a NULL entry in either array
    assert call(geom=_geom(c=0)) == INVALID and call(geom=_geom(h=0)) == INVALID
    assert call(geom=_geom(w=1)) == INVALID                                   # the blur reflects: two columns at least
    assert call(geom=_geom(h=1)) == INVALID                                   # ... and two rows
    assert call(geom=_geom(h=4, h_global=3)) == INVALID and call(geom=_geom(h=4, h_global=6, row_offset=3)) == INVALID
    assert call(geom=_geom(layout=nv.LAYOUT_NHWC)) == UNSUPPORTED and call(geom=_geom(layout=nv.LAYOUT_NHWC_BGR)) == UNSUPPORTED
    assert call(std_mode=4) == INVALID and call(std_mode=-1) == INVALID
    assert call(std_mode=nv.STD_EXPLICIT, std=None) == INVALID
    # a row band: no halo is built here
    assert call(geom=_geom(h=4, h_global=12, row_offset=4)) == UNSUPPORTED
    assert call(geom=_geom(h=4, h_global=8)) == UNSUPPORTED and call(geom=_geom(h=4, h_global=8, row_offset=4)) == UNSUPPORTED
    short = _geom()
    short.image_stride = 47
    assert call(geom=short) == INVALID
    assert call(dtype=3) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(max_code=0.0) == UNSUPPORTED and call(dtype=U8, max_code=float("nan")) == UNSUPPORTED
    # ---- what ct_linearize_std refuses for (xb, sigma_eff), with its status ----
    assert call(model=None) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=256, interp=7)) == INVALID
    assert call(model=nv.Icrf(lut_dev=None, n_points=256, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1, interp=nv.INTERP_LINEAR)) == INVALID
    for mode in (nv.STD_NONE, nv.STD_CONSTANT, nv.STD_MULTIPLIER):            # LOOKUP: sigma_eff always has the dark term
        assert call(model=lookup, std_mode=mode) == NO_GRADIENT
    assert call(model=lookup, std_mode=nv.STD_EXPLICIT, std=fake) == NO_GRADIENT
    assert call(geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE               # 2^31 elements per frame
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL)) == TOO_LARGE   # the LDS budget
    assert call(geom=_geom(c=1 << 17, h=2, w=2), model=nv.Icrf(lut_dev=None, n_points=0, interp=nv.INTERP_NONE)) == TOO_LARGE
    # ---- pointers that are not aligned to their element ----
    odd = ctypes.c_void_p(0x1002)
    assert call(frames=ctypes.c_void_p(0x1001)) == INVALID and call(dtype=F32, frames=odd) == INVALID
    assert call(std_mode=nv.STD_EXPLICIT, std=odd) == INVALID
    assert call(lin=odd) == INVALID and call(std_out=odd) == INVALID
    assert call(darks=ptrs(2, 0x3002)) == INVALID and call(dark_stds=ptrs(2, 0x3002)) == INVALID
    # the first refusal wins, in the pair's order: the blur's come before the linearization's
    assert call(geom=_geom(w=1), model=lookup) == INVALID
    assert call(geom=_geom(layout=nv.LAYOUT_NHWC), model=None) == UNSUPPORTED
    assert call(geom=_geom(h=4, h_global=8), model=lookup) == UNSUPPORTED
    assert call(dtype=3, model=lookup) == UNSUPPORTED
    assert call(model=lookup, geom=_geom(h=1 << 15, w=1 << 15)) == NO_GRADIENT


def test_front_end_refuses_where_the_pair_does():
    from clair_torch_amd import ops
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)
    x = torch.zeros((2, 3, 4, 4), dtype=torch.uint8)
    dark = torch.zeros((2, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):      # as dark_field_blur / linearize_frames on CPU frames
        ops.linearize_dark_frames(x, dark, dark, lut, std_mode="multiplier", std_value=0.05)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linearize_frames(x, lut)
    with pytest.raises(TypeError):
        ops.linearize_dark_frames([1, 2], dark, dark, lut)
    assert "linearize_dark_frames" in dir(ops) and ops.MAX_LINEARIZE_DARK_FRAMES == 16


def test_front_end_shape_errors():
    """The shape errors come before anything touches a device: a meta tensor stands for the frames (is_cuda is all the front
    asks of it), so this runs without a GPU."""
    from clair_torch_amd import ops
    x = torch.zeros((2, 3, 4, 4), dtype=torch.uint8)
    dark = torch.zeros((2, 3, 4, 4))
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)

    class _OnDevice(torch.Tensor):
        is_cuda = True

    xd = x.as_subclass(_OnDevice)
    with pytest.raises(ValueError, match="must be \\(N, C, H, W\\)"):                    # _check_stack
        ops.linearize_dark_frames(xd[0], dark, dark, lut)
    with pytest.raises(TypeError, match="unsupported"):
        ops.linearize_dark_frames(xd.double(), dark, dark, lut)
    with pytest.raises(ValueError, match="dark_stds is required"):
        ops.linearize_dark_frames(xd, dark, None, lut)
    with pytest.raises(ValueError, match="3 darks for 2 frames"):
        ops.linearize_dark_frames(xd, [dark[0]] * 3, [dark[0]] * 3, lut)
    with pytest.raises(ValueError, match="with F = 2"):
        ops.linearize_dark_frames(xd, dark[:1], dark[:1], lut)
    with pytest.raises(ValueError, match="unknown std_mode"):
        ops.linearize_dark_frames(xd, dark, dark, lut, std_mode="bogus")


def _plan(probe, transforms, **kw):
    from clair_torch_amd.common.transforms import plan_staging
    return plan_staging(probe, transforms, planar=True, **kw)


def test_dark_field_route_decision():
    from clair_torch_amd.common.transforms import CastTo, Normalize, StridedDownscale
    from clair_torch_amd.inference.dark_field import DarkField
    fuses = DarkField.fuses_with_linearize
    u16, u8, px = torch.zeros((1, 3, 6, 5), dtype=torch.uint16), torch.zeros((1, 3, 6, 5), dtype=torch.uint8), torch.zeros((1, 3, 6, 5))
    pair16, pair8 = [CastTo("float32"), Normalize(65535, 0)], [CastTo("float32"), Normalize(255, 0)]
    for interp in ("linear", "catmull"):
        # the code route (raw codes and their max_code) and bare float32 pixels
        assert _plan(u16, pair16).route == "code" and fuses(u16, _plan(u16, pair16), interp)
        assert fuses(u8, _plan(u8, pair8), interp)
        assert fuses(u16, _plan(u16, [CastTo("float32"), Normalize(4095, 0)]), interp)
        assert _plan(px, []).route == "torch" and fuses(px, _plan(px, []), interp)
        # a black-level chain (route "ingest"), a data-dependent Normalize, a StridedDownscale, 3-D frames
        black = [CastTo("float32"), Normalize(65535, 64)]
        assert _plan(u16, black).route == "ingest" and not fuses(u16, _plan(u16, black), interp)
        data = [CastTo("float32"), Normalize()]
        assert not fuses(u16, _plan(u16, data), interp)
        assert _plan(u16, data, on_device=True).route == "ingest_data" and not fuses(u16, _plan(u16, data, on_device=True), interp)
        for chain in (pair16 + [StridedDownscale(2)], [StridedDownscale(2)] + pair16):
            assert not fuses(u16, _plan(u16, chain), interp) and not fuses(u16, _plan(u16, chain, step_in_kernel=True), interp)
        assert not fuses(px, _plan(px, [StridedDownscale(2)]), interp)
        assert not fuses(u16[0], _plan(u16[0], pair16), interp) and not fuses(px[0], _plan(px[0], []), interp)
        assert not fuses(px, _plan(px, [Normalize(1.0, 0.0)]), interp)       # float32 behind a list: torch ops run
        assert not fuses(u16, _plan(u16, []), interp)                       # bare codes never reach a kernel
        assert not fuses(px.double(), _plan(px.double(), []), interp) and not fuses(object(), _plan(px, []), interp)
    # LOOKUP: no gradient path; the frame-by-frame route raises it at the first matched frame
    assert not fuses(u16, _plan(u16, pair16), "lookup") and not fuses(px, _plan(px, []), "lookup")


def test_generator_has_the_keyword():
    import inspect
    from clair_torch_amd.inference import linearize_dataset_generator
    from clair_torch_amd.inference import linearization
    p = inspect.signature(linearize_dataset_generator).parameters
    assert "fused_dark" in p and isinstance(p["fused_dark"].default, bool)
    assert p["fused_dark"].default is linearization.FUSED_DARK_DEFAULT
    assert inspect.signature(linearization._pipelined).parameters["dark"].default is None


def test_cache_key_follows_in_place_edits():
    """The device cache keys a matched host pair by (address, version, shape, dtype) of both tensors: the same pair again is
    the same key (views of one image included, as ArtefactStack hands them out), an in-place edit of either is a new one."""
    from clair_torch_amd.datasets import ArtefactStack
    from clair_torch_amd.inference.dark_field import DarkField
    art = ArtefactStack(torch.rand((3, 4, 5)), torch.rand((3, 4, 5)))
    _, d1, s1, _ = art.get_matching_artefact_images([0])
    _, d2, s2, _ = art.get_matching_artefact_images([7])
    key = DarkField.cache_key(d1, s1)
    assert DarkField.cache_key(d2, s2) == key
    assert key[0] == (d1.data_ptr(), d1._version, (1, 3, 4, 5), torch.float32)
    art.value.mul_(2.0)
    edited = DarkField.cache_key(*art.get_matching_artefact_images([0])[1:3])
    assert edited != key and edited[1] == key[1]
    art.std[0, 0, 0] = 1.0
    assert DarkField.cache_key(*art.get_matching_artefact_images([0])[1:3])[1] != key[1]
    other = ArtefactStack(torch.rand((3, 4, 5)), art.std)
    assert DarkField.cache_key(*other.get_matching_artefact_images([0])[1:3])[0] != edited[0]
    assert DarkField.cache_key(d1.double(), s1)[0][3] == torch.float64
    assert DarkField.CACHE_PAIRS == 4
