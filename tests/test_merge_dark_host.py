"""The fused dark-field blur + merge without a GPU: ct_hdr_merge_dark_batch is declared, exported and refuses every malformed
call with the status of the pair it replaces (ct_dark_field_blur, then ct_hdr_merge_batch) before any launch; the ops front
raises where the fronts of those two raise; DarkField decides the route."""
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


def test_ct_hdr_merge_dark_batch_is_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ct_hdr_merge_dark_batch\s*\(([^)]*)\)", header)
    assert m, "not declared in include/clair_hip.h"
    assert "ct_hdr_merge_dark_batch" in nv.EXPORTS and hasattr(lib, "ct_hdr_merge_dark_batch")
    assert "ct_merge_dark.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "clair_torch_amd", "csrc", "ct_merge_dark.hip"))
    assert len(lib.ct_hdr_merge_dark_batch.argtypes) == len(m.group(1).split(",")) == 24
    assert lib.ct_hdr_merge_dark_batch.restype is ctypes.c_int32


def test_ct_hdr_merge_dark_batch_refuses_before_any_launch(lib):
    """Every call below is malformed and made-up pointers stand for device memory: a status comes back, nothing is read."""
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    FIRST, FINAL, CLOSED = nv.MERGE_FIRST_BATCH, nv.MERGE_FINALIZE, nv.MERGE_CLOSED_FORM
    fake = ctypes.c_void_p(0x1000)
    linear = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LINEAR)
    lookup = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_LOOKUP)
    catmull = nv.Icrf(lut_dev=0x2000, n_points=256, interp=nv.INTERP_CATMULL)
    missing = object()

    def call(stack=fake, dtype=U16, max_code=65535.0, batch=2, geom=missing, halo=None, std=None, std_mode=nv.STD_MULTIPLIER,
             dark=fake, dark_std=fake, dark_batch=2, expo=fake, model=linear, weight=nv.WEIGHT_GAUSS, state=(None, None, None),
             mean_out=fake, std_out=fake, flags=FIRST | FINAL):
        geom = _geom() if geom is missing else geom
        gp = None if geom is None else ctypes.byref(geom)
        mp = None if model is None else ctypes.byref(model)
        return lib.ct_hdr_merge_dark_batch(stack, dtype, max_code, batch, gp, halo, std, std_mode, 0.05, dark, dark_std, dark_batch,
                                           0.05, 50.0, expo, mp, weight, state[0], state[1], state[2], mean_out, std_out, flags, None)

    # ---- what ct_dark_field_blur refuses, with its status ----
    assert call(stack=None) == INVALID and call(geom=None) == INVALID and call(dark=None) == INVALID
    assert call(batch=0) == INVALID and call(batch=-1) == INVALID
    assert call(geom=_geom(c=0)) == INVALID and call(geom=_geom(h=0)) == INVALID
    assert call(geom=_geom(w=1)) == INVALID                                   # the blur reflects: two columns at least
    assert call(geom=_geom(h=1)) == INVALID                                   # ... and two global rows
    assert call(geom=_geom(h=4, h_global=3)) == INVALID and call(geom=_geom(h=4, h_global=6, row_offset=3)) == INVALID
    assert call(geom=_geom(layout=nv.LAYOUT_NHWC)) == UNSUPPORTED and call(geom=_geom(layout=nv.LAYOUT_NHWC_BGR)) == UNSUPPORTED
    assert call(dark_batch=3) == INVALID and call(dark_batch=0) == INVALID    # neither shared nor one per frame
    assert call(dark_batch=1) == UNSUPPORTED                                  # shared dark + its std + B > 1: another quantity
    assert call(std_mode=4) == INVALID and call(std_mode=-1) == INVALID
    assert call(std_mode=nv.STD_EXPLICIT, std=None) == INVALID
    band = _geom(h=4, h_global=12, row_offset=4)
    assert call(geom=band) == INVALID                                         # a band without its halo
    assert call(geom=_geom(h=4, h_global=8)) == INVALID and call(geom=_geom(h=4, h_global=8, row_offset=4)) == INVALID
    assert call(geom=_geom(h=1, h_global=8), halo=fake) == UNSUPPORTED        # a one-row band that would reflect onto the halo
    short = _geom()
    short.image_stride = 47
    assert call(geom=short) == INVALID
    assert call(dtype=3) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(max_code=0.0) == UNSUPPORTED and call(dtype=U8, max_code=float("nan")) == UNSUPPORTED
    # ---- what ct_hdr_merge_batch refuses for (xb, sigma_eff), with its status ----
    assert call(expo=None) == INVALID and call(model=None) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=256, interp=7)) == INVALID
    assert call(model=nv.Icrf(lut_dev=None, n_points=256, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1, interp=nv.INTERP_LINEAR)) == INVALID
    assert call(weight=2) == INVALID
    for flags in (FIRST | FINAL, FIRST | FINAL | CLOSED):                     # LOOKUP, unit weights, uncertainties
        assert call(model=lookup, weight=nv.WEIGHT_NONE, flags=flags) == NO_GRADIENT
    assert call(flags=FIRST) == INVALID and call(flags=FINAL) == INVALID and call(flags=0) == INVALID   # no state: one batch only
    assert call(flags=0, state=(fake, fake, None)) == INVALID                 # a dark std needs the variance state
    assert call(flags=FIRST, state=(fake, None, fake)) == INVALID
    assert call(mean_out=None) == INVALID and call(std_out=None) == INVALID
    assert call(geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE
    # ---- the routes this entry point does not have ----
    for flag in (nv.MERGE_F64_MOMENTS, nv.MERGE_REFERENCE_ORDER, nv.MERGE_OUT_AS_INPUT):
        assert call(flags=FIRST | FINAL | flag) == UNSUPPORTED, flag
    assert call(model=lookup) == UNSUPPORTED and call(model=catmull) == UNSUPPORTED   # reference order unless CLOSED_FORM
    assert call(model=nv.Icrf(lut_dev=0x2000, n_points=1 << 20, interp=nv.INTERP_CATMULL), flags=FIRST | FINAL | CLOSED) == TOO_LARGE
    assert call(batch=1 << 16, dark_batch=1 << 16) == TOO_LARGE               # 8 B per exposure exceed the LDS
    # ---- pointers that are not aligned to their element ----
    odd = ctypes.c_void_p(0x1002)
    assert call(stack=ctypes.c_void_p(0x1001)) == INVALID and call(dtype=F32, stack=odd) == INVALID
    assert call(dark=odd) == INVALID and call(dark_std=odd) == INVALID and call(expo=ctypes.c_void_p(0x1004)) == INVALID
    assert call(std_out=odd) == INVALID and call(mean_out=ctypes.c_void_p(0x1004)) == INVALID
    # the first refusal wins, in the pair's order: the blur's come before the merge's
    assert call(geom=_geom(w=1), model=lookup, weight=nv.WEIGHT_NONE) == INVALID
    assert call(dark_batch=1, model=lookup, weight=nv.WEIGHT_NONE) == UNSUPPORTED
    assert call(geom=_geom(layout=nv.LAYOUT_NHWC), expo=None) == UNSUPPORTED


def test_front_end_refuses_where_the_pair_does():
    from clair_torch_amd import ops
    lut = torch.stack([torch.linspace(0, 1, 16)] * 3)
    x = torch.zeros((2, 3, 4, 4), dtype=torch.uint8)
    dark = torch.zeros((2, 3, 4, 4))
    t = torch.tensor([1.0, 2.0])
    with pytest.raises(RuntimeError, match="no CPU path"):      # as dark_field_blur / hdr_merge_batch on a CPU stack
        ops.hdr_merge_dark_batch(x, t, dark, dark, lut=lut, std_mode="multiplier", std_value=0.05)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dark_field_blur(x, dark, dark)
    with pytest.raises(TypeError):
        ops.hdr_merge_dark_batch([1, 2], t, dark, dark)
    assert "hdr_merge_dark_batch" in dir(ops)


def test_dark_field_route_decision():
    from clair_torch_amd.inference.dark_field import DarkField
    codes, px = torch.zeros((2, 3, 4, 4), dtype=torch.uint16), torch.zeros((2, 3, 4, 4))
    fuses = DarkField.fuses_with_merge
    for images in (codes, px, codes.to(torch.uint8)):
        assert fuses(images, "nchw", "linear", None) and fuses(images, "nchw", None, None)
        assert fuses(images, "nchw", "linear", False) and fuses(images, "nchw", "catmull", False) and fuses(images, "nchw", "lookup", False)
        # the reference-order kernel is not fused: asked for, or the default of LOOKUP / CATMULL with uncertainties
        assert not fuses(images, "nchw", "linear", True) and not fuses(images, "nchw", None, True)
        assert not fuses(images, "nchw", "catmull", None) and not fuses(images, "nchw", "lookup", None)
    assert not fuses(torch.zeros((2, 4, 4, 3), dtype=torch.uint8), "nhwc_bgr", "linear", None)   # OpenCV-order frames
    assert not fuses(px.double(), "nchw", "linear", None) and not fuses(object(), "nchw", "linear", None)


def test_compute_hdr_image_has_the_keyword():
    import inspect
    from clair_torch_amd.inference import compute_hdr_image
    p = inspect.signature(compute_hdr_image).parameters
    assert "fused_dark" in p and isinstance(p["fused_dark"].default, bool)
