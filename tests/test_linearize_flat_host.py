"""The flat-field correction inside the linearization launches, without a GPU: ct_linearize_std_flat, ct_linearize_ingest_flat
and ct_linearize_ingest_strided_flat are declared, bound and refuse every malformed call before any launch -- the parent's
refusals in the parent's order, then the flat field's own --, the ops fronts check ``flat=`` without a device, and
``linearize_dataset_generator`` checks ``fused_flat``."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ct_linearize_std_flat": 15, "ct_linearize_ingest_flat": 17, "ct_linearize_ingest_strided_flat": 18}


@pytest.fixture(scope="module")
def lib():
    from clair_torch_amd import build, _native
    build.build()
    return _native.load()


def test_symbols_are_declared_and_bound(lib):
    from clair_torch_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "clair_hip.h")).read()
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    for name, n_args in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in nv.EXPORTS and hasattr(lib, name), name
        entry = getattr(lib, name)
        # the parent's arguments, then flat, flat std and flat mean in front of the stream
        parent = getattr(lib, name[:-len("_flat")] if name != "ct_linearize_ingest_flat" else "ct_linearize_ingest_data")
        assert len(entry.argtypes) == n_args == len(parent.argtypes) + 3, name
        assert list(entry.argtypes[:len(parent.argtypes) - 1]) == list(parent.argtypes[:-1]), name


def _front(ops, name, kw):
    """ops.<name>, or ops.<name>_flat for a call with ``flat``."""
    return getattr(ops, name + "_flat" if "flat" in kw else name)


def _geom(nv, **kw):
    a = dict(channels=3, h_tile=7, width=13, h_global=7, row_offset=0, image_stride=3 * 7 * 13, layout=nv.LAYOUT_NCHW)
    a.update(kw)
    return nv.Geometry(**a)


FAKE, ODD = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002)


def _flat_refusals(call, INVALID):
    """Behind every refusal of the parent: flat or its mean NULL, any of the three misaligned, no std output."""
    assert call(flat=None) == INVALID and call(mean=None) == INVALID
    assert call(flat=ODD) == INVALID and call(flat_std=ODD) == INVALID and call(mean=ODD) == INVALID
    assert call(std_out=None) == INVALID
    assert call(std_out=None, flat_std=None) == INVALID


def test_std_flat_refuses_before_any_launch(lib):
    """Never-dereferenced pointers: every call returns from validation, ct_linearize_std's refusals first."""
    from clair_torch_amd import _native as nv
    INVALID, UNSUPPORTED, NO_GRAD = nv.ERR_INVALID_ARGUMENT, nv.ERR_UNSUPPORTED, nv.ERR_NO_GRADIENT_PATH

    def call(g=None, std=None, std_mode=nv.STD_NONE, interp=nv.INTERP_LINEAR, lut=FAKE, n_points=16, frames=FAKE, lin=FAKE,
             std_out=FAKE, dtype=nv.DTYPE_U16, n=2, max_code=65535.0, flat=FAKE, flat_std=FAKE, mean=FAKE):
        g = g or _geom(nv)
        icrf = nv.Icrf(lut_dev=lut, n_points=n_points, interp=interp)
        return lib.ct_linearize_std_flat(frames, dtype, max_code, n, ctypes.byref(g), std, std_mode, 0.05, ctypes.byref(icrf), lin,
                                         std_out, flat, flat_std, mean, None)

    # the parent's, whatever the flat field is
    for ff in (dict(), dict(flat=None, mean=None, std_out=None)):
        assert call(frames=None, **ff) == INVALID and call(n=0, **ff) == INVALID and call(n=-1, **ff) == INVALID
        assert call(g=_geom(nv, h_tile=0, h_global=0), **ff) != 0
        assert call(std_mode=nv.STD_EXPLICIT, std=None, **ff) == INVALID
        assert call(std_mode=99, **ff) == INVALID
        assert call(interp=nv.INTERP_LOOKUP, std_mode=nv.STD_CONSTANT, **ff) == NO_GRAD
        assert call(dtype=7, **ff) == UNSUPPORTED
    assert call(lin=None) == INVALID
    _flat_refusals(call, INVALID)
    assert call(dtype=nv.DTYPE_F32, flat=None) == INVALID and call(dtype=nv.DTYPE_U8, max_code=255.0, mean=None) == INVALID


def _ingest_call(lib, nv, strided):
    affine = (nv.IngestStage * 1)()
    affine[0].kind, affine[0].sub, affine[0].div, affine[0].mul, affine[0].add = nv.INGEST_AFFINE, 64.0, 4031.0, 1.0, 0.0

    def call(g=None, step=2, stages=affine, n_stages=1, std=None, std_mode=nv.STD_NONE, interp=nv.INTERP_LINEAR, lut=FAKE,
             n_points=16, frames=FAKE, lin=FAKE, std_out=FAKE, consts=None, dtype=nv.DTYPE_U16, n=2, flat=FAKE, flat_std=FAKE,
             mean=FAKE):
        g = g or _geom(nv)
        icrf = nv.Icrf(lut_dev=lut, n_points=n_points, interp=interp)
        head = (frames, dtype, n, ctypes.byref(g)) + ((step,) if strided else ())
        entry = lib.ct_linearize_ingest_strided_flat if strided else lib.ct_linearize_ingest_flat
        return entry(*head, stages, n_stages, std, std_mode, 0.05, ctypes.byref(icrf), lin, std_out, consts, flat, flat_std, mean,
                     None)

    return call


@pytest.mark.parametrize("strided", [False, True])
def test_ingest_flat_refuses_before_any_launch(lib, strided):
    """ct_linearize_ingest's order (test_linearize_strided_host.py: the step and the row band in front for the strided entry),
    pointers last, and the flat field's refusals behind the pointers'."""
    from clair_torch_amd import _native as nv
    INVALID, UNSUPPORTED, NO_GRAD, TOO_LARGE = (nv.ERR_INVALID_ARGUMENT, nv.ERR_UNSUPPORTED, nv.ERR_NO_GRADIENT_PATH,
                                                nv.ERR_TOO_LARGE)
    call = _ingest_call(lib, nv, strided)
    data = (nv.IngestStage * 1)()
    data[0].kind, data[0].mul, data[0].add = nv.INGEST_AFFINE_DATA, 1.0, 0.0
    for ff in (dict(), dict(flat=None, mean=None, std_out=None)):  # the parent's, whatever the flat field is
        if strided:
            assert call(step=0, **ff) == INVALID
            assert call(g=_geom(nv, h_tile=4, h_global=7, row_offset=3, image_stride=3 * 4 * 13), **ff) == INVALID
        assert call(interp=nv.INTERP_LOOKUP, std_mode=nv.STD_CONSTANT, **ff) == NO_GRAD
        assert call(interp=nv.INTERP_LOOKUP, std_mode=nv.STD_CONSTANT, frames=None, **ff) == NO_GRAD
        assert call(std_mode=nv.STD_EXPLICIT, std=None, **ff) == INVALID
        assert call(stages=data, **ff) == INVALID                       # AFFINE_DATA without constants
        assert call(stages=data, consts=ODD, **ff) == INVALID
        assert call(n_stages=5, **ff) == INVALID and call(dtype=7, **ff) == INVALID and call(n=-1, **ff) == INVALID
        assert call(g=_geom(nv, layout=nv.LAYOUT_NHWC, channels=4, image_stride=4 * 7 * 13), **ff) == UNSUPPORTED
        assert call(g=_geom(nv, image_stride=10), **ff) == INVALID
        assert call(n_points=20000, interp=nv.INTERP_CATMULL, **ff) == TOO_LARGE
        assert call(n=0, frames=None, lin=None, **ff) == 0              # nothing to do
        assert call(frames=None, **ff) == INVALID
    assert call(lin=None) == INVALID and call(frames=ctypes.c_void_p(0x1001)) == INVALID and call(std_out=ODD) == INVALID
    _flat_refusals(call, INVALID)
    assert call(stages=data, consts=FAKE, flat=None) == INVALID          # the data-dependent form likewise
    if strided:
        assert call(step=1, mean=None) == INVALID


def test_ops_front_checks_without_a_device(monkeypatch):
    """The checks of ``flat=`` that need no device: CPU tensors stand in for device tensors (the device check is taken out) and
    the library is never reached."""
    from clair_torch_amd import ops
    monkeypatch.setattr(ops, "_require_device", lambda t, name: None)
    monkeypatch.setattr(ops.nv, "load", lambda: pytest.fail("the library was reached"))
    frames = torch.zeros((2, 3, 7, 13), dtype=torch.uint16)
    lut = torch.linspace(0, 1, 16).repeat(3, 1)
    stages = [("affine", 64.0, 4031.0, 1.0, 0.0)]
    fronts = {
        "std": (lambda **kw: _front(ops, "linearize_frames", kw)(frames, lut, "linear", **kw), (3, 7, 13)),
        "ingest": (lambda **kw: _front(ops, "linearize_ingest_frames", kw)(frames, stages, lut, "linear", **kw), (3, 7, 13)),
        "strided": (lambda **kw: _front(ops, "linearize_ingest_frames_strided", kw)(frames, 2, stages, lut, "linear", **kw), (3, 4, 7)),
    }
    for what, (front, chw) in fronts.items():
        flat, mean = torch.ones(chw), torch.ones(3)
        for bad in (flat, (flat, None), (flat, None, mean, None), "flat"):
            with pytest.raises(ValueError, match="flat must be"):
                front(flat=bad)
        with pytest.raises(ValueError, match="want_std"):
            front(flat=(flat, None, mean), want_std=False)
        other = torch.ones((3, 7, 12))
        for bad, name in (((other, None, mean), r"flat\[0\]"), ((flat, other, mean), r"flat\[1\]"),
                          ((flat.double(), None, mean), r"flat\[0\]"), ((None, None, mean), r"flat\[0\]"),
                          ((flat, None, torch.ones(2)), r"flat\[2\]"), ((flat, flat, mean.double()), r"flat\[2\]")):
            with pytest.raises((ValueError, TypeError), match=name):
                front(flat=bad)
    # behind a downscale the flat field has the downscaled shape, not the frames'
    with pytest.raises(ValueError, match=r"flat\[0\]"):
        fronts["strided"][0](flat=(torch.ones((3, 7, 13)), None, torch.ones(3)))
    # nothing to do: checked all the same, never launched
    empty = ops.linearize_ingest_frames_flat(frames[:0], stages, lut, flat=(torch.ones((3, 7, 13)), None, torch.ones(3)))
    assert empty[0].shape == (0, 3, 7, 13)
    # a mean computed before is a constant of the run
    value = torch.zeros((2, 3, 7, 13))
    with pytest.raises(ValueError, match="through_mean"):
        ops.flatfield_correct(value[0], None, torch.ones((3, 7, 13)), None, input_is_variance=False, through_mean=True,
                              flat_mean=torch.ones(3))
    with pytest.raises(ValueError, match="flat_mean"):
        ops.flatfield_correct(value, value.clone(), torch.ones((3, 7, 13)), None, input_is_variance=False, through_mean=False,
                              flat_mean=torch.ones(4))


def test_custom_ops_are_registered():
    import clair_torch_amd.torch_ops  # noqa: F401
    for name in ("flatfield_mean", "linearize_std_flat", "linearize_ingest_flat", "linearize_ingest_strided_flat"):
        assert hasattr(torch.ops.clair_hip, name), name


def test_fused_flat_argument():
    from clair_torch_amd.inference import linearization as L
    sig = inspect.signature(L.linearize_dataset_generator)
    assert sig.parameters["fused_flat"].default is L.FUSED_FLAT_DEFAULT and isinstance(L.FUSED_FLAT_DEFAULT, bool)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="fused_flat"):
            next(L.linearize_dataset_generator(None, "cpu", None, fused_flat=bad))
    # ... and it is read in front of everything else only for its type: a bool leaves the usual checks their turn
    with pytest.raises(Exception) as info:
        next(L.linearize_dataset_generator(None, "cpu", None, fused_flat=True))
    assert "fused_flat" not in str(info.value)
