"""The fused chain + pair kernels without a GPU: ct_pair_residual_ingest_fwd / _bwd are declared, exported and validate every
argument before any launch; the ops fronts refuse float32 frames and wrong std shapes with the siblings' messages;
train_icrf / measure_linearity hand raw codes behind a chain to the fused ops; and -- a condition of the GPU tests, not a
tolerance -- no chain of tests/_pairs_ingest_cases.py masks its scene away: the CPU reference has a nonzero mask popcount in
every (pair, channel) and at least a quarter of all pair pixels are valid overall."""
import ctypes
import os
import re

import pytest
import torch

import _pairs_ingest_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, NO_GRADIENT_PATH, TOO_LARGE = 0, -1, -2, -4, -5


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


def _params(std_mode=0, unc=1):
    from clair_torch_amd import _native as nv
    return nv.PairParams(lower=1 / 255, upper=254 / 255, weight_scale=10.0, use_relative=1, use_uncertainty_weighting=unc,
                         std_mode=std_mode, std_value=0.01, pair_band=0)


def test_entry_points_are_declared_and_exported(lib):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clair_hip.h")).read(), flags=re.S)
    for name, n_args in (("ct_pair_residual_ingest_fwd", 18), ("ct_pair_residual_ingest_bwd", 21)):
        assert re.search(rf"\bint\s+{name}\s*\(", header)
        assert name in nv.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == n_args
        # the siblings' arguments with max_code replaced by (stages, n_stages, consts_dev)
        assert len(getattr(lib, name).argtypes) == len(getattr(lib, name.replace("_ingest", "")).argtypes) + 2
    assert re.search(r"#define\s+CT_ABI_VERSION\s+3\b", header)
    assert lib.ct_abi_version() == 3 and nv.ABI_VERSION == 3
    assert "ct_pairs_ingest.hip" in build.SOURCES and "ct_pairs.hip" in build.SOURCES and "ct_pairs_kernel.hpp" in build.HEADERS
    for f in ("ct_pairs_ingest.hip", "ct_pairs.hip", "ct_pairs_kernel.hpp"):
        assert os.path.exists(os.path.join(build.CSRC, f))


def test_validation_comes_before_any_launch(lib):
    """Every refusal below returns with fake device pointers that are never dereferenced (a launch on them would fault) and
    without a device in this process."""
    from clair_torch_amd import _native as nv
    U8, U16, F32 = nv.DTYPE_U8, nv.DTYPE_U16, nv.DTYPE_F32
    NHWC, BGR = nv.LAYOUT_NHWC, nv.LAYOUT_NHWC_BGR
    fake = ctypes.c_void_p(0x1000)
    linear = nv.Icrf(lut_dev=0x2000, n_points=64, interp=nv.INTERP_LINEAR)
    lookup = nv.Icrf(lut_dev=0x2000, n_points=64, interp=nv.INTERP_LOOKUP)
    none = nv.Icrf(lut_dev=None, n_points=0, interp=nv.INTERP_NONE)
    one = _stages(nv.INGEST_AFFINE)

    def fwd(frames=fake, dtype=U16, stages=one, n_stages=1, consts=None, n_images=3, geom=None, std=None, model=linear,
            n_pairs=2, params=None, level=1, idx=fake):
        geom = _geom() if geom is None else geom
        params = _params() if params is None else params
        return lib.ct_pair_residual_ingest_fwd(frames, dtype, stages, n_stages, consts, n_images,
                                               None if geom is False else ctypes.byref(geom), std, ctypes.byref(model), idx, idx,
                                               idx, n_pairs, None if params is False else ctypes.byref(params), level, None, idx,
                                               None)

    def bwd(frames=fake, dtype=U16, stages=one, n_stages=1, consts=None, n_images=3, geom=None, std=None, model=linear,
            n_pairs=2, params=None, smean=None, ws=fake, ws_bytes=1 << 20, idx=fake):
        geom = _geom() if geom is None else geom
        params = _params() if params is None else params
        return lib.ct_pair_residual_ingest_bwd(frames, dtype, stages, n_stages, consts, n_images,
                                               None if geom is False else ctypes.byref(geom), std, ctypes.byref(model), idx, n_pairs,
                                               idx, idx, idx, None if params is False else ctypes.byref(params), idx, smean, idx,
                                               ws, ws_bytes, None)

    for call in (fwd, bwd):
        # nothing to do: CT_OK without a launch
        assert call(n_pairs=0) == OK and call(n_pairs=0, dtype=U8, geom=_geom(layout=BGR)) == OK
        assert call(n_pairs=0, stages=None, n_stages=0) == OK
        assert call(n_pairs=0, stages=_stages(nv.INGEST_AFFINE, nv.INGEST_AFFINE_DATA), n_stages=2, consts=fake) == OK
        # geometry
        assert call(geom=False) == INVALID and call(params=False) == INVALID
        assert call(geom=_geom(c=0)) == INVALID and call(geom=_geom(h=-1)) == INVALID
        assert call(geom=_geom(h=0)) == INVALID                         # the pair kernels take no empty plane
        assert call(geom=_geom(h=4, h_global=3)) == INVALID and call(geom=_geom(h=4, h_global=6, row_offset=3)) == INVALID
        assert call(geom=_geom(layout=3)) == INVALID
        assert call(geom=_geom(h=1 << 15, w=1 << 15)) == TOO_LARGE
        short = _geom()
        short.image_stride = 47
        assert call(geom=short) == INVALID
        assert call(geom=_geom(c=4, layout=NHWC)) == UNSUPPORTED
        # the stage list
        assert call(stages=_stages(7)) == INVALID                       # a bad stage kind
        assert call(stages=_stages(*[nv.INGEST_AFFINE] * 5), n_stages=5) == INVALID   # too many stages
        assert call(n_stages=-1) == INVALID and call(stages=None, n_stages=1) == INVALID
        assert call(stages=_stages(nv.INGEST_AFFINE_DATA)) == INVALID   # without consts_dev
        assert call(stages=_stages(nv.INGEST_AFFINE_DATA, nv.INGEST_AFFINE_DATA), n_stages=2, consts=fake) == INVALID
        assert call(consts=ctypes.c_void_p(0x1002)) == INVALID          # misaligned consts
        by_channel = _stages(nv.INGEST_CLAMP)
        by_channel[0].hi[2] = 0.5
        assert call(geom=_geom(c=5), stages=by_channel) == UNSUPPORTED
        # dtype: float32 frames have no copy to save
        assert call(dtype=F32) == UNSUPPORTED and call(dtype=F32, n_pairs=0) == UNSUPPORTED
        assert call(dtype=3) == INVALID
        # what the siblings refuse
        assert call(n_images=1) == INVALID and call(n_images=1, n_pairs=0) == INVALID
        assert call(frames=None) == INVALID and call(n_pairs=-1) == INVALID
        assert call(frames=ctypes.c_void_p(0x1001)) == INVALID          # uint16 frames at an odd address
        assert call(model=nv.Icrf(lut_dev=0x2000, n_points=64, interp=7)) == INVALID
        assert call(model=nv.Icrf(lut_dev=None, n_points=64, interp=nv.INTERP_LINEAR)) == INVALID
        assert call(params=_params(std_mode=3)) == INVALID              # EXPLICIT without its pointer
        assert call(params=_params(std_mode=3), std=ctypes.c_void_p(0x1002)) == INVALID
        assert call(idx=None) == INVALID
    # LOOKUP with a std mode has no gradient path
    assert fwd(model=lookup, params=_params(std_mode=1)) == NO_GRADIENT_PATH
    assert bwd(model=lookup, params=_params(std_mode=1), smean=fake) == NO_GRADIENT_PATH
    assert bwd(model=lookup, params=_params(std_mode=2), smean=fake, dtype=U8) == NO_GRADIENT_PATH
    # forward only / backward only
    assert fwd(level=2) == INVALID and fwd(level=-1) == INVALID
    assert bwd(model=none) == INVALID and bwd(params=_params(std_mode=1)) == INVALID   # no model / no smean
    assert bwd(ws_bytes=-1) == INVALID


def test_ops_fronts_refuse_like_their_siblings(monkeypatch):
    from clair_torch_amd import ops

    def reached_the_device(*a, **kw):
        raise AssertionError("the call reached the device")

    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pair_residual_ingest_sums(torch.zeros((3, 3, 4, 4), dtype=torch.uint8), [("affine", 0.0, 1.0, 1.0, 0.0)], None, lut=None,
                                      interp=None, lower=0.0, upper=1.0, use_relative=True, use_unc_weight=False)
    monkeypatch.setattr(ops, "_require_device", lambda t, name: None)
    monkeypatch.setattr(ops, "_stream", reached_the_device)
    monkeypatch.setattr(ops.nv, "load", reached_the_device)
    i, j = torch.tensor([0, 0, 1]), torch.tensor([1, 2, 2])
    pairs = ops.PairList(i, j, torch.tensor([0.5, 0.25, 0.5], dtype=torch.float64), 3, torch.device("cpu"))
    u16 = torch.zeros((3, 3, 4, 4), dtype=torch.uint16)
    lut = torch.rand((3, 16))
    stages = [("affine", 64.0, 959.0, 1.0, 0.0)]
    kw = dict(lut=lut, interp="linear", lower=0.0, upper=1.0, use_relative=True, use_unc_weight=True)

    def both(frames, match, exc, stages=stages, pairs=pairs, **extra):
        with pytest.raises(exc, match=match):
            ops.pair_residual_ingest_sums(frames, stages, pairs, **kw, **extra)
        with pytest.raises(exc, match=match):
            ops.pair_residual_ingest_lut_grad(frames, stages, pairs, torch.zeros((3, 3)), smean=torch.zeros((3, 3)), **kw, **extra)

    both(torch.zeros((3, 3, 4, 4)), "takes uint8 / uint16 codes \\(float32 pixels: ingest_transform", TypeError)
    shape_message = "std must be a float32 tensor of shape \\(3, 3, 4, 4\\) \\(planar, like the"
    both(u16, shape_message, ValueError, std=torch.zeros((3, 3, 4, 5)))
    both(u16, shape_message, ValueError, std=torch.zeros((3, 3, 4, 4), dtype=torch.float64))
    interleaved = torch.zeros((3, 4, 4, 3), dtype=torch.uint16)
    both(interleaved, shape_message, ValueError, std=torch.zeros((3, 4, 4, 3)), layout="nhwc_bgr")   # the std is planar
    both(torch.zeros((3, 4, 4, 2), dtype=torch.uint8), "takes \\(B, H, W, 3\\) frames", ValueError, layout="nhwc")
    both(u16, "unknown layout", ValueError, layout="hwc")
    both(u16.permute(0, 1, 3, 2), "stack must be contiguous", ValueError)
    both(u16[:2], "pair list was built for 3 images", ValueError)
    both(u16, "at most 4 stages", ValueError, stages=stages * 5)
    both(u16, "expected \\('affine'", ValueError, stages=[("affine_data", 1.0, 0.0)])      # without consts
    both(u16, "consts must be the 4-element float32 tensor", ValueError, stages=[("affine_data", 1.0, 0.0)], consts=torch.zeros(3))
    both(u16, "unknown std_mode", ValueError, std_mode="poisson")


class _Recorder:
    """Stands in for clair_torch_amd.ops inside the staging and training/linearity.py: records which fronts are called."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):   # PairList, TileGeometry, ingest_shape, check_ingest_consts, ...
        from clair_torch_amd import ops
        return getattr(ops, name)

    def strided_downscale(self, images, step, layout="nchw"):
        assert step == 1
        return images

    def ingest_transform(self, images, stages, layout="nchw", consts=None):
        from clair_torch_amd import ops
        self.calls.append(("ingest_transform", images.dtype, layout))
        return torch.zeros(ops.ingest_shape(tuple(images.shape), layout))

    def _sums(self, name, frames, pairs, kw):
        self.calls.append((name, frames.dtype, kw.get("layout", "nchw"), kw.get("level")))
        return torch.ones((pairs.n_pairs, 3, 5), dtype=torch.float64)

    def pair_residual_sums(self, stack, pairs, **kw):
        return self._sums("pair_residual_sums", stack, pairs, kw)

    def pair_residual_ingest_sums(self, frames, stages, pairs, **kw):
        assert "max_code" not in kw and tuple(stages) == (("affine", 64, 959, 1.0, 0.0),)
        return self._sums("pair_residual_ingest_sums", frames, pairs, kw)


def test_measure_linearity_routes(monkeypatch):
    """A black level on raw codes goes to the fused front (never ct_ingest_transform), in either layout; fused_ingest=False,
    float32 frames behind the chain and the "code" route go where they always went."""
    from clair_torch_amd.common import transforms as T
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import _staging
    from clair_torch_amd.training import linearity
    from torch.utils.data import DataLoader
    cpu = torch.device("cpu")
    monkeypatch.setattr(linearity, "resolve_device", lambda device: cpu)
    u16 = (torch.arange(4 * 3 * 2 * 5, dtype=torch.int32) * 500).reshape(4, 3, 2, 5).to(torch.uint16)
    f32 = torch.rand((4, 3, 2, 5))
    black = [T.CastTo("float32"), T.Normalize(1023, 64)]

    def run(frames, chain, **kw):
        rec = _Recorder()
        monkeypatch.setattr(linearity, "ops", rec)
        monkeypatch.setattr(_staging, "ops", rec)
        loader = DataLoader(StackDataset(frames, [0.001, 0.002, 0.004, 0.008]), batch_size=4, shuffle=False, collate_fn=custom_collate)
        linearity.measure_linearity(loader, "cuda", gpu_transforms=chain, **kw)
        return rec.calls

    for kw in ({}, {"fused_ingest": True}):
        assert run(u16, black, **kw) == [("pair_residual_ingest_sums", torch.uint16, "nchw", 1)] * 2
    assert run(u16, black, fused_ingest=False) == [("ingest_transform", torch.uint16, "nchw")] + [("pair_residual_sums", torch.float32, "nchw", 1)] * 2
    for flag in (True, False):
        assert run(f32, black, fused_ingest=flag) == [("ingest_transform", torch.float32, "nchw")] + [("pair_residual_sums", torch.float32, "nchw", 1)] * 2
        assert run(u16, [T.CastTo("float32"), T.Normalize(65535, 0)], fused_ingest=flag) == [("pair_residual_sums", torch.uint16, "nchw", 1)] * 2
        assert run(f32, None, fused_ingest=flag) == [("pair_residual_sums", torch.float32, "nchw", 1)] * 2


@pytest.mark.parametrize("chain,dtype,plane,interp", pc.reference_cases())
def test_no_chain_masks_its_scene_away(chain, dtype, plane, interp):
    """The condition of the GPU tests: with everything masked a wrong kernel would still agree with the reference."""
    cs = pc.build(chain, dtype, plane, interp)
    valid = pc.reference(cs, True, want_grad=False).valid               # (P, C, H, W)
    assert valid.shape[0] == 26 and valid.shape[1] == 3
    popcount = valid.sum(dim=(2, 3))
    assert int(popcount.min()) > 0, (cs.name, popcount)
    assert float(valid.float().mean()) >= 0.25, (cs.name, float(valid.float().mean()))
    # the chain is the one stage_images would fuse, and its CPU evaluation is float32
    stages, data = pc.stages_of(cs.codes, chain, dtype)
    assert 1 <= len(stages) <= 4 and data == (chain == "data") and cs.x.dtype == torch.float32


def _admissible_cases():
    out = [("none", chain, ("u16", "u8")[k % 2], pc.PLANES[k % 3], ("linear", "catmull")[k % 2]) for k, chain in enumerate(pc.CHAINS)]
    return out + [tuple(u[:5]) for u in pc.uncertainty_cases()] + [("none", "clamp_channels", "u8", (13, 17), "catmull")]


@pytest.mark.parametrize("smode,chain,dtype,plane,interp", _admissible_cases())
def test_tolerances_cover_the_eager_oracle_on_these_cases(smode, chain, dtype, plane, interp):
    """pr.TOL is four times the float32 eager oracle's deviation from the float64 reference on the inputs of
    tests/_pair_refs.py.  The inputs here are others, so the same condition is asserted on each case that the GPU tests
    compare with the reference: the reference project's own float32 arithmetic stays within a quarter of the tolerance."""
    import numpy as np
    import _pair_refs as pr
    from _util import rel_norm
    cs = pc.build(chain, dtype, plane, interp)
    sd = pr.std_stack(smode, cs.x, cs.seed)
    for rel in (True, False):
        for unc in ((True, False) if smode != "none" else (False,)):
            ref = pc.reference(cs, rel, unc, sd, want_grad=False)
            s0, s1, s3 = pr.eager_sums_f32(cs.x, sd, cs.exposures, cs.lut, cs.interp, cs.threshold, cs.lo, cs.hi, rel, unc)
            pairs = {"den": (s0.clamp(min=1e-8), ref.den), "num": (s1, ref.sums[..., 1])}
            if s3 is not None:
                pairs["errsum"] = (s3, ref.sums[..., 3])
            for q, (got, want) in pairs.items():
                got, want = got.double().numpy(), want.numpy()
                med = float(np.median(np.abs(want)))
                worst = float(np.max(np.abs(got - want) / (np.abs(want) + med)))
                assert worst * 4 <= pr.TOL[q][0] and rel_norm(got, want) * 4 <= pr.TOL[q][1], (cs.name, smode, rel, unc, q)
