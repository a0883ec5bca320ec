"""The pair kernels on raw frames behind a gpu_transforms chain (ct_pair_residual_ingest_fwd / _bwd, csrc/ct_pairs_ingest.hip).

Two comparands.  (1) The two-launch route, ops.ingest_transform then ops.pair_residual_sums / _lut_grad on its float32 stack:
every staged sample has the same bits and the tiles are walked alike, so the results differ by the order of the float64
atomics only -- ORDER, the kernel-against-kernel tolerance of tests/test_gpu_pairs_uncertainty.py, and torch.equal on the
mask popcounts.  (2) The float64 reference of tests/_pair_refs.py on the chain's output, evaluated on the CPU with the
transform classes of common/transforms.py, at pr.TOL.  Inputs: tests/_pairs_ingest_cases.py (seeded scenes of _pair_refs,
N = 9, 64-point LUTs with distinct rows, planes 13x17 / 12x20 / 8x64); tests/test_pairs_ingest_host.py asserts on the CPU that
no chain masks its scene away."""
import pytest
import torch
from torch.utils.data import DataLoader

import _pair_refs as pr
import _pairs_ingest_cases as pc
from _util import assert_parity

pytestmark = pytest.mark.gpu

ORDER = dict(rtol=1e-9, norm_tol=1e-12)   # kernel against kernel: float64 atomic order


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _par(got, want, q, what):
    assert_parity(got.detach().cpu().numpy(), want.numpy(), rtol=pr.TOL[q][0], norm_tol=pr.TOL[q][1], what=f"pairs ingest {what} {q}")


def _order(got, want, what):
    assert_parity(got.detach().cpu().numpy(), want.detach().cpu().numpy(), what=f"pairs ingest {what}", **ORDER)


def _staged(cs, dev, layout):
    """(raw frames in ``layout`` on the device, stages, consts | None) of a case, as stage_images(defer_ingest=True) leaves them."""
    from clair_torch_amd import ops
    frames = pc.to_layout(cs.codes, layout).to(dev)
    stages, data = pc.stages_of(cs.codes, cs.chain, cs.dtype)
    consts = None
    if data:
        consts = ops.ingest_extrema(frames, ops.data_stage_prefix(stages), layout)
        ops.check_ingest_consts(consts)
    return frames, stages, consts


def _pairs(cs, dev):
    from clair_torch_amd import ops
    i, j, r = pr.exposure_pairs(cs.exposures, cs.threshold)
    return ops.PairList(i, j, r, len(cs.exposures), dev)


def _kw(cs, rel, unc, std_kw=None):
    from clair_torch_amd import ops
    kw = dict(lower=cs.lo, upper=cs.hi, use_relative=rel, use_unc_weight=unc)
    if cs.h_global is not None:
        kw["tile"] = ops.TileGeometry(h_global=cs.h_global, row_offset=cs.row_offset)
    kw.update(std_kw or {})
    return kw


def _lut(cs, dev, interp):
    return None if interp is None else cs.lut.to(dev)


# ---- 1. fused against two launches ---------------------------------------------------------------------------------------
def _fused_equals_two_launches(cs, dev, layout, interps=("lookup", "linear", "catmull", None), std_kw=None, unc=False):
    from clair_torch_amd import ops
    frames, stages, consts = _staged(cs, dev, layout)
    x = ops.ingest_transform(frames, stages, layout, consts=consts)
    assert torch.equal(x.cpu(), cs.x), f"{cs.name} {layout}: ct_ingest_transform is the CPU chain bit for bit"
    pairs = _pairs(cs, dev)
    coef = pr.seeded_coef(cs, pairs.n_pairs).to(dev)
    for interp in interps:
        lut = _lut(cs, dev, interp)
        for rel in (True, False):
            kw = _kw(cs, rel, unc, std_kw)
            what = f"{cs.name} {layout} {interp} {'rel' if rel else 'abs'}"
            two = ops.pair_residual_sums(x, pairs, lut=lut, interp=interp, level=1, **kw)
            one = ops.pair_residual_ingest_sums(frames, stages, pairs, lut=lut, interp=interp, level=1, consts=consts, layout=layout, **kw)
            assert torch.isfinite(one).all() and int(one[..., 4].min()) > 0, what
            assert torch.equal(one[..., 4], two[..., 4]), what + ": mask popcounts"
            _order(one, two, what + " level 1")
            center = two[..., 1] / two[..., 0].clamp(min=1e-8)
            _order(ops.pair_residual_ingest_sums(frames, stages, pairs, lut=lut, interp=interp, level=1, center=center, consts=consts,
                                                 layout=layout, **kw),
                   ops.pair_residual_sums(x, pairs, lut=lut, interp=interp, level=1, center=center, **kw), what + " centered")
            zero = ops.pair_residual_ingest_sums(frames, stages, pairs, lut=lut, interp=interp, level=0, consts=consts, layout=layout, **kw)
            _order(zero[..., :2], two[..., :2], what + " level 0")
            assert not zero[..., 2:].any(), what + ": level 0 leaves sums 2..4 alone"
            if interp is None or (interp == "lookup" and unc):
                continue
            for lane in (True, False):
                g2 = ops.pair_residual_lut_grad(x, pairs, coef, lut=lut, interp=interp, smean=center, lane_kernel=lane, **kw)
                g1 = ops.pair_residual_ingest_lut_grad(frames, stages, pairs, coef, lut=lut, interp=interp, smean=center,
                                                       lane_kernel=lane, consts=consts, layout=layout, **kw)
                assert torch.isfinite(g1).all() and g1.abs().sum() > 0, what
                _order(g1, g2, what + f" gradient lane={lane}")


@pytest.mark.parametrize("plane", pc.PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("layout", pc.LAYOUTS)
@pytest.mark.parametrize("dtype", ["u8", "u16"])
def test_fused_equals_two_launches(dev, dtype, layout, plane):
    """The four-stage chain with a per-channel clamp: LOOKUP / LINEAR / CATMULL / no model, relative and absolute loss, levels 0
    and 1, the centered second pass, the backward with and without the lane kernel."""
    _fused_equals_two_launches(pc.build("four", dtype, plane, "linear"), dev, layout)


def test_fused_equals_two_launches_data_dependent(dev):
    """One data-dependent Normalize with the constants of ops.ingest_extrema, raw BGR frames."""
    _fused_equals_two_launches(pc.build("data", "u16", (12, 20), "linear"), dev, "nhwc_bgr")


# ---- 2. fused against the float64 reference ------------------------------------------------------------------------------
def _check_against_reference(cs, dev, layout, smode="none", unc=False):
    from clair_torch_amd import ops
    from clair_torch_amd.inference._staging import DeferredIngest
    from clair_torch_amd.training import linearity_loss, spatial_statistics
    frames, stages, consts = _staged(cs, dev, layout)
    pairs = _pairs(cs, dev)
    sd = pr.std_stack(smode, cs.x, cs.seed)
    std_kw = pr.std_kwargs(smode, sd)
    if "std" in std_kw:
        std_kw["std"] = std_kw["std"].to(dev)        # planar beside frames of any layout
    lut = cs.lut.to(dev)
    out = {}
    for rel in (True, False):
        ref = pc.reference(cs, rel, unc, sd)
        kw = _kw(cs, rel, unc, std_kw)
        what = f"{cs.name} {layout} {smode} {'unc' if unc else 'nounc'} {'rel' if rel else 'abs'}"
        args = dict(lut=lut, interp=cs.interp, consts=consts, layout=layout, **kw)
        sums = ops.pair_residual_ingest_sums(frames, stages, pairs, level=1, **args)
        centered = ops.pair_residual_ingest_sums(frames, stages, pairs, level=1, center=ref.mean.to(dev), **args)
        assert torch.isfinite(sums).all() and torch.isfinite(centered).all(), what
        assert torch.equal(sums[..., 4].cpu(), ref.sums[..., 4]), what + ": mask popcounts"
        _par(sums[..., 0].clamp(min=1e-8), ref.den, "den", what)
        _par(sums[..., 1], ref.sums[..., 1], "num", what)
        mean, sdev, err = spatial_statistics(sums, centered, smode != "none")
        _par(mean, ref.mean, "mean", what)
        _par(sdev, ref.std, "std", what)
        if smode != "none":
            _par(sums[..., 3], ref.sums[..., 3], "errsum", what)
            _par(err, ref.err, "err", what)
        coef = pr.seeded_coef(cs, pairs.n_pairs)
        g = ops.pair_residual_ingest_lut_grad(frames, stages, pairs, coef.to(dev), smean=ref.mean.to(dev), **args)
        assert torch.isfinite(g).all(), what
        _par(g, ref.grad_coef, "grad", what + " coef")
        param = cs.lut.to(dev).requires_grad_(True)
        lin, sp = linearity_loss(param, DeferredIngest(frames, stages, layout, consts), pairs, interp=cs.interp, group=False, **kw)
        g_lin = torch.autograd.grad(lin.sum(), param)[0]
        assert torch.isfinite(g_lin).all() and torch.isfinite(lin).all(), what
        _par(lin, ref.linloss, "linloss", what)
        _par(sp, ref.mean, "mean", what + " linearity_loss")
        _par(g_lin.double(), ref.grad_lin, "grad", what + " autograd")
        out[rel] = (sums, g)
    return out


@pytest.mark.parametrize("k", range(len(pc.CHAINS)), ids=pc.CHAINS)
def test_fused_against_float64_reference(dev, k):
    """A black level, a target range, a scalar clamp, a per-channel clamp, four stages, a data-dependent Normalize: sums, the
    centered pass, the gradient for a given coef and linearity_loss + autograd.grad."""
    chain = pc.CHAINS[k]
    cs = pc.build(chain, ("u16", "u8")[k % 2], pc.PLANES[k % 3], ("linear", "catmull")[k % 2])
    _check_against_reference(cs, dev, pc.LAYOUTS[k % 3])


# ---- 3. uncertainties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smode,chain,dtype,plane,interp,layout", pc.uncertainty_cases(), ids=pr.STD_MODES)
def test_uncertainties(dev, smode, chain, dtype, plane, interp, layout):
    """CONSTANT / MULTIPLIER on the chain's output and an explicit planar std stack (beside BGR frames), uncertainty weighting
    on and off: against the reference, and against the two launches with the same planar std."""
    cs = pc.build(chain, dtype, plane, interp)
    std_kw = pr.std_kwargs(smode, pr.std_stack(smode, cs.x, cs.seed))
    if "std" in std_kw:
        std_kw["std"] = std_kw["std"].to(dev)
    for unc in (True, False):
        _check_against_reference(cs, dev, layout, smode, unc)
        _fused_equals_two_launches(cs, dev, layout, interps=(interp, None), std_kw=std_kw, unc=unc)


# ---- 4. row bands --------------------------------------------------------------------------------------------------------
def test_row_bands(dev):
    """Two bands of 11 x 32 that start on tile boundaries (6 * 32 = 3 * 64 pixels) add up to the whole at the order of the
    float64 atomics; one band of 13 x 17 that cuts through tiles matches the reference with the global geometry."""
    from clair_torch_amd import ops
    whole = pc.build("black", "u16", (11, 32), "linear")
    pairs = _pairs(whole, dev)
    coef = pr.seeded_coef(whole, pairs.n_pairs).to(dev)
    lut = whole.lut.to(dev)
    for layout in ("nchw", "nhwc_bgr"):
        frames, stages, consts = _staged(whole, dev, layout)
        kw = dict(lut=lut, interp="linear", layout=layout, **_kw(whole, True, False))
        s_whole = ops.pair_residual_ingest_sums(frames, stages, pairs, level=1, **kw)
        g_whole = ops.pair_residual_ingest_lut_grad(frames, stages, pairs, coef, **kw)
        s_sum, g_sum = 0, 0
        for r0, r1 in ((0, 6), (6, 11)):
            band = pc.band_of(whole, r0, r1 - r0)
            bframes, _, _ = _staged(band, dev, layout)
            bkw = dict(kw, **_kw(band, True, False))
            s_sum = s_sum + ops.pair_residual_ingest_sums(bframes, stages, pairs, level=1, **bkw)
            g_sum = g_sum + ops.pair_residual_ingest_lut_grad(bframes, stages, pairs, coef, **bkw)
        _order(s_sum, s_whole, f"bands = whole sums {layout}")
        _order(g_sum, g_whole, f"bands = whole gradient {layout}")
    band = pc.band_of(pc.build("clamp_channels", "u8", (13, 17), "catmull"), *pr.BAND)
    _check_against_reference(band, dev, "nhwc")


# ---- 5. public interface -------------------------------------------------------------------------------------------------
def _api_loader(seed=77):
    from clair_torch_amd.datasets import StackDataset, custom_collate
    exposures = pr.base_exposures()
    codes, _, _ = pr.scene(seed, exposures, (3, 12, 20), "u16")
    return DataLoader(StackDataset(codes, exposures), batch_size=len(exposures), shuffle=False, collate_fn=custom_collate)


def _api_chain():
    from clair_torch_amd.common import transforms as T
    return [T.CastTo("float32"), T.Normalize(65535, 64)]


def _train(fused, epochs=3):
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training import train_icrf
    model = ICRFModelDirect(n_points=64, channels=3, interpolation_mode=InterpMode.LINEAR, initial_power=2.5).to("cuda")
    opts = [torch.optim.Adam(model.channel_params(c), lr=1e-3, amsgrad=False) for c in range(3)]
    train_icrf(_api_loader(), 9, "cuda", model, optimizers=opts, use_uncertainty_weighting=False, epochs=epochs, patience=200,
               alpha=10.0, exposure_ratio_threshold=0.25, gpu_transforms=_api_chain(), verbose=False, fused_ingest=fused)
    return model


def test_public_interface_fused_equals_unfused(dev):
    """measure_linearity and three epochs of train_icrf on raw uint16 codes behind a black level, fused_ingest on and off:
    statistics at the order of the atomics, the trained curve at the 2e-6 that tests/test_gpu_training.py asks of its
    five-epoch runs against the reference."""
    from clair_torch_amd.inference import measure_linearity
    got = [measure_linearity(_api_loader(), "cuda", use_uncertainty_weighting=False, gpu_transforms=_api_chain(), fused_ingest=f)
           for f in (True, False)]
    assert torch.equal(got[0][0], got[1][0]) and got[0][3] is None and got[1][3] is None
    for a, b, q in zip(got[0][1:3], got[1][1:3], ("mean", "std")):
        assert torch.isfinite(a).all() and a.abs().sum() > 0
        _order(a, b, f"measure_linearity {q}")
    fused, plain, start = _train(True), _train(False), _train(True, epochs=0)
    assert (fused.icrf.detach() - start.icrf.detach()).abs().max() > 1e-4, "three epochs moved the curve"
    worst = (fused.icrf.detach() - plain.icrf.detach()).abs().max().item()
    assert worst < 2e-6, worst


def test_public_interface_takes_the_fused_route(dev, monkeypatch):
    from clair_torch_amd import ops
    from clair_torch_amd.inference import measure_linearity
    seen = []
    for name in ("pair_residual_ingest_sums", "pair_residual_ingest_lut_grad", "pair_residual_sums", "pair_residual_lut_grad",
                 "ingest_transform"):
        def spy(*a, _f=getattr(ops, name), _n=name, **kw):
            seen.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    for kw in ({}, {"fused_ingest": True}):
        del seen[:]
        measure_linearity(_api_loader(), "cuda", use_uncertainty_weighting=False, gpu_transforms=_api_chain(), **kw)
        assert seen == ["pair_residual_ingest_sums"] * 2
    del seen[:]
    measure_linearity(_api_loader(), "cuda", use_uncertainty_weighting=False, gpu_transforms=_api_chain(), fused_ingest=False)
    assert seen == ["ingest_transform", "pair_residual_sums", "pair_residual_sums"]
    del seen[:]
    _train(True, epochs=2)     # the first step is the reference's dead step: no backward
    assert seen == ["pair_residual_ingest_sums", "pair_residual_ingest_sums", "pair_residual_ingest_lut_grad"]
    del seen[:]
    _train(False, epochs=2)
    assert seen == ["ingest_transform", "pair_residual_sums", "ingest_transform", "pair_residual_sums", "pair_residual_lut_grad"]


# ---- 6. zero range -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_zero_range_still_raises(dev, fused):
    """A data-dependent Normalize over a constant stack: the reference's ValueError on both routes."""
    from clair_torch_amd.common import transforms as T
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import measure_linearity
    frames = torch.full((4, 3, 5, 7), 300, dtype=torch.int32).to(torch.uint16)
    loader = DataLoader(StackDataset(frames, [0.001, 0.002, 0.004, 0.008]), batch_size=4, shuffle=False, collate_fn=custom_collate)
    with pytest.raises(ValueError, match="Normalization range is zero"):
        measure_linearity(loader, "cuda", gpu_transforms=[T.CastTo("float32"), T.Normalize()], fused_ingest=fused)
