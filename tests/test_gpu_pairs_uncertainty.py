"""The uncertainty-weighted paths of the two pair kernels (csrc/ct_pairs.hip) against the float64 reference of
tests/_pair_refs.py.

Inputs are seeded (tests/_pair_refs.py), tolerances are the ones tests/test_pair_refs_host.py measures on the CPU (4x the
float32 eager oracle's deviation from the reference), and every comparison goes through _util.assert_parity (labels
"pairs ..." in parity_observed.json).  Kernel against kernel (band sums, interleaved against planar, level 0 against 1) the
results differ by the order of float64 atomics only: rtol 1e-9, norm-wise 1e-12, as the existing tests use for exactly that.

All comparisons go through ops.pair_residual_sums and ops.pair_residual_lut_grad -- the latter with coef and smean from the
reference, so the backward is tested apart from the forward -- and through training.linearity_loss + autograd.grad, the
route train_icrf takes.

Path -> test:

| path | test |
|---|---|
| CT_STD_CONSTANT / MULTIPLIER / EXPLICIT, forward (level 1, weight on and off, all five sums, centered pass) and backward | test_matrix (case names say which) |
| scalar staging (13x17: odd plane, ragged last tile), vector staging (12x20: partial last tile; 8x64: whole tiles), float32 / uint16 / uint8, LINEAR / CATMULL | test_matrix |
| gathered staging (interleaved stacks + explicit std in the same layout; 12x20 vector groups, 13x17 scalar) forward and backward | test_interleaved_explicit_std |
| once_term_unc<true> (relative) and once_term_unc<false> (absolute) | every backward test runs both (`rel` loop) |
| grouped (kGroup = 4) and tail partners: the base geometry gives samples 0 .. 4 i-side partners | test_matrix; 127 .. 0 partners: test_many_exposures_and_narrow_tiles |
| forward without a model (f' = 1), each std mode | test_no_model |
| level 0 = level 1 in sums 0 and 1 | test_level0_equals_level1 |
| row bands with explicit std: two ragged, tile-aligned bands = whole; one band cutting through tiles, global geometry = reference | test_row_bands_explicit_std |
| narrow (32-column) tiles; pair list of 8128 > 4 * 256 pairs (eight forward launches) with STD | test_many_exposures_and_narrow_tiles[many_exposures] |
| STD backward at 32 columns where the plain backward takes 64 (N = 96, L = 256) | test_many_exposures_and_narrow_tiles[narrow_std_only] |
| clamp branch `Ij >= 1e-6f ? inv_ijs : 0` and the forward's clamp(min=1e-6): LUT foot exactly 0, lower = 0 | test_edge_clamp_branch |
| pixel values 0, 1, on / beside the validity thresholds, on LUT knots | test_edge_thresholds_and_knots |
| residual exactly 0 (two identical frames of equal exposure): zero gradient contribution | test_edge_zero_residual |
| masked pixels with huge finite stds: nothing leaks through the mask | test_edge_masked_huge_std |
| a coef that is zero for one channel (the channel's workgroups return at once), and for all | test_edge_zero_coef_channel |
| refusals: LOOKUP with a std mode (forward, backward), backward without smean, std of the wrong shape | test_refusals |
| measure_linearity / linearity_loss through std_arguments: explicit std images, std_hint constant | test_api_explicit_and_constant_hint |

Dropped from the matrix's full product (3 std modes x 2 interps x 3 dtypes x 3 planes = 54 -> 10 cases, every PAIR of
values present; tests/_pair_refs.py, matrix_cases): std mode, interp and dtype act in the staging of one sample (which
sigma, which dfdx, which to_pixel), the plane only picks the stager and the shape of the last tile; no three of them share
code that two do not.  relative / absolute x weight on / off run inside every case.  The two large stacks run the relative
loss only (the absolute one differs in once_term_unc alone, which the small cases cover at every shape)."""
import functools

import pytest
import torch
from torch.utils.data import DataLoader

import _pair_refs as pr
from _util import assert_parity

pytestmark = pytest.mark.gpu

ORDER = dict(rtol=1e-9, norm_tol=1e-12)   # kernel against kernel: float64 atomic order


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(name):
    return pr.build_case(name)


def _reference(cs, rel, unc, want_grad=True, **kw):
    n_pairs = pr.exposure_pairs(cs.exposures, cs.threshold)[0].numel()
    return pr.pair_step_f64(cs.x, cs.sd, cs.exposures, cs.lut, cs.interp, cs.threshold, cs.lo, cs.hi, rel, unc,
                            coef=pr.seeded_coef(cs, n_pairs), h_global=cs.h_global, row_offset=cs.row_offset,
                            want_grad=want_grad and cs.interp is not None, **kw)


def _to_layout(t, layout):
    if layout == "nchw":
        return t.contiguous()
    return (t.flip(1) if layout == "nhwc_bgr" else t).permute(0, 2, 3, 1).contiguous()


def _launch_args(cs, dev, rel, unc, layout="nchw"):
    """(stack, PairList, keyword arguments shared by ops.pair_residual_sums / _lut_grad / linearity_loss)."""
    from clair_torch_amd import ops
    i, j, r = pr.exposure_pairs(cs.exposures, cs.threshold)
    pairs = ops.PairList(i, j, r, len(cs.exposures), dev)
    kw = dict(interp=cs.interp, lower=cs.lo, upper=cs.hi, use_relative=rel, use_unc_weight=unc, max_code=cs.max_code,
              layout=layout)
    if cs.h_global is not None:
        kw["tile"] = ops.TileGeometry(h_global=cs.h_global, row_offset=cs.row_offset)
    std_kw = pr.std_kwargs(cs.smode, cs.sd)
    if "std" in std_kw:
        std_kw["std"] = _to_layout(std_kw["std"], layout).to(dev)
    kw.update(std_kw)
    return _to_layout(cs.stored, layout).to(dev), pairs, kw


def _lut(cs, dev):
    return None if cs.lut is None else cs.lut.to(dev)


def _par(got, want, q, what):
    assert_parity(got.detach().cpu().numpy(), want.numpy(), rtol=pr.TOL[q][0], norm_tol=pr.TOL[q][1], what=f"pairs {what} {q}")


def _check_forward(cs, dev, rel, unc, layout="nchw"):
    """Level 1: all five sums and the centered second pass against the reference.  Returns the (P, C, 5) sums."""
    from clair_torch_amd import ops
    from clair_torch_amd.training import spatial_statistics
    ref = _reference(cs, rel, unc, want_grad=False)
    stack, pairs, kw = _launch_args(cs, dev, rel, unc, layout)
    sums = ops.pair_residual_sums(stack, pairs, lut=_lut(cs, dev), level=1, **kw)
    centered = ops.pair_residual_sums(stack, pairs, lut=_lut(cs, dev), level=1, center=ref.mean.to(dev), **kw)
    what = f"{cs.name} {'rel' if rel else 'abs'} {'unc' if unc else 'nounc'} {layout}"
    assert torch.isfinite(sums).all() and torch.isfinite(centered).all(), what
    assert torch.equal(sums[..., 4].cpu(), ref.sums[..., 4]), what + ": mask popcounts"
    _par(sums[..., 0].clamp(min=1e-8), ref.den, "den", what)
    _par(sums[..., 1], ref.sums[..., 1], "num", what)
    _par(sums[..., 3], ref.sums[..., 3], "errsum", what)
    mean, sd, err = spatial_statistics(sums, centered, True)
    _par(mean, ref.mean, "mean", what)
    _par(sd, ref.std, "std", what)
    _par(err, ref.err, "err", what)
    return sums


def _check_backward(cs, dev, rel, layout="nchw"):
    """use_unc_weight=True: ops.pair_residual_lut_grad with the reference's coef and smean, and linearity_loss +
    autograd.grad.  Returns the two gradients."""
    from clair_torch_amd import ops
    from clair_torch_amd.training import linearity_loss
    ref = _reference(cs, rel, True)
    stack, pairs, kw = _launch_args(cs, dev, rel, True, layout)
    what = f"{cs.name} {'rel' if rel else 'abs'} {layout}"
    coef = pr.seeded_coef(cs, pairs.n_pairs)
    g = ops.pair_residual_lut_grad(stack, pairs, coef.to(dev), lut=_lut(cs, dev), smean=ref.mean.to(dev), **kw)
    assert torch.isfinite(g).all(), what
    _par(g, ref.grad_coef, "grad", what + " coef")
    lut = cs.lut.to(dev).requires_grad_(True)
    lin, sp = linearity_loss(lut, stack, pairs, group=False, **kw)
    g_lin = torch.autograd.grad(lin.sum(), lut)[0]
    assert torch.isfinite(g_lin).all() and torch.isfinite(lin).all(), what
    _par(sp, ref.mean, "mean", what + " loss route")
    _par(lin, ref.linloss, "linloss", what)
    # the gradient leaves linearity_loss in the LUT's float32: 6e-8 relative, inside every entry of the table
    _par(g_lin.double(), ref.grad_lin, "grad", what + " linloss")
    return g, g_lin


@pytest.mark.parametrize("name", [m[0] for m in pr.matrix_cases()])
def test_matrix(dev, name):
    cs = _case(name)
    for rel in (True, False):
        for unc in (True, False):
            _check_forward(cs, dev, rel, unc)
        _check_backward(cs, dev, rel)


@pytest.mark.parametrize("smode", pr.STD_MODES)
def test_no_model(dev, smode):
    """interp None: f' = 1, the linearized std is the std itself."""
    cs = _case(f"nomodel_{smode}")
    for rel in (True, False):
        _check_forward(cs, dev, rel, True)


def test_level0_equals_level1(dev):
    from clair_torch_amd import ops
    for name in ("explicit_linear_f32_8x64", "constant_linear_f32_13x17"):
        cs = _case(name)
        for rel in (True, False):
            stack, pairs, kw = _launch_args(cs, dev, rel, True)
            s1 = ops.pair_residual_sums(stack, pairs, lut=_lut(cs, dev), level=1, **kw)
            s0 = ops.pair_residual_sums(stack, pairs, lut=_lut(cs, dev), level=0, **kw)
            assert_parity(s0[..., :2].cpu().numpy(), s1[..., :2].cpu().numpy(), what="pairs level 0 = level 1", **ORDER)
            assert not s0[..., 2:].any()


def test_row_bands_explicit_std(dev):
    """Two ragged bands (6 and 5 rows of 11 x 32: three whole tiles, and two and a half) add up to the whole image.  The
    bands start on tile boundaries (6 * 32 = 3 * 64 pixels), so every tile holds the pixels it holds in the whole image,
    its float32 partial sums are the same and only the order of the float64 atomics differs.  (Bands that cut through a
    tile regroup the float32 partial sums; tests/test_gpu_training.py checks those at 1e-6.)  Then one band of the 13 x 17
    image that does cut through tiles (rows [3, 10), scalar staging) against the reference evaluated on that band with
    the global geometry."""
    from clair_torch_amd import ops
    whole = _case("bands_11x32")
    h = whole.x.shape[2]
    for rel in (True, False):
        ref = _reference(whole, rel, True)
        _check_forward(whole, dev, rel, True)
        stack, pairs, kw = _launch_args(whole, dev, rel, True)
        coef = pr.seeded_coef(whole, pairs.n_pairs).to(dev)
        s_whole = ops.pair_residual_sums(stack, pairs, lut=_lut(whole, dev), level=1, **kw)
        g_whole = ops.pair_residual_lut_grad(stack, pairs, coef, lut=_lut(whole, dev), smean=ref.mean.to(dev), **kw)
        s_sum, g_sum = 0, 0
        for r0, r1 in ((0, 6), (6, h)):
            band = pr.band_of(whole, r0, r1 - r0)
            bstack, _, bkw = _launch_args(band, dev, rel, True)
            s_sum = s_sum + ops.pair_residual_sums(bstack, pairs, lut=_lut(whole, dev), level=1, **bkw)
            g_sum = g_sum + ops.pair_residual_lut_grad(bstack, pairs, coef, lut=_lut(whole, dev), smean=ref.mean.to(dev), **bkw)
        assert_parity(s_sum.cpu().numpy(), s_whole.cpu().numpy(), what="pairs bands = whole sums", **ORDER)
        assert_parity(g_sum.cpu().numpy(), g_whole.cpu().numpy(), what="pairs bands = whole gradient", **ORDER)
        band = pr.band_of(_case("whole_13x17"), *pr.BAND)
        _check_forward(band, dev, rel, True)
        _check_backward(band, dev, rel)


@pytest.mark.parametrize("name", ["layout_12x20", "layout_13x17"])
def test_interleaved_explicit_std(dev, name):
    cs = _case(name)
    for rel in (True, False):
        planar_s = _check_forward(cs, dev, rel, True)
        planar_g = _check_backward(cs, dev, rel)
        for layout in ("nhwc", "nhwc_bgr"):
            s = _check_forward(cs, dev, rel, True, layout)
            g = _check_backward(cs, dev, rel, layout)
            assert_parity(s.cpu().numpy(), planar_s.cpu().numpy(), what=f"pairs {layout} = planar sums", **ORDER)
            assert_parity(g[0].cpu().numpy(), planar_g[0].cpu().numpy(), what=f"pairs {layout} = planar gradient", **ORDER)


@pytest.mark.parametrize("name", ["many_exposures", "narrow_std_only"])
def test_many_exposures_and_narrow_tiles(dev, name):
    cs = _case(name)
    _check_forward(cs, dev, True, True)
    _check_backward(cs, dev, True)


def test_edge_clamp_branch(dev):
    cs = _case("clamp")
    for rel in (True, False):
        _check_forward(cs, dev, rel, True)
        _check_backward(cs, dev, rel)


def test_edge_thresholds_and_knots(dev):
    cs = _case("thresholds")
    for rel in (True, False):
        _check_forward(cs, dev, rel, True)
        _check_backward(cs, dev, rel)


def test_edge_zero_residual(dev):
    from clair_torch_amd import ops
    cs = _case("equal_frames")
    for rel in (True, False):
        sums = _check_forward(cs, dev, rel, True)
        _check_backward(cs, dev, rel)
        ref = _reference(cs, rel, True, want_grad=False)
        p = int(torch.nonzero((ref.i == 3) & (ref.j == 4))[0])
        assert float(ref.ratio[p]) == 1.0 and not sums[p, :, 1].any() and float(sums[p, :, 4].min()) > 0
        stack, pairs, kw = _launch_args(cs, dev, rel, True)
        coef = torch.zeros((pairs.n_pairs, 3), dtype=torch.float64)
        coef[p] = 1.0   # that pair alone: v = 0 everywhere, sign(0) = 0 and (v - mean) = 0: no gradient at all
        g = ops.pair_residual_lut_grad(stack, pairs, coef.to(dev), lut=_lut(cs, dev), smean=ref.mean.to(dev), **kw)
        assert not g.any()


def test_edge_masked_huge_std(dev):
    cs = _case("masked_huge_std")
    for rel in (True, False):
        _check_forward(cs, dev, rel, True)
        _check_backward(cs, dev, rel)


def test_edge_zero_coef_channel(dev):
    """A coef that is zero for one channel: that channel's workgroups leave at once and it contributes nothing, the other
    channels' contributions are unchanged.  (The gradient ROW of that channel is not zero: the reference's LUT-row rule,
    flat index mod C, spreads every channel's samples over all rows -- so "nothing" is checked as additivity, exactly,
    and against the reference.)"""
    from clair_torch_amd import ops
    cs = _case("explicit_linear_f32_8x64")
    for rel in (True, False):
        ref = _reference(cs, rel, True)
        stack, pairs, kw = _launch_args(cs, dev, rel, True)
        coef = pr.seeded_coef(cs, pairs.n_pairs)

        def grad(cf):
            return ops.pair_residual_lut_grad(stack, pairs, cf.to(dev), lut=_lut(cs, dev), smean=ref.mean.to(dev), **kw)

        only = [grad(coef * torch.eye(3, dtype=torch.float64)[k]) for k in range(3)]
        zeroed = coef.clone()
        zeroed[:, 1] = 0.0
        part = grad(zeroed)
        assert torch.isfinite(part).all()
        want = pr.pair_step_f64(cs.x, cs.sd, cs.exposures, cs.lut, cs.interp, cs.threshold, cs.lo, cs.hi, rel, True, coef=zeroed)
        _par(part, want.grad_coef, "grad", f"{cs.name} zero coef channel")
        assert_parity(part.cpu().numpy(), (only[0] + only[2]).cpu().numpy(), what="pairs zero coef: channel 1 adds nothing", **ORDER)
        assert_parity((part + only[1]).cpu().numpy(), grad(coef).cpu().numpy(), what="pairs zero coef: the others unchanged", **ORDER)
        assert not grad(torch.zeros_like(coef)).any()


def test_refusals(dev):
    from clair_torch_amd import ops
    cs = _case("explicit_linear_f32_8x64")
    stack, pairs, kw = _launch_args(cs, dev, True, True)
    coef = pr.seeded_coef(cs, pairs.n_pairs).to(dev)
    smean = torch.ones((pairs.n_pairs, 3), dtype=torch.float64, device=dev)
    lut = _lut(cs, dev)
    for std_kw in (dict(std=kw["std"]), dict(std_mode="constant", std_value=0.01), dict(std_mode="multiplier", std_value=0.05)):
        lk = dict(kw, interp="lookup", std=None)
        lk.update(std_kw)
        with pytest.raises(RuntimeError, match="does not require grad"):
            ops.pair_residual_sums(stack, pairs, lut=lut, **lk)
        with pytest.raises(RuntimeError, match="does not require grad"):
            ops.pair_residual_lut_grad(stack, pairs, coef, lut=lut, smean=smean, **lk)
    with pytest.raises(ValueError, match="spatial means"):
        ops.pair_residual_lut_grad(stack, pairs, coef, lut=lut, **kw)
    for bad in (kw["std"][:, :, :-1].contiguous(), kw["std"][:-1].contiguous(), kw["std"][:, :2].contiguous()):
        with pytest.raises(ValueError, match="std shape"):
            ops.pair_residual_sums(stack, pairs, lut=lut, **dict(kw, std=bad))
        with pytest.raises(ValueError, match="std shape"):
            ops.pair_residual_lut_grad(stack, pairs, coef, lut=lut, smean=smean, **dict(kw, std=bad))


def test_api_explicit_and_constant_hint(dev):
    """measure_linearity and linearity_loss fed from a StackDataset through std_arguments: explicit std images, and a
    dataset that only carries std_hint = ("constant", 0.01)."""
    from clair_torch_amd import ops
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import measure_linearity
    from clair_torch_amd.inference._staging import std_arguments
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training import linearity_loss
    explicit, constant = _case("api_explicit"), _case("api_constant")
    sets = ((explicit, StackDataset(explicit.x, explicit.exposures, stds=explicit.sd)),
            (constant, StackDataset(constant.x, constant.exposures, missing_std_mode=MissingStdMode.CONSTANT,
                                    missing_std_value=pr.STD_CONSTANT, materialize_std=False)))
    for cs, ds in sets:
        loader = DataLoader(ds, batch_size=len(ds), shuffle=False, collate_fn=custom_collate)
        mode = InterpMode.CATMULL if cs.interp == "catmull" else InterpMode.LINEAR
        model = ICRFModelDirect(icrf=cs.lut.clone(), interpolation_mode=mode).to(dev)
        # measure_linearity's own thresholds: ratio >= 0.2, [1/255, 254/255]
        assert (cs.threshold, cs.lo, cs.hi) == (0.2, 1 / 255, 254 / 255)
        ref = _reference(cs, True, True)
        ratio, mean, sd, err = measure_linearity(loader, "cuda", True, True, model)
        assert torch.equal(ratio.cpu(), ref.ratio)
        _par(mean, ref.mean, "mean", f"{cs.name} measure_linearity")
        # the centered pass runs around the kernel's own mean: second order in the mean's error
        _par(sd, ref.std, "std", f"{cs.name} measure_linearity")
        _par(err, ref.err, "err", f"{cs.name} measure_linearity")
        _, val_batch, std_batch, _ = next(iter(loader))
        std, std_mode, std_value = std_arguments(std_batch, ds, dev)
        assert std_mode == cs.smode and (std is None) == (cs.smode != "explicit")
        i, j, r = pr.exposure_pairs(cs.exposures, cs.threshold)
        pairs = ops.PairList(i, j, r, len(ds), dev)
        lut = cs.lut.to(dev).requires_grad_(True)
        lin, sp = linearity_loss(lut, val_batch.to(dev), pairs, interp=cs.interp, lower=cs.lo, upper=cs.hi, use_relative=True,
                                 use_unc_weight=True, std=std, std_mode=std_mode, std_value=std_value, group=False)
        _par(lin, ref.linloss, "linloss", f"{cs.name} linearity_loss via std_arguments")
        _par(torch.autograd.grad(lin.sum(), lut)[0].double(), ref.grad_lin, "grad", f"{cs.name} linearity_loss via std_arguments")
