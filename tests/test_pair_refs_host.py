"""The float64 reference of tests/_pair_refs.py against the recorded vectors and the float32 eager oracle, on the CPU.

This is also where the tolerances of tests/test_gpu_pairs_uncertainty.py are measured: the float32 eager oracle
(oracle/eager_torch, the reference project's order of operations) is compared with the float64 reference on the very
inputs the GPU test uses, and every entry of _pair_refs.TOL must hold 4x the worst deviation seen, in both measures of
_util.assert_parity.  Run with -s to see the measured figures."""
import numpy as np
import pytest
import torch

import _pair_refs as pr
from _util import assert_parity, golden, rel_norm
from oracle import ct_oracle as oc
from oracle import eager_torch as oe


def _elem_err(got, ref):
    """Worst element error in the metric of _util.assert_parity."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.abs(got - ref) / (np.abs(ref) + np.median(np.abs(ref)))))


def combos(name):
    """(use_relative, use_unc_weight) the GPU test runs on a case: all four on the matrix (the forward meets the weight
    switched off), both residuals on the rest, the relative one alone on the two large stacks."""
    if name in ("many_exposures", "narrow_std_only"):
        return [(True, True)]
    if name in {m[0] for m in pr.matrix_cases()}:
        return [(True, True), (True, False), (False, True), (False, False)]
    return [(True, True), (False, True)]


def all_cases():
    for name in pr.GENERAL_CASES:
        cs = pr.build_case(name)
        yield cs
        if name == "whole_13x17":
            yield pr.band_of(cs, *pr.BAND)


@pytest.fixture(scope="module")
def measured():
    """name -> {(rel, unc): (reference, eager figures)} for every case, computed once."""
    out = {}
    for cs in all_cases():
        out[cs.name] = (cs, {})
        for rel, unc in combos(cs.name.split("_band")[0]):
            coef = pr.seeded_coef(cs, pr.exposure_pairs(cs.exposures, cs.threshold)[0].numel())
            ref = pr.pair_step_f64(cs.x, cs.sd, cs.exposures, cs.lut, cs.interp, cs.threshold, cs.lo, cs.hi, rel, unc,
                                   coef=coef, h_global=cs.h_global, row_offset=cs.row_offset, want_grad=unc)
            t = torch.tensor(cs.exposures, dtype=torch.float64)
            _, sp, sp_std, sp_err = oe.linearity_statistics(cs.x, cs.sd, t, cs.lut, cs.interp, cs.threshold, cs.lo, cs.hi,
                                                            rel, unc)
            s0, s1, s3 = pr.eager_sums_f32(cs.x, cs.sd, cs.exposures, cs.lut, cs.interp, cs.threshold, cs.lo, cs.hi, rel, unc)
            eager = dict(den=s0.clamp(min=1e-8), num=s1, mean=sp.detach(), std=sp_std.detach(), err=sp_err.detach(),
                         errsum=s3, linloss=torch.sqrt((sp.detach() ** 2).sum(dim=0)))
            if ref.grad_lin is not None:
                _, _, eager["grad"], eager["grad_coef"] = pr.eager_grads_f32(
                    cs.x, cs.sd, cs.exposures, cs.lut, cs.interp, cs.threshold, cs.lo, cs.hi, rel, unc, coef * ref.den)
            out[cs.name][1][(rel, unc)] = (ref, eager)
    return out


def test_matrix_is_pairwise():
    """Every std mode meets every interp, dtype and plane; every interp every dtype and plane; every dtype every plane."""
    cases = pr.matrix_cases()
    assert len({m[0] for m in cases}) == len(cases)
    axes = (pr.STD_MODES, pr.INTERPS, pr.DTYPES, pr.PLANES)
    for a in range(4):
        for b in range(a + 1, 4):
            assert {(m[1 + a], m[1 + b]) for m in cases} == {(u, v) for u in axes[a] for v in axes[b]}, (a, b)


def test_reference_reproduces_golden_training_vectors():
    """tests/golden/training.npz at the tolerances tests/test_gpu_training.py holds the kernels to."""
    g = golden("training")
    x = torch.from_numpy(oc.normalize_codes(g["train_codes"]))
    sd = pr.std_stack("multiplier", x)
    lut = torch.from_numpy(g["train_lut0"])
    for mode in ("linear", "catmull"):
        for rel in (True, False):
            for unc in (True, False):
                ref = pr.pair_step_f64(x, sd, g["train_exposures"], lut, mode, 0.25, 1 / 255, 254 / 255, rel, unc, want_grad=unc)
                key = f"train_multiplier_{mode}_{'rel' if rel else 'abs'}_{'unc' if unc else 'nounc'}"
                assert np.array_equal(ref.sums[..., 4].numpy(), g["train_multiplier_mask_popcount"].astype(np.float64))
                assert_parity(g[key + "_spatial"], ref.mean.numpy(), rtol=1e-5, norm_tol=2e-6, what=key + " mean")
                assert_parity(g[key + "_spatial_std"], ref.std.numpy(), rtol=1e-5, norm_tol=2e-6, what=key + " std")
                assert_parity(g[key + "_spatial_err"], ref.err.numpy(), rtol=1e-5, norm_tol=2e-6, what=key + " err")
                if unc:
                    assert_parity(g[key + "_linloss"], ref.linloss.numpy(), rtol=1e-5, norm_tol=2e-6, what=key + " linloss")
                    assert_parity(g[key + "_lingrad"], ref.grad_lin.numpy(), norm_tol=2e-6, elem_tol=1e-5, what=key + " lingrad")


def test_restated_sums_are_the_eager_oracles(measured):
    """eager_sums_f32 is oe.linearity_statistics' own arithmetic: its quotients equal the oracle's output bit for bit."""
    for name, (cs, runs) in measured.items():
        for key, (ref, eager) in runs.items():
            assert torch.equal(eager["num"] / eager["den"], eager["mean"]), (name, key)
            n_valid = ref.sums[..., 4].clamp(min=1e-8).to(eager["errsum"].dtype)
            assert torch.equal(eager["errsum"] / n_valid, eager["err"]), (name, key)


def test_tolerances_hold_four_times_the_eager_oracles_deviation(measured):
    worst = {q: [0.0, 0.0, None, None] for q in pr.TOL}
    for name, (cs, runs) in measured.items():
        for key, (ref, eager) in runs.items():
            pairs = [("den", ref.den), ("num", ref.sums[..., 1]), ("mean", ref.mean), ("std", ref.std), ("err", ref.err),
                     ("errsum", ref.sums[..., 3]), ("linloss", ref.linloss)]
            if "grad" in eager:
                pairs += [("grad", ref.grad_lin), ("grad_coef", ref.grad_coef)]
            for q, want in pairs:
                got = eager[q].double().numpy()
                e, nrm = _elem_err(got, want.numpy()), rel_norm(got, want.numpy())
                slot = worst["grad" if q == "grad_coef" else q]
                if e > slot[0]:
                    slot[0], slot[2] = e, (name, key)
                if nrm > slot[1]:
                    slot[1], slot[3] = nrm, (name, key)
    for q, (e, nrm, at_e, at_n) in worst.items():
        print(f"pairs: float32 eager oracle against float64: {q:8s} element {e:.3e} {at_e}  norm-wise {nrm:.3e} {at_n}")
    for q, (e, nrm, at_e, at_n) in worst.items():
        assert e * 4 <= pr.TOL[q][0] and nrm * 4 <= pr.TOL[q][1], (q, e, at_e, nrm, at_n)


def test_case_conditions(measured):
    for name, (cs, runs) in measured.items():
        for key, (ref, eager) in runs.items():
            for q, v in eager.items():
                assert torch.isfinite(v).all(), (name, key, q)
            assert float(ref.sums[..., 4].min()) >= 1, (name, key, "a (pair, channel) without a valid pixel")
            small = ref.valid & (ref.resid < pr.RESIDUAL_BOUND)
            if cs.keep_zero is not None:
                assert (ref.resid[cs.keep_zero] == 0).all() and (ref.valid & cs.keep_zero).sum() > 100
                small &= ~cs.keep_zero
            if name == "clamp":   # the flat foot of its curve: both values exactly 0, in every precision
                small &= ~ref.both_zero
            assert not small.any(), (name, key, int(small.sum()))
            if cs.interp is not None:   # no valid sample sits on the float32 tie of clamp(I_j, 1e-6)
                used = torch.zeros(cs.x.shape, dtype=torch.bool)
                used[ref.j] |= ref.valid
                assert not (used & ((ref.lin / 1e-6 - 1).abs() < pr.CLAMP_GAP)).any(), (name, key)
    # the edge cases reach what they are for
    ref = measured["clamp"][1][(True, True)][0]
    below = torch.zeros(ref.lin.shape, dtype=torch.bool)
    below[ref.j] |= ref.valid
    below &= ref.lin < 1e-6
    assert int(below.sum()) > 50 and int((below & (ref.lin > 0)).sum()) > 5, "the clamp branch needs valid partners below 1e-6"
    cs = measured["masked_huge_std"][0]
    assert int((cs.sd == pr.HUGE_STD).sum()) > 100
    cs = measured["thresholds"][0]
    assert float(cs.x.min()) == 0.0 and float(cs.x.max()) == 1.0


def test_narrow_tile_case_follows_pick_tile():
    """The STD backward of "narrow_std_only" takes 32 columns where the plain backward takes 64; "many_exposures" takes 32
    either way (csrc/ct_pairs.hip: pick_tile, bwd_launch_once; 8 bytes per LINEAR LUT entry)."""
    assert pr.pick_tile_columns(pr.NARROW_N, pr.NARROW_L, 3, with_std=True) == 32
    assert pr.pick_tile_columns(pr.NARROW_N, pr.NARROW_L, 3, with_std=False) == 64
    assert pr.pick_tile_columns(128, 32, 3, with_std=True) == 32
    cs = pr.build_case("narrow_std_only")
    assert len(cs.exposures) == pr.NARROW_N and cs.lut.shape[1] == pr.NARROW_L and cs.interp == "linear"
    i, _, _ = pr.exposure_pairs(pr.build_case("many_exposures").exposures, None)
    assert i.numel() == 8128 > 4 * 256   # more pairs than one forward launch walks
    # base geometry: between 0 and 4 i-side partners per sample (the kGroup = 4 body and its tail)
    i, _, _ = pr.exposure_pairs(pr.base_exposures(), 0.25)
    assert sorted(set(torch.bincount(i, minlength=9).tolist())) == [0, 1, 2, 3, 4]
