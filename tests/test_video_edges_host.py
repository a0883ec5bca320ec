"""The inputs, the unit and the bounds of tests/_video_edge_cases.py, on the CPU.

The bounds of tests/test_gpu_video_edges.py are measured here: oracle.eager_torch.video_mean_std (the reference's own float32
arithmetic) against float64 on every case, the worst error in u per family; _video_edge_cases.MEASURED records it, BOUND is 4x
that with a floor of 1 u.  A bound is worth having only if it catches something: two wrong float32 algorithms (one-pass m2, a
merge without its delta^2 term) must exceed it on every low-variance family.  Run with -s to see the figures."""
import numpy as np
import pytest
import torch

import _video_edge_cases as ve
from oracle import eager_torch as oe


def linearize(x, lut, mode):
    return x if mode is None else oe.icrf_forward(torch.from_numpy(x), torch.from_numpy(lut), mode).numpy()


def oracle(x, lut, mode, sched):
    mean, std = oe.video_mean_std(torch.from_numpy(x), None if mode is None else torch.from_numpy(lut), mode, list(sched))
    return mean.numpy(), std.numpy()


def _ref(case):
    return ve.reference(case, linearize, oracle)


FAMILIES = sorted(ve.MEASURED)


def _family(f):
    return [c for c in ve.CASES if c.family == f]


def test_case_table_covers_every_walk():
    """Every walk (cached 16, cached 32, two passes, several batches with BMAX 16 / 32) meets every interpolation and every
    dtype, every interpolation every dtype; every family every schedule it is defined on; names are unique."""
    walks = {"cached16", "cached32", "twopass", "multi16", "multi32"}
    dtypes = {"u8", "u16", "f32"}
    assert len({c.name for c in ve.CASES}) == len(ve.CASES)
    assert {c.family for c in ve.CASES} == set(FAMILIES) == set("ABCDEFG")
    assert {(w, c.mode) for c in ve.CASES for w in ve.walks_of(c.sched)} == {(w, m) for w in walks for m in ve.MODES}
    assert {(w, c.dtype) for c in ve.CASES for w in ve.walks_of(c.sched)} == {(w, d) for w in walks for d in dtypes}
    assert {(c.mode, c.dtype) for c in ve.CASES} == {(m, d) for m in ve.MODES for d in dtypes}
    assert {c.shape for c in ve.CASES} == set(ve.SHAPES)
    for f in "ACDE":
        assert {c.sched for c in _family(f)} == set(ve.SCHEDULES), f
    assert {c.sched for c in _family("G")} == set(ve.LONG_SCHEDULES)
    assert all(sum(c.sched) == (256 if c.family == "G" else 64) for c in ve.CASES if c.family != "F")
    # A: every variant on every schedule; uint16 at both max codes
    assert {(c.dtype, c.max_code, c.arg, c.sched) for c in _family("A")} == {v + (s,) for v in ve.A_VARIANTS for s in ve.SCHEDULES}
    # B: the step in the first, in the last and in a middle batch of (3, 5, 7, 11, 13, 25)
    ragged = ve.SCHEDULES[4]
    batch_of = np.repeat(np.arange(len(ragged)), ragged)
    assert {int(batch_of[c.arg]) for c in _family("B") if c.sched == ragged} >= {0, 3, len(ragged) - 1}
    # F: every count of frames before with every walk
    assert {(c.arg, c.sched) for c in _family("F")} == {(b, (n,)) for b in (1, 1000, 2 ** 24) for n in (4, 17, 33)}
    # a schedule never asks one call for more batches than it takes
    assert all(len(part) <= ve.MAX_BATCHES for c in ve.CASES for _, part in ve.chunks(c.sched))


def test_input_conditions():
    """With the reference alone: A, B and G have a float64 std above 0 everywhere and std / mean in the family's range; C has
    a float64 std of exactly 0; every pixel of every case is compared (a finite reference and unit, or one of E's marked
    non-finite pixels)."""
    for case in ve.CASES:
        r = _ref(case)
        n = r.inp.frames_before + sum(case.sched)
        marked = np.zeros(case.shape, dtype=bool)
        for idx in r.inp.special:
            marked[idx] = True
        finite = np.isfinite(r.mean64) & np.isfinite(r.std64) & np.isfinite(r.u)
        assert np.array_equal(finite, ~marked), case.name
        assert len(r.inp.special) == (3 if case.kind == "nonfinite" else 0)
        assert r.inp.x.shape == (sum(case.sched),) + case.shape and r.inp.x.dtype == np.float32
        if case.family in ve.LOW_VARIANCE:
            lo, hi = ve.RATIO_RANGE[case.family]
            ratio = r.std64 * np.sqrt(n) / r.mean64
            assert r.std64.min() > 0 and lo < ratio.min() and ratio.max() < hi, (case.name, ratio.min(), ratio.max())
        if case.family == "C":
            assert np.all(r.std64 == 0), case.name
            assert np.any(r.u == 0) and np.any(r.inp.x == 0) and np.any(r.inp.x == 1)
            if case.max_code == 4095:
                assert np.any(r.inp.x > 1)              # above max_code: clamps to the top of the LUT
        if case.family == "D":
            x = r.inp.x
            assert np.all((x == 0) | (x == 1)) and np.all(x.min(axis=0) == 0) and np.all(x.max(axis=0) == 1)
        if case.kind == "range":
            assert r.inp.x.min() < 0 and r.inp.x.max() > 1
        if case.family == "F":
            assert r.inp.frames_before == case.arg and r.mean0.dtype == np.float32 and r.m20.dtype == np.float32
    # B: but for one frame, every frame of a pixel is the same
    for case in _family("B"):
        x = _ref(case).inp.x
        rest = np.delete(x, case.arg, axis=0)
        assert np.all(rest == rest[0]) and np.all(x[case.arg] > rest[0])


def _measure(case, mean, std):
    r = _ref(case)
    em, es = ve.worst_errors(r, mean, std)
    return float(em.max()), float(es.max())


def test_bounds_from_the_eager_oracle():
    """The reference's own float32 arithmetic against float64, per family: no worse than recorded, and the bounds are 4x the
    record with a floor of 1 u.  On E's non-finite pixels the reference is non-finite too."""
    for f in FAMILIES:
        worst_m = worst_s = 0.0
        for case in _family(f):
            r = _ref(case)
            em, es = _measure(case, r.mean_o, r.std_o)
            worst_m, worst_s = max(worst_m, em), max(worst_s, es)
            for idx in r.inp.special:
                assert not np.isfinite(r.mean_o[idx]) and np.isnan(r.std_o[idx]), (case.name, idx)
            assert not np.isnan(np.where(np.isfinite(r.mean64), r.std_o, 0.0)).any(), case.name
        print(f"video edges {f}: float32 reference against float64: mean {worst_m:.4g} u, std {worst_s:.4g} u; "
              f"recorded {ve.MEASURED[f]}, bound {ve.BOUND[f]}")
        assert worst_m <= ve.MEASURED[f][0] and worst_s <= ve.MEASURED[f][1], (f, worst_m, worst_s)
        # the record is not padded either: it is what was measured, rounded up in the third digit
        assert worst_m > 0.98 * ve.MEASURED[f][0] - 1e-3 and worst_s > 0.98 * ve.MEASURED[f][1] - 1e-3, (f, worst_m, worst_s)
        assert ve.BOUND[f] == (max(1.0, 4 * ve.MEASURED[f][0]), max(1.0, 4 * ve.MEASURED[f][1]))


def test_float32_restatement_is_the_eager_oracle():
    """stream_f32 (F's float32 reference, and the base of the wrong algorithms below) is the reference's arithmetic: from an
    empty state it is within a rounding or two of oe.video_mean_std (torch may associate a batch's sum differently)."""
    for case in ve.CASES:
        if case.family == "F" or case.kind == "nonfinite":
            continue
        r = _ref(case)
        mean, std = ve.stream_f32(r.x_lin, case.sched)
        em, es = _measure(case, mean, std)
        assert em <= ve.BOUND[case.family][0] and es <= ve.BOUND[case.family][1], (case.name, em, es)


@pytest.mark.parametrize("wrong", ["one_pass", "drop_delta"])
def test_bounds_reject_wrong_algorithms(wrong):
    """m2 of a batch as sum x^2 - n mean^2, and a merge that drops (W_A W_B / W) delta^2, in float32 on the same inputs: each
    exceeds the std bound of every low-variance family."""
    for f in ve.LOW_VARIANCE:
        worst = 0.0
        for case in _family(f):
            r = _ref(case)
            mean, std = ve.stream_f32(r.x_lin, case.sched, **{wrong: True})
            worst = max(worst, _measure(case, mean, std)[1])
        print(f"video edges {f}: {wrong}: std off by {worst:.4g} u (bound {ve.BOUND[f][1]:.4g})")
        assert worst > ve.BOUND[f][1], (f, wrong, worst)


def test_unit_and_errors():
    x = np.zeros((4, 1, 1, 3))
    x[:, 0, 0, 1] = (0.5, -2.0, 1.0, 0.25)
    x[2, 0, 0, 2] = np.nan
    u = ve.unit(x)
    assert u[0, 0, 0] == 0 and u[0, 0, 1] == 2.0 ** -23 and np.isnan(u[0, 0, 2])
    ref = np.array([[[0.0, 1.0, np.nan]]])
    assert np.array_equal(ve.errors_in_u(ref, ref, u), np.zeros((1, 1, 3)))
    got = np.array([[[1e-30, 1.0 + 3 * 2.0 ** -23, 5.0]]])
    err = ve.errors_in_u(got, ref, u)
    assert err[0, 0, 0] == np.inf and err[0, 0, 1] == 3.0 and err[0, 0, 2] == 0.0
    assert ve.errors_in_u(np.array([[[0.0, np.nan, 0.0]]]), ref, u)[0, 0, 1] == np.inf
    # the float64 merge of stats_f64 is the float64 statistics of the whole stream
    rng = np.random.default_rng(3)
    y = rng.random((12, 2, 2, 2))
    m_a, s_a = ve.stats_f64(y[:5])
    m2_a = (s_a * np.sqrt(5)) ** 2 * 4
    m, s = ve.stats_f64(y[5:], 5, m_a, m2_a)
    m_w, s_w = ve.stats_f64(y)
    assert np.allclose(m, m_w, rtol=1e-14, atol=0) and np.allclose(s, s_w, rtol=1e-13, atol=0)
