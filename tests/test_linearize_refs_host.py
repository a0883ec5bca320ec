"""The float64 references of tests/_linearize_refs.py against the pinned float32 oracles, on the CPU.

This is also where the tolerances of tests/test_gpu_linearize_paths.py are measured: the float32 oracles (oc.linearize_std,
oc.icrf_forward; autograd of oe.icrf_forward for the backward) are compared with the float64 references on the very inputs
the GPU test uses, bands included, and every entry of _linearize_refs.TOL must hold 4x the worst deviation seen, in both
measures of _util.assert_parity.  Run with -s to see the measured figures."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import _linearize_refs as lr
from _util import rel_norm
from oracle import ct_oracle as oc

ALL_NAMES = [c[0] for c in lr.ALL_FORWARD]


def _elem_err(got, ref):
    """Worst element error in the metric of _util.assert_parity (0 for two all-zero arrays)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    den = np.abs(ref) + np.median(np.abs(ref))
    err = np.abs(got - ref)
    return float(np.max(np.where(err == 0, 0.0, err / np.where(den == 0, 1.0, den))))


def oracle_forward(cs, band):
    """(lin, std | None) of the float32 oracle on the band (or the whole image) of a forward case."""
    x = lr.band_rows(cs.x, cs) if band else cs.x
    sg = lr.band_rows(cs.sigma, cs) if band else cs.sigma
    tile = cs.tile if band else None
    lin, sd = oc.linearize_std(x, sg, cs.lut, "nomodel" if cs.mode is None else cs.mode, tile=tile)
    return lin, (None if cs.std == "nostd" else sd)


@pytest.fixture(scope="module")
def forward_runs():
    """[(case, band?, float64 (lin, std), oracle (lin, std))] for the band and the whole image of every forward case."""
    out = []
    for name in ALL_NAMES:
        cs = lr.forward_case(name)
        for band in ((True, False) if cs.tile is not None else (True,)):
            x = lr.band_rows(cs.x, cs) if band else cs.x
            sg = lr.band_rows(cs.sigma, cs) if band else cs.sigma
            out.append((cs, band, lr.linearize_f64(x, sg, cs.lut, cs.mode, cs.tile if band else None), oracle_forward(cs, band)))
    return out


@pytest.fixture(scope="module")
def backward_runs():
    """[(case, label, float64 (grad_x, lut_grad), eager (grad_x, lut_grad))] for the whole and both bands of every case."""
    out = []
    for name in lr.BACKWARD_NAMES:
        cs = lr.backward_case(name)
        for label, r0, rows, tile in lr.backward_bands(cs):
            ref = lr.icrf_backward_f64(cs.x[:, :, r0:r0 + rows], cs.grad_out[:, :, r0:r0 + rows], cs.lut, cs.mode, tile)
            out.append((cs, label, ref, lr.eager_backward(cs, r0, rows)))
    return out


def test_references_agree_with_the_oracles(forward_runs, backward_runs):
    for cs, band, (lin, sd), (lin_o, sd_o) in forward_runs:
        what = f"{cs.name} {'band' if band else 'whole'}"
        lr.check(lin_o, lin, ("lin", cs.mode), what + " lin")
        if sd_o is not None:
            lr.check(sd_o, sd, ("std", cs.mode), what + " std")
    for cs, label, (gx, gl), (gx_o, gl_o) in backward_runs:
        what = f"{cs.name} {label}"
        if cs.kind == "plain":      # (the flush cases: see test_tolerances_hold_four_times_the_oracles_deviation)
            lr.check(gl_o, gl, ("lut_grad", cs.mode), what + " lut_grad")
        if gx_o is not None:
            lr.check(gx_o, gx, ("grad_x", cs.mode), what + " grad_x")
        else:
            assert not gx.any()


def test_tolerances_hold_four_times_the_oracles_deviation(forward_runs, backward_runs):
    worst = {q: [0.0, 0.0, None, None] for q in lr.TOL}

    def note(q, got, want, at):
        e, nrm = _elem_err(got, want), (rel_norm(got, want) if np.any(want) or np.any(got) else 0.0)
        slot = worst[q]
        if e > slot[0]:
            slot[0], slot[2] = e, at
        if nrm > slot[1]:
            slot[1], slot[3] = nrm, at

    for cs, band, (lin, sd), (lin_o, sd_o) in forward_runs:
        note(("lin", cs.mode), lin_o, lin, (cs.name, band))
        if sd_o is not None:
            note(("std", cs.mode), sd_o, sd, (cs.name, band))
    for cs, label, (gx, gl), (gx_o, gl_o) in backward_runs:
        # The cases built to load the flush (hot, cancel, untouched) are not compared at TOL[("lut_grad", mode)] on the GPU
        # (flush_keeps_margin), and the oracle is no yardstick for them: its one sequential float32 scatter-add puts
        # thousands of terms into a hot bin.  They are held to order_bound; TOL keeps the inputs it was measured on.
        if cs.kind == "plain":
            note(("lut_grad", cs.mode), gl_o, gl, (cs.name, label))
        else:
            assert not lr.flush_keeps_margin(cs.name)
        if gx_o is not None:
            note(("grad_x", cs.mode), gx_o, gx, (cs.name, label))
    for q, (e, nrm, at_e, at_n) in worst.items():
        print(f"linearize: float32 oracle against float64: {str(q):24s} element {e:.3e} {at_e}  norm-wise {nrm:.3e} {at_n}")
    for q, (e, nrm, at_e, at_n) in worst.items():
        assert e * 4 <= lr.TOL[q][0] and nrm * 4 <= lr.TOL[q][1], (q, e, at_e, nrm, at_n)


def test_band_rule_is_exact():
    """The reference on a band with its tile equals the rows of the reference on the whole image, bit for bit; without
    the tile it does not (so the comparison can tell)."""
    told = 0
    for name in lr.FORWARD_NAMES:
        cs = lr.forward_case(name)
        if cs.tile is None:
            continue
        whole = lr.linearize_f64(cs.x, cs.sigma, cs.lut, cs.mode)
        band = lr.linearize_f64(lr.band_rows(cs.x, cs), lr.band_rows(cs.sigma, cs), cs.lut, cs.mode, cs.tile)
        for a, b in zip(whole, band):
            assert np.array_equal(lr.band_rows(a, cs), b), name
        if cs.mode in ("linear", "catmull") and cs.C > 1:
            plain = lr.linearize_f64(lr.band_rows(cs.x, cs), lr.band_rows(cs.sigma, cs), cs.lut, cs.mode)
            told += not np.array_equal(plain[0], band[0])
            assert not np.array_equal(lr.lut_rows(cs.C, cs.h, cs.w, cs.mode), lr.lut_rows(cs.C, cs.h, cs.w, cs.mode, cs.tile)), name
    assert told >= 10
    for name in lr.BACKWARD_NAMES:
        cs = lr.backward_case(name)
        gx_w, gl_w = lr.icrf_backward_f64(cs.x, cs.grad_out, cs.lut, cs.mode)
        total = np.zeros_like(gl_w)
        for label, r0, rows, tile in lr.backward_bands(cs)[1:]:
            gx, gl = lr.icrf_backward_f64(cs.x[:, :, r0:r0 + rows], cs.grad_out[:, :, r0:r0 + rows], cs.lut, cs.mode, tile)
            assert np.array_equal(gx, gx_w[:, :, r0:r0 + rows]), (name, label)
            total += gl
        scale = lr.icrf_backward_f64(cs.x, cs.grad_out, cs.lut, cs.mode, absolute=True)[1]
        assert np.all(np.abs(total - gl_w) <= cs.x.size * 2.0 ** -53 * scale), name   # two orders of one float64 sum


def test_every_path_is_reached_with_every_mode_dtype_and_std():
    seen = {}
    for name in ALL_NAMES:
        cs = lr.forward_case(name)
        slot = seen.setdefault(lr.case_path(cs), dict(mode=set(), dtype=set(), std=set(), band=0))
        slot["mode"].add(cs.mode)
        slot["dtype"].add(cs.dtype)
        slot["std"].add("none" if cs.std == "nostd" else cs.std)
        slot["band"] += cs.r0 > 0 and cs.hg > cs.h
    # "planar+tail" has no inputs: see test_planar_tail_and_planar_packets_of_eight_are_unreachable
    assert set(seen) == set(lr.PATHS) - {"planar+tail"}
    for path, slot in seen.items():
        assert slot["mode"] == {None, "lookup", "linear", "catmull"}, path
        assert slot["dtype"] == {"u8", "u16", "f32"}, path
        assert slot["std"] == {"none", "constant", "multiplier"} | (set() if path == "rgb" else {"explicit"}), (path, slot["std"])
        assert slot["band"] >= 1, path
    # both std-less forms (no output / CT_STD_NONE) and both interleaved orders reach the rgb kernel
    rgb = [lr.forward_case(n) for n in ALL_NAMES if lr.case_path(lr.forward_case(n)) == "rgb"]
    assert {c.std for c in rgb} >= {"nostd", "none"} and {c.layout for c in rgb} == {"nhwc", "nhwc_bgr"}
    # planar frames never form packets of eight: behind a padded stride of 8 k with Q % 4 != 0 they go element by element
    pads = [lr.forward_case(n) for n in ALL_NAMES if n.startswith("sc_band_pad_")]
    assert len(pads) == 2 and all(c.layout == "nchw" and (c.C * c.h * c.w + c.pad) % 8 == 0 and (c.C * c.h * c.w) % 4 != 0
                                  and c.F > 1 and lr.case_path(c) == "scalar" for c in pads)


def test_planar_tail_and_planar_packets_of_eight_are_unreachable():
    """lin_typed launches the planar kernel only with out_stride % 4 == 0, and ct_linearize_std sets out_stride = Q: the
    tail launch behind it (Q % 4 != 0) has no inputs.  And linearize_kernel<8> never sees planar frames, whatever the
    pointers and strides: its packet stores would sit at f * Q + q0, 4-byte aligned only for Q % 4 != 0."""
    for dtype, C, plane, std, a, pad in itertools.product(("u8", "u16", "f32"), (1, 2, 3, 4), range(1, 41), ("none", "explicit"),
                                                          (0, 4, 16), (0, 1, 3, 4, 8)):
        Q = C * plane
        al = {"frames": a, "lin": 0, "std_out": 0}
        path = lr.linearize_path_of(dtype, "nchw", C, plane, Q, 2, std, al, (Q + pad, Q))
        assert path in ("planar", "scalar"), (dtype, C, plane, a, pad)
        assert (path == "planar") == (Q % 4 == 0 and pad % 4 == 0 and a % (4 * lr.ITEMSIZE[dtype]) == 0), (dtype, C, plane, a, pad)
    # the restatement itself knows the tail (an output stride that ct_linearize_std never forms)
    assert lr.linearize_path_of("u8", "nchw", 1, 7, 7, 1, "none", {}, (8, 8)) == "planar+tail"


def test_shapes_reach_the_edges_they_are_for():
    for name in lr.FORWARD_NAMES:
        cs = lr.forward_case(name)
        for edge, held in lr.case_edges(cs).items():
            assert held or not lr.edge_applies(cs, edge), (name, edge)
    # the exceptions are the listed ones and no others: each has a std, no underflowing sample, and the stated reason
    for name in lr.NO_UNDERFLOW:
        cs = lr.forward_case(name)
        assert lr.case_edges(cs)["underflow"] is False, name
        assert (cs.mode is None and (cs.std == "constant" or cs.dtype != "f32")) or \
            (cs.mode == "catmull" and cs.std == "multiplier" and cs.dtype != "f32"), name
    for name in lr.BACKWARD_NAMES:
        cs = lr.backward_case(name)
        for lo, hi in ((0, cs.split), (cs.split, cs.hg)):
            x = cs.x[:, :, lo:hi]
            if cs.kind == "untouched":      # the one case whose x is confined: bins outside [0.3, 0.6] stay empty
                assert x.min() >= np.float32(0.3) and x.max() <= np.float32(0.6), name
                continue
            assert (x == 0).any() and (x == 1).any() and (x < 0).any() and (x > 1).any(), name
    # row bands: the geometry terms of the LUT row are no multiples of C
    for name in lr.FORWARD_NAMES:
        cs = lr.forward_case(name)
        if cs.tile is not None and cs.C > 1 and name.split("_")[1] == "band":
            assert ((cs.hg - cs.h) * cs.w) % cs.C != 0 or (cs.r0 * cs.w) % cs.C != 0, name
    rgb_bands = [lr.forward_case(n) for n in lr.FORWARD_NAMES if n.startswith("rgb_band")]
    assert {(c.hg * c.w) % 3 for c in rgb_bands} >= {1, 2} and all((c.r0 * c.w) % 3 != 0 for c in rgb_bands[:3])
    # planar: packet counts around one and two strides of a workgroup (256 threads x 3 packets), straddled planes
    packets = {n: lr.forward_case(n).C * lr.forward_case(n).h * lr.forward_case(n).w // 4 for n in lr.FORWARD_NAMES if n.startswith("pl_")}
    assert packets["pl_c1_4x257_u8"] == 257 and packets["pl_c4_27x19_u16"] == 513 and packets["pl_c1_4x1025_f32"] == 768 + 257
    assert (27 * 19) % 2 == 1 and (86 * 3) % 4 == 2
    assert lr.frame_walk_of(lr.MANY_FRAMES_N) == (65535, 3) and lr.frame_walk_of(3) == (2, 2)


def test_backward_grids():
    grids = {n: lr.bwd_grid_of(lr.backward_case(n).C * lr.backward_case(n).hg * lr.backward_case(n).w, lr.backward_case(n).N,
                               lr.backward_case(n).C, lr.backward_case(n).L, lr.backward_case(n).mode, 256) for n in lr.BACKWARD_NAMES}
    g = grids["bw_repeat_linear_c3"]
    assert g.repeats and g.slots == 1 and (g.gx, g.gy) == (32, 8)
    assert not any(v.repeats for n, v in grids.items() if n != "bw_repeat_linear_c3")
    assert {v.image_rounds for n, v in grids.items() if lr.BACKWARD_KIND[n] == "plain"} == {1, 2}
    assert lr.BACKWARD_NAMES.index("bw_repeat_linear_c3") == 9      # (the seeds of the cases follow their positions)
    cases = [lr.backward_case(n) for n in lr.BACKWARD_NAMES[:9]]
    assert {(c.mode, c.C) for c in cases} == set(itertools.product(("lookup", "linear", "catmull"), (1, 3, 4)))
    assert all({c.N for c in cases if c.mode == m} == {1, 8, 11} for m in ("lookup", "linear", "catmull"))


# ---- the flush of the LUT gradient: linearize_bwd_kernel's summation restated, and every order of its float32 atomics ----
# The study below (flush_study) takes about 4 s on one CPU core: 13 + 24 + 8 + 6 orders of at most 256 float32 adds over at
# most 3 x 2048 bins, for the whole image and both bands of the 15 backward cases.
CUS = 256                      # compute units of the MI355X: the grid the GPU test meets (it asserts 256 for the capped case)
N_GLOBAL, N_BIN = 24, 8        # seeded random orders: of the workgroups (one order for all bins), and per bin


def flush_orders(parts, rng):
    """(name, order) of the study: ascending workgroups, random orders, and per bin the adversarial ones -- positive
    partials first then negative, ascending magnitude, descending value (positive descending, then negative by growing
    magnitude: the largest running sums) -- and the reverse of each."""
    p = parts.partials
    yield "ascending", np.arange(p.shape[0])
    yield "descending", np.arange(p.shape[0])[::-1]
    for k in range(N_GLOBAL):
        yield f"workgroups#{k}", rng.permutation(p.shape[0])
    for k in range(N_BIN):
        yield f"per bin#{k}", np.argsort(rng.random(p.shape, dtype=np.float32), axis=0)
    for label, key in (("positive first", p <= 0), ("ascending magnitude", np.abs(p)), ("descending value", -p)):
        o = np.argsort(key, axis=0, kind="stable")
        yield label, o
        yield label + ", reversed", o[::-1]


@pytest.fixture(scope="module")
def flush_runs():
    """[(case, label, bwd_partials, float64 lut_grad)] for the whole and both bands of every backward case."""
    out = []
    for name in lr.BACKWARD_NAMES:
        cs = lr.backward_case(name)
        for label, r0, rows, tile in lr.backward_bands(cs):
            ref = lr.icrf_backward_f64(cs.x[:, :, r0:r0 + rows], cs.grad_out[:, :, r0:r0 + rows], cs.lut, cs.mode, tile)[1]
            out.append((cs, label, lr.bwd_partials(cs, r0, rows, tile, CUS), ref))
    return out


@pytest.fixture(scope="module")
def flush_study(flush_runs):
    """{case: [(label, order, within order_bound?, |error| / bound, element error, norm-wise error)]} against the float64
    reference in the two measures of _util.assert_parity."""
    rng = np.random.default_rng(20261020)
    out = {}
    for cs, label, parts, ref in flush_runs:
        bound = lr.order_bound(parts)
        for order_name, order in flush_orders(parts, rng):
            got = lr.flush_in_order(parts.partials, order).astype(np.float64)
            err = np.abs(got - parts.S)
            out.setdefault(cs.name, []).append((label, order_name, bool(np.all(err <= bound)), float(np.max(err / np.where(bound > 0, bound, 1.0))),
                                                _elem_err(got, ref), rel_norm(got, ref)))
    return out


def test_flush_restatement_agrees_with_the_float64_reference(flush_runs):
    """S, the float64 sum of the restated partials, is the float64 reference up to the roundings of the float32 products and
    of the partials (E of bwd_partials: 0 / 2 / 7 roundings of a product for LOOKUP / LINEAR / CATMULL, the latter of the
    weight's terms, and 2^-24 A); every sample is owned by one workgroup; ascending workgroup order stays within order_bound
    and passes the assertions the GPU test makes."""
    for cs, label, parts, ref in flush_runs:
        what = f"{cs.name} {label}"
        assert parts.partials.shape[0] == parts.grid.gx * parts.grid.gy and parts.partials.dtype == np.float32, what
        assert np.all(np.abs(parts.S - ref) <= parts.E), (what, float(np.max(np.abs(parts.S - ref) / np.where(parts.E > 0, parts.E, 1))))
        assert np.array_equal(parts.S == 0, ref == 0) or cs.mode == "catmull" or cs.kind == "cancel", what
        if cs.mode == "lookup":       # products are go itself: the partials add up to the reference to a float32 rounding each
            assert np.all(np.abs(parts.S - ref) <= 2.0 ** -24 * parts.A), what
        used = lr.assert_flush(lr.flush_in_order(parts.partials, np.arange(parts.partials.shape[0])), parts, what)
        assert used <= 1.0


def test_flush_cases_hold_their_conditions(flush_runs):
    by = {(cs.name, label): (cs, parts) for cs, label, parts, ref in flush_runs}
    plain_m = max(int(parts.m.max()) for (name, label), (cs, parts) in by.items() if cs.kind == "plain" and name != "bw_repeat_linear_c3")
    assert plain_m <= 24                                                       # the cases before these: a few tens at the most
    for name in lr.BACKWARD_NAMES:
        cs, parts = by[(name, "whole")]
        touched = parts.A > 0
        if cs.kind == "hot":      # >= 64 workgroups flush a nonzero partial into one bin; 8 per compute unit, grid.x uncapped
            assert parts.m.max() >= 64 and parts.m.max() == parts.grid.gx * parts.grid.gy, (name, int(parts.m.max()))
            assert parts.grid.slots == 8 and parts.grid.gx == -(-cs.C * cs.hg * cs.w // 256) and not parts.grid.repeats, name
        if cs.kind == "cancel":   # a quarter of the touched bins cancel
            cancelled = touched & (np.abs(parts.S) < 1e-3 * parts.A)
            assert cancelled.sum() * 4 >= touched.sum() and (touched & ~cancelled).sum() * 4 >= touched.sum(), (name, int(cancelled.sum()), int(touched.sum()))
            assert parts.m[cancelled].min() >= 2, name                         # (and not within one workgroup's float64 sum)
        if cs.kind == "untouched":
            top = cs.L - 1
            lo, hi = int(np.floor(0.3 * top)) - 1, int(np.ceil(0.6 * top)) + 2   # CATMULL taps reach one below and two above
            for label in ("whole", "band0", "band1"):
                p = by[(name, label)][1]
                assert not p.partials[:, :, :lo].any() and not p.partials[:, :, hi + 1:].any() and not p.slack[:, :, :lo].any(), (name, label)
                assert lr.order_bound(p)[:, :lo].max() == 0 and lr.order_bound(p)[:, hi + 1:].max() == 0
            band0 = by[(name, "band0")][1]
            assert band0.m[:2].max() > 0 and not band0.partials[:, 2:].any() and lr.order_bound(band0)[2:].max() == 0, name
            assert all(by[(name, label)][1].m.min(axis=1).max() == 0 and (by[(name, label)][1].m.max(axis=1) > 0).sum() == (2 if label == "band0" else 4)
                       for label in ("whole", "band0", "band1")), name
    assert {lr.backward_case(n).mode for n in lr.BACKWARD_NAMES if lr.BACKWARD_KIND[n] == "hot"} == {"lookup", "linear", "catmull"}


def test_every_flush_order_stays_within_order_bound(flush_runs, flush_study):
    """The flush-order study.  Every order is within order_bound; the bound is not vacuous (some order uses 1 / 64 of it
    wherever two partials meet: the bound grows like m where sign-mixed rounding errors grow like sqrt(m), m <= 256, and
    CATMULL's contraction slack allows 15 roundings where one or two occur); the recorded figures of _linearize_refs
    (ORDER_BOUND_USED, FLUSH_SHARE_OF_TOL) are what the study measures, and they decide which cases the GPU test still
    compares with the float64 reference at TOL."""
    met = {name: 0 for name in lr.BACKWARD_NAMES}
    for cs, label, parts, ref in flush_runs:
        met[cs.name] = max(met[cs.name], int(parts.m.max()))
    for name, rows in flush_study.items():
        mode = lr.backward_case(name).mode
        outside = [(label, order) for label, order, within, *_ in rows if not within]
        assert not outside, (name, outside)
        used = max(rows, key=lambda r: r[3])
        elem = max(rows, key=lambda r: r[4])
        norm = max(rows, key=lambda r: r[5])
        tol_e, tol_n = lr.TOL[("lut_grad", mode)]
        print(f"linearize flush orders: {name:24s} |error| / bound {used[3]:.4f} ({used[0]}, {used[1]})  element {elem[4]:.3e} = {elem[4] / tol_e:.3f} TOL "
              f"({elem[0]}, {elem[1]})  norm-wise {norm[5]:.3e} = {norm[5] / tol_n:.3f} TOL ({norm[0]}, {norm[1]})")
        assert used[3] <= 1.0 and (used[3] >= 1 / 64 or met[name] < 2), (name, used)
        for measured, recorded in ((used[3], lr.ORDER_BOUND_USED[name]), (elem[4] / tol_e, lr.FLUSH_SHARE_OF_TOL[name][0]),
                                   (norm[5] / tol_n, lr.FLUSH_SHARE_OF_TOL[name][1])):
            assert recorded * 0.98 <= measured <= recorded * 1.02, (name, measured, recorded)
        if not lr.flush_keeps_margin(name):
            assert norm[5] * 4 <= lr.TOL[("lut_grad any order", name)][1] <= norm[5] * 4.2, (name, norm[5])
    assert set(lr.ORDER_BOUND_USED) == set(lr.FLUSH_SHARE_OF_TOL) == set(lr.BACKWARD_NAMES)
    assert {q[1] for q in lr.TOL if q[0] == "lut_grad any order"} == {n for n in lr.BACKWARD_NAMES if not lr.flush_keeps_margin(n)}


def test_order_bound_is_no_weaker_than_the_tolerance_it_replaces(flush_runs):
    """Where the GPU test takes order_bound in place of the element test of TOL (flush_keeps_margin is False): the share of
    touched bins whose allowance got smaller, and the largest factor by which one got larger.  The old allowance is
    TOL (|ref| + median |ref|); the new one is order_bound, about parts.S, which is within E of ref."""
    for cs, label, parts, ref in flush_runs:
        if lr.flush_keeps_margin(cs.name):
            continue
        old = lr.TOL[("lut_grad", cs.mode)][0] * (np.abs(ref) + np.median(np.abs(ref)))
        new = lr.order_bound(parts)
        touched = new > 0
        smaller = float((new[touched] < old[touched]).mean())
        larger = float(np.max(new[touched] / np.where(old[touched] > 0, old[touched], np.inf))) if touched.any() else 0.0
        print(f"linearize flush orders: {cs.name:24s} {label:6s} allowance smaller in {smaller:.3f} of the touched bins, at most {larger:.2f} x the old one; "
              f"untouched bins: {int((~touched).sum())} now exactly 0")
        assert np.all(new[~touched] == 0)
        assert smaller >= lr.ALLOWANCE_VS_TOL[cs.name][0] and larger <= lr.ALLOWANCE_VS_TOL[cs.name][1], (cs.name, label, smaller, larger)


def test_flush_assertions_tell_a_wrong_kernel(flush_runs):
    """assert_flush passes what some flush order gives and fails three wrong kernels: one that flushes a partial twice; one
    whose ownership is off by one workgroup (workgroup bx starts at element (bx + 1) 256, so the first 256 elements of
    every image have no owner); one that writes a float32 ulp, or -0.0, into a bin that no sample reaches.  (Which
    workgroup owns a sample does not change what lut_grad adds up to: a shift that still owns every sample once moves
    roundings only, within order_bound by construction.)"""
    rng = np.random.default_rng(7)
    untouched = 0
    for cs, label, parts, ref in flush_runs:
        p = parts.partials
        what = f"{cs.name} {label}"
        good = lr.flush_in_order(p, rng.permutation(p.shape[0]))
        lr.assert_flush(good, parts, what)
        k = int(np.argmax(np.abs(p).sum(axis=(1, 2))))
        with pytest.raises(AssertionError):
            lr.assert_flush(lr.flush_in_order(np.concatenate([p, p[k:k + 1]]), np.arange(p.shape[0] + 1)), parts, what)
        if label == "whole":
            go = cs.grad_out.copy()
            go.reshape(cs.N, -1)[:, :256] = 0
            late = lr.bwd_partials(SimpleNamespace(**{**vars(cs), "grad_out": go}), 0, cs.hg, None, CUS)
            with pytest.raises(AssertionError):
                lr.assert_flush(lr.flush_in_order(late.partials, np.arange(p.shape[0])), parts, what)
        empty = lr.order_bound(parts) == 0
        if empty.any():
            c, i = np.argwhere(empty)[0]
            for v in (np.spacing(np.float32(max(np.abs(good[c]).max(), 1e-30))), np.float32(-0.0)):
                bad = good.copy()
                bad[c, i] = v
                with pytest.raises(AssertionError):
                    lr.assert_flush(bad, parts, what)
            untouched += 1
    assert untouched >= 12
