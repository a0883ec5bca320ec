"""The float64 references of tests/_linearize_refs.py against the pinned float32 oracles, on the CPU.

This is also where the tolerances of tests/test_gpu_linearize_paths.py are measured: the float32 oracles (oc.linearize_std,
oc.icrf_forward; autograd of oe.icrf_forward for the backward) are compared with the float64 references on the very inputs
the GPU test uses, bands included, and every entry of _linearize_refs.TOL must hold 4x the worst deviation seen, in both
measures of _util.assert_parity.  Run with -s to see the measured figures."""
import itertools

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
        note(("lut_grad", cs.mode), gl_o, gl, (cs.name, label))
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
    assert {v.image_rounds for v in grids.values()} == {1, 2}
    cases = [lr.backward_case(n) for n in lr.BACKWARD_NAMES[:-1]]
    assert {(c.mode, c.C) for c in cases} == set(itertools.product(("lookup", "linear", "catmull"), (1, 3, 4)))
    assert all({c.N for c in cases if c.mode == m} == {1, 8, 11} for m in ("lookup", "linear", "catmull"))
