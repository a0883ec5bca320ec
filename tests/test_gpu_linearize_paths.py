"""Every launch path and row band of the linearize kernels (csrc/ct_linearize.hip) against the float32 oracles bit for bit
and against the float64 references of tests/_linearize_refs.py.

Inputs are seeded (tests/_linearize_refs.py), tolerances are the ones tests/test_linearize_refs_host.py measures on the
CPU, and every comparison with a tolerance goes through _util.assert_parity (labels "lin ..." in parity_observed.json).

Path -> cases (the case table and the conditions behind its shapes are in _linearize_refs.FORWARD_CASES; the host test
checks that every path meets every interpolation mode, dtype and std mode it supports, and a row band):

| path | cases |
|---|---|
| linearize_rgb_kernel: nhwc / nhwc_bgr, 8 of 64 lanes active, a second wavefront of 3 active and 6 more loading lanes, bands with base % 3 and plane_global % 3 not 0 | rgb_* |
| linearize_planar_kernel: 257 / 513 / 1025 packets (live[1], live[2] false; two workgroups), packets straddling planes for C = 2, 4, bands with chan_skip % C != 0, a padded image stride | pl_* |
| linearize_kernel<8>, interleaved: C = 4, C = 1, C = 3 with an explicit std stack | p8_* |
| linearize_kernel<8> + <1> behind a padded stride (the C entry point): interleaved C = 4, 1, 3 (plane % 4 != 0) | pt_* |
| linearize_kernel<1>: nchw with Q % 4 = 1, 2, 3 and every std mode, Q < 4, a frame pointer 1 element into its allocation, frames [1:] of odd Q, several frames of Q % 4 != 0 behind a padded stride of 8 k (sc_band_pad_*); interleaved of Q % 8 != 0 | sc_*, se_* |
| the frame walk f += gridDim.y three times (131 073 frames), planar and rgb | test_many_frames |
| ct_linearize_bwd: 3 modes x C = 1, 3, 4 x n_images = 1, 8, 11, whole image and two bands, need_x / need_lut alone, a grid-stride loop that runs twice | test_backward: bw_lookup_*, bw_linear_*, bw_catmull_*, bw_repeat_linear_c3 |
| the flush of the LUT gradient, one hot bin: 64 / 72 / 80 workgroups (8 per compute unit, grid.x uncapped) flush a nonzero partial into the same bins, one case per mode | test_backward: bw_hot_lookup_c1, bw_hot_linear_c3, bw_hot_catmull_c2 |
| the flush, cancellation: a quarter of the touched bins add up to less than 1e-3 of their partials' magnitudes | test_backward: bw_cancel_linear_c3 |
| the flush, untouched bins: LUT ranges no sample reaches, and in the one-row band two whole LUT rows; exactly +0.0, with and without grad_x | test_backward: bw_untouched_catmull_c4 |
| torch.ops.clair_hip.icrf_forward / icrf_backward with h_global, row_offset | test_dispatcher_ops_take_bands |

The LUT gradient is the one result here that float32 global atomics add up, so its last bits follow the order in which the
workgroups flush.  Order-free, and so the same in every run: grad_x bit for bit; _linearize_refs.assert_flush (every bin
within order_bound of the restated sum of the workgroups' partials, untouched bins +0.0, bins of one partial equal to it);
the additivity over the bands at flush_bound (order_bound is not uniformly tighter than flush_bound: CATMULL carries a
contraction slack); the dispatcher's 2 flush_bound.  The comparison of lut_grad with the float64 reference at
TOL[("lut_grad", mode)] is four times ONE order's error and is kept only for the cases in which every order of the CPU
study (test_linearize_refs_host.py) leaves that factor (flush_keeps_margin); the others are compared norm-wise at
TOL[("lut_grad any order", case)].
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _linearize_refs as lr
from oracle import ct_oracle as oc

pytestmark = pytest.mark.gpu

_DT = {"u8": 0, "u16": 1, "f32": 2}
_MARGIN = 8          # floats of sentinel before and after the outputs of a call through the C entry point
_SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _to(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)      # a copy: the cases' arrays are shared and read-only


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _tile(cs, band):
    from clair_torch_amd import ops
    return ops.TileGeometry(h_global=cs.hg, row_offset=cs.r0) if band and cs.tile is not None else None


def _rows(a, cs, band):
    return None if a is None else (lr.band_rows(a, cs) if band else a)


def _placed(a, dev, offset=0):
    """The array on the device, `offset` elements into an allocation of its dtype (0: the allocation itself)."""
    t = _to(a, dev)
    if offset == 0:
        return t
    buf = torch.empty((t.numel() + offset,), dtype=t.dtype, device=dev)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _run_ops(dev, cs, band, layout):
    """ops.linearize_frames on the band (or the whole image) of a case, its stack in `layout`."""
    from clair_torch_amd import ops
    stored = lr.to_layout(_rows(cs.planar_stored, cs, band), layout)
    sigma = _rows(cs.sigma, cs, band)
    size = lr.ITEMSIZE[cs.dtype]
    if cs.slice:     # frames [1:] of a stack one frame longer
        frames = _to(np.concatenate([stored[:1], stored]), dev)[cs.slice:]
        sigma_d = None if cs.std != "explicit" else _to(np.concatenate([lr.to_layout(sigma, layout)[:1], lr.to_layout(sigma, layout)]), dev)[cs.slice:]
    else:
        frames = _placed(stored, dev, cs.offset)
        sigma_d = None if cs.std != "explicit" else _placed(lr.to_layout(sigma, layout), dev, cs.offset)
    q = stored[0].size
    assert frames.is_contiguous() and frames.data_ptr() % 32 == (cs.offset * size + cs.slice * q * size) % 32
    lin, sd = ops.linearize_frames(frames, None if cs.mode is None else _to(cs.lut, dev), cs.mode, max_code=cs.max_code,
                                   tile=_tile(cs, band), layout=layout, **lr.std_kwargs(cs, sigma_d))
    assert lin.data_ptr() % 32 == 0 and (sd is None or sd.data_ptr() % 32 == 0)
    return lin.cpu().numpy(), None if sd is None else sd.cpu().numpy()


def _run_raw(dev, cs, band):
    """ct_linearize_std itself with image_stride = Q + pad: the padding holds values that would show (the largest code /
    NaN), the outputs sit inside larger buffers whose margins must stay as they were."""
    from clair_torch_amd import _native as nv
    from clair_torch_amd import ops
    stored = lr.to_layout(_rows(cs.planar_stored, cs, band), cs.layout)
    sigma = _rows(cs.sigma, cs, band)
    f = stored.shape[0]
    h = cs.h if band else cs.hg
    q, stride = stored[0].size, stored[0].size + cs.pad
    fill = np.nan if cs.dtype == "f32" else np.iinfo(lr.NP_DTYPE[cs.dtype]).max

    def padded(a, fill):
        buf = np.full((f, stride), fill, dtype=a.dtype)
        buf[:, :q] = a.reshape(f, q)
        return _to(buf, dev)

    frames = padded(stored, fill)
    sigma_d = padded(lr.to_layout(sigma, cs.layout), np.nan) if cs.std == "explicit" else None
    outs = [torch.full((f * q + 2 * _MARGIN,), _SENTINEL, dtype=torch.float32, device=dev) for _ in range(1 if cs.std == "nostd" else 2)]
    views = [o[_MARGIN:_MARGIN + f * q] for o in outs]
    assert frames.data_ptr() % 32 == 0 and all(v.data_ptr() % 32 == 0 for v in views)
    hg, r0 = (cs.hg, cs.r0) if band and cs.tile is not None else (h, 0)
    geom = nv.Geometry(channels=cs.C, h_tile=h, width=cs.w, h_global=hg, row_offset=r0, image_stride=stride, layout=ops._LAYOUT[cs.layout])
    lut_d = None if cs.mode is None else _to(cs.lut, dev)
    icrf = nv.Icrf(lut_dev=None if lut_d is None else lut_d.data_ptr(), n_points=0 if lut_d is None else cs.L, interp=ops._INTERP[cs.mode])
    std_mode = ops._STD["none" if cs.std == "nostd" else cs.std]
    rc = nv.load().ct_linearize_std(_ptr(frames), _DT[cs.dtype], float(cs.max_code or 1.0), f, ctypes.byref(geom), _ptr(sigma_d), std_mode,
                                    float(cs.std_value), ctypes.byref(icrf), _ptr(views[0]), _ptr(views[1]) if len(views) > 1 else None,
                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, rc
    for o in outs:
        host = o.cpu().numpy()
        assert np.all(host[:_MARGIN] == _SENTINEL) and np.all(host[-_MARGIN:] == _SENTINEL), cs.name
    shape = (f, cs.C, h, cs.w)
    return views[0].cpu().numpy().reshape(shape), (views[1].cpu().numpy().reshape(shape) if len(views) > 1 else None)


def _run(dev, cs, band, layout=None):
    if cs.pad and layout is None:
        return _run_raw(dev, cs, band)
    return _run_ops(dev, cs, band, layout or cs.layout)


def _oracle(cs, band):
    lin, sd = oc.linearize_std(_rows(cs.x, cs, band), _rows(cs.sigma, cs, band), cs.lut, "nomodel" if cs.mode is None else cs.mode,
                               tile=cs.tile if band else None)
    return lin, (None if cs.std == "nostd" else sd)


def _check_forward(cs, band, got, what):
    lin, sd = got
    lin_o, sd_o = _oracle(cs, band)
    ref_lin, ref_sd = lr.linearize_f64(_rows(cs.x, cs, band), _rows(cs.sigma, cs, band), cs.lut, cs.mode, cs.tile if band else None)
    print(f"{what}: lin differs from the oracle in {int((lin != lin_o).sum())} of {lin.size}"
          + ("" if sd is None else f", std in {int((sd != sd_o).sum())}"))
    assert np.array_equal(lin, lin_o), what + " lin vs oracle"
    lr.check(lin, ref_lin, ("lin", cs.mode), f"lin {what} lin vs f64")
    assert (sd is None) == (sd_o is None)
    if sd is not None:
        assert np.array_equal(sd, sd_o), what + " std vs oracle"
        lr.check(sd, ref_sd, ("std", cs.mode), f"lin {what} std vs f64")


@pytest.mark.parametrize("name", lr.FORWARD_NAMES)
def test_forward_paths(dev, name):
    """The band of a case: bit for bit with the oracle given the same tile (value and std), within the measured
    tolerance of the float64 reference, and bit for bit the rows of the whole-image launch.  Interleaved stacks give the
    bits of the planar launch of the same data; float32 stacks without std those of ct_linearize_fwd."""
    from clair_torch_amd import ops
    cs = lr.forward_case(name)
    got = _run(dev, cs, True)
    _check_forward(cs, True, got, f"{name} [{lr.case_path(cs)}]")
    if cs.tile is not None:
        whole = _run(dev, cs, False)
        _check_forward(cs, False, whole, f"{name} whole [{lr.case_path(cs, False)}]")
        for a, b in zip(got, whole):
            assert (a is None and b is None) or np.array_equal(a, lr.band_rows(b, cs)), name + ": band vs rows of the whole"
    if cs.layout != "nchw":
        planar = _run(dev, cs, True, layout="nchw")
        for a, b in zip(got, planar):
            assert (a is None and b is None) or np.array_equal(a, b), name + ": interleaved vs planar"
    if cs.dtype == "f32" and cs.layout == "nchw" and cs.mode is not None and cs.std in ("nostd", "none") and not cs.pad:
        x = _placed(lr.band_rows(cs.planar_stored, cs), dev, cs.offset)
        out = ops.icrf_forward(x, _to(cs.lut, dev), cs.mode, tile=_tile(cs, True))
        assert np.array_equal(out.cpu().numpy(), got[0]), name + ": ct_linearize_fwd"
        assert np.array_equal(got[0], oc.icrf_forward(lr.band_rows(cs.x, cs), cs.lut, cs.mode, tile=cs.tile))


@pytest.mark.parametrize("name", [c[0] for c in lr.MANY_FRAMES])
def test_many_frames(dev, name):
    """2 * 65535 + 3 frames: grid.y is capped at 65535, so workgroups 0..2 walk frames y, y + 65535 and y + 131070."""
    cs = lr.forward_case(name)
    assert lr.frame_walk_of(cs.F) == (65535, 3) and lr.case_path(cs) == ("rgb" if cs.layout == "nhwc" else "planar")
    _check_forward(cs, True, _run(dev, cs, True), name)


# ---- backward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lr.BACKWARD_NAMES)
def test_backward(dev, name):
    """The whole image and its two bands.  grad_x: bit for bit with autograd of the eager oracle (signed zeros aside; LOOKUP:
    zeros), the same bits with and without the LUT gradient.  lut_grad, with and without grad_x: per bin within order_bound
    of the sum of the partials that the workgroups of the device's grid flush, untouched bins +0.0, bins of one partial
    equal to it (_linearize_refs.check_lut_grad; the share of the bound used goes to parity_observed.json); against the
    float64 reference at the measured tolerance where every flush order keeps its margin, else norm-wise; and additive
    over the two bands up to the flush order (_linearize_refs.flush_bound)."""
    from clair_torch_amd import ops
    cs = lr.backward_case(name)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    lut_d = _to(cs.lut, dev)
    got, groups = {}, {}
    for label, r0, rows, tile in lr.backward_bands(cs):
        x_d, go_d = _to(cs.x[:, :, r0:r0 + rows], dev), _to(cs.grad_out[:, :, r0:r0 + rows], dev)
        tg = None if tile is None else ops.TileGeometry(h_global=tile[0], row_offset=tile[1])
        gx, gl = ops.icrf_backward(x_d, go_d, lut_d, cs.mode, True, True, tile=tg)
        gx_only, none = ops.icrf_backward(x_d, go_d, lut_d, cs.mode, True, False, tile=tg)
        none2, gl_only = ops.icrf_backward(x_d, go_d, lut_d, cs.mode, False, True, tile=tg)
        assert none is None and none2 is None
        ref_gx, ref_gl = lr.icrf_backward_f64(cs.x[:, :, r0:r0 + rows], cs.grad_out[:, :, r0:r0 + rows], cs.lut, cs.mode, tile)
        gx_o, _ = lr.eager_backward(cs, r0, rows)
        what = f"{name} {label}"
        assert torch.equal(gx, gx_only), what
        if gx_o is None:
            assert not gx.cpu().numpy().any(), what
        else:
            assert np.array_equal(gx.cpu().numpy(), gx_o), what + " grad_x vs autograd"
            lr.check(gx.cpu().numpy(), ref_gx, ("grad_x", cs.mode), f"lin {what} grad_x vs f64")
        parts = lr.bwd_partials(cs, r0, rows, tile, cus)
        for g, form in ((gl, "both"), (gl_only, "lut only")):
            used = lr.check_lut_grad(g.cpu().numpy(), cs, parts, ref_gl, f"lin {what} lut_grad ({form})")
            print(f"{what} lut_grad ({form}): worst |error| / order_bound {used:.4f}, {parts.grid.gx} x {parts.grid.gy} workgroups, m <= {int(parts.m.max())}")
        got[label] = gl.cpu().numpy().astype(np.float64)
        grid = lr.bwd_grid_of(cs.C * rows * cs.w, cs.N, cs.C, cs.L, cs.mode, cus)
        groups[label] = grid.gx * grid.gy
        if name == "bw_repeat_linear_c3" and label == "whole":
            assert grid.repeats and cus == 256
    scale = lr.icrf_backward_f64(cs.x, cs.grad_out, cs.lut, cs.mode, absolute=True)[1]
    bound = sum(lr.flush_bound(scale, w) for w in groups.values())
    excess = np.abs(got["band0"] + got["band1"] - got["whole"]) - bound
    print(f"{name}: bands against whole, worst |difference| / bound {float(np.max(np.abs(got['band0'] + got['band1'] - got['whole']) / np.where(bound > 0, bound, 1))):.3f}")
    assert np.all(excess <= 0), (name, float(excess.max()))


def test_dispatcher_ops_take_bands(dev):
    """torch.ops.clair_hip.icrf_forward / icrf_backward with h_global and row_offset are ops.* with that tile."""
    from clair_torch_amd import ops, torch_ops  # noqa: F401
    cs = lr.backward_case("bw_catmull_c3")
    r0, rows = cs.split, cs.hg - cs.split
    x, go, lut = _to(cs.x[:, :, r0:], dev), _to(cs.grad_out[:, :, r0:], dev), _to(cs.lut, dev)
    tile = ops.TileGeometry(h_global=cs.hg, row_offset=r0)
    for mode in ("lookup", "linear", "catmull"):
        out = torch.ops.clair_hip.icrf_forward(x, lut, mode, cs.hg, r0)
        assert torch.equal(out, ops.icrf_forward(x, lut, mode, tile=tile))
        assert np.array_equal(out.cpu().numpy(), oc.icrf_forward(cs.x[:, :, r0:], cs.lut, mode, tile=(cs.hg, r0)))
        assert not torch.equal(out, ops.icrf_forward(x, lut, mode)) or mode == "lookup"      # the tile matters
        gx, gl = torch.ops.clair_hip.icrf_backward(x, go, lut, mode, True, True, cs.hg, r0)
        rx, rl = ops.icrf_backward(x, go, lut, mode, True, True, tile=tile)
        assert torch.equal(gx, rx)
        parts = lr.bwd_partials(SimpleNamespace(**{**vars(cs), "mode": mode}), r0, rows, (cs.hg, r0), torch.cuda.get_device_properties(dev).multi_processor_count)
        for g, via in ((gl, "dispatcher"), (rl, "ops")):
            lr.assert_flush(g.cpu().numpy(), parts, f"{via} {mode} lut_grad")
        scale = lr.icrf_backward_f64(cs.x[:, :, r0:], cs.grad_out[:, :, r0:], cs.lut, mode, (cs.hg, r0), absolute=True)[1]
        grid = lr.bwd_grid_of(cs.C * rows * cs.w, cs.N, cs.C, cs.L, mode, torch.cuda.get_device_properties(dev).multi_processor_count)
        assert np.all(np.abs(gl.cpu().numpy().astype(np.float64) - rl.cpu().numpy()) <= 2 * lr.flush_bound(scale, grid.gx * grid.gy))
    # the registered autograd formula carries the band
    xg, lg = x.clone().requires_grad_(True), lut.clone().requires_grad_(True)
    ax, al = torch.autograd.grad(torch.ops.clair_hip.icrf_forward(xg, lg, "catmull", cs.hg, r0), (xg, lg), go)
    rx, rl = ops.icrf_backward(x, go, lut, "catmull", True, True, tile=tile)
    assert torch.equal(ax, rx)
    lr.check_lut_grad(al.cpu().numpy(), cs, lr.bwd_partials(cs, r0, rows, (cs.hg, r0), torch.cuda.get_device_properties(dev).multi_processor_count),
                      lr.icrf_backward_f64(cs.x[:, :, r0:], cs.grad_out[:, :, r0:], cs.lut, "catmull", (cs.hg, r0))[1], "lin dispatcher lut_grad")
