"""Plain float64 references of the linearize kernels (ct_linearize_std / ct_linearize_fwd / ct_linearize_bwd,
csrc/ct_linearize.hip), a restatement of their launch paths, the seeded inputs and the tolerances their tests share.

NumPy only (eager_backward alone runs the pinned eager oracle under torch autograd), written from include/clair_hip.h,
csrc/ct_device.hpp and the reference's formulas (ICRFModelBase.forward, linearize_dataset_generator) and calling none of
the code under test.  tests/test_linearize_refs_host.py validates it
against the pinned oracles on the CPU and measures the tolerances below; tests/test_gpu_linearize_paths.py compares the
kernels with it.

Discrete decisions are taken in float32 exactly as the kernels and the oracles take them -- the LUT row from the global
index, the LUT coordinate fl(x (L - 1)) with its clamp, floor(.) or rint(.) of it, the tap indices -- and handed to the
float64 arithmetic, so a comparison measures arithmetic, not ties."""
import functools
from types import SimpleNamespace

import numpy as np

# ---- tolerances ----------------------------------------------------------------------------------------------------
# TOL[(quantity, mode)] = (element tolerance, norm-wise tolerance) in the two measures of _util.assert_parity.  Each is 4x
# what the float32 oracle (oc.linearize_std for lin / std, autograd of oe.icrf_forward for the backward) shows against the
# float64 reference, worst over every input of the GPU test (the band and the whole image of every case of
# FORWARD_CASES + MANY_FRAMES, both bands and the whole of every case of BACKWARD_CASES), rounded up.
# test_linearize_refs_host.py re-measures every entry and asserts measured * 4 <= tolerance.  Measured (element, norm-wise)
# in the comments.  0.0: the operation has no arithmetic (a gather, a copy, |1 * sigma|) and must be exact.
TOL = {
    ("lin", "lookup"): (0.0, 0.0),              # a gather
    ("lin", None): (0.0, 0.0),                  # a copy
    ("lin", "linear"): (3.0e-7, 1.4e-7),        # measured 7.301e-8, 3.378e-8 (se_band_c3_4x67of5_u16e whole / sc_c3_19x23_u16)
    ("lin", "catmull"): (5.9e-7, 2.3e-7),       # measured 1.456e-7, 5.707e-8 (pl_pad_band_c4_5x7of8_f32 whole / p8_c3_4x8_u8e)
    ("std", "lookup"): (0.0, 0.0),              # no gradient path: zeros
    ("std", None): (1.3e-23, 9.2e-25),          # measured 3.017e-24, 2.277e-25 (sc_c1_5x5_f32): |1 * sigma| is exact unless
                                                # sigma^2 underflows (sigma = 5e-21), and such a sigma is 1e-24 of the median
    ("std", "linear"): (3.2e-7, 1.8e-7),        # measured 7.923e-8, 4.428e-8 (se_band_c3_4x67of5_u16e / many_planar_1x1x4)
    ("std", "catmull"): (2.3e-4, 8.1e-5),       # measured 5.679e-5, 2.006e-5 (pl_c4_27x19_u16 / pt_c1_5x7_u16): the reference's
                                                # float32 autograd order cancels ~100x (ct_device.hpp, catmull_backward_ref)
    ("grad_x", "lookup"): (0.0, 0.0),           # no gradient path: zeros
    ("grad_x", "linear"): (4.1e-4, 1.2e-4),     # measured 1.011e-4, 2.862e-5 (bw_repeat_linear_c3: (G g1 - G g0) 2047 cancels 1e3-fold)
    ("grad_x", "catmull"): (5.4e-5, 1.2e-5),    # measured 1.327e-5, 2.885e-6 (bw_catmull_c4 band1 / bw_catmull_c1 band1)
    ("lut_grad", "lookup"): (1.8e-6, 5.1e-7),   # measured 4.271e-7, 1.267e-7 (bw_lookup_c4 band0 / bw_lookup_c1 whole)
    ("lut_grad", "linear"): (9.9e-6, 5.3e-7),   # measured 2.467e-6, 1.322e-7 (bw_repeat_linear_c3 whole: 2048 bins of a few +- terms)
    ("lut_grad", "catmull"): (3.2e-6, 7.3e-7),  # measured 7.811e-7, 1.821e-7 (bw_catmull_c1 band0 / bw_catmull_c3 whole)
    # The cases in which some order of the kernel's float32 flushes leaves less than the factor 4 of the three entries above
    # (FLUSH_SHARE_OF_TOL below): element-wise they are held to order_bound (inf here), norm-wise to 4x the worst error of
    # the orders of the flush-order study against the float64 reference -- measured on the restatement bwd_partials /
    # flush_in_order, not on the kernel -- rounded up.  Measured norm-wise in the comments.
    ("lut_grad any order", "bw_catmull_c3"): (np.inf, 7.9e-7),            # 1.958e-7 (whole, descending value reversed)
    ("lut_grad any order", "bw_repeat_linear_c3"): (np.inf, 4.3e-6),      # 1.060e-6 (whole, descending value reversed)
    ("lut_grad any order", "bw_hot_lookup_c1"): (np.inf, 6.8e-6),         # 1.699e-6 (whole, positive first)
    ("lut_grad any order", "bw_hot_linear_c3"): (np.inf, 3.5e-6),         # 8.686e-7 (whole, positive first reversed)
    ("lut_grad any order", "bw_hot_catmull_c2"): (np.inf, 2.5e-6),        # 6.067e-7 (whole, descending value reversed)
    ("lut_grad any order", "bw_cancel_linear_c3"): (np.inf, 1.7e-6),      # 4.149e-7 (whole, descending value)
    ("lut_grad any order", "bw_untouched_catmull_c4"): (np.inf, 6.5e-7),  # 1.624e-7 (band1, descending value)
}

def check(got, ref, key, what):
    """got against the float64 reference at TOL[key] in both measures of _util.assert_parity; exactly where TOL is 0."""
    from _util import assert_parity
    elem, norm = TOL[key]
    assert np.isfinite(elem), key     # ("lut_grad any order": check_lut_grad)
    if elem == 0.0:
        assert np.array_equal(np.asarray(got, dtype=np.float64), ref), what
    else:
        assert_parity(got, ref, norm_tol=norm, elem_tol=elem, what=what)


STD_CONSTANT, STD_MULTIPLIER = 0.01, 0.05
PATHS = ("rgb", "planar", "planar+tail", "packet8", "packet8+tail", "scalar")
ITEMSIZE = {"u8": 1, "u16": 2, "f32": 4}
NP_DTYPE = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


# ---- the LUT-row rule ----------------------------------------------------------------------------------------------
def lut_rows(c, h, w, mode, tile=None):
    """(C, H, W) LUT row of every element of a band of rows [row_offset, row_offset + H) of a (C, h_global, W) image;
    tile = (h_global, row_offset) or None for the whole image.  LOOKUP: the channel.  LINEAR / CATMULL: the flat index of
    the element in the GLOBAL image, (c * h_global + row_offset + y) * W + x, modulo C (the exposure index n contributes
    n * C * h_global * W, a multiple of C)."""
    hg, r0 = (h, 0) if tile is None else tile
    cc = np.arange(c, dtype=np.int64).reshape(c, 1, 1)
    yy = np.arange(h, dtype=np.int64).reshape(1, h, 1)
    xx = np.arange(w, dtype=np.int64).reshape(1, 1, w)
    if mode == "lookup":
        return np.broadcast_to(cc, (c, h, w)).copy()
    return ((cc * hg + r0 + yy) * w + xx) % c


# ---- the references ------------------------------------------------------------------------------------------------
def _coordinate(x, top):
    """float32 decisions of LINEAR / CATMULL: (interval i0, fraction t as float64, inside) of fl(x top) clamped to
    [0, top].  t = s - floor(s) is exact in float32 (and in float64)."""
    s = (np.asarray(x, dtype=np.float32) * np.float32(top)).astype(np.float32)
    inside = (s >= 0) & (s <= np.float32(top))
    sc = np.minimum(np.maximum(s, np.float32(0)), np.float32(top))
    fl = np.floor(sc)
    return fl.astype(np.int64), sc.astype(np.float64) - fl.astype(np.float64), inside


def _catmull_basis(t):
    t2 = t * t
    t3 = t2 * t
    return (-0.5 * t3 + t2 - 0.5 * t, 1.5 * t3 - 2.5 * t2 + 1.0, -1.5 * t3 + 2.0 * t2 + 0.5 * t, 0.5 * t3 - 0.5 * t2)


def _catmull_dbasis(t):
    t2 = t * t
    return (-1.5 * t2 + 2.0 * t - 0.5, 4.5 * t2 - 5.0 * t, -4.5 * t2 + 4.0 * t + 0.5, 1.5 * t2 - t)


def _taps(x, lut, mode, tile):
    """[(weight, d weight / dx, row, index)] of the taps of every sample of x (N, C, H, W), float64 weights."""
    n, c, h, w = x.shape
    top = lut.shape[1] - 1
    rows = np.broadcast_to(lut_rows(c, h, w, mode, tile), x.shape)
    if mode == "lookup":
        r = np.rint((x.astype(np.float32) * np.float32(top)).astype(np.float32))   # half to even, as torch.round
        idx = np.minimum(np.maximum(r, 0), top).astype(np.int64)
        one = np.ones(x.shape)
        return [(one, np.zeros(x.shape), rows, idx)]
    i0, t, inside = _coordinate(x, top)
    chain = top * inside.astype(np.float64)              # d s / d x where the clamp passes the gradient
    if mode == "linear":
        return [(1.0 - t, -chain, rows, i0), (t, chain, rows, np.minimum(i0 + 1, top))]
    return [(b, d * chain, rows, np.clip(i0 + k, 0, top))
            for b, d, k in zip(_catmull_basis(t), _catmull_dbasis(t), (-1, 0, 1, 2))]


def linearize_f64(x, sigma, lut, mode, tile=None):
    """(lin, |f'(x) sigma|) in float64 for float32 pixel values x (F, C, H, W), planar; sigma the float32 per-sample
    uncertainties or None (the second result is then zero); lut (C, L) float32; mode "lookup" / "linear" / "catmull" or
    None (no model: f(x) = x); tile = (h_global, row_offset) or None."""
    x = np.asarray(x, dtype=np.float32)
    if mode is None:
        lin, dfdx = x.astype(np.float64), np.ones(x.shape)
    else:
        lut64 = np.asarray(lut, dtype=np.float32).astype(np.float64)
        lin, dfdx = np.zeros(x.shape), np.zeros(x.shape)
        for wgt, dw, rows, idx in _taps(x, lut64, mode, tile):
            g = lut64[rows, idx]
            lin += wgt * g
            dfdx += dw * g
    if sigma is None:
        return lin, np.zeros(x.shape)
    return lin, np.abs(dfdx * np.asarray(sigma, dtype=np.float32).astype(np.float64))


def icrf_backward_f64(x, grad_out, lut, mode, tile=None, absolute=False):
    """(grad_x (N, C, H, W), lut_grad (C, L)) of sum(grad_out * f(x)) in float64.  LOOKUP has no gradient to x (zeros).
    absolute: lut_grad becomes sum |grad_out * weight| per bin, the scale of a bin's rounding errors."""
    x = np.asarray(x, dtype=np.float32)
    go = np.asarray(grad_out, dtype=np.float32).astype(np.float64)
    lut64 = np.asarray(lut, dtype=np.float32).astype(np.float64)
    grad_x, lut_grad = np.zeros(x.shape), np.zeros(lut64.shape)
    for wgt, dw, rows, idx in _taps(x, lut64, mode, tile):
        grad_x += go * dw * lut64[rows, idx]
        term = go * wgt
        np.add.at(lut_grad, (rows.reshape(-1), idx.reshape(-1)), (np.abs(term) if absolute else term).reshape(-1))
    return grad_x, lut_grad


# ---- launch paths --------------------------------------------------------------------------------------------------
def linearize_path_of(dtype, layout, C, plane, Q, n_frames, std_mode, alignments, strides):
    """Which kernels lin_typed (ct_linearize.hip) launches, restated: "rgb" (linearize_rgb_kernel), "planar"
    (linearize_planar_kernel), "planar+tail" (that and linearize_kernel<1> on the last Q % 4 elements), "packet8"
    (linearize_kernel<8>: interleaved frames only), "packet8+tail" (that and linearize_kernel<1> on the last Q % 8), "scalar"
    (linearize_kernel<1>).
    alignments: byte address modulo 32 of "frames", "std", "lin", "std_out" (a missing key is a NULL pointer, which is
    aligned); strides = (image_stride, out_stride) in elements.  n_frames does not choose a kernel (frame_walk_of)."""
    assert n_frames > 0 and Q == C * plane
    size = ITEMSIZE[dtype]
    image_stride, out_stride = strides

    def al(name, nbytes):
        return alignments.get(name, 0) % nbytes == 0

    V = 8
    vec_ok = (layout != "nchw" and al("frames", size * V) and image_stride % V == 0 and al("std", 4 * V)
              and al("lin", 4 * V) and al("std_out", 4 * V))
    if (layout != "nchw" and C == 3 and std_mode != "explicit" and plane % 4 == 0 and al("frames", 16)
            and image_stride % 4 == 0 and al("lin", 16) and al("std_out", 16) and out_stride % 4 == 0):
        return "rgb"
    if (layout == "nchw" and Q >= 4 and al("frames", size * 4) and image_stride % 4 == 0 and al("std", 16)
            and al("lin", 16) and al("std_out", 16) and out_stride % 4 == 0):
        return "planar" if Q % 4 == 0 else "planar+tail"
    q_vec = (Q // V) * V if vec_ok else 0
    if q_vec == 0:
        return "scalar"
    return "packet8" if q_vec == Q else "packet8+tail"


def frame_walk_of(n_frames):
    """(grid.y, most frames one workgroup walks) of the three forward kernels: two frames per workgroup, grid.y <= 65535."""
    gy = min(max((n_frames + 1) // 2, 1), 65535)
    return gy, -(-n_frames // gy)


def bwd_grid_of(Q, n_images, C, L, mode, compute_units):
    """bwd_launch restated: grid (gx, gy), LDS bytes, workgroups per compute unit, and whether the grid-stride loop over
    the elements of an image runs more than once for some thread (`repeats`)."""
    entry = {"lookup": 4, "linear": 8, "catmull": 16}[mode]
    gy = min(max(n_images, 1), 8)
    lds = ((C * L * entry + 15) & ~15) + 8 * C * L
    assert lds <= 160 * 1024
    slots = max(1, min(160 * 1024 // lds, 2048 // 256))
    cap = max(1, compute_units * slots // gy)
    gx = min((Q + 255) // 256, cap)
    return SimpleNamespace(gx=gx, gy=gy, lds=lds, slots=slots, repeats=gx * 256 < Q, image_rounds=-(-n_images // gy))


# ---- inputs --------------------------------------------------------------------------------------------------------
def case_lut(C, L):
    """(C, L) float32: one distinct gamma curve per row, so that a wrong row shows; the second knot is 1e-19, so that
    the LINEAR slope of the first interval times any ordinary sigma is below 1e-18 (the branch of the kernels that forms
    sqrt(gs * gs) because the square underflows)."""
    g = np.linspace(0.0, 1.0, L, dtype=np.float64)
    lut = np.stack([g ** p for p in (1.7, 2.0, 2.3, 2.6)[:C]]).astype(np.float32)
    lut[:, 1] = np.float32(1e-19)
    return lut


def _l_of(dtype, max_code):
    """LUT length per container, (L - 1) a divisor of max_code so that knots are whole codes."""
    return {("u8", 255.0): 52, ("u16", 65535.0): 256, ("u16", 4095.0): 64}.get((dtype, max_code), 33)


def edge_values(dtype, max_code, L):
    """The values every case carries (stored form): 0, 1, exact knots, their two neighbours, values inside the first LUT
    interval, and out of range ones (float32 below 0 and above 1; uint16 codes above max_code = 4095)."""
    top = L - 1
    if dtype == "f32":
        k1, k2 = np.float32(5) / np.float32(top), np.float32(top - 1) / np.float32(top)
        return np.array([0.0, 1.0, k1, np.nextafter(k1, np.float32(0)), np.nextafter(k1, np.float32(1)), k2,
                         np.nextafter(k2, np.float32(0)), np.nextafter(k2, np.float32(1)), -0.25, 1.5, 1e-19,
                         0.5 / top, 0.5 - 0.5 / top], dtype=np.float32)
    step = int(max_code) // top
    assert step * top == int(max_code)
    v = [0, int(max_code), 5 * step, 5 * step - 1, 5 * step + 1, (top - 1) * step, (top - 1) * step - 1,
         (top - 1) * step + 1, 1, step - 1, step // 2 + 1, step]
    if dtype == "u16" and max_code == 4095.0:
        v += [4096, 9000, 65535]
    return np.array(v, dtype=NP_DTYPE[dtype])


def to_pixels(stored, dtype, max_code):
    """CastTo(float32) + Normalize(0, max_code): one correctly rounded float32 division."""
    if dtype == "f32":
        return stored
    return (stored.astype(np.float32) / np.float32(max_code)).astype(np.float32)


def to_layout(planar, layout):
    """Planar (F, C, H, W) -> the memory form of `layout`: nchw as is, nhwc (F, H, W, C), nhwc_bgr with the channel
    order reversed in memory (memory channel k holds planar channel C - 1 - k)."""
    if layout == "nchw":
        return np.ascontiguousarray(planar)
    if layout == "nhwc_bgr":
        planar = planar[:, ::-1]
    return np.ascontiguousarray(planar.transpose(0, 2, 3, 1))


def _place(band_view, values):
    """Writes `values` at evenly spread flat positions of a (F, C, h, W) view."""
    n = band_view.size
    k = min(len(values), n)
    pos = (np.arange(k) * (n // k)) if k else np.zeros(0, dtype=np.int64)
    idx = np.unravel_index(pos, band_view.shape)
    band_view[idx] = values[:k]
    return idx


# Forward cases.  (name, layout, dtype, C, h, w, h_global, row_offset, F, mode, std, extras): the band is rows
# [row_offset, row_offset + h) of the (C, h_global, w) image (h_global == h: no band).  std: "nostd" (no std output),
# "none" (CT_STD_NONE: zeros), "constant", "multiplier", "explicit".  extras: max_code (uint16 with 4095), pad (elements
# added to image_stride: through the C entry point), offset (elements the frame pointer is moved into its allocation),
# slice (the stack is frames [1:] of a stack one frame longer).  Shapes follow from the conditions of lin_typed:
#   rgb          nhwc / nhwc_bgr, C = 3, plane % 4 == 0, no explicit std.  4 x 8: 8 of 64 lanes active; 4 x 67 = 4 (64 + 3)
#                pixels, 804 elements: 3 lanes of the second wavefront active, its 36 elements are 9 packets loaded by
#                lanes 0..8, so 6 more lanes only load; 3 frames: a workgroup walks two
#   planar       nchw, Q % 4 == 0.  257 / 513 / 1025 packets: live[1] / live[2] false in the last workgroup (768 packets per
#                workgroup); C = 4 with an odd plane and C = 2 with plane % 4 == 2: packets straddle channel planes
#   packet8      nhwc, Q % 8 == 0 and not rgb: C = 4, C = 1, C = 3 with an explicit std
#   packet8+tail image_stride % 8 == 0 with Q % 8 != 0: only with a padded stride.  Interleaved only: packets of eight are
#                never formed from planar frames (sc_band_pad_*: nchw, Q % 4 != 0 behind image_stride % 8 == 0, several frames)
#   scalar       everything else: contiguous frames of Q % 8 != 0 (nhwc) or Q % 4 != 0 (nchw), Q < 4, a misaligned pointer
#   planar+tail  cannot be reached: it needs out_stride % 4 == 0 and Q % 4 != 0, and out_stride is Q
FORWARD_CASES = [
    # ---- rgb
    ("rgb_4x8_nhwc_u8", "nhwc", "u8", 3, 4, 8, 4, 0, 3, "linear", "constant", {}),
    ("rgb_4x8_bgr_u16", "nhwc_bgr", "u16", 3, 4, 8, 4, 0, 2, "catmull", "multiplier", {"max_code": 4095.0}),
    ("rgb_4x8_nhwc_f32", "nhwc", "f32", 3, 4, 8, 4, 0, 1, "lookup", "nostd", {}),
    ("rgb_4x8_bgr_f32", "nhwc_bgr", "f32", 3, 4, 8, 4, 0, 3, None, "constant", {}),
    ("rgb_4x67_nhwc_u16", "nhwc", "u16", 3, 4, 67, 4, 0, 3, None, "multiplier", {}),
    ("rgb_4x67_bgr_u8", "nhwc_bgr", "u8", 3, 4, 67, 4, 0, 2, "lookup", "none", {}),
    ("rgb_4x67_nhwc_f32", "nhwc", "f32", 3, 4, 67, 4, 0, 3, "catmull", "constant", {}),
    ("rgb_4x67_bgr_f32", "nhwc_bgr", "f32", 3, 4, 67, 4, 0, 2, "linear", "multiplier", {}),
    ("rgb_4x67_nhwc_u8", "nhwc", "u8", 3, 4, 67, 4, 0, 3, "catmull", "nostd", {}),
    ("rgb_band_4x8of7_bgr_u8", "nhwc_bgr", "u8", 3, 4, 8, 7, 2, 3, "catmull", "multiplier", {}),          # base % 3 = 1, plane_global % 3 = 2
    ("rgb_band_4x67of5_nhwc_u16", "nhwc", "u16", 3, 4, 67, 5, 1, 2, "linear", "constant", {"max_code": 4095.0}),  # 1, 2
    ("rgb_band_4x8of5_nhwc_f32", "nhwc", "f32", 3, 4, 8, 5, 1, 3, "linear", "none", {}),                  # base % 3 = 2, plane_global % 3 = 1
    ("rgb_band_4x67of8_bgr_f32", "nhwc_bgr", "f32", 3, 4, 67, 8, 3, 2, "catmull", "constant", {}),        # 0, 2
    # ---- planar
    ("pl_c1_4x257_u8", "nchw", "u8", 1, 4, 257, 4, 0, 3, "linear", "multiplier", {}),                      # 257 packets
    ("pl_c4_27x19_u16", "nchw", "u16", 4, 27, 19, 27, 0, 2, "catmull", "explicit", {}),                    # 513 packets, odd plane
    ("pl_c2_86x3_f32", "nchw", "f32", 2, 86, 3, 86, 0, 3, "linear", "constant", {}),                       # plane % 4 = 2
    ("pl_c1_4x1025_f32", "nchw", "f32", 1, 4, 1025, 4, 0, 2, "lookup", "nostd", {}),                       # 1025 packets: 2 workgroups
    ("pl_c3_4x8_u8", "nchw", "u8", 3, 4, 8, 4, 0, 3, None, "explicit", {}),
    ("pl_c3_4x8_u16", "nchw", "u16", 3, 4, 8, 4, 0, 1, "lookup", "none", {"max_code": 4095.0}),
    ("pl_c2_86x3_u8", "nchw", "u8", 2, 86, 3, 86, 0, 2, "catmull", "nostd", {}),
    ("pl_c4_27x19_f32", "nchw", "f32", 4, 27, 19, 27, 0, 3, None, "multiplier", {}),
    ("pl_band_c3_4x8of6_u16", "nchw", "u16", 3, 4, 8, 6, 1, 3, "linear", "explicit", {}),                  # chan_skip % 3 = 1
    ("pl_band_c4_27x19of30_f32", "nchw", "f32", 4, 27, 19, 30, 2, 2, "catmull", "multiplier", {}),         # chan_skip % 4 = 1
    ("pl_band_c2_86x3of87_u8", "nchw", "u8", 2, 86, 3, 87, 1, 3, "linear", "constant", {}),                # chan_skip % 2 = 1
    ("pl_band_c4_27x19of29_u16", "nchw", "u16", 4, 27, 19, 29, 1, 2, "linear", "none", {"max_code": 4095.0}),  # chan_skip % 4 = 2
    ("pl_pad_c4_5x5_u8", "nchw", "u8", 4, 5, 5, 7, 1, 3, "catmull", "constant", {"pad": 4}),               # padded stride, planar kernel
    # ---- scalar, nchw: Q % 4 in {1, 2, 3} with every std mode, Q < 4, misaligned pointers
    ("sc_c1_5x5_u8", "nchw", "u8", 1, 5, 5, 5, 0, 3, "linear", "none", {}),
    ("sc_c1_5x5_u16", "nchw", "u16", 1, 5, 5, 5, 0, 2, "catmull", "constant", {}),
    ("sc_c1_5x5_f32", "nchw", "f32", 1, 5, 5, 5, 0, 3, None, "multiplier", {}),
    ("sc_c1_5x5_f32e", "nchw", "f32", 1, 5, 5, 5, 0, 2, "linear", "explicit", {}),
    ("sc_c2_7x9_u16", "nchw", "u16", 2, 7, 9, 7, 0, 3, "lookup", "none", {"max_code": 4095.0}),
    ("sc_c2_7x9_f32", "nchw", "f32", 2, 7, 9, 7, 0, 2, "linear", "constant", {}),
    ("sc_c2_7x9_u8", "nchw", "u8", 2, 7, 9, 7, 0, 3, "catmull", "multiplier", {}),
    ("sc_c2_7x9_u8e", "nchw", "u8", 2, 7, 9, 7, 0, 2, None, "explicit", {}),
    ("sc_c3_19x23_f32", "nchw", "f32", 3, 19, 23, 19, 0, 2, "catmull", "nostd", {}),
    ("sc_c3_19x23_u8", "nchw", "u8", 3, 19, 23, 19, 0, 3, None, "constant", {}),
    ("sc_c3_19x23_u16", "nchw", "u16", 3, 19, 23, 19, 0, 2, "linear", "multiplier", {}),
    ("sc_c3_19x23_u16e", "nchw", "u16", 3, 19, 23, 19, 0, 3, "catmull", "explicit", {"max_code": 4095.0}),
    ("sc_band_c3_19x23of21_u8", "nchw", "u8", 3, 19, 23, 21, 1, 2, "linear", "explicit", {}),              # chan_skip % 3 = 1
    ("sc_c1_1x3_f32", "nchw", "f32", 1, 1, 3, 1, 0, 8, "catmull", "constant", {}),                         # Q < 4
    ("sc_offset_c3_4x8_f32", "nchw", "f32", 3, 4, 8, 6, 1, 3, "linear", "multiplier", {"offset": 1}),      # a planar shape, pointer + 4 B
    ("sc_offset_c3_4x8_u8", "nchw", "u8", 3, 4, 8, 6, 1, 3, "catmull", "constant", {"offset": 1}),         # pointer + 1 B
    ("sc_slice_c3_5x7_f32", "nchw", "f32", 3, 5, 7, 5, 0, 3, "catmull", "explicit", {"slice": 1}),         # Q = 105: frames [1:]
    ("sc_slice_c3_5x7_u8", "nchw", "u8", 3, 5, 7, 5, 0, 3, "linear", "multiplier", {"slice": 1}),
    # ---- element-wise, interleaved: packet8
    ("p8_c4_5x6_u8", "nhwc", "u8", 4, 5, 6, 5, 0, 3, "linear", "constant", {}),
    ("p8_c1_4x10_u16", "nhwc", "u16", 1, 4, 10, 4, 0, 2, "catmull", "multiplier", {}),
    ("p8_c3_4x8_f32e", "nhwc", "f32", 3, 4, 8, 4, 0, 3, None, "explicit", {}),
    ("p8_c4_5x6_f32", "nhwc_bgr", "f32", 4, 5, 6, 5, 0, 2, "lookup", "none", {}),
    ("p8_c3_4x8_u8e", "nhwc_bgr", "u8", 3, 4, 8, 4, 0, 2, "catmull", "explicit", {}),
    ("p8_c1_4x10_f32", "nhwc", "f32", 1, 4, 10, 4, 0, 3, "linear", "nostd", {}),
    ("p8_band_c4_5x6of8_u16", "nhwc_bgr", "u16", 4, 5, 6, 8, 1, 3, "linear", "multiplier", {"max_code": 4095.0}),  # chan_skip % 4 = 2
    ("p8_band_c3_4x8of6_u16e", "nhwc", "u16", 3, 4, 8, 6, 1, 2, "linear", "explicit", {}),
    ("p8_band_c1_4x10of6_u8", "nhwc", "u8", 1, 4, 10, 6, 1, 2, None, "constant", {}),
    # ---- element-wise, interleaved: packet8 + tail (padded stride); planar frames behind such a stride: scalar, planar
    ("pt_c4_5x5_u8", "nhwc", "u8", 4, 5, 5, 5, 0, 3, "linear", "constant", {"pad": 4}),                    # 96 + 4
    ("pt_c1_5x7_u16", "nhwc", "u16", 1, 5, 7, 5, 0, 3, "catmull", "multiplier", {"pad": 5}),               # 32 + 3
    ("pt_c3_6x7_f32", "nhwc_bgr", "f32", 3, 6, 7, 6, 0, 2, "lookup", "none", {"pad": 2}),                  # plane % 4 != 0: 120 + 6
    ("pt_c3_6x7_f32n", "nhwc", "f32", 3, 6, 7, 6, 0, 3, None, "explicit", {"pad": 2}),
    ("pt_band_c3_6x7of9_u16e", "nhwc", "u16", 3, 6, 7, 9, 2, 3, "linear", "explicit", {"pad": 2, "max_code": 4095.0}),
    ("pt_band_c4_5x5of7_f32", "nhwc_bgr", "f32", 4, 5, 5, 7, 1, 2, "catmull", "nostd", {"pad": 4}),
    ("sc_band_pad_c3_5x7of7_u8", "nchw", "u8", 3, 5, 7, 7, 1, 3, "linear", "multiplier", {"pad": 7}),      # Q = 105, stride 112: scalar; chan_skip % 3 = 2
    ("pl_pad_band_c4_5x7of8_f32", "nchw", "f32", 4, 5, 7, 8, 2, 2, "catmull", "explicit", {"pad": 4}),    # Q = 140: padded stride, planar kernel
    ("sc_band_pad_c2_5x7of6_u16", "nchw", "u16", 2, 5, 7, 6, 1, 2, "catmull", "constant", {"pad": 2}),    # Q = 70, stride 72: scalar; chan_skip % 2 = 1
    # ---- element-wise, interleaved: scalar
    ("se_c4_5x5_u16", "nhwc", "u16", 4, 5, 5, 5, 0, 3, "linear", "constant", {}),
    ("se_c1_5x7_u8", "nhwc", "u8", 1, 5, 7, 5, 0, 2, "catmull", "multiplier", {}),
    ("se_c3_19x23_f32", "nhwc_bgr", "f32", 3, 19, 23, 19, 0, 2, "lookup", "nostd", {}),                   # C = 3, plane % 4 != 0
    ("se_c3_4x67_f32e", "nhwc_bgr", "f32", 3, 4, 67, 4, 0, 3, "catmull", "explicit", {}),                 # the rgb shape with an explicit std
    ("se_c3_19x23_u8", "nhwc", "u8", 3, 19, 23, 19, 0, 3, None, "none", {}),
    ("se_band_c4_5x5of7_u8", "nhwc_bgr", "u8", 4, 5, 5, 7, 1, 3, None, "explicit", {}),                   # chan_skip % 4 = 2
    ("se_band_c3_19x23of21_u16", "nhwc", "u16", 3, 19, 23, 21, 1, 2, "linear", "multiplier", {"max_code": 4095.0}),
    ("se_band_c3_4x67of5_u16e", "nhwc", "u16", 3, 4, 67, 5, 1, 2, "linear", "explicit", {}),
    ("se_band_c1_5x7of6_f32", "nhwc", "f32", 1, 5, 7, 6, 1, 3, "linear", "constant", {}),
]

# (name, layout, C, h, w): 2 * 65535 + 3 uint8 frames, so that a workgroup's `f += gridDim.y` walk runs three times
MANY_FRAMES_N = 2 * 65535 + 3
MANY_FRAMES = [("many_planar_1x1x4", "nchw", "u8", 1, 1, 4, 1, 0, MANY_FRAMES_N, "linear", "multiplier", {}),
               ("many_rgb_1x4x3", "nhwc", "u8", 3, 1, 4, 1, 0, MANY_FRAMES_N, "linear", "multiplier", {})]

ALL_FORWARD = FORWARD_CASES + MANY_FRAMES
FORWARD_NAMES = [c[0] for c in FORWARD_CASES]


@functools.lru_cache(maxsize=None)
def forward_case(name):
    """Namespace of a forward case: the fields of its row; planar_stored / x / sigma (F, C, h_global, w) for the WHOLE
    image (stored form, float32 pixels, float32 per-sample sigma or None); lut; seed.  The arrays are shared: do not
    write to them."""
    k = [c[0] for c in ALL_FORWARD].index(name)
    _, layout, dtype, C, h, w, hg, r0, F, mode, std, extras = ALL_FORWARD[k]
    cs = SimpleNamespace(name=name, layout=layout, dtype=dtype, C=C, h=h, w=w, hg=hg, r0=r0, F=F, mode=mode, std=std,
                         pad=extras.get("pad", 0), offset=extras.get("offset", 0), slice=extras.get("slice", 0),
                         seed=3000 + k)
    cs.max_code = None if dtype == "f32" else extras.get("max_code", 255.0 if dtype == "u8" else 65535.0)
    cs.L = _l_of(dtype, cs.max_code)
    cs.lut = case_lut(C, cs.L)
    cs.tile = None if hg == h else (hg, r0)
    cs.std_value = {"constant": STD_CONSTANT, "multiplier": STD_MULTIPLIER}.get(std, 0.0)
    rng = np.random.default_rng(cs.seed)
    shape = (F, C, hg, w)
    if dtype == "f32":
        stored = (rng.random(shape, dtype=np.float32) * np.float32(1.1) - np.float32(0.05)).astype(np.float32)
    else:
        stored = rng.integers(0, int(cs.max_code) + 1, size=shape).astype(NP_DTYPE[dtype])
    band = stored[:, :, r0:r0 + h]
    _place(band, edge_values(dtype, cs.max_code, cs.L))
    cs.planar_stored = stored
    cs.x = to_pixels(stored, dtype, cs.max_code)
    if std in ("nostd", "none"):
        cs.sigma = None
    elif std == "constant":
        cs.sigma = np.full(shape, np.float32(STD_CONSTANT), dtype=np.float32)
    elif std == "multiplier":
        cs.sigma = (cs.x * np.float32(STD_MULTIPLIER)).astype(np.float32)   # datasets/base.py:133, float32
    else:
        sg = (np.float32(0.02) * np.abs(cs.x) + np.float32(1e-3) + np.float32(2e-3) * rng.random(shape, dtype=np.float32)).astype(np.float32)
        n = sg[:, :, r0:r0 + h].size
        if n >= 8:   # zeros, and sigmas whose products are far below 1e-18 (denormal and vanishing squares)
            idx = np.unravel_index((np.arange(5) * (n // 5) + 1) % n, sg[:, :, r0:r0 + h].shape)
            sg[:, :, r0:r0 + h][idx] = np.array([0.0, 3e-20, 1e-30, 0.0, 2e-19], dtype=np.float32)
        cs.sigma = sg
    for a in (cs.planar_stored, cs.x, cs.lut) + (() if cs.sigma is None else (cs.sigma,)):
        a.setflags(write=False)
    return cs


def band_rows(a, cs):
    """Rows of the band of a planar (F, C, h_global, w) array."""
    return None if a is None else a[:, :, cs.r0:cs.r0 + cs.h]


def case_path(cs, band=True):
    """The launch path of a case's band (or of its whole image) as the tests run it: allocations are 256-byte aligned,
    outputs dense."""
    h = cs.h if band else cs.hg
    plane = h * cs.w
    Q = cs.C * plane
    size = ITEMSIZE[cs.dtype]
    al = {"frames": (cs.offset * size + cs.slice * Q * size) % 32, "lin": 0}
    if cs.std != "nostd":
        al["std_out"] = 0
    if cs.std == "explicit":
        al["std"] = (cs.offset * 4 + cs.slice * Q * 4) % 32
    return linearize_path_of(cs.dtype, cs.layout, cs.C, plane, Q, cs.F, cs.std, al, (Q + cs.pad, Q))


def case_edges(cs):
    """Which edge conditions the band of a case holds: name -> bool."""
    x, sg = band_rows(cs.x, cs), band_rows(cs.sigma, cs)
    top = cs.L - 1
    s = (x * np.float32(top)).astype(np.float32)
    knot = (s == np.floor(s)) & (s > 0) & (s < top)
    near = 1e-4 if cs.dtype == "f32" else 1.01 * top / cs.max_code     # one code, in units of the LUT coordinate
    inner = (s > 1) & (s < top) & ~knot
    out = {"zero": bool((x == 0).any()), "one": bool((x == 1).any()), "knot": bool(knot.any()),
           "below_knot": bool((inner & (np.ceil(s) - s <= near)).any()),
           "above_knot": bool((inner & (s - np.floor(s) <= near)).any()),
           "below_zero": bool((x < 0).any()), "above_one": bool((x > 1).any())}
    if sg is not None:
        _, gs = linearize_f64(x, sg, cs.lut, cs.mode, cs.tile)
        out["zero_std"] = bool((sg == 0).any())
        out["underflow"] = bool(((gs > 0) & (gs < 1e-18)).any())
    return out


# Cases with a propagated std (a gradient path and a sigma) whose band holds no 0 < |f'(x) sigma| < 1e-18: f' or sigma
# cannot get small enough there.  No model: f' = 1 against sigma = 0.01, or 0.05 x with x a whole code.  CATMULL on whole
# codes with sigma = 0.05 x: f' is tiny only at x = 0 (the 1e-19 knot), where that sigma is 0.  Every other such case must
# hold the edge, and the host test checks that this list is exact.
NO_UNDERFLOW = ("rgb_4x8_bgr_f32", "sc_c3_19x23_u8", "p8_band_c1_4x10of6_u8",                                  # no model, 0.01
                "rgb_4x67_nhwc_u16",                                                                          # no model, 0.05 x
                "rgb_4x8_bgr_u16", "rgb_band_4x8of7_bgr_u8", "sc_c2_7x9_u8", "p8_c1_4x10_u16", "pt_c1_5x7_u16",
                "se_c1_5x7_u8")                                                                               # CATMULL, 0.05 x


def edge_applies(cs, edge):
    """Whether the band of a case must hold an edge condition."""
    if edge == "below_zero":
        return cs.dtype == "f32"
    if edge == "above_one":
        return cs.dtype == "f32" or (cs.dtype == "u16" and cs.max_code == 4095.0)
    if edge == "zero_std":            # a constant sigma is never 0; multiplier: at x = 0
        return cs.std in ("multiplier", "explicit")
    if edge == "underflow":
        return cs.name not in NO_UNDERFLOW
    return True


def std_kwargs(cs, sigma_dev):
    """How a case's std source is handed to ops.linearize_frames (sigma_dev: the explicit stack in the frames' layout)."""
    if cs.std == "nostd":
        return dict(want_std=False)
    if cs.std == "explicit":
        return dict(std=sigma_dev)
    return dict(std_mode=cs.std, std_value=cs.std_value)


# ---- backward cases ------------------------------------------------------------------------------------------------
# (name, mode, C, h_global, w, split, n_images, L): the whole image and its two bands [0, split) and [split, h_global).
# Every mode meets C = 1, 3, 4 and n_images = 1, 8, 11 (grid.y is capped at 8); for C = 3, 4 both bands have
# chan_skip % C != 0 and the second one base % C != 0.  "repeat": 98304 B of LDS, one workgroup per compute unit, grid.x
# capped at 256 / 8 = 32 on 256 compute units, 8241 > 32 * 256 elements per image: the grid-stride loop runs twice.
BACKWARD_CASES = [
    ("bw_lookup_c1", "lookup", 1, 17, 13, 5, 8, 52),
    ("bw_lookup_c3", "lookup", 3, 17, 13, 7, 11, 64),
    ("bw_lookup_c4", "lookup", 4, 9, 7, 3, 1, 33),
    ("bw_linear_c1", "linear", 1, 9, 7, 4, 11, 33),
    ("bw_linear_c3", "linear", 3, 17, 13, 7, 1, 64),
    ("bw_linear_c4", "linear", 4, 9, 7, 3, 8, 52),
    ("bw_catmull_c1", "catmull", 1, 17, 13, 5, 1, 64),
    ("bw_catmull_c3", "catmull", 3, 17, 13, 7, 8, 33),
    ("bw_catmull_c4", "catmull", 4, 9, 7, 3, 11, 52),
    ("bw_repeat_linear_c3", "linear", 3, 41, 67, 19, 8, 2048),
    # ---- cases that put weight on the flush of the LUT gradient (BACKWARD_KIND; conditions asserted on the CPU from
    # bwd_partials by test_linearize_refs_host.py::test_flush_cases_hold_their_conditions)
    # "hot": L = 9, so 8 workgroups fit a compute unit and grid.x is Q / 256 uncapped; three quarters of the pixels sit at
    # x = 0.55 (LUT coordinate 4.4), so every one of the gx * 8 >= 64 workgroups flushes a nonzero partial into the same
    # bins: the largest m the kernel produces at test size
    ("bw_hot_lookup_c1", "lookup", 1, 32, 64, 13, 8, 9),        # gx = 8: 64 workgroups
    ("bw_hot_linear_c3", "linear", 3, 24, 32, 11, 8, 9),        # gx = 9: 72 workgroups, one hot interval per LUT row
    ("bw_hot_catmull_c2", "catmull", 2, 32, 40, 13, 11, 9),     # gx = 10: 80 workgroups, two images per workgroup for some
    # "cancel": images 4..7 repeat the pixels of images 0..3 (other workgroups: grid.y = 8), and where x < 0.4 their
    # upstream gradient is minus that of images 0..3 up to 1e-4: the bins below 0.4 (L - 1) cancel to |S| < 1e-3 A
    ("bw_cancel_linear_c3", "linear", 3, 17, 29, 7, 8, 64),
    # "untouched": x in [0.3, 0.6], so the bins below and above get nothing; C = 4 and w = 2 with an even h_global, so the
    # one-row band [0, 1) reaches LUT rows 0 and 1 only (row = 2 ((c h_global + y) % 2) + x) and rows 2, 3 stay empty
    ("bw_untouched_catmull_c4", "catmull", 4, 64, 2, 1, 8, 64),
]
BACKWARD_NAMES = [c[0] for c in BACKWARD_CASES]
BACKWARD_KIND = {n: ({"hot": "hot", "cancel": "cancel", "untouched": "untouched"}.get(n.split("_")[1], "plain")) for n in BACKWARD_NAMES}
HOT_X = np.float32(0.55)


@functools.lru_cache(maxsize=None)
def backward_case(name):
    """Namespace: mode, C, hg, w, split, N, L, kind, lut, x and grad_out (N, C, hg, w) float32 (x with the float32 edge
    values, below 0 and above 1 included; not for kind "untouched", whose x stays in [0.3, 0.6]), seed.  Shared arrays: do
    not write to them."""
    k = BACKWARD_NAMES.index(name)
    _, mode, C, hg, w, split, N, L = BACKWARD_CASES[k]
    cs = SimpleNamespace(name=name, mode=mode, C=C, hg=hg, w=w, split=split, N=N, L=L, seed=5000 + k, kind=BACKWARD_KIND[name])
    g = np.linspace(0.0, 1.0, L, dtype=np.float64)
    cs.lut = np.stack([g ** p for p in (1.5, 2.0, 2.5, 3.0)[:C]]).astype(np.float32)
    rng = np.random.default_rng(cs.seed)
    x = (rng.random((N, C, hg, w), dtype=np.float32) * np.float32(1.1) - np.float32(0.05)).astype(np.float32)
    go = rng.standard_normal((N, C, hg, w), dtype=np.float32)
    if cs.kind == "hot":
        x[rng.random(x.shape) < 0.75] = HOT_X
    elif cs.kind == "cancel":
        half = N // 2
        x[half:] = x[:half]
        delta = (np.float32(1) + np.float32(1e-4) * rng.standard_normal(x[:half].shape, dtype=np.float32)).astype(np.float32)
        go[half:] = np.where(x[:half] < np.float32(0.4), -(go[:half] * delta), go[half:]).astype(np.float32)
    elif cs.kind == "untouched":
        x = (np.float32(0.3) + np.float32(0.3) * rng.random(x.shape, dtype=np.float32)).astype(np.float32)
    if cs.kind != "untouched":
        edges = edge_values("f32", None, L)
        for lo, hi in ((0, split), (split, hg)):
            _place(x[:, :, lo:hi], edges)     # (cancel: an edge value breaks its pair, 26 of 5916)
    cs.x = x
    cs.grad_out = go
    for a in (cs.lut, cs.x, cs.grad_out):
        a.setflags(write=False)
    return cs


def eager_backward(cs, r0, rows):
    """(grad_x rows | None, lut_grad) of the float32 eager oracle (autograd of oe.icrf_forward) run on the WHOLE image with
    the upstream gradient zero outside rows [r0, r0 + rows).  On one thread: the scatter-add of the LUT gradient is an
    atomic float32 sum whose order (and last bits) would otherwise change from run to run."""
    import torch
    from oracle import eager_torch as oe
    go = np.zeros_like(cs.grad_out)
    go[:, :, r0:r0 + rows] = cs.grad_out[:, :, r0:r0 + rows]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        x = torch.from_numpy(cs.x.copy()).requires_grad_(cs.mode != "lookup")
        lut = torch.from_numpy(cs.lut.copy()).requires_grad_(True)
        grads = torch.autograd.grad(oe.icrf_forward(x, lut, cs.mode), [lut] + ([x] if cs.mode != "lookup" else []), torch.from_numpy(go))
    finally:
        torch.set_num_threads(threads)
    return (grads[1].numpy()[:, :, r0:r0 + rows] if cs.mode != "lookup" else None), grads[0].numpy()


def backward_bands(cs):
    """[(label, row 0, rows, tile)] of a backward case: the whole image and its two bands."""
    return [("whole", 0, cs.hg, None), ("band0", 0, cs.split, (cs.hg, 0)), ("band1", cs.split, cs.hg - cs.split, (cs.hg, cs.split))]


def flush_bound(abs_bins, workgroups):
    """Bound on |float32 lut_grad - exact sum of the float32 products| per bin, from linearize_bwd_kernel: a workgroup adds
    its samples' float32 products in a float64 LDS histogram (n 2^-53: nothing), rounds each bin to float32 once (2^-24 of
    its partial sum) and adds it to the output with a float32 atomic (2^-24 of the running sum, once per workgroup).
    Every partial and running sum is at most abs_bins = sum |product| in magnitude, so the error of one launch is at most
    (workgroups + 1) 2^-24 abs_bins, whatever the order of the flushes.  (1.001: abs_bins comes from the float64
    reference, the products are float32.)"""
    return (workgroups + 1) * 2.0 ** -24 * np.asarray(abs_bins) * 1.001


# ---- the summation of linearize_bwd_kernel, restated ---------------------------------------------------------------
_U = 2.0 ** -24          # unit roundoff of float32
_CATMULL_COEF = ((-0.5, 1.0, -0.5, 0.0), (1.5, -2.5, 0.0, 1.0), (-1.5, 2.0, 0.5, 0.0), (0.5, -0.5, 0.0, 0.0))   # t^3, t^2, t, 1


def _bwd_products(x, go, L, mode):
    """[(bin index, float32 product, slack, rounding)] per tap, for the samples x / go (any shape, float32), formed as
    linearize_bwd_kernel forms them.  LOOKUP (go itself) and LINEAR (fl(go fl(1 - t)), fl(go t)) are restated bit for bit:
    x * top, the clamp, floor, s - floor(s) (exact), 1 - t and the two products are single float32 operations with
    nothing for the compiler to contract; slack None.  CATMULL: the weights are the float32 left-to-right evaluation of
    the polynomials, which the compiler may contract into FMAs in several ways; slack bounds |kernel's product - this
    product| (see order_bound).  rounding bounds |this product - go * (the exact weight of the float32 t)|: 0 for LOOKUP,
    2 roundings of the product for LINEAR (1 - t and the product), the weight's 6 2^-24 T and the product's own for
    CATMULL."""
    top = np.float32(L - 1)
    s = (x * top).astype(np.float32)
    if mode == "lookup":
        r = np.minimum(np.maximum(np.rint(s), np.float32(0)), top)
        return [(r.astype(np.int64), go, None, np.zeros(go.shape))]
    s = np.minimum(np.maximum(s, np.float32(0)), top)
    fl = np.floor(s)
    i0 = fl.astype(np.int64)
    t = (s - fl).astype(np.float32)
    if mode == "linear":
        p0, p1 = (go * (np.float32(1) - t).astype(np.float32)).astype(np.float32), (go * t).astype(np.float32)
        return [(i0, p0, None, 2.001 * _U * np.abs(p0.astype(np.float64))),
                (np.minimum(i0 + 1, L - 1), p1, None, _U * np.abs(p1.astype(np.float64)))]
    t2 = (t * t).astype(np.float32)
    t3 = (t2 * t).astype(np.float32)
    f = np.float32
    w = ((f(-0.5) * t3 + t2) - f(0.5) * t, (f(1.5) * t3 - f(2.5) * t2) + f(1.0), (f(-1.5) * t3 + f(2.0) * t2) + f(0.5) * t, f(0.5) * t3 - f(0.5) * t2)
    t64 = t.astype(np.float64)
    ago = np.abs(go.astype(np.float64))
    out = []
    for wk, coef, idx in zip(w, _CATMULL_COEF, (np.maximum(i0 - 1, 0), i0, np.minimum(i0 + 1, L - 1), np.minimum(i0 + 2, L - 1))):
        assert wk.dtype == np.float32
        terms = abs(coef[0]) * t64 ** 3 + abs(coef[1]) * t64 ** 2 + abs(coef[2]) * t64 + abs(coef[3])
        has_sum = sum(c != 0 for c in coef) > 1          # (every weight here is a sum; kept for the derivation's sake)
        slack = ago * (15 * _U * terms * has_sum) + (ago + 1) * 2.0 ** -126 * (t64 != 0)
        out.append((idx, (go * wk).astype(np.float32), slack, ago * 7.001 * _U * terms + (ago + 1) * 2.0 ** -126))
    return out


def bwd_partials(cs, r0, rows, tile, compute_units):
    """What every workgroup of linearize_bwd_kernel flushes into every bin for rows [r0, r0 + rows) of a backward case,
    restated from the kernel and bwd_launch (bwd_grid_of).  Workgroup (bx, by) owns the elements q = bx 256 + tid,
    += gx 256 of the images n = by, += gy; the LUT row of an element is lut_rows; the products are those of
    _bwd_products; a workgroup adds them per bin in float64 (the LDS histogram) and rounds the bin to float32 once.
    Namespace: grid; partials (gx gy, C, L) float32 in the order by * gx + bx; per bin m (nonzero partials), A (sum
    |partial|), S (float64 sum of the partials: what the flushes add up to before their own rounding), E (how far S may
    be from the float64 reference icrf_backward_f64: the roundings of the float32 products, _bwd_products, and 2^-24 A for
    the rounding of the partials); slack (gx gy, C, L) float64, how far the kernel's partial may be from this one
    (order_bound)."""
    x = np.ascontiguousarray(cs.x[:, :, r0:r0 + rows])
    go = np.ascontiguousarray(cs.grad_out[:, :, r0:r0 + rows])
    N, C, h, w = x.shape
    Q, L = C * h * w, cs.L
    grid = bwd_grid_of(Q, N, C, L, cs.mode, compute_units)
    W = grid.gx * grid.gy
    bx = (np.arange(Q, dtype=np.int64) // 256) % grid.gx
    by = np.arange(N, dtype=np.int64) % grid.gy
    wg = by[:, None] * grid.gx + bx[None, :]
    row = lut_rows(C, h, w, cs.mode, tile).reshape(1, Q)
    base = ((wg * C + row) * L).reshape(-1)
    size = W * C * L
    total, absolute, count, loose = np.zeros(size), np.zeros(size), np.zeros(size, dtype=np.int64), np.zeros(size)
    rounding = np.zeros(C * L)
    for idx, prod, slack, rnd in _bwd_products(x.reshape(N, Q), go.reshape(N, Q), L, cs.mode):
        assert prod.dtype == np.float32
        flat, p64 = base + idx.reshape(-1), prod.reshape(-1).astype(np.float64)
        total += np.bincount(flat, weights=p64, minlength=size)
        absolute += np.bincount(flat, weights=np.abs(p64), minlength=size)
        count += np.bincount(flat, weights=(p64 != 0), minlength=size).astype(np.int64)
        if slack is not None:
            loose += np.bincount(flat, weights=slack.reshape(-1), minlength=size)
        rounding += np.bincount((np.broadcast_to(row, idx.shape) * L + idx).reshape(-1), weights=rnd.reshape(-1), minlength=C * L)
    partials = total.astype(np.float32)
    # the float64 LDS atomics are unordered too: a sum of n float32 products moves by at most n 2^-53 of sum |product|, and
    # the rounding of the bin to float32 turns that (and the CATMULL slack) into at most one float32 spacing more.  One
    # product is its own sum: exact.
    moved = loose + 2 * count * 2.0 ** -53 * absolute
    slack = np.where((count > 1) | (loose > 0), moved + 2.0 ** -23 * (np.abs(partials) + moved) + 2.0 ** -149, 0.0)
    shape = (W, C, L)
    partials, slack = partials.reshape(shape), slack.reshape(shape)
    p64 = partials.astype(np.float64)
    A = np.abs(p64).sum(axis=0)
    E = rounding.reshape(C, L) + _U * A + N * Q * 2.0 ** -51 * absolute.reshape(shape).sum(axis=0)
    return SimpleNamespace(grid=grid, partials=partials, slack=slack, m=(partials != 0).sum(axis=0), A=A, S=p64.sum(axis=0), E=E)


def flush_in_order(partials, order):
    """The float32 lut_grad that the flushes of `partials` (workgroups, C, L) give in a given order: np.float32 adds to a
    zero-filled output, zero partials skipped as the kernel skips them (adding them would change nothing).  order: a
    permutation of the workgroups, or a (workgroups, C, L) integer array holding one permutation per bin."""
    order = np.asarray(order)
    p = partials[order] if order.ndim == 1 else np.take_along_axis(partials, order, axis=0)
    assert p.dtype == np.float32
    acc = np.zeros(p.shape[1:], dtype=np.float32)
    for k in range(p.shape[0]):
        acc = acc + p[k]
    return acc


# The flush-order study of test_linearize_refs_host.py (test_every_flush_order_stays_within_order_bound): the whole image
# and both bands of every backward case on 256 compute units; the workgroups ascending and descending, 24 seeded random
# orders of the workgroups, 8 seeded random orders per bin, and per bin the adversarial orders (positive partials first,
# ascending magnitude, descending value, and the reverse of each).  The study re-measures these figures (to 2 %).
# ORDER_BOUND_USED: the largest |flush_in_order - S| / order_bound: the bound is not vacuous, an order uses this share of
# it.  (0: one workgroup, nothing to order.  CATMULL and m >= 64 use least: 15 roundings of slack per product where one or
# two occur, and a bound linear in m.)
ORDER_BOUND_USED = {
    "bw_lookup_c1": 0.6406, "bw_lookup_c3": 0.3385, "bw_lookup_c4": 0.0,           # band0 ascending / band0 per bin#2 / -
    "bw_linear_c1": 0.2915, "bw_linear_c3": 0.9026, "bw_linear_c4": 0.9784,        # band0 / band1 / band0, all ascending
    "bw_catmull_c1": 0.0, "bw_catmull_c3": 0.0345, "bw_catmull_c4": 0.0747,        # - / band1 descending magnitude / band0 ascending value
    "bw_repeat_linear_c3": 0.9549,                                                 # band0 ascending
    "bw_hot_lookup_c1": 0.0981, "bw_hot_linear_c3": 0.0913, "bw_hot_catmull_c2": 0.0257,   # descending / ascending / descending value
    "bw_cancel_linear_c3": 0.2278, "bw_untouched_catmull_c4": 0.0405,              # band1 descending value / band0 workgroups#18
}
# FLUSH_SHARE_OF_TOL: the largest share of TOL[("lut_grad", mode)] (element, norm-wise) that some order uses against the
# float64 reference.  TOL is 4x the error of ONE order (the sequential scatter-add of the CPU oracle); a case whose worst
# order leaves less than that factor 4 (a share above 0.25) is not compared at TOL on the GPU, where the order is the
# scheduler's, but by assert_flush and norm-wise at TOL[("lut_grad any order", case)] (flush_keeps_margin).
# bw_repeat_linear_c3, whole image: per bin positive partials first gives an element error of 3.202e-5 = 3.23 TOL (the bins
# at both ends of the LUT, where the 5 % of samples below 0 and above 1 pile up 250 sign-mixed partials that cancel
# 30-fold); descending value, reversed, a norm-wise error of 1.060e-6 = 2.0 TOL; the worst of the 32 random orders 6.1e-6 =
# 0.62 TOL.  bw_untouched_catmull_c4: the median |ref| is 0, so the element measure is relative to |ref| alone.
FLUSH_SHARE_OF_TOL = {
    "bw_lookup_c1": (0.1347, 0.1902), "bw_lookup_c3": (0.2296, 0.2025), "bw_lookup_c4": (0.0316, 0.0520),
    "bw_linear_c1": (0.0318, 0.2015), "bw_linear_c3": (0.0208, 0.0914), "bw_linear_c4": (0.0283, 0.1615),
    "bw_catmull_c1": (0.2478, 0.1016), "bw_catmull_c3": (0.3014, 0.2682), "bw_catmull_c4": (0.1360, 0.1295),
    "bw_repeat_linear_c3": (3.2345, 2.0006),
    "bw_hot_lookup_c1": (0.9695, 3.3307), "bw_hot_linear_c3": (0.1619, 1.6389), "bw_hot_catmull_c2": (0.5371, 0.8311),
    "bw_cancel_linear_c3": (0.3413, 0.7828), "bw_untouched_catmull_c4": (730.5, 0.2224),
}
# Where order_bound replaces the element test of TOL: (least share of the touched bins whose allowance got smaller, largest
# factor by which one got larger), over the whole image and both bands; old allowance TOL (|ref| + median |ref|).  Bins
# that nothing reaches had an allowance and now have none.  The large factors are bins whose partials cancel (|ref| far
# below A: no tolerance relative to |ref| holds in every order there) and, for CATMULL, the contraction slack.
ALLOWANCE_VS_TOL = {
    "bw_catmull_c3": (0.0, 14.8), "bw_repeat_linear_c3": (0.996, 248.0), "bw_hot_lookup_c1": (0.0, 43.2),
    "bw_hot_linear_c3": (0.111, 5.31), "bw_hot_catmull_c2": (0.0, 141.4), "bw_cancel_linear_c3": (0.213, 17.0),
    "bw_untouched_catmull_c4": (0.0, 7.2e5),
}


def flush_keeps_margin(name):
    """Whether every studied flush order of a backward case leaves the factor 4 of TOL[("lut_grad", mode)] in both measures."""
    return max(FLUSH_SHARE_OF_TOL[name]) * 4 <= 1


def order_bound(parts):
    """Per-bin bound on |float32 lut_grad - parts.S| of one launch of linearize_bwd_kernel, whatever the order in which
    its workgroups flush; parts from bwd_partials.  From the code:

    * lut_grad is zero-filled; a workgroup flushes v = (float)hist[k] with atomicAdd(&lut_grad[k], v) unless v == 0.  With
      the partials v_1..v_m of a bin given, the first add (to +0.0) is exact and each of the other m - 1 rounds a running
      sum r to float32: an error of at most 2^-24 |r|, and |r| <= A (1 + 2^-24)^m with A = sum |v_j|, in every order.
      Hence |lut_grad - sum v_j| <= (m - 1) 2^-24 A (1 + m 2^-24).
    * What the restatement cannot pin is whether the kernel's v_j are parts.partials (parts.slack, per workgroup and bin):
      - LOOKUP, LINEAR: the products are restated bit for bit (_bwd_products), so only the order of the float64 LDS atomics
        is left.  A float64 sum of n float32 products moves by at most n 2^-53 sum |product| between two orders, which
        changes its float32 rounding only at a rounding tie, and then by one spacing: slack = 2^-23 |v| (+ twice that
        movement, + 2^-149), and 0 where a workgroup has one nonzero product for the bin (its sum is the product) or none.
      - CATMULL: with t2 = fl(t t), t3 = fl(t2 t) (relative errors 2^-24 and 2 2^-24; no addition to contract with), a
        weight sum_k c_k t^k of at most three nonzero terms is evaluated with one rounding per coefficient product (none if
        it is contracted or c_k is a power of two) and two additions, each rounding a partial sum of at most T = sum_k
        |c_k| t^k: |w - exact| <= (3 + 2) 2^-24 T, taken as 6 2^-24 T, for every contraction.  Two evaluations differ by at
        most 12 2^-24 T, their products with go by 12 2^-24 |go| T plus the two product roundings, 2 2^-24 |go| T: taken
        as 15 2^-24 |go| T per tap, plus (|go| + 1) 2^-126 for t so small that t^2, t^3 or the product underflow.  These
        add up over a workgroup's samples, and the rounding of the bin adds one spacing as above.
      A partial that may be nonzero in the kernel (slack > 0) counts in m; A takes the slacks in.
    * bound = (m - 1) 2^-24 A (1 + m 2^-24) + sum of the slacks.  A bin no workgroup has a nonzero product for has bound 0:
      the kernel skips zero partials, so the zero-filled +0.0 stays.  A bin with m = 1 has only its slack.
    Measured use of the bound: ORDER_BOUND_USED above."""
    live = (parts.partials != 0) | (parts.slack > 0)
    m = live.sum(axis=0)
    loose = parts.slack.sum(axis=0)
    a = parts.A + loose
    return np.where(m > 0, np.maximum(m - 1, 0) * _U * a * (1 + m * _U) + loose, 0.0)


def assert_flush(got, parts, what):
    """The order-free assertions on a float32 lut_grad of one launch, against bwd_partials: every bin within order_bound of
    parts.S; a bin no workgroup has a nonzero product for is +0.0 (bound 0, and no sign bit); a bin one workgroup feeds is
    that workgroup's partial up to its slack (its bound: there is no add to round).  Returns the largest |error| / bound."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == parts.S.shape, what
    bound = order_bound(parts)
    err = np.abs(got.astype(np.float64) - parts.S)
    live = ((parts.partials != 0) | (parts.slack > 0)).sum(axis=0)
    empty, single = live == 0, live == 1
    assert not got[empty].any() and not np.signbit(got[empty]).any(), f"{what}: {int((got[empty] != 0).sum())} untouched bins are not +0.0"
    one = np.abs(got.astype(np.float64) - parts.partials.astype(np.float64).sum(axis=0))[single]
    assert np.all(one <= parts.slack.sum(axis=0)[single]), f"{what}: {int((one > parts.slack.sum(axis=0)[single]).sum())} bins of one partial differ from it"
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} bins beyond order_bound, worst |error| / bound "
                           f"{float(np.max(err[bad] / bound[bad])) if np.all(bound[bad] > 0) else float('inf'):.3f}")
    return float(np.max(err / np.where(bound > 0, bound, 1.0)))


def check_lut_grad(got, cs, parts, ref, what):
    """A float32 lut_grad of one launch on a band of a backward case: the order-free assertions (assert_flush, its use of the
    bound recorded in _util.OBSERVED as "elem" against an "elem_tol" of 1), and against the float64 reference ref at
    TOL[("lut_grad", mode)] where every flush order keeps that tolerance's margin, else norm-wise at
    TOL[("lut_grad any order", case)]."""
    import os
    from _util import OBSERVED, rel_norm
    used = assert_flush(got, parts, what)
    test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0].split("::")[-1].split("[")[0]
    OBSERVED.append({"test": test, "what": what + " |error| / order_bound", "norm": rel_norm(got, parts.S) if parts.S.any() else 0.0, "norm_tol": 0.0,
                     "elem": used, "elem_tol": 1.0, "n": int(parts.S.size)})
    if flush_keeps_margin(cs.name):
        check(got, ref, ("lut_grad", cs.mode), what + " vs f64")
    else:
        norm_tol = TOL[("lut_grad any order", cs.name)][1]
        norm = rel_norm(got, ref)
        OBSERVED.append({"test": test, "what": what + " vs f64, norm-wise", "norm": norm, "norm_tol": norm_tol, "elem": 0.0, "elem_tol": 1.0, "n": int(ref.size)})
        assert norm <= norm_tol, f"{what}: norm-wise rel error {norm:.3e} > {norm_tol:.1e}"
    return used
