"""Plain float64 references of the four side kernels (ct_video_stats_batch, ct_flatfield_sums / ct_flatfield_apply,
ct_band_stats, ct_dark_field_blur), the seeded inputs and the tolerances their tests share.

NumPy only, no device code, written from the formulas in include/clair_hip.h and the kernel headers and calling none of
the code under test.  tests/test_side_refs_host.py validates every function against the pinned oracles on the CPU and
measures the tolerances below; tests/test_gpu_side_kernels.py compares the kernels with them."""
import itertools
import math

import numpy as np

# ---- tolerances ----------------------------------------------------------------------------------------------------
# Each is 4x what the float32 form of the same operation (the reference's precision and order of operations: the pinned
# oracle, or a restatement of it where the oracle lacks a flag) shows against the float64 reference on every input the GPU
# test uses, the large ones included, in the element metric of _util.assert_parity: |got - ref| / (|ref| + median|ref|).
# test_side_refs_host.py re-measures every one of them and asserts measured * 4 <= tolerance.
VIDEO_MEAN_TOL = 5.1e-7   # measured 1.261e-7 (oe.video_mean_std over every case of video_cases() and VIDEO_SPECIAL)
VIDEO_STD_TOL = 4.7e-7    # measured 1.167e-7
FLAT_VALUE_TOL = 2.8e-7   # measured 6.83e-8 (float32 values of FLAT_CASES and FLAT_LARGE, every flag honoured; float64 values
                          # are at 1e-16, and the flat field's float32 mean may differ in its last bit, 6e-8)
FLAT_STD_TOL = 4.6e-7     # measured 1.139e-7 (the same cases; the worst is the 725 x 725 plane, 7.1e-8 on the small ones)
DARK_XB_TOL = 5.1e-7      # measured 1.264e-7 (oe.conditional_gaussian_blur on DARK_CASES and DARK_EXTRA; 9.5e-8 on the small ones)
DARK_SIGMA_TOL = 2.5e-6   # measured 6.20e-7 (float32 restatement of sqrt(sigma^2 + (dterm sigma_D)^2) from oe.gaussian_blur3;
                          # the worst is CT_STD_NONE, where sigma_eff = |dterm sigma_D| keeps the cancellation of blur(x) - x)


def sum_tol(n, abs_sum):
    """Error bound of any order of n float64 additions: n 2^-53 relative to sum |x| (derived, not measured)."""
    return n * 2.0 ** -53 * abs_sum


# ---- video statistics ----------------------------------------------------------------------------------------------
def video_stats_f64(x_lin, batch_sizes):
    """Per-pixel mean and standard deviation of the mean, sqrt(m2 / (n - 1)) / sqrt(n), over the first sum(batch_sizes)
    frames of x_lin (N, C, H, W) in float64.  The batches only say how many frames there are: the exact result does not
    depend on how the frames are grouped."""
    n = int(sum(batch_sizes))
    x = np.asarray(x_lin, dtype=np.float64)[:n]
    mean = x.sum(axis=0) / n
    m2 = ((x - mean) ** 2).sum(axis=0)
    return mean, np.sqrt(m2 / (n - 1)) / math.sqrt(n)


VIDEO_SCHEDULES = [(16,), (17,), (32,), (33,), (1, 40), (5, 17, 2), (3, 16)]
VIDEO_SHAPES = [(3, 20, 23), (3, 5, 7), (1, 1, 3), (1, 4, 8)]
VIDEO_MODES = [None, "lookup", "linear", "catmull"]
VIDEO_DTYPES = ["u8", "u16", "f32"]


def video_kernel_of(batch):
    """Which kernel ct_video_stats_batch launches for a batch (ct_stats.hip, stats_launch_layout)."""
    return "cached16" if batch <= 16 else ("cached32" if batch <= 32 else "twopass")


def video_cases():
    """(schedule, shape, mode, dtype) for every schedule x shape, the mode and dtype rotated so that every kernel meets
    every mode and every dtype and every mode meets every dtype (test_side_refs_host.py checks the coverage)."""
    out = []
    for (s, sched), (j, shape) in itertools.product(enumerate(VIDEO_SCHEDULES), enumerate(VIDEO_SHAPES)):
        out.append((sched, shape, VIDEO_MODES[(s + j) % 4], VIDEO_DTYPES[(s + s // 3 + 2 * j + j // 2) % 3]))
    return out


def video_lut(channels, n_points=256):
    """(C, L) float32 gamma curves, one distinct row per channel so that a wrong row shows."""
    g = np.linspace(0.0, 1.0, n_points, dtype=np.float64)
    return np.stack([g ** p for p in (1.8, 2.2, 2.6)[:channels]]).astype(np.float32)


def video_frames(seed, n, shape, dtype, max_code=None):
    """n frames of `shape`, every sample drawn uniformly over the whole code range (the per-pixel standard deviation
    is then far from cancellation).  Returns (stored frames, float32 pixel values as Normalize(0, max_code) gives them)."""
    rng = np.random.default_rng(seed)
    if dtype == "f32":
        x = rng.random((n,) + tuple(shape), dtype=np.float32)
        return x, x
    np_t, top = (np.uint8, 255) if dtype == "u8" else (np.uint16, 65535)
    top = int(max_code) if max_code is not None else top
    codes = rng.integers(0, top + 1, size=(n,) + tuple(shape)).astype(np_t)
    return codes, (codes.astype(np.float32) / np.float32(top)).astype(np.float32)


def video_seed(k):
    return 100 + k


# (name, schedule, shape, mode, dtype, max_code): the cases of the GPU test outside video_cases(); seeds 200 + index
VIDEO_SPECIAL = [("max4095", (5, 17, 2), (3, 5, 7), "linear", "u16", 4095.0),
                 ("band", (3, 16), (3, 20, 23), "catmull", "u16", None),
                 ("padded_stride", (17,), (3, 5, 7), "linear", "u8", None),
                 ("frames_offset", (33,), (3, 4, 8), "lookup", "f32", None),
                 ("state_offset", (1, 40), (3, 4, 8), "catmull", "u16", None)]


# ---- flat field ----------------------------------------------------------------------------------------------------
def _flat_den(flat):
    # the reference forms flat + 1e-6 on its float32 flat-field tensor: the denominator IS that float32 sum
    return (np.asarray(flat, dtype=np.float32) + np.float32(1e-6)).astype(np.float64)


def flatfield_sums_f64(value, flat):
    """(C, 2) float64 = [sum flat, sum value / (flat + 1e-6)] per channel, exactly summed (math.fsum); value (C, H, W)
    or None (the second column is then 0)."""
    flat = np.asarray(flat, dtype=np.float32)
    c = flat.shape[0]
    den = _flat_den(flat).reshape(c, -1)
    out = np.zeros((c, 2), dtype=np.float64)
    for k in range(c):
        out[k, 0] = math.fsum(flat[k].astype(np.float64).ravel())
        if value is not None:
            out[k, 1] = math.fsum(np.asarray(value, dtype=np.float64).reshape(c, -1)[k] / den[k])
    return out


def flatfield_f64(value, var_or_std, flat, flat_std, M, through, input_is_variance):
    """ct_flatfield_apply in float64: value (C, H, W) or (F, C, H, W); M (C) the flat field's mean, through (C) or None.
        value' = value / (flat + 1e-6) * M
        grad   = -value * M / (flat + 1e-6)^2 + through[c]
        std'   = sqrt(var + (grad * flat_std)^2),  var = var_or_std or var_or_std^2
    Returns (value', std' or None)."""
    v = np.asarray(value, dtype=np.float64)
    c = v.shape[-3]
    den = _flat_den(flat)
    m = np.asarray(M, dtype=np.float64).reshape(c, 1, 1)
    out = v / den * m
    if var_or_std is None:
        return out, None
    var = np.asarray(var_or_std, dtype=np.float64)
    if not input_is_variance:
        var = var * var
    if flat_std is not None:
        grad = -v * m / (den * den)
        if through is not None:
            grad = grad + np.asarray(through, dtype=np.float64).reshape(c, 1, 1)
        var = var + (grad * np.asarray(flat_std, dtype=np.float64)) ** 2
    return out, np.sqrt(var)


def flatfield_inputs(seed, frames, shape, f64):
    """value ((F,) C, H, W), its std, flat in [0.5, 1), flat_std: seeded, the same on the host and in the GPU test."""
    rng = np.random.default_rng(seed)
    full = (tuple(shape) if frames is None else (frames,) + tuple(shape))
    value = rng.random(full) if f64 else rng.random(full, dtype=np.float32)
    std = (np.float32(0.002) + np.float32(0.03) * rng.random(full, dtype=np.float32)).astype(np.float32)
    flat = (np.float32(0.5) + np.float32(0.5) * rng.random(shape, dtype=np.float32)).astype(np.float32)
    flat_std = (np.float32(0.001) + np.float32(0.01) * rng.random(shape, dtype=np.float32)).astype(np.float32)
    return value, std, flat, flat_std


# (name, value is float64, frames or None, (C, H, W), input is variance, flat_std, var_or_std, through_mean): the GPU
# test's apply cases; seeds 300 + index.  7x9 is odd (VEC = 1 sums), 12x10 a multiple of 4.
FLAT_CASES = [("f64_7x9_var_through", True, None, (3, 7, 9), True, True, True, True),
              ("f64_12x10_var_through", True, None, (3, 12, 10), True, True, True, True),
              ("f64_12x10_std_nothrough", True, None, (3, 12, 10), False, True, True, False),
              ("f32_7x9_std_nothrough", False, None, (3, 7, 9), False, True, True, False),
              ("f32_12x10_var_through", False, None, (3, 12, 10), True, True, True, True),
              ("f32_7x9_std_through", False, None, (3, 7, 9), False, True, True, True),
              ("f32_3frames_std", False, 3, (3, 12, 10), False, True, True, False),
              ("f32_3frames_var", False, 3, (3, 7, 9), True, True, True, False),
              ("f32_3frames_no_flat_std", False, 3, (3, 12, 10), False, False, True, False),
              ("f64_no_flat_std", True, None, (3, 7, 9), True, False, True, True),
              ("f32_no_var", False, 3, (3, 7, 9), False, True, False, False),
              ("f64_no_var", True, None, (3, 12, 10), True, True, False, True)]


# the two larger planes (multi-workgroup sums; grid-stride loops), same fields, seeds 350 and 351
FLAT_LARGE = [("multi_workgroup", False, None, (3, 260, 260), False, True, True, True),
              ("grid_stride", False, None, (1, 725, 725), True, True, True, True)]


# ---- band statistics -----------------------------------------------------------------------------------------------
def band_stats_f64(mean, std):
    """(6, C) float64 rows: min mean, max mean, sum mean, min std, max std, sum std (std None: zero rows).  Sums are
    exact (math.fsum).  min / max are IEEE minNum / maxNum as include/clair_hip.h documents: a NaN is skipped, and a
    channel without any number keeps the identities +inf / -inf; the sums carry NaN and inf like any addition."""
    mean = np.asarray(mean, dtype=np.float64)
    c = mean.shape[0]
    out = np.zeros((6, c), dtype=np.float64)
    for row, data in ((0, mean), (3, std)):
        if data is None:
            continue
        flat = np.asarray(data).reshape(c, -1).astype(np.float64)
        for k in range(c):
            out[row, k] = np.fmin.reduce(flat[k], initial=np.inf)
            out[row + 1, k] = np.fmax.reduce(flat[k], initial=-np.inf)
            out[row + 2, k] = math.fsum(flat[k])
    return out


# ---- dark field ----------------------------------------------------------------------------------------------------
def dark_blur_f64(x, dark, dark_std, sigma, threshold=0.05, alpha=50.0, halo=None, h_global=None, row_offset=0):
    """ct_dark_field_blur in float64 for pixel values x (B, C, H, W):
        m = 1 / (1 + exp(-alpha (dark - threshold))),  xb = m blur(x) + (1 - m) x
        blur: separable [e^-1/2, 1, e^-1/2] / sum with reflect padding (-1 -> 1, N -> N - 2)
        sigma_eff = sqrt(sigma^2 + (dterm dark_std)^2),  dterm = (blur(x) - x) alpha m (1 - m)
    dark / dark_std are (1 | B, C, H, W); sigma is the per-sample uncertainty (None: 0).  For a row band of a taller
    image give h_global, row_offset and halo (B, C, 2, W) = the global rows above and below the band; an edge of the
    band that is an edge of the global image is reflected and its halo row ignored.
    Returns (xb, sigma_eff or None when dark_std is None)."""
    x = np.asarray(x, dtype=np.float64)
    b, c, h, w = x.shape
    hg = h if h_global is None else h_global
    top_edge, bottom_edge = row_offset == 0, row_offset + h == hg
    if not (top_edge and bottom_edge):
        halo = np.asarray(halo, dtype=np.float64)
    above = x[:, :, 1:2] if top_edge else halo[:, :, 0:1]
    below = x[:, :, h - 2:h - 1] if bottom_edge else halo[:, :, 1:2]
    rows = np.concatenate([above, x, below], axis=2)                       # (B, C, H + 2, W)
    cols = np.concatenate([rows[..., 1:2], rows, rows[..., w - 2:w - 1]], axis=3)
    side = math.exp(-0.5)
    k0, k1 = 1.0 / (1.0 + 2.0 * side), side / (1.0 + 2.0 * side)
    horiz = k1 * cols[..., :-2] + k0 * cols[..., 1:-1] + k1 * cols[..., 2:]
    blurred = k1 * horiz[:, :, :-2] + k0 * horiz[:, :, 1:-1] + k1 * horiz[:, :, 2:]
    d = np.broadcast_to(np.asarray(dark, dtype=np.float64), x.shape)
    m = 1.0 / (1.0 + np.exp(-alpha * (d - threshold)))
    xb = m * blurred + (1.0 - m) * x
    if dark_std is None:
        return xb, None
    sg = np.zeros_like(x) if sigma is None else np.asarray(sigma, dtype=np.float64)
    dterm = (blurred - x) * (alpha * m * (1.0 - m))
    ds = dterm * np.broadcast_to(np.asarray(dark_std, dtype=np.float64), x.shape)
    return xb, np.sqrt(sg * sg + ds * ds)


def dark_inputs(seed, shape, dtype, max_code=None):
    """Stack of `shape` = (B, C, H, W) (stored, float32 pixels), explicit sigma, one dark field per frame straddling the
    0.05 threshold (the mask is neither 0 nor 1) and its std."""
    stored, x = video_frames(seed, shape[0], shape[1:], dtype, max_code)
    rng = np.random.default_rng(seed + 1000)
    sd = (np.float32(0.002) + np.float32(0.03) * rng.random(shape, dtype=np.float32)).astype(np.float32)
    dark = (np.float32(0.1) * rng.random(shape, dtype=np.float32)).astype(np.float32)
    dark_std = (np.float32(0.002) + np.float32(0.01) * rng.random(shape, dtype=np.float32)).astype(np.float32)
    return stored, x, sd, dark, dark_std


# (name, (B, C, H, W), dtype, max_code, std mode, std value): the GPU test's whole-image cases; seeds 400 + index
DARK_CASES = [("u8_constant", (2, 3, 2, 2), "u8", None, "constant", 0.01),
              ("u16_multiplier_4095", (2, 3, 13, 9), "u16", 4095.0, "multiplier", 0.05),
              ("f32_explicit", (1, 1, 2, 17), "f32", None, "explicit", 0.0),
              ("f32_none", (2, 3, 13, 9), "f32", None, "none", 0.0),
              ("u8_max_code_100", (2, 3, 13, 9), "u8", 100.0, "multiplier", 0.05)]

# (seed, case): the row-band stack and the grid-stride stack of the GPU test
DARK_EXTRA = [(450, ("bands_u16", (2, 3, 13, 9), "u16", None, "multiplier", 0.05)),
              (452, ("grid_stride", (4, 3, 300, 300), "f32", None, "explicit", 0.0))]


def dark_sigma(mode, value, x, explicit):
    """The per-sample sigma of a std mode in float64 (std_value is a float32 argument of the C ABI)."""
    v = float(np.float32(value))
    x = np.asarray(x, dtype=np.float64)
    return {"none": None, "constant": np.full_like(x, v), "multiplier": v * x,
            "explicit": np.asarray(explicit, dtype=np.float64)}[mode]
