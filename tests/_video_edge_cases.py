"""Inputs, float64 reference and error unit of the video-statistics edge tests (tests/test_video_edges_host.py on the CPU,
tests/test_gpu_video_edges.py on the device).  NumPy only; calls none of the code under test.

The streaming mean / std family (ct_stats.hip, ct_stats_multi.hip, ct_stats_ingest.hip, ct_stats_ingest_multi.hip and
ct_stats_merge.hpp) computes a variance.  The inputs of tests/_side_refs.py keep it far from cancellation; the ones here are
what a camera staring at a static scene gives: a level per pixel plus a code or two of noise, one step, nothing at all, the
full swing, values out of range, a resumed state, a long stream.

THE UNIT.  A relative tolerance on a std that is 1e-6 of the mean means nothing, so errors are counted per pixel in units of
one rounding of a linearised sample,
    u = 2^-24 max_n |x_lin[n]|,      err_mean = |mean - mean64| / u,      err_std = |std - std64| / u,
x_lin the float64 copy of the float32 linearised samples (oracle.eager_torch.icrf_forward), std the standard deviation of the
mean as compute_video_mean_and_std returns it.  A pixel with u == 0 (every sample 0) is compared exactly.

THE BOUNDS are not chosen: test_video_edges_host.py measures, per family, the worst error of oracle.eager_torch.video_mean_std
(the reference's own float32 arithmetic) against float64 over the family's cases; the bound is 4x that with a floor of 1 u --
the kernel may differ from eager torch by a contracted multiply-add in the LUT interpolation and by one differently rounded
division, each at most one rounding per sample, the order of the reference's own error.  MEASURED below is what was seen
(rounded up in the third digit); the host test fails when a re-measurement exceeds it, and shows that two wrong algorithms
(one-pass m2, a merge without its delta^2 term) exceed the bounds on every low-variance family."""
import collections
import math

import numpy as np

import _side_refs as sr

EPS = 2.0 ** -24

SHAPES = [(3, 5, 7), (3, 8, 16)]   # Q = 105: V = 4 body and a tail of 1, interleaved plane no multiple of 4; whole packets
SCHEDULES = [(4,) * 16, (1,) * 64, (16, 17, 31), (33, 31), (3, 5, 7, 11, 13, 25)]
LONG_SCHEDULES = [(4,) * 64, (1,) * 256]
MODES = sr.VIDEO_MODES
MAX_BATCHES = 16                    # batches one call of ops.video_stats_batches takes (CT_STATS_MAX_BATCHES)
LOW_VARIANCE = ("A", "B", "G")

# family -> (worst err_mean, worst err_std) of oe.video_mean_std against float64, in u, over the family's cases
# (test_video_edges_host.py::test_bounds_from_the_eager_oracle prints them with -s).  F: the float32 restatement of the merge
# (statistics.py:250-251) on the given state, oe.video_mean_std takes none.
MEASURED = {
    "A": (8.07, 0.143),     # mean: +-64 codes as (1,)*64, catmull (64 merges, each a rounding of the mean); std: float32 frames
    "B": (5.38, 0.0912),    # uint16 / 4095, the step in frame 0 of (1,)*64
    "C": (4.40, 0.554),     # float32 as (33, 31): torch's sum of 33 equal values is not 33 times the value
    "D": (0.0, 0.0313),     # means of 0 / 1 samples are exact
    "E": (6.66, 0.179),
    "F": (7.40, 0.0910),    # a batch of 33 summed in sequence
    "G": (25.8, 0.0880),    # (1,)*256: the drift of 256 merges
}
BOUND = {f: (max(1.0, 4.0 * m), max(1.0, 4.0 * s)) for f, (m, s) in MEASURED.items()}

# std of one sample / mean, float64, per low-variance family: what "low variance" means here (asserted on the CPU)
# A: +-64 codes on a level of 300 under a gamma of 2.6 is 64 / sqrt(3) / 300 * 2.6 = 0.32 at the most; B: one frame a code up
# is a sample std of 1/8 code, on uint8 at level 32 under that gamma 2.6 / 32 / 8 = 0.0102; G: +-1 code, 2.6 / 32 * 0.82 = 0.067
RATIO_RANGE = {"A": (1e-7, 0.35), "B": (1e-7, 0.011), "G": (1e-7, 0.07)}

Case = collections.namedtuple("Case", "name family sched shape mode dtype max_code seed kind arg")
Inputs = collections.namedtuple("Inputs", "stored x frames_before special")


def sched_id(sched):
    return f"{sched[0]}x{len(sched)}" if len(set(sched)) == 1 and len(sched) > 1 else "-".join(map(str, sched))


def walks_of(sched):
    """The walks a schedule meets: the single-batch kernels of its batches, and the several-batches kernel (BMAX from the
    largest batch) where ops.video_stats_batches takes it in one launch."""
    w = {sr.video_kernel_of(b) for b in sched}
    if len(sched) > 1 and max(sched) <= 32:
        w.add("multi16" if max(sched) <= 16 else "multi32")
    return w


def chunks(sched):
    """The schedule in calls of at most MAX_BATCHES batches: [(first frame, batch sizes)]."""
    out, k = [], 0
    for i in range(0, len(sched), MAX_BATCHES):
        part = sched[i:i + MAX_BATCHES]
        out.append((k, part))
        k += sum(part)
    return out


# ---- the case list -------------------------------------------------------------------------------------------------------
# (dtype, max_code, noise amplitude in codes | float32 noise)
A_VARIANTS = [("u16", 65535, 1), ("u16", 65535, 8), ("u16", 65535, 64), ("u16", 4095, 1), ("u16", 4095, 8), ("u16", 4095, 64),
              ("u8", 255, 1), ("f32", None, 1e-5)]
PM1_VARIANTS = [("u16", 65535, 1), ("u16", 4095, 1), ("u8", 255, 1), ("f32", None, 1e-5)]
LEVELS = {65535: (20000, 60000), 4095: (300, 3800), 255: (32, 223), None: (0.05, 0.95)}
F32_STEP = 2.0 ** -16               # "one code" of a float32 frame


def lookup_ok(dtype, max_code, amp):
    """LOOKUP on a 256-point LUT rounds to the nearest of 255 intervals: noise that stays inside one of them has no
    variance at all, which is family C's subject, not that of A, B and G."""
    return dtype == "u8" or (max_code == 4095 and amp >= 64)


def _mode(k, dtype, max_code, amp):
    m = MODES[k % 4]
    return m if (m != "lookup" or lookup_ok(dtype, max_code, amp)) else MODES[(k + 2) % 4]


def _vname(dtype, max_code, amp=None):
    s = dtype if dtype != "u16" else f"u16m{max_code}"
    return s if amp is None else f"{s}-pm{amp:g}"


def cases():
    out = []

    def add(family, sched, shape, mode, dtype, max_code, kind, arg, tag):
        name = f"{family}-{tag}-{sched_id(sched)}-{shape[1]}x{shape[2]}-{mode}"
        out.append(Case(name, family, tuple(sched), shape, mode, dtype, max_code, 1000 + len(out), kind, arg))

    # A: a level per pixel plus uniform noise
    for v, (dtype, mc, amp) in enumerate(A_VARIANTS):
        for s, sched in enumerate(SCHEDULES):
            add("A", sched, SHAPES[(v + s) % 2], _mode(v + s, dtype, mc, amp), dtype, mc, "noise", amp, _vname(dtype, mc, amp))
    # B: every frame at the level but one, a code above it
    b_table = [(SCHEDULES[4], 0), (SCHEDULES[4], 15), (SCHEDULES[4], 25), (SCHEDULES[4], 63), (SCHEDULES[1], 0), (SCHEDULES[1], 63),
               (SCHEDULES[0], 0), (SCHEDULES[2], 63), (SCHEDULES[3], 0), (SCHEDULES[3], 63), (SCHEDULES[3], 32), (SCHEDULES[2], 16)]
    for i, (sched, pos) in enumerate(b_table):
        dtype, mc, amp = PM1_VARIANTS[(i + i // 4) % 4]
        add("B", sched, SHAPES[i % 2], _mode(i + 1, dtype, mc, 1), dtype, mc, "step", pos, f"{_vname(dtype, mc)}-at{pos}")
    # C: constant pixels, D: full swing
    for i in range(10):
        dtype, mc, _ = PM1_VARIANTS[i % 4]
        add("C", SCHEDULES[i % 5], SHAPES[i % 2], MODES[(i + i // 4) % 4], dtype, mc, "constant", None, _vname(dtype, mc))
    for i in range(10):
        dtype, mc, _ = PM1_VARIANTS[(i + 1) % 4]
        add("D", SCHEDULES[(i + 2) % 5], SHAPES[(i + 1) % 2], MODES[(i + 1 + i // 4) % 4], dtype, mc, "swing", None, _vname(dtype, mc))
    # E: float32 out of range -- below 0 and above 1 with a model; NaN, +inf, -inf without one
    for i, sched in enumerate(SCHEDULES):
        add("E", sched, SHAPES[i % 2], MODES[1 + i % 3], "f32", None, "range", None, "f32-range")
    for i, sched in enumerate(SCHEDULES):
        add("E", sched, SHAPES[(i + 1) % 2], None, "f32", None, "nonfinite", None, "f32-nonfinite")
    # F: one call into a given state
    for i, before in enumerate((1, 1000, 2 ** 24)):
        for j, batch in enumerate((4, 17, 33)):
            dtype, mc, amp = PM1_VARIANTS[(i + j) % 4]
            add("F", (batch,), SHAPES[(i + j) % 2], _mode(i + 2 * j, dtype, mc, 1), dtype, mc, "resumed", before,
                f"{_vname(dtype, mc)}-after{before}")
    # G: 256 frames of A at +-1 code
    for s, sched in enumerate(LONG_SCHEDULES):
        for v, (dtype, mc, amp) in enumerate(PM1_VARIANTS):
            add("G", sched, SHAPES[(v + s) % 2], _mode(v + 2 * s + 1, dtype, mc, 1), dtype, mc, "noise", amp, _vname(dtype, mc, amp))
    return out


CASES = cases()


# ---- inputs --------------------------------------------------------------------------------------------------------------
def to_pixels(codes, top):
    """float32 pixel values of integer codes as CastTo(float32), Normalize(top, 0) gives them (a correctly rounded division)."""
    return (codes.astype(np.float32) / np.float32(top)).astype(np.float32)


def _finish(case, vals):
    """vals: int64 codes, or float32 pixels -> (stored, x)."""
    if case.dtype == "f32":
        x = np.ascontiguousarray(vals, dtype=np.float32)
        return x, x
    np_t = np.uint8 if case.dtype == "u8" else np.uint16
    assert vals.min() >= 0 and vals.max() <= np.iinfo(np_t).max
    codes = np.ascontiguousarray(vals.astype(np_t))
    return codes, to_pixels(codes, case.max_code)


def inputs(case):
    """Inputs(stored frames (N, C, H, W), their float32 pixel values, frames_before, {(c, row, col): what} of the pixels
    family E makes non-finite)."""
    rng = np.random.default_rng(case.seed)
    n, shape, f32 = sum(case.sched), tuple(case.shape), case.dtype == "f32"
    lo, hi = LEVELS[case.max_code]
    level = rng.uniform(lo, hi, size=shape).astype(np.float32) if f32 else rng.integers(lo, hi + 1, size=shape)
    q = int(np.prod(shape))
    flat = np.arange(q).reshape(shape)
    before, special = 0, {}
    if case.kind in ("noise", "resumed"):
        amp = case.arg if case.kind == "noise" else (1e-5 if f32 else 1)
        if f32:
            vals = (level[None] + rng.uniform(-amp, amp, size=(n,) + shape).astype(np.float32)).astype(np.float32)
        else:
            vals = level[None] + rng.integers(-amp, amp + 1, size=(n,) + shape)
            vals[0], vals[1] = level - amp, level + amp      # every pixel spans its noise: no float64 std is 0
    elif case.kind == "step":
        vals = np.repeat(level[None], n, axis=0)
        vals[case.arg] = level + (np.float32(F32_STEP) if f32 else 1)
    elif case.kind == "constant":
        top = 1.0 if f32 else case.max_code
        level = level.copy()
        level.reshape(-1)[[0, 5, q - 1]] = 0                   # code 0, in a packet and as the last element
        level.reshape(-1)[[1, 6, q - 2]] = top
        if case.max_code == 4095:                              # 12-bit data in a uint16 container: above max_code
            level.reshape(-1)[[2, 7]] = (5000, 65535)
        vals = np.repeat(level[None], n, axis=0)
    elif case.kind == "swing":
        top = np.float32(1.0) if f32 else case.max_code
        frame = np.arange(n)
        batch = np.repeat(np.arange(len(case.sched)), case.sched)
        on = np.stack([frame % 2, (frame + 1) % 2, batch % 2])   # from 0, from the top, a batch at 0 and the next at the top
        vals = np.moveaxis(on[flat % 3], -1, 0) * top
    elif case.kind == "range":
        vals = rng.uniform(-0.25, 1.25, size=(n,) + shape).astype(np.float32)
        vals[0].reshape(-1)[:4] = (-0.25, 1.25, 0.0, 1.0)
    elif case.kind == "nonfinite":
        vals = (level[None] + rng.uniform(-1e-5, 1e-5, size=(n,) + shape).astype(np.float32)).astype(np.float32)
        for what, value, f, frame in (("nan", np.nan, 41, 20), ("+inf", np.inf, 50, 0), ("-inf", -np.inf, q - 1, n - 1)):
            vals[frame].reshape(-1)[f] = value
            special[tuple(int(i) for i in np.unravel_index(f, shape))] = what
    else:
        raise ValueError(case.kind)
    stored, x = _finish(case, vals)
    if case.kind == "resumed":
        before = case.arg
    return Inputs(stored, x, before, special)


def resumed_state(x_lin32, before):
    """Family F's float32 state: mean = the level (the pixel's first linearised sample), m2 = (before - 1) s^2 with s one
    code's worth, 2e-5 of the level."""
    mean0 = np.ascontiguousarray(x_lin32[0], dtype=np.float32)
    s = mean0.astype(np.float64) * 2e-5
    return mean0, ((before - 1) * s * s).astype(np.float32)


# ---- reference and unit --------------------------------------------------------------------------------------------------
def stats_f64(x_lin, before=0, mean0=None, m20=None):
    """Float64 mean and std of the mean of the frames x_lin (N, C, H, W); with ``before`` > 0 merged into the float32 state
    (mean0, m20) of that many frames by the merge formula (statistics.py:250-251), in float64."""
    x = np.asarray(x_lin, dtype=np.float64)
    n = x.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        mean = x.sum(axis=0) / n
        m2 = ((x - mean) ** 2).sum(axis=0)
        if before:
            ma, va = np.asarray(mean0, dtype=np.float64), np.asarray(m20, dtype=np.float64)
            w = float(before) + n
            delta = mean - ma
            m2 = va + m2 + (before * n / w) * delta * delta
            mean = ma + (n / w) * delta
            n = before + n
        return mean, np.sqrt(m2 / (n - 1)) / math.sqrt(n)


def unit(x_lin):
    with np.errstate(invalid="ignore"):
        return EPS * np.abs(np.asarray(x_lin, dtype=np.float64)).max(axis=0)


def errors_in_u(got, ref, u):
    """Per-pixel |got - ref| / u; where u == 0 (every sample 0) 0 for an exact match and inf otherwise; a pixel whose
    reference is not finite is not measured here (0): the caller compares it by kind."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref) / u
        err = np.where(u == 0, np.where(got == ref, 0.0, np.inf), err)
    err = np.where(np.isfinite(ref) & np.isfinite(u), err, 0.0)
    return np.where(np.isnan(err), np.inf, err)               # a NaN where the reference has a number


def describe_worst(err, x_lin, case, what):
    """The pixel of the worst error: channel, row, column, its samples' min and max, the error in u, the walks."""
    idx = np.unravel_index(int(np.argmax(err)), err.shape)
    s = np.asarray(x_lin, dtype=np.float64)[(slice(None),) + tuple(idx)]
    return (f"{case.name} {what}: pixel (c, row, col) = {tuple(int(i) for i in idx)}, samples in [{s.min():.9g}, {s.max():.9g}], "
            f"error {err[idx]:.3f} u, walks {sorted(walks_of(case.sched))}")


# ---- float32 algorithms: the reference's merge restated, and two wrong ones -------------------------------------------------
def stream_f32(x_lin32, sched, one_pass=False, drop_delta=False, before=0, mean0=None, m20=None):
    """The WBOMeanVar stream in NumPy float32 over the batches of ``sched`` -> (mean, std of the mean) float32.
    one_pass: m2 of a batch as sum x^2 - n mean^2; drop_delta: a merge without (W_A W_B / W) delta^2."""
    f = np.float32
    x = np.asarray(x_lin32, dtype=f)
    wa = f(before)
    ma, va = (None, None) if not before else (np.asarray(mean0, dtype=f), np.asarray(m20, dtype=f))
    k = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for b in sched:
            xb = x[k:k + b]
            k += b
            wb = f(b)
            mb = xb.sum(axis=0, dtype=f) / wb
            m2b = (xb * xb).sum(axis=0, dtype=f) - wb * mb * mb if one_pass else ((xb - mb) ** 2).sum(axis=0, dtype=f)
            if wa == 0:
                ma, va = mb, m2b
            else:
                w = wa + wb
                delta = mb - ma
                va = va + m2b if drop_delta else va + m2b + (wa * wb / w) * (delta * delta)
                ma = ma + (wb / w) * delta
            wa = wa + wb
        n = before + k
        return ma, np.sqrt(va * f(1 / (n - 1))) / f(math.sqrt(n))


# ---- a case's reference, computed once --------------------------------------------------------------------------------------
Reference = collections.namedtuple("Reference", "inp lut x_lin u mean64 std64 mean_o std_o mean0 m20")
_REFERENCES = {}


def pixel_reference(case, x, linearize, oracle, before=0):
    """Float64 and float32-reference statistics of the float32 pixel values x of a case.  linearize(x, lut, mode) -> float32
    array and oracle(x, lut, mode, sched) -> (mean, std) are the callers' wrappers of oracle.eager_torch (this module stays
    NumPy only).  Family F has a state, which oe.video_mean_std does not take: its float32 reference is stream_f32."""
    lut = sr.video_lut(case.shape[0])
    x_lin = np.asarray(linearize(x, lut, case.mode), dtype=np.float32)
    mean0 = m20 = None
    if before:
        mean0, m20 = resumed_state(x_lin, before)
        mean_o, std_o = stream_f32(x_lin, case.sched, before=before, mean0=mean0, m20=m20)
    else:
        mean_o, std_o = oracle(x, lut, case.mode, case.sched)
    mean64, std64 = stats_f64(x_lin, before, mean0, m20)
    return lut, x_lin, unit(x_lin), mean64, std64, np.asarray(mean_o), np.asarray(std_o), mean0, m20


def reference(case, linearize, oracle):
    if case.name not in _REFERENCES:
        inp = inputs(case)
        _REFERENCES[case.name] = Reference(inp, *pixel_reference(case, inp.x, linearize, oracle, inp.frames_before))
    return _REFERENCES[case.name]


def worst_errors(ref, mean, std):
    """(err_mean, err_std) per pixel in u against float64."""
    return errors_in_u(mean, ref.mean64, ref.u), errors_in_u(std, ref.std64, ref.u)
