"""Plain float64 reference of one train / measure step of the exposure-pair linearity statistic (ct_pair_residual_fwd /
ct_pair_residual_bwd, csrc/ct_pairs.hip), the seeded inputs and the tolerances its tests share.

Written directly in torch float64 from oracle/eager_torch.linearity_statistics' semantics and calling none of the code
under test.  tests/test_pair_refs_host.py validates it against the pinned vectors and the float32 eager oracle on the CPU
and measures the tolerances below; tests/test_gpu_pairs_uncertainty.py compares the kernels with it.

Discrete decisions are taken in float32 exactly as the eager oracle takes them -- the validity mask on the raw value, the
LUT coordinate fl(x (L - 1)) with its interval index, the clamps -- and handed to the float64 arithmetic, so a comparison measures arithmetic, not ties."""
from types import SimpleNamespace

import numpy as np
import torch

# ---- tolerances ----------------------------------------------------------------------------------------------------
# TOL[quantity] = (element tolerance, norm-wise tolerance) in the two measures of _util.assert_parity.  Each is 4x what
# the float32 eager oracle (oracle/eager_torch, the reference project's own order of operations; for the raw sums a
# restatement that test_pair_refs_host.py pins to it bit for bit) shows against this float64 reference, worst over every
# input of the GPU test (all_cases(): every case x relative / absolute x uncertainty weighting on / off), rounded up.
# test_pair_refs_host.py re-measures every entry and asserts measured * 4 <= tolerance.  Measured values are in the comments
# (element, norm-wise).
TOL = {
    "den": (1.3e-6, 8.5e-7),       # sum w m          measured 3.068e-7, 2.107e-7 (constant_catmull_u16_12x20, relative)
    "num": (3.9e-6, 2.3e-6),       # sum v w m        measured 9.711e-7, 5.645e-7 (constant_catmull_u16_12x20 / explicit_catmull_u16_13x17, absolute)
    "mean": (3.6e-6, 2.0e-6),      # spatial mean     measured 8.922e-7, 4.997e-7 (explicit_catmull_u16_13x17, absolute)
    "std": (3.1e-6, 1.3e-6),       # spatial std      measured 7.581e-7, 3.167e-7 (thresholds / explicit_catmull_u16_13x17, absolute)
    "err": (2.8e-6, 1.9e-6),       # spatial error    measured 6.886e-7, 4.667e-7 (multiplier_catmull_f32_12x20 / explicit_catmull_u16_13x17, absolute)
    "errsum": (2.4e-6, 1.7e-6),    # sum err m        measured 5.806e-7, 4.228e-7 (explicit_catmull_u16_13x17, absolute)
    "linloss": (1.3e-6, 1.4e-6),   # linearity loss   measured 3.080e-7, 3.445e-7 (thresholds / explicit_catmull_u16_13x17)
    "grad": (5.3e-5, 5.4e-6),      # LUT gradients of lin.sum() and of sum coef D mean: measured 1.313e-5, 1.331e-6 (both on
                                   # "thresholds": a sparsely filled 52-point LUT whose smallest bins hold a few +- terms)
}

RESIDUAL_BOUND = 1e-6   # smallest |I_i - r I_j| / (|I_i| + r |I_j| + 1e-6) of a valid sample that is not exactly zero
CLAMP_GAP = 1e-3        # smallest relative distance of a valid sample's linearized value from the clamp at 1e-6
LO, HI = 1 / 255, 254 / 255
STD_CONSTANT, STD_MULTIPLIER = 0.01, 0.05


# ---- the reference -------------------------------------------------------------------------------------------------
def exposure_pairs(exposures, threshold):
    """(i, j, t_i / t_j) of the upper triangle, ratio >= threshold (None: every pair), in triu order."""
    t = torch.as_tensor(exposures, dtype=torch.float64)
    n = t.numel()
    i, j = torch.triu_indices(n, n, offset=1)
    r = t[i] / t[j]
    if threshold is not None:
        keep = r >= threshold
        i, j, r = i[keep], j[keep], r[keep]
    return i, j, r


def lut_rows(n, c, h, w, h_global=None, row_offset=0):
    """The reference's LUT-row rule: flat (N, C, H, W) index mod C, evaluated with the global geometry for a row band."""
    hg = h if h_global is None else h_global
    cc = torch.arange(c).view(1, c, 1, 1)
    hh = torch.arange(h).view(1, 1, h, 1) + row_offset
    ww = torch.arange(w).view(1, 1, 1, w)
    nn = torch.arange(n).view(n, 1, 1, 1)
    return (((nn * c + cc) * hg + hh) * w + ww) % c


def _basis(t, mode):
    if mode == "linear":
        return (1.0 - t, t), (0, 1)
    t2 = t * t
    t3 = t2 * t
    return ((-0.5 * t3 + t2 - 0.5 * t, 1.5 * t3 - 2.5 * t2 + 1.0, -1.5 * t3 + 2.0 * t2 + 0.5 * t, 0.5 * t3 - 0.5 * t2),
            (-1, 0, 1, 2))


def pair_step_f64(x, std, exposures, lut, mode, ratio_threshold=0.25, lo=LO, hi=HI, use_relative=True,
                  use_unc_weight=True, center=None, coef=None, h_global=None, row_offset=0, want_grad=True):
    """One step in float64.  x (N, C, H, W) float32 pixel values, std the float32 std stack or None, lut (C, L) float32 or
    None, mode "linear" / "catmull" / None.  Returns a namespace: i, j, ratio; sums (P, C, 5) = [sum w m, sum v w m,
    sum (v - center)^2 w m, sum err m, sum m] (center None: the spatial mean); den = max(sum w m, 1e-8); mean, std, err
    (P, C; err None without std); linloss (C); grad_lin = d linloss.sum() / d lut and grad_coef = d sum(coef den mean) /
    d lut with den held constant ((C, L) float64; None without a model, want_grad or coef); lin (N, C, H, W) float64,
    valid (P, C, H, W) bool, resid (P, C, H, W) = |I_i - r I_j| / (|I_i| + r |I_j| + 1e-6) and both_zero (I_i and I_j exactly
    0: a residual that is 0 in every precision) for the case conditions."""
    x = torch.as_tensor(x, dtype=torch.float32)
    n, c, h, w = x.shape
    i, j, r = exposure_pairs(exposures, ratio_threshold)
    x64 = x.double().requires_grad_(True)
    taps, tap_index, rows = [], [], None
    if lut is None or mode is None:
        lin = x64 * 1.0
        lin32 = x
    else:
        lut32 = torch.as_tensor(lut, dtype=torch.float32)
        lut64 = lut32.double()
        top = lut32.shape[1] - 1
        rows = lut_rows(n, c, h, w, h_global, row_offset).reshape(-1)
        s32 = x * top                                         # float32 decisions: clamp, interval
        inside = (s32 >= 0) & (s32 <= top)
        s32c = s32.clamp(0, top)
        i0 = s32c.floor().long()
        # The LUT coordinate is the oracle's float32 product fl(x top), taken as data: on a knot its fraction is exactly 0,
        # which decides the interval (an exact product of the float32 pixel value would fall 1e-8 to either side of it and
        # leak that share of the sample's gradient into a neighbouring bin).  Its derivative is top where it is not clamped.
        s64 = s32c.double() + (x64 - x64.detach()) * (top * inside.double())
        basis, offs = _basis(s64 - i0.double(), mode)         # t is never clamped in float32: no clamp here either
        basis32, _ = _basis(s32c - i0.float(), mode)
        lin, lin32 = 0.0, 0.0
        for b, b32, k in zip(basis, basis32, offs):
            ix = (i0 + k).clamp(0, top).reshape(-1)
            tap = lut64[rows, ix].reshape(n, c, h, w).clone().requires_grad_(True)
            taps.append(tap)
            tap_index.append(ix)
            lin = lin + b * tap
            lin32 = lin32 + b32 * lut32[rows, ix].reshape(n, c, h, w)
    lsd = None
    if std is not None:                                       # |f'(x) sigma|, detached from the LUT
        g = torch.autograd.grad(lin.sum(), x64, retain_graph=True)[0]
        lsd = (g * torch.as_tensor(std, dtype=torch.float32).double()).abs()
    xi, xj = x[i], x[j]
    valid = (xi >= lo) & (xi <= hi) & (xj >= lo) & (xj <= hi)  # float32 against the Python scalar, as the oracle
    m = valid.double()
    xd = x.double()
    gauss = torch.exp(-10.0 * (xd - 0.5) ** 2)
    rr = r.view(-1, 1, 1, 1)
    li, lj = lin[i], lin[j]
    expected = lj * rr
    diff = li - expected
    safe = expected + 1e-6
    v = (diff / safe if use_relative else diff).abs()
    err = None
    if lsd is not None:
        si, sj = lsd[i], lsd[j]
        if use_relative:
            clamped = lin32[j] < 1e-6                          # float32 decision of lj.clamp(min=1e-6)
            ljc = torch.where(clamped, torch.full_like(lj, 1e-6), lj)
            err = torch.sqrt((si / safe) ** 2 + ((li * sj) / (safe * ljc)) ** 2 + 1e-6)
        else:
            err = torch.sqrt(si ** 2 + (rr * sj) ** 2)
    wts = gauss[i] + gauss[j]
    if err is not None and use_unc_weight:
        wts = wts + 1.0 / (err + 1e-6)
    wm = wts * m
    s0 = wm.sum(dim=(2, 3))
    s1 = (v * wm).sum(dim=(2, 3))
    den = s0.clamp(min=1e-8)
    mean = s1 / den
    cen = mean.detach() if center is None else torch.as_tensor(center, dtype=torch.float64)
    s2 = (((v - cen.view(-1, c, 1, 1)) ** 2) * wm).sum(dim=(2, 3))
    s4 = m.sum(dim=(2, 3))
    s3 = (err * m).sum(dim=(2, 3)) if err is not None else torch.zeros_like(s4)
    linloss = torch.sqrt((mean ** 2).sum(dim=0))
    out = SimpleNamespace(i=i, j=j, ratio=r, den=den.detach(), mean=mean.detach(), std=torch.sqrt(s2 / den).detach(),
                          err=None if err is None else (s3 / s4.clamp(min=1e-8)).detach(), linloss=linloss.detach(),
                          sums=torch.stack([s0, s1, s2, s3, s4], dim=-1).detach(), grad_lin=None, grad_coef=None,
                          lin=lin.detach(), valid=valid,
                          resid=(diff.abs() / (li.abs() + expected.abs() + 1e-6)).detach(),
                          both_zero=((li == 0) & (lj == 0)).detach())

    def scatter(objective):
        grads = torch.autograd.grad(objective, taps, retain_graph=True)
        acc = torch.zeros((c, lut.shape[1]), dtype=torch.float64)
        for gk, ix in zip(grads, tap_index):
            acc.index_put_((rows, ix), gk.reshape(-1), accumulate=True)
        return acc

    if taps and want_grad:
        out.grad_lin = scatter(linloss.sum())
        if coef is not None:
            out.grad_coef = scatter((torch.as_tensor(coef, dtype=torch.float64) * den.detach() * mean).sum())
    return out


# ---- the float32 side: the eager oracle's pieces returning what it does not ----------------------------------------
def eager_sums_f32(x, std, exposures, lut, mode, ratio_threshold, lo, hi, use_relative, use_unc_weight):
    """(sum w m, sum v w m, sum err m | None) in float32 / float64 exactly as oe.linearity_statistics forms them (the same
    operations in the same order; it returns only their quotients).  test_pair_refs_host.py asserts that the quotients of
    these sums equal the oracle's output bit for bit."""
    from oracle import eager_torch as oe
    i, j, r = oe.exposure_pairs(torch.as_tensor(exposures, dtype=torch.float64), ratio_threshold)
    xi, xj = x[i], x[j]
    mask = (xi >= lo) & (xi <= hi) & (xj >= lo) & (xj <= hi)
    gw = oe.gaussian_weight(xi, 10.0) + oe.gaussian_weight(xj, 10.0)
    xg = x.clone().requires_grad_(std is not None)
    lin = oe.icrf_forward(xg, lut, mode) if lut is not None else xg
    lsd = None
    if std is not None:
        lsd = (torch.autograd.grad(lin, xg, torch.ones_like(lin))[0] * std).abs()
    lin = lin.detach()
    rr = r.view(-1, 1, 1, 1)
    li, lj = lin[i], lin[j]
    expected = lj * rr
    diff = li - expected
    safe = expected + 1e-6
    if use_relative:
        diff = diff / safe
    loss = diff.abs()
    err = None
    if lsd is not None:
        si, sj = lsd[i], lsd[j]
        if use_relative:
            err = torch.sqrt((si / safe) ** 2 + ((li * sj) / (safe * lj.clamp(min=1e-6))) ** 2 + 1e-6)
        else:
            err = torch.sqrt(si ** 2 + (rr * sj) ** 2)
    weights = torch.zeros_like(loss)
    if err is not None and use_unc_weight:
        weights = weights + 1 / (err + 1e-6)
    weights = weights + gw
    mm = mask.to(loss.dtype)
    vv, ww = loss * mm, weights * mm
    s0 = ww.sum(dim=(2, 3), keepdim=True)
    s1 = (vv * ww).sum(dim=(2, 3), keepdim=True)
    s3 = None if err is None else ((err * mm) * mm).sum(dim=(2, 3), keepdim=True).squeeze((2, 3))
    return s0.squeeze((2, 3)), s1.squeeze((2, 3)), s3


def eager_grads_f32(x, std, exposures, lut, mode, ratio_threshold, lo, hi, use_relative, use_unc_weight, coef_den):
    """The float32 eager chain's LUT gradients of lin.sum() and of sum(coef_den * spatial mean), the per-sample tap
    gradients scattered in float64 as oe.linearity_lut_grad_f64 does (explicit tap leaves of the same float32 arithmetic
    as oe.icrf_forward).  Returns (linloss, spatial mean, grad_lin, grad_coef)."""
    from oracle import eager_torch as oe
    n, c, h, w = x.shape
    size = lut.shape[1]
    top = size - 1
    lut = lut.detach()
    rows = torch.arange(c).repeat(n * h * w)
    taps, tap_index = [], []

    def take(ix):
        tap_index.append(ix.reshape(-1))
        taps.append(lut[rows, ix.reshape(-1)].reshape(n, c, h, w).clone().requires_grad_(True))
        return taps[-1]

    def forward(xx):
        s = (xx * top).clamp(0, top)
        i0 = s.floor().long()
        if mode == "linear":
            fr = s - i0.float()
            return take(i0) * (1.0 - fr) + take((i0 + 1).clamp(0, top)) * fr
        t = (s - i0.float()).clamp(0, 1)
        t2 = t * t
        t3 = t2 * t
        basis = (-0.5 * t3 + t2 - 0.5 * t, 1.5 * t3 - 2.5 * t2 + 1.0, -1.5 * t3 + 2.0 * t2 + 0.5 * t, 0.5 * t3 - 0.5 * t2)
        return torch.stack([b * take((i0 + k).clamp(0, top)) for b, k in zip(basis, (-1, 0, 1, 2))], dim=0).sum(dim=0)

    _, sp, _, _ = oe.linearity_statistics(x, std, torch.as_tensor(exposures, dtype=torch.float64), lut, mode, ratio_threshold,
                                          lo, hi, use_relative, use_unc_weight, forward=forward)
    linloss = torch.sqrt((sp ** 2).sum(dim=0))

    def scatter(objective):
        grads = torch.autograd.grad(objective, taps, retain_graph=True)
        acc = torch.zeros((c, size), dtype=torch.float64)
        for gk, ix in zip(grads, tap_index):
            acc.index_put_((rows, ix), gk.reshape(-1).double(), accumulate=True)
        return acc

    return linloss.detach(), sp.detach(), scatter(linloss.sum()), scatter((coef_den * sp).sum())


# ---- inputs --------------------------------------------------------------------------------------------------------
def base_exposures(n=9, stops=0.5):
    return [0.001 * 2.0 ** (k * stops) for k in range(n)]


def base_lut(n_points=64, channels=3):
    """One distinct gamma curve per row, so that a wrong LUT row shows."""
    g = torch.linspace(0, 1, n_points, dtype=torch.float64)
    return torch.stack([g ** p for p in (1.9, 2.2, 2.5)[:channels]]).float()


def normalize(codes):
    """CastTo + Normalize as the reference computes them (oracle.ct_oracle.normalize_codes)."""
    from oracle import ct_oracle as oc
    return torch.from_numpy(oc.normalize_codes(np.ascontiguousarray(codes)))


def scene(seed, exposures, shape, dtype):
    """A gamma-2.2 scene with 1 % noise, exposed over `exposures`: residuals of order 1e-2, far from the sign's tie.
    Returns (stored stack -- float32 pixels or integer codes --, float32 pixel values, max_code)."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.tensor(exposures, dtype=torch.float64)
    e = torch.rand(shape, generator=gen, dtype=torch.float64) * (2.0 / float(torch.sqrt(t[0] * t[-1])))
    x = ((e.unsqueeze(0) * t.view(-1, 1, 1, 1)).clamp(0, 1) ** (1 / 2.2)).float()
    x = (x + 0.01 * torch.randn(x.shape, generator=gen)).clamp(0, 1)
    if dtype == "f32":
        return x, x, None
    top, np_t = (255, np.uint8) if dtype == "u8" else (65535, np.uint16)
    codes = torch.round(x * top).to(torch.int32).numpy().astype(np_t)
    return torch.from_numpy(codes), normalize(codes), float(top)


def std_stack(mode, x, seed=0):
    """The three std sources as the reference builds them, float32: constant 0.01, multiplier 0.05 x, and an explicit
    stack expressible as neither (0.02 x + 1e-3 plus seeded noise)."""
    if mode == "none":
        return None
    if mode == "constant":
        return torch.full_like(x, STD_CONSTANT)
    if mode == "multiplier":
        return x * torch.tensor(STD_MULTIPLIER)
    gen = torch.Generator().manual_seed(7000 + seed)
    return (0.02 * x + 1e-3 + 2e-3 * torch.rand(x.shape, generator=gen)).float()


def std_kwargs(mode, sd):
    """How a std source is handed to ops.pair_residual_* / linearity_loss."""
    if mode == "explicit":
        return dict(std=sd)
    if mode == "none":
        return {}
    return dict(std_mode=mode, std_value=STD_CONSTANT if mode == "constant" else STD_MULTIPLIER)


def repair(stored, max_code, exposures, lut, mode, threshold, lo=LO, hi=HI, keep_zero=None, zero_foot=False):
    """Moves every sample whose pair residual is closer to zero than RESIDUAL_BOUND (sign() would then differ between two
    float32 orders) by one code / 2^-10, until none is left.  Deterministic; `keep_zero` (P, C, H, W) bool marks samples
    placed at exactly zero on purpose, `zero_foot` allows pairs whose two linearized values are exactly 0 (a curve with a
    flat foot at 0: the residual is 0 in every precision).  Returns (stored, float32 pixel values)."""
    stored = stored.clone()
    for _ in range(8):
        x = stored if max_code is None else normalize(stored.numpy())
        ref = pair_step_f64(x, None, exposures, lut, mode, threshold, lo, hi, want_grad=False)
        bad = ref.valid & (ref.resid < RESIDUAL_BOUND)
        if keep_zero is not None:
            bad &= ~keep_zero
        if zero_foot:
            bad &= ~ref.both_zero
        if not bad.any():
            return stored, x
        p, cc, hh, ww = torch.nonzero(bad, as_tuple=True)
        ni = ref.i[p]
        if max_code is None:
            stored[ni, cc, hh, ww] += 2.0 ** -10
        else:
            a = stored.numpy()
            a[ni.numpy(), cc.numpy(), hh.numpy(), ww.numpy()] += 1
    raise AssertionError("repair did not converge")


# (name, std mode, interp, dtype, (H, W)): the matrix.  Base geometry: 9 exposures at half-stop steps, threshold 0.25
# (samples have 0 .. 4 i-side partners: the kGroup = 4 body and its tail), C = 3, a 64-point LUT.  Every std mode meets
# every interp, dtype and plane; every interp meets every dtype and plane; every dtype meets every plane (pairwise; the
# host test checks it).  The full product (54) is thinned to 10 because std mode, interp and dtype act in the staging of ONE
# sample (sigma source, dfdx, to_pixel) and the plane only decides which stager runs and how the last tile ends: beyond
# pairs the axes do not interact.  relative / absolute and uncertainty weighting on / off run inside every case.
STD_MODES = ("constant", "multiplier", "explicit")
INTERPS = ("linear", "catmull")
DTYPES = ("f32", "u16", "u8")
PLANES = ((13, 17), (12, 20), (8, 64))


def matrix_cases():
    out = []
    for s, sm in enumerate(STD_MODES):
        for d, dt in enumerate(DTYPES):
            interp = INTERPS[(s + d) % 2]
            plane = PLANES[(s + d) % 3]
            out.append((f"{sm}_{interp}_{dt}_{plane[0]}x{plane[1]}", sm, interp, dt, plane))
    # the one pair the 3 x 3 rotation leaves out (interp and plane both follow s + d)
    out.append(("explicit_catmull_u16_8x64", "explicit", "catmull", "u16", (8, 64)))
    return out


def build_case(name):
    """Namespace of a named case: stored (what the kernel gets), x (float32 pixel values), max_code, sd (float32 std stack),
    smode, interp, exposures, threshold, lut, lo, hi, and for a band h_global / row_offset."""
    cs = SimpleNamespace(name=name, exposures=base_exposures(), threshold=0.25, lut=base_lut(), lo=LO, hi=HI,
                         h_global=None, row_offset=0, keep_zero=None)
    table = {m[0]: m for m in matrix_cases()}
    if name in table:
        _, cs.smode, cs.interp, dtype, plane = table[name]
        seed = 1000 + sorted(table).index(name)
        stored, _, cs.max_code = scene(seed, cs.exposures, (3,) + plane, dtype)
    elif name.startswith("nomodel_"):
        cs.smode, cs.interp, cs.lut = name.split("_")[1], None, None
        seed = 1100 + STD_MODES.index(cs.smode)
        stored, _, cs.max_code = scene(seed, cs.exposures, (3, 13, 17), ("f32", "u16", "u8")[seed % 3])
    elif name in ("whole_13x17", "layout_12x20", "layout_13x17"):   # bands / interleaved: explicit std
        cs.smode, cs.interp = "explicit", "catmull" if name == "layout_13x17" else "linear"
        seed = {"whole_13x17": 1200, "layout_12x20": 1201, "layout_13x17": 1202}[name]
        shape = (3, 12, 20) if name == "layout_12x20" else (3, 13, 17)
        stored, _, cs.max_code = scene(seed, cs.exposures, shape, "u16" if name == "layout_12x20" else "f32")
    elif name == "bands_11x32":        # row bands whose starts fall on tile boundaries (see test_row_bands_explicit_std)
        cs.smode, cs.interp, seed = "explicit", "linear", 1203
        stored, _, cs.max_code = scene(seed, cs.exposures, (3, 11, 32), "f32")
    elif name in ("api_explicit", "api_constant"):   # measure_linearity's own ratio threshold, 0.2
        cs.smode, cs.interp, cs.threshold = name.split("_")[1], "linear" if name == "api_explicit" else "catmull", 0.2
        seed = 1210 + (name == "api_constant")
        stored, _, cs.max_code = scene(seed, cs.exposures, (3, 13, 17), "f32")
    elif name == "many_exposures":     # 128 exposures, every pair: 32-column tiles, eight forward launches
        cs.smode, cs.interp, cs.threshold = "multiplier", "linear", None
        cs.exposures, cs.lut, seed = [0.001 * 2.0 ** (k / 16.0) for k in range(128)], base_lut(32), 1300
        stored, _, cs.max_code = scene(seed, cs.exposures, (3, 12, 20), "f32")
    elif name == "narrow_std_only":    # N, L from pick_tile's budget: 32 columns with the std array, 64 without
        cs.smode, cs.interp = "multiplier", "linear"
        cs.exposures, cs.lut, seed = [0.001 * 2.0 ** (k / 8.0) for k in range(NARROW_N)], base_lut(NARROW_L), 1301
        cs.threshold = 0.5
        stored, _, cs.max_code = scene(seed, cs.exposures, (3, 12, 20), "u8")
    elif name == "clamp":              # a LUT whose first entries are exactly 0, lower = 0: linearized values below 1e-6
        cs.smode, cs.interp, cs.lo, seed = "explicit", "linear", 0.0, 1400
        lut = base_lut()
        lut[:, :6] = 0.0
        lut[:, 6] = lut[:, 7] * 1e-4   # a shallow interval: values on both sides of 1e-6 at non-zero slope
        cs.lut = lut
        stored, _, cs.max_code = scene(seed, cs.exposures, (3, 13, 17), "f32")
        stored = stored.clone()
        flat = stored[:4].reshape(-1)  # the four shortest exposures: a third of their samples at the foot of the curve
        gen = torch.Generator().manual_seed(seed)
        flat[::3] = torch.rand(flat[::3].shape, generator=gen) * (7.5 / 63.0)
    elif name == "thresholds":         # values exactly 0 and 1, on the thresholds, one code either side, on LUT knots
        cs.smode, cs.interp, seed = "constant", "catmull", 1401
        cs.lut = base_lut(52)          # 65535 / 51 = 1285: the knots are whole codes
        stored, _, cs.max_code = scene(seed, cs.exposures, (3, 13, 17), "u16")
        u = np.arange(65536, dtype=np.float32) / np.float32(65535.0)
        c_lo, c_hi = int(np.argmax(u >= np.float32(LO))), int(65535 - np.argmax(u[::-1] <= np.float32(HI)))
        knots = [k * 1285 for k in (1, 2, 25, 26, 50)]
        special = np.array([0, 65535, c_lo - 1, c_lo, c_lo + 1, c_hi - 1, c_hi, c_hi + 1] + knots
                           + [k - 1 for k in knots], dtype=np.uint16)
        a = stored.numpy()
        for frame in (0, 3, 8):
            a[frame].reshape(-1)[frame:frame + special.size] = special
        a[4].reshape(-1)[:special.size] = special[::-1]
    elif name == "equal_frames":       # two frames with equal exposure time and identical pixels: residual exactly 0
        cs.smode, cs.interp, seed = "multiplier", "linear", 1402
        cs.exposures = base_exposures()
        cs.exposures[4] = cs.exposures[3]
        stored, _, cs.max_code = scene(seed, cs.exposures, (3, 13, 17), "u8")
        stored[4] = stored[3]
    elif name == "masked_huge_std":    # masked-out pixels carrying large finite explicit stds
        cs.smode, cs.interp, seed = "explicit", "linear", 1403
        stored, _, cs.max_code = scene(seed, cs.exposures, (3, 13, 17), "f32")
    else:
        raise KeyError(name)
    cs.seed = seed
    if name == "equal_frames":
        i, j, _ = exposure_pairs(cs.exposures, cs.threshold)
        cs.keep_zero = torch.zeros((i.numel(),) + tuple(stored.shape[1:]), dtype=torch.bool)
        cs.keep_zero[(i == 3) & (j == 4)] = True
    cs.stored, cs.x = repair(stored, cs.max_code, cs.exposures, cs.lut, cs.interp, cs.threshold, cs.lo, cs.hi, cs.keep_zero,
                             zero_foot=name == "clamp")
    cs.sd = std_stack(cs.smode, cs.x, seed)
    if name == "masked_huge_std":      # every sample outside [lo, hi] gets HUGE_STD
        cs.sd = torch.where((cs.x < cs.lo) | (cs.x > cs.hi), torch.tensor(HUGE_STD), cs.sd)
    return cs


# The largest power of ten at which the float32 eager oracle stays finite: its absolute-residual error squares the float32
# |f' sigma| <= 2.5 sigma (1e19 would overflow), while the relative one runs in float64 once the float64 exposure ratio enters
# (test_pair_refs_host.py checks finiteness).  The kernels' float32 pair arithmetic overflows long before: a masked sample at
# the foot of the curve has err ~ sigma f' 1e12, squared.
HUGE_STD = 1.0e18

# Narrow tiles for the std backward only, from pick_tile's constants (csrc/ct_pairs.hip): budget 144 KiB, fixed part =
# align16(C L 8 [LINEAR entry] + C L 8 [histogram]) + 256, per sample and column 20 bytes (24 with the linearized std).
NARROW_N, NARROW_L = 96, 256


def pick_tile_columns(n_images, n_points, channels, with_std, entry_bytes=8):
    """pick_tile of the generic backward restated: the widest of 64 / 32 columns whose staging fits 144 KiB."""
    lut_bytes = (channels * n_points * entry_bytes + 15) & ~15
    fixed = ((lut_bytes + channels * n_points * 8 + 15) & ~15) + 256
    for tp in (64, 32):
        if fixed + n_images * (tp + 1) * (24 if with_std else 20) <= 144 * 1024:
            return tp
    return 0


GENERAL_CASES = ([m[0] for m in matrix_cases()] + [f"nomodel_{s}" for s in STD_MODES]
                 + ["whole_13x17", "bands_11x32", "layout_12x20", "layout_13x17", "api_explicit", "api_constant", "many_exposures", "narrow_std_only",
                    "clamp", "thresholds", "equal_frames", "masked_huge_std"])
BAND = (3, 7)   # rows [3, 10) of the 13-row image: start a multiple of C = 3 and 7 = 13 (mod 3) rows, so that the LUT-row
                # rule picks the same rows for the band alone as inside the whole image (test_config_c3_full_shape)


def band_of(cs, r0, rows):
    """The row band [r0, r0 + rows) of a case with the global geometry attached."""
    out = SimpleNamespace(**vars(cs))
    out.name = f"{cs.name}_band{r0}+{rows}"
    out.stored, out.x, out.sd = (t[:, :, r0:r0 + rows].contiguous() for t in (cs.stored, cs.x, cs.sd))
    out.h_global, out.row_offset = cs.x.shape[2], r0
    return out


def seeded_coef(cs, n_pairs):
    """(P, C) upstream coefficients of one sign (LUT bins do not cancel), seeded per case."""
    gen = torch.Generator().manual_seed(9000 + cs.seed)
    return (0.5 + torch.rand((n_pairs, 3), generator=gen, dtype=torch.float64)) * 1e-4
