"""The float64 references of tests/_side_refs.py against the pinned oracles and the recorded vectors, on the CPU.

This is also where the tolerances of tests/test_gpu_side_kernels.py are measured: the float32 oracle of each operation
(the reference's order of operations) is compared with the float64 reference on the very inputs the GPU test uses, and
each tolerance in _side_refs.py must hold 4x the worst element error seen (the kernels sum sequentially where torch may
associate differently; both orders are within a small multiple of B 2^-24).  Run with -s to see the measured figures."""
import math

import numpy as np
import torch

import _side_refs as sr
from _util import assert_parity, golden
from oracle import ct_oracle as oc
from oracle import eager_torch as oe


def _elem_err(got, ref):
    """Worst element error in the metric of _util.assert_parity."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / (np.abs(ref) + np.median(np.abs(ref)))))


def _linearize(x, lut, mode):
    return x if mode is None else oe.icrf_forward(torch.from_numpy(x), torch.from_numpy(lut), mode).numpy()


def test_video_case_table_is_pairwise():
    """Every kernel meets every mode and every dtype, every mode meets every dtype, every schedule every shape."""
    cases = sr.video_cases()
    assert len(cases) == len(sr.VIDEO_SCHEDULES) * len(sr.VIDEO_SHAPES)
    main = {s: sr.video_kernel_of(max(s)) for s in sr.VIDEO_SCHEDULES}
    kernels = {"cached16", "cached32", "twopass"}
    assert set(main.values()) == kernels
    assert {(main[s], m) for s, _, m, _ in cases} == {(k, m) for k in kernels for m in sr.VIDEO_MODES}
    assert {(main[s], d) for s, _, _, d in cases} == {(k, d) for k in kernels for d in sr.VIDEO_DTYPES}
    assert {(m, d) for _, _, m, d in cases} == {(m, d) for m in sr.VIDEO_MODES for d in sr.VIDEO_DTYPES}
    # merged into a non-empty state (WA != 0) with each kernel
    merged = {sr.video_kernel_of(b) for s in sr.VIDEO_SCHEDULES for b in s[1:]}
    assert merged == kernels


def test_video_stats_f64_against_eager_oracle_and_golden():
    worst_mean = worst_std = 0.0
    min_std = math.inf
    todo = [(sr.video_seed(k), s, shape, m, d, None) for k, (s, shape, m, d) in enumerate(sr.video_cases())]
    todo += [(200 + k, s, shape, m, d, mc) for k, (_, s, shape, m, d, mc) in enumerate(sr.VIDEO_SPECIAL)]
    for seed, sched, shape, mode, dtype, max_code in todo:
        _, x = sr.video_frames(seed, sum(sched), shape, dtype, max_code)
        lut = sr.video_lut(shape[0])
        mean, std = sr.video_stats_f64(_linearize(x, lut, mode), sched)
        mean_o, std_o = oe.video_mean_std(torch.from_numpy(x), None if mode is None else torch.from_numpy(lut), mode, list(sched))
        worst_mean = max(worst_mean, _elem_err(mean_o.numpy(), mean))
        worst_std = max(worst_std, _elem_err(std_o.numpy(), std))
        min_std = min(min_std, float(std.min()))
    print(f"video: float32 oracle against float64: mean {worst_mean:.3e}, std {worst_std:.3e}; smallest std {min_std:.3e}")
    assert min_std > 0.01      # the inputs keep the standard deviation away from cancellation
    assert worst_mean * 4 <= sr.VIDEO_MEAN_TOL and worst_std * 4 <= sr.VIDEO_STD_TOL
    # the vectors recorded from the reference (11 uint8 frames of 3x9x14, not drawn uniformly: some pixels are close to
    # cancellation), at the tolerances tests/test_gpu_video_stats.py holds the kernel to on them
    g = golden("video_stats")
    x = oc.normalize_codes(g["vid_codes"])
    for mname, mode in (("nomodel", None), ("linear", "linear"), ("catmull", "catmull")):
        mean, std = sr.video_stats_f64(_linearize(x, g["vid_lut"], mode), [11])
        for bname in ("b4", "b11", "b1"):
            assert_parity(g[f"vid_{mname}_{bname}_mean"], mean, rtol=1e-6, norm_tol=1e-7, what="golden video mean")
            assert_parity(g[f"vid_{mname}_{bname}_std"], std, rtol=1e-5, norm_tol=1e-6, what="golden video std")


def _flatfield_f32_order(value, var_or_std, flat, flat_std, M, through, input_is_variance):
    """The flat-field epilogue in the precision and order of operations of the C oracle (oracle/ct_oracle.c,
    cto_flatfield_merge for float64 values, cto_flatfield_linearize for float32 ones) with every flag of
    ct_flatfield_apply honoured, so that the configurations neither oracle function covers are measured too."""
    f32 = np.float32
    den = flat + f32(1e-6)
    c = flat.shape[0]
    m = np.asarray(M, dtype=f32).reshape(c, 1, 1)
    thr = None if through is None else np.asarray(through, dtype=np.float64).reshape(c, 1, 1)
    if value.dtype == np.float64:
        d, md = den.astype(np.float64), m.astype(np.float64)
        out = value / d * md
        grad = (-value * md / (d * d) + (0.0 if thr is None else thr)).astype(f32)
    else:
        out = (value / den) * m
        grad = -(m * value) / (den * den)
        if thr is not None:
            grad = grad + thr.astype(f32)
    if var_or_std is None:
        return out, None
    var = var_or_std if input_is_variance else var_or_std * var_or_std
    if flat_std is not None:
        gs = grad * flat_std
        var = var + gs * gs
    assert var.dtype == f32
    return out, np.sqrt(var)


def test_flatfield_f64_against_oracle_and_golden():
    worst_val = worst_std = 0.0
    todo = [(300 + k, c) for k, c in enumerate(sr.FLAT_CASES)] + [(350 + k, c) for k, c in enumerate(sr.FLAT_LARGE)]
    for seed, (name, f64, frames, shape, is_var, has_fstd, has_var, through) in todo:
        value, std, flat, fstd = sr.flatfield_inputs(seed, frames, shape, f64)
        plane = shape[1] * shape[2]
        sums = sr.flatfield_sums_f64(value if through else None, flat)
        M = (sums[:, 0] / plane).astype(np.float32)
        thr = sums[:, 1] / plane if through else None
        vin = (std ** 2 if is_var else std) if has_var else None
        fs = fstd if has_fstd else None
        # the configuration the GPU test runs, flags included, in float32 order against float64
        ref_v, ref_s = sr.flatfield_f64(value, vin, flat, fs, M, thr, is_var)
        got_v, got_s = _flatfield_f32_order(value, vin, flat, fs, M, thr, is_var)
        if f64:
            assert _elem_err(got_v, ref_v) < 1e-15
        else:
            worst_val = max(worst_val, _elem_err(got_v, ref_v))
        if has_var:
            worst_std = max(worst_std, _elem_err(got_s, ref_s))
        # where the C oracle covers the configuration, the restatement above is that oracle and the reference agrees with it
        if f64 and through and has_fstd and has_var and is_var:
            o_v, o_s = oc.flatfield_merge(value, std, flat, fstd)
            assert np.array_equal(o_v, got_v)
            assert_parity(o_s, got_s, rtol=2e-7, norm_tol=2e-7, what="restated merge epilogue")   # var -> std -> var: two roundings
            worst_std = max(worst_std, _elem_err(o_s, ref_s))
        if not f64 and not through and has_var and not is_var:
            v4, s4 = (value, std) if frames is not None else (value[None], std[None])
            o_v, o_s = oc.flatfield_linearize(v4, s4, flat, fs)
            assert np.array_equal(o_v.reshape(value.shape), got_v) and np.array_equal(o_s.reshape(value.shape), got_s)
    print(f"flat field: float32 order against float64: value {worst_val:.3e}, std {worst_std:.3e}")
    assert worst_val * 4 <= sr.FLAT_VALUE_TOL and worst_std * 4 <= sr.FLAT_STD_TOL
    # the recorded vectors, at the tolerances tests/test_oracle_golden.py holds the C oracle to
    g = golden("flatfield")
    x = oc.normalize_codes(g["ff_codes"])
    sd = x * np.float32(0.05)
    t, lut, flat, fstd = g["ff_exposures"], g["ff_lut"], g["ff_flat"], g["ff_flat_std"]
    plane = flat.shape[1] * flat.shape[2]
    for pname, part in (("6", [6]), ("33", [3, 3])):
        mean, std = oc.hdr_merge(x, sd, t, lut, "linear", True, part)
        sums = sr.flatfield_sums_f64(mean, flat)
        mc, sc = sr.flatfield_f64(mean, std.astype(np.float32) ** 2, flat, fstd, (sums[:, 0] / plane).astype(np.float32),
                                  sums[:, 1] / plane, True)
        assert_parity(mc, g[f"ffmerge_ffstd_{pname}_mean"], rtol=1e-6, norm_tol=1e-6, what="golden ff mean")
        assert_parity(sc, g[f"ffmerge_ffstd_{pname}_std"], norm_tol=1e-5, elem_tol=2e-5, what="golden ff std")
    M = (sr.flatfield_sums_f64(None, flat)[:, 0] / plane).astype(np.float32)
    for fsname, fs in (("ffstd", fstd), ("noffstd", None)):
        for sname in ("none", "multiplier"):
            lin, so = oc.linearize_std(x[:3], None if sname == "none" else sd[:3], lut, "linear")
            lc, sc = sr.flatfield_f64(lin, so, flat, fs, M, None, False)
            assert_parity(lc, g[f"fflin_{fsname}_{sname}_val"], rtol=2e-7, norm_tol=1e-7, what="golden ff lin")
            assert_parity(sc, g[f"fflin_{fsname}_{sname}_std"], rtol=1e-6, norm_tol=1e-6, what="golden ff lin std")


def test_flatfield_sums_f64_is_the_plain_sum():
    value, _, flat, _ = sr.flatfield_inputs(7, None, (2, 5, 3), True)
    sums = sr.flatfield_sums_f64(value, flat)
    for c in range(2):
        assert sums[c, 0] == math.fsum(float(f) for f in flat[c].ravel())
        assert sums[c, 1] == math.fsum(float(v) / float(np.float32(f) + np.float32(1e-6)) for v, f in zip(value[c].ravel(), flat[c].ravel()))


def test_dark_blur_f64_against_eager_restatement():
    worst_xb = worst_sig = 0.0
    for seed, (name, shape, dtype, max_code, mode, value) in [(400 + k, c) for k, c in enumerate(sr.DARK_CASES)] + sr.DARK_EXTRA:
        _, x, sd, dark, dark_std = sr.dark_inputs(seed, shape, dtype, max_code)
        xb, sig = sr.dark_blur_f64(x, dark, dark_std, sr.dark_sigma(mode, value, x, sd))
        xt, dt, dst = torch.from_numpy(x), torch.from_numpy(dark), torch.from_numpy(dark_std)
        worst_xb = max(worst_xb, _elem_err(oe.conditional_gaussian_blur(xt, dt).numpy(), xb))
        # float32 restatement of the effective sigma, as tests/test_gpu_darkfield.py writes it
        m = torch.sigmoid((dt - 0.05) * 50.0)
        dterm = (oe.gaussian_blur3(xt) - xt) * (50.0 * m * (1 - m))
        sg = {"none": torch.zeros_like(xt), "constant": torch.full_like(xt, value), "multiplier": np.float32(value) * xt,
              "explicit": torch.from_numpy(sd)}[mode]
        worst_sig = max(worst_sig, _elem_err(torch.sqrt(sg ** 2 + (dterm * dst) ** 2).numpy(), sig))
        # the blur alone (mask = 1) is the restated torchvision blur
        far = np.full_like(dark, 10.0)
        assert _elem_err(oe.gaussian_blur3(xt).numpy(), sr.dark_blur_f64(x, far, None, None)[0]) <= sr.DARK_XB_TOL
    print(f"dark field: float32 restatement against float64: xb {worst_xb:.3e}, sigma_eff {worst_sig:.3e}")
    assert worst_xb * 4 <= sr.DARK_XB_TOL and worst_sig * 4 <= sr.DARK_SIGMA_TOL


def test_dark_blur_f64_bands_equal_whole():
    """The reference's band form (halo rows, reflection at the global edges) reproduces its whole-image form exactly."""
    _, x, sd, dark, dark_std = sr.dark_inputs(11, (2, 3, 9, 5), "f32")
    xb, sig = sr.dark_blur_f64(x, dark, dark_std, sd)
    for r0, r1 in ((0, 4), (4, 5), (5, 9)):
        halo = np.zeros((2, 3, 2, 5), dtype=np.float32)
        if r0 > 0:
            halo[:, :, 0] = x[:, :, r0 - 1]
        if r1 < 9:
            halo[:, :, 1] = x[:, :, r1]
        xt, st = sr.dark_blur_f64(x[:, :, r0:r1], dark[:, :, r0:r1], dark_std[:, :, r0:r1], sd[:, :, r0:r1], halo=halo,
                                  h_global=9, row_offset=r0)
        assert np.array_equal(xt, xb[:, :, r0:r1]) and np.array_equal(st, sig[:, :, r0:r1])


def test_band_stats_f64_against_fsum():
    rng = np.random.default_rng(5)
    mean = rng.random((3, 7, 9)) * 3.0 - 1.0
    std = rng.random((3, 7, 9), dtype=np.float32)
    out = sr.band_stats_f64(mean, std)
    ch = [float(v) for v in mean[1].ravel()]
    assert out[0, 1] == min(ch) and out[1, 1] == max(ch) and out[2, 1] == math.fsum(ch)
    sch = [float(v) for v in std[1].ravel()]
    assert out[3, 1] == min(sch) and out[4, 1] == max(sch) and out[5, 1] == math.fsum(sch)
    assert np.array_equal(sr.band_stats_f64(mean, None)[3:], np.zeros((3, 3)))
    # the documented NaN rule: min / max skip it, the sum carries it
    mean[0, 2, 2] = np.nan
    out = sr.band_stats_f64(mean, None)
    rest = [float(v) for v in mean[0].ravel() if not math.isnan(v)]
    assert out[0, 0] == min(rest) and out[1, 0] == max(rest) and math.isnan(out[2, 0])
    allnan = sr.band_stats_f64(np.full((1, 2, 2), np.nan), None)
    assert allnan[0, 0] == math.inf and allnan[1, 0] == -math.inf and math.isnan(allnan[2, 0])
