"""Every launch path of the four side kernels against the float64 references of tests/_side_refs.py.

Inputs are seeded (tests/_side_refs.py), tolerances are the ones tests/test_side_refs_host.py measures on the CPU, and
every comparison goes through _util.assert_parity (labels "side ..." in parity_observed.json).

Path -> test:

| path | test |
|---|---|
| video: B <= 16 / B <= 32 / two-pass kernel x {none, lookup, linear, catmull} x {u8, u16, f32}, pairwise, from an empty state and merged into one (WA != 0), V=4 only (Q = 1380, 32) / V=1 only (Q = 105, 3), plane not divisible by C | test_video_stats_schedules |
| video: uint16 with max_code = 4095 | test_video_stats_max_code_4095 |
| video: row band (h_global > h_tile, row_offset > 0, neither offset a multiple of C) | test_video_stats_row_band |
| video: V=4 body + V=1 tail in ONE call (image_stride % 4 == 0, Q % 4 != 0) | test_video_stats_padded_stride_body_and_tail |
| video: misaligned frame pointer / state pointer -> all-scalar path | test_video_stats_offset_frames, test_video_stats_offset_state |
| flat field: sums<*,1> (7x9) and <*,4> (12x10), value float32 / float64 / NULL; apply float32 / float64, std or variance in, n_frames 3, flat_std NULL, var_or_std NULL, through on / off (float32 + through: the fixed branch) | test_flatfield_cases |
| flat field: several workgroups per channel, float64 atomics (3x260x260) | test_flatfield_multi_workgroup |
| flat field: 512-workgroup cap and grid-stride loops of sums and apply (1x725x725) | test_flatfield_grid_stride |
| flat field: flat pointer offset by one float -> VEC = 1 with plane % 4 == 0 | test_flatfield_sums_offset_flat |
| flat field: through_mean with several frames refused | test_flatfield_through_mean_needs_one_image |
| band stats: plane 1, 7x9 (VEC = 1), 530x512 (512-slice cap, grid stride, fold loop), without std | test_band_stats_against_f64 |
| band stats: mean offset by one double / std by one float -> VEC = 1 on an even plane | test_band_stats_offset_pointers |
| band stats: NaN, +inf, -0.0 | test_band_stats_nan_inf_negative_zero |
| dark field: u8 + constant, u16 + multiplier (max_code 4095), f32 + explicit, CT_STD_NONE with a dark std, max_code below the container range, W = 2 and H = 2 | test_dark_blur_cases |
| dark field: bands with uint16 halos, one-row interior band | test_dark_blur_bands_u16_halo |
| dark field: one-row band at the global top / bottom, band without halo | test_dark_blur_refusals |
| dark field: grid-stride loop (4x3x300x300) | test_dark_blur_grid_stride |
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import _side_refs as sr
from _util import assert_parity

pytestmark = pytest.mark.gpu

_NP_DTYPE = {"u8": 0, "u16": 1, "f32": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _to(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- video statistics ----------------------------------------------------------------------------------------------
def _video_reference(x, lut, mode, sched):
    """(float64 mean, float64 std, float32 eager mean, float32 eager std) of the pixel values x."""
    from oracle import eager_torch as oe
    lut_t = None if mode is None else torch.from_numpy(lut)
    lin = x if mode is None else oe.icrf_forward(torch.from_numpy(x), lut_t, mode).numpy()
    mean, std = sr.video_stats_f64(lin, sched)
    mean_o, std_o = oe.video_mean_std(torch.from_numpy(x), lut_t, mode, list(sched))
    return mean, std, mean_o.numpy(), std_o.numpy()


def _std_of(m2, n):
    return np.sqrt(m2.double().cpu().numpy() / (n - 1)) / math.sqrt(n)


def _check_video(mean, m2, n, ref, what):
    mean_r, std_r, mean_o, std_o = ref
    got_mean, got_std = mean.cpu().numpy(), _std_of(m2, n)
    assert_parity(got_mean, mean_r, rtol=sr.VIDEO_MEAN_TOL, norm_tol=sr.VIDEO_MEAN_TOL, what="side video mean vs f64")
    assert_parity(got_std, std_r, rtol=sr.VIDEO_STD_TOL, norm_tol=sr.VIDEO_STD_TOL, what="side video std vs f64")
    # the suite's element tolerances against the float32 oracle; a norm-wise error cannot exceed the worst element's
    assert_parity(got_mean, mean_o, rtol=1e-6, norm_tol=1e-6, what="side video mean vs eager")
    assert_parity(got_std, std_o, rtol=1e-4, norm_tol=1e-6, what="side video std vs eager")


def _run_video_ops(dev, stored, sched, state_shape, mode, lut, max_code=None, tile=None):
    from clair_torch_amd import ops
    frames = _to(stored, dev)
    mean = torch.full(state_shape, float("nan"), dtype=torch.float32, device=dev)   # an empty state is never read
    m2 = torch.full(state_shape, float("nan"), dtype=torch.float32, device=dev)
    lut_d = None if mode is None else _to(lut, dev)
    k = 0
    for b in sched:
        ops.video_stats_batch(frames[k:k + b], mean, m2, k, lut=lut_d, interp=mode, max_code=max_code, tile=tile)
        k += b
    return mean, m2


@pytest.mark.parametrize("k", range(len(sr.video_cases())), ids=lambda k: "-".join(
    ["x".join(map(str, sr.video_cases()[k][0])), "x".join(map(str, sr.video_cases()[k][1])), str(sr.video_cases()[k][2]), sr.video_cases()[k][3]]))
def test_video_stats_schedules(dev, k):
    sched, shape, mode, dtype = sr.video_cases()[k]
    n = sum(sched)
    stored, x = sr.video_frames(sr.video_seed(k), n, shape, dtype)
    lut = sr.video_lut(shape[0])
    mean, m2 = _run_video_ops(dev, stored, sched, shape, mode, lut)
    _check_video(mean, m2, n, _video_reference(x, lut, mode, sched), f"video {sched} {shape} {mode} {dtype}")


def _special(name):
    k = [s[0] for s in sr.VIDEO_SPECIAL].index(name)
    _, sched, shape, mode, dtype, max_code = sr.VIDEO_SPECIAL[k]
    stored, x = sr.video_frames(200 + k, sum(sched), shape, dtype, max_code)
    return sched, shape, mode, dtype, max_code, stored, x, sr.video_lut(shape[0])


def test_video_stats_max_code_4095(dev):
    sched, shape, mode, dtype, max_code, stored, x, lut = _special("max4095")
    assert stored.dtype == np.uint16 and stored.max() <= 4095
    mean, m2 = _run_video_ops(dev, stored, sched, shape, mode, lut, max_code=max_code)
    _check_video(mean, m2, sum(sched), _video_reference(x, lut, mode, sched), "video max_code 4095")


def test_video_stats_row_band(dev):
    """Rows [7, 14) of a 20-row image: the LUT row of LINEAR / CATMULL follows the GLOBAL flat index, which the band's
    geometry enters through row_offset * W and (h_global - h_tile) * W.  Neither is a multiple of C here, so a dropped
    or mis-scaled row_offset or h_global picks other LUT rows."""
    from clair_torch_amd import ops
    sched, shape, mode, dtype, _, stored, x, lut = _special("band")
    r0, r1 = 7, 14
    c, h, w = shape
    assert mode in ("linear", "catmull") and (r0 * w) % c != 0 and ((h - (r1 - r0)) * w) % c != 0
    ref = tuple(a[:, r0:r1] for a in _video_reference(x, lut, mode, sched))
    mean, m2 = _run_video_ops(dev, stored[:, :, r0:r1], sched, (c, r1 - r0, w), mode, lut,
                              tile=ops.TileGeometry(h_global=h, row_offset=r0))
    _check_video(mean, m2, sum(sched), ref, "video row band")


def _raw_video(dev, frames_t, dtype, batch, shape, stride, mode, lut_d, before, mean_t, m2_t, max_code=None):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import ops
    c, h, w = shape
    geom = nv.Geometry(channels=c, h_tile=h, width=w, h_global=h, row_offset=0, image_stride=stride, layout=nv.LAYOUT_NCHW)
    icrf = nv.Icrf(lut_dev=None if mode is None else lut_d.data_ptr(), n_points=0 if mode is None else lut_d.shape[1],
                   interp=ops._INTERP[mode])
    default = {"u8": 255.0, "u16": 65535.0, "f32": 1.0}[dtype]
    rc = nv.load().ct_video_stats_batch(_ptr(frames_t), _NP_DTYPE[dtype], float(max_code or default), batch, ctypes.byref(geom),
                                        ctypes.byref(icrf), float(before), _ptr(mean_t), _ptr(m2_t), _stream(dev))
    assert rc == 0, rc


def test_video_stats_padded_stride_body_and_tail(dev):
    """Q = 105 with image_stride = 108: elements 0..103 through the V=4 kernel, element 104 through the V=1 kernel."""
    sched, shape, mode, dtype, _, stored, x, lut = _special("padded_stride")
    n, q, stride = sum(sched), int(np.prod(shape)), 108
    assert q % 4 != 0 and stride % 4 == 0 and len(sched) == 1
    padded = np.full((n, stride), 255, dtype=stored.dtype)   # the padding is never read: it would pull the mean up
    padded[:, :q] = stored.reshape(n, q)
    frames = _to(padded, dev)
    mean = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    m2 = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    assert frames.data_ptr() % 16 == 0 and mean.data_ptr() % 16 == 0 and m2.data_ptr() % 16 == 0
    _raw_video(dev, frames, dtype, n, shape, stride, mode, _to(lut, dev), 0, mean, m2)
    _check_video(mean, m2, n, _video_reference(x, lut, mode, sched), "video padded stride")


def test_video_stats_offset_frames(dev):
    """Frames one element into an allocation: not 16-byte aligned, so every element takes the V=1 kernel."""
    sched, shape, mode, dtype, _, stored, x, lut = _special("frames_offset")
    n, q = sum(sched), int(np.prod(shape))
    assert q % 4 == 0 and len(sched) == 1      # the offset alone forces the scalar path
    buf = torch.zeros((n * q + 1,), dtype=torch.float32, device=dev)
    frames = buf[1:]
    frames.copy_(_to(stored.reshape(-1), dev))
    assert frames.data_ptr() % 16 == 4
    mean = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    m2 = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    _raw_video(dev, frames, dtype, n, shape, q, mode, _to(lut, dev), 0, mean, m2)
    _check_video(mean, m2, n, _video_reference(x, lut, mode, sched), "video offset frames")


def test_video_stats_offset_state(dev):
    """The mean state one float into an allocation (two batches: the second merges into it); its neighbours stay."""
    sched, shape, mode, dtype, _, stored, x, lut = _special("state_offset")
    n, q = sum(sched), int(np.prod(shape))
    assert q % 4 == 0
    frames = _to(stored, dev)
    buf = torch.full((q + 2,), -7.0, dtype=torch.float32, device=dev)
    mean = buf[1:q + 1]
    m2 = torch.full((q,), float("nan"), dtype=torch.float32, device=dev)
    assert mean.data_ptr() % 16 == 4 and frames.data_ptr() % 16 == 0 and m2.data_ptr() % 16 == 0
    lut_d, k = _to(lut, dev), 0
    for b in sched:
        _raw_video(dev, frames[k:k + b], dtype, b, shape, q, mode, lut_d, k, mean, m2)
        k += b
    assert float(buf[0]) == -7.0 and float(buf[q + 1]) == -7.0
    _check_video(mean.reshape(shape), m2.reshape(shape), n, _video_reference(x, lut, mode, sched), "video offset state")


# ---- flat field ----------------------------------------------------------------------------------------------------
def _check_sums(got, value, flat, what):
    """(C, 2) device sums against the exact sums: any order of n float64 additions is within n 2^-53 sum |x|."""
    ref = sr.flatfield_sums_f64(value, flat)
    got = got.cpu().numpy()
    c = flat.shape[0]
    n = flat[0].size
    den = (flat + np.float32(1e-6)).astype(np.float64).reshape(c, -1)
    for ch in range(c):
        tol_f = sr.sum_tol(n, math.fsum(np.abs(flat[ch].astype(np.float64)).ravel()))
        assert abs(got[ch, 0] - ref[ch, 0]) <= tol_f, (what, ch, got[ch, 0], ref[ch, 0], tol_f)
        if value is None:
            assert got[ch, 1] == 0.0
        else:
            tol_v = sr.sum_tol(n, math.fsum(np.abs(np.asarray(value, dtype=np.float64).reshape(c, -1)[ch]) / den[ch]))
            assert abs(got[ch, 1] - ref[ch, 1]) <= tol_v, (what, ch, got[ch, 1], ref[ch, 1], tol_v)
    rt = n * 2.0 ** -53       # all terms are positive here: sum |x| = |sum x|
    assert_parity(got[:, 0], ref[:, 0], rtol=rt, norm_tol=rt, what="side flat-field sum flat")
    if value is not None:
        assert_parity(got[:, 1], ref[:, 1], rtol=rt, norm_tol=rt, what="side flat-field sum value/flat")
    return ref


def _run_flat_case(dev, seed, f64, frames, shape, is_var, has_fstd, has_var, through, what):
    from clair_torch_amd import ops
    value, std, flat, fstd = sr.flatfield_inputs(seed, frames, shape, f64)
    plane = shape[1] * shape[2]
    vin = std ** 2 if is_var else std
    captured = []
    v_d, s_d = _to(value, dev), (_to(vin, dev) if has_var else None)
    out_v, out_s = ops.flatfield_correct(v_d, s_d, _to(flat, dev), _to(fstd, dev) if has_fstd else None,
                                         input_is_variance=is_var, through_mean=through, reduce=lambda t: captured.append(t.clone()))
    sums = _check_sums(captured[0], value if through else None, flat, what)
    M = (sums[:, 0] / plane).astype(np.float32)
    ref_v, ref_s = sr.flatfield_f64(value, vin if has_var else None, flat, fstd if has_fstd else None, M,
                                    sums[:, 1] / plane if through else None, is_var)
    assert out_v.dtype == (torch.float64 if f64 else torch.float32)
    assert_parity(out_v.cpu().numpy(), ref_v, rtol=sr.FLAT_VALUE_TOL, norm_tol=sr.FLAT_VALUE_TOL, what="side flat-field value")
    if has_var:
        assert_parity(out_s.cpu().numpy(), ref_s, rtol=sr.FLAT_STD_TOL, norm_tol=sr.FLAT_STD_TOL, what="side flat-field std")
        if through and has_fstd:   # the term through the mean matters on these inputs (guards the test)
            without = sr.flatfield_f64(value, vin, flat, fstd, M, None, is_var)[1]
            assert np.max(np.abs(without - ref_s) / ref_s) > 100 * sr.FLAT_STD_TOL
    else:
        assert out_s is None


@pytest.mark.parametrize("k", range(len(sr.FLAT_CASES)), ids=[c[0] for c in sr.FLAT_CASES])
def test_flatfield_cases(dev, k):
    name, f64, frames, shape, is_var, has_fstd, has_var, through = sr.FLAT_CASES[k]
    _run_flat_case(dev, 300 + k, f64, frames, shape, is_var, has_fstd, has_var, through, name)


def test_flatfield_multi_workgroup(dev):
    """3 x 260 x 260 float32 (0.8 MB): 67 workgroups per channel add into one pair of float64 accumulators."""
    name, f64, frames, shape, is_var, has_fstd, has_var, through = sr.FLAT_LARGE[0]
    assert shape == (3, 260, 260)
    _run_flat_case(dev, 350, f64, frames, shape, is_var, has_fstd, has_var, through, name)


def test_flatfield_grid_stride(dev):
    """1 x 725 x 725 float32 (2.1 MB, odd plane): the sums run VEC = 1 on the 512-workgroup cap, so every thread loops
    four or five times; the apply kernel's grid is capped at what the device holds at once (8 workgroups of 256 threads
    per compute unit), which the plane exceeds, so its loop runs twice for some threads."""
    name, f64, frames, shape, is_var, has_fstd, has_var, through = sr.FLAT_LARGE[1]
    plane = shape[1] * shape[2]
    resident = torch.cuda.get_device_properties(dev).multi_processor_count * (2048 // 256)   # ct_device.hpp resident_workgroups
    assert plane % 4 != 0 and plane > 512 * 256 * 4 and plane > resident * 256
    _run_flat_case(dev, 351, f64, frames, shape, is_var, has_fstd, has_var, through, name)


def test_flatfield_sums_offset_flat(dev):
    """A flat field one float into an allocation: VEC = 1 although the plane is a multiple of 4."""
    from clair_torch_amd import _native as nv
    value, _, flat, _ = sr.flatfield_inputs(352, None, (3, 12, 10), True)
    buf = torch.zeros((flat.size + 1,), dtype=torch.float32, device=dev)
    flat_d = buf[1:]
    flat_d.copy_(_to(flat.reshape(-1), dev))
    assert flat_d.data_ptr() % 16 == 4
    for val, is_f64 in ((value, 1), (value.astype(np.float32), 0), (None, 1)):
        sums = torch.zeros((3, 2), dtype=torch.float64, device=dev)
        v_d = None if val is None else _to(val, dev)
        rc = nv.load().ct_flatfield_sums(None if val is None else _ptr(v_d), is_f64, _ptr(flat_d), 3, 120, _ptr(sums), _stream(dev))
        assert rc == 0
        _check_sums(sums, val, flat, "offset flat")


def test_flatfield_through_mean_needs_one_image(dev):
    """The term through the flat field's mean is per image: several frames are refused, not given a zero term."""
    from clair_torch_amd import ops
    value, std, flat, fstd = sr.flatfield_inputs(353, 3, (3, 7, 9), False)
    with pytest.raises(ValueError, match="through_mean"):
        ops.flatfield_correct(_to(value, dev), _to(std, dev), _to(flat, dev), _to(fstd, dev), input_is_variance=False,
                              through_mean=True)


# ---- band statistics -----------------------------------------------------------------------------------------------
def _band_inputs(seed, shape):
    rng = np.random.default_rng(seed)
    return rng.random(shape) * 3.0 - 1.0, rng.random(shape, dtype=np.float32)


def _check_band(out, mean, std, what):
    ref = sr.band_stats_f64(mean, std)
    got = out.cpu().numpy()
    c, n = mean.shape[0], mean[0].size
    assert got.shape == (6, c)
    assert np.array_equal(got[[0, 1, 3, 4]], ref[[0, 1, 3, 4]]), what     # min / max: exact
    rts = []
    for row, data in ((2, mean), (5, std)):
        if data is None:
            assert np.array_equal(got[row], np.zeros(c))
            continue
        for ch in range(c):
            abs_sum = math.fsum(np.abs(data[ch].astype(np.float64)).ravel())
            tol = sr.sum_tol(n, abs_sum)
            assert abs(got[row, ch] - ref[row, ch]) <= tol, (what, row, ch, got[row, ch], ref[row, ch], tol)
            rts.append(tol / abs(ref[row, ch]))
    rows = [2] if std is None else [2, 5]
    assert_parity(got[rows], ref[rows], rtol=max(rts), norm_tol=max(rts), what="side band sums")


@pytest.mark.parametrize("shape,with_std", [((1, 1, 1), True), ((3, 7, 9), True), ((3, 7, 9), False), ((3, 530, 512), True)],
                         ids=["1", "7x9", "7x9-nostd", "530x512"])
def test_band_stats_against_f64(dev, shape, with_std):
    """530 x 512 / 2 per load = 135 680 groups > 512 slices x 256 threads: the slice cap and the grid stride of the first
    kernel, and the k += 256 loop of the fold kernel (512 slices)."""
    from clair_torch_amd import ops
    mean, std = _band_inputs(500 + shape[1], shape)
    std = std if with_std else None
    out = ops.band_stats(_to(mean, dev), None if std is None else _to(std, dev))
    _check_band(out, mean, std, f"band {shape}")


@pytest.mark.parametrize("which", ["mean", "std"])
def test_band_stats_offset_pointers(dev, which):
    """A mean one double (a std one float) into its allocation: not aligned for the 16-byte (8-byte) loads, so the even
    plane runs VEC = 1.  ops.band_stats' .contiguous() keeps such a view, offset included."""
    from clair_torch_amd import ops
    shape = (3, 8, 10)
    mean, std = _band_inputs(520, shape)
    n = mean.size
    mean_d, std_d = _to(mean, dev), _to(std, dev)
    if which == "mean":
        buf = torch.zeros((n + 1,), dtype=torch.float64, device=dev)
        buf[1:].copy_(mean_d.reshape(-1))
        mean_d = buf[1:].view(shape)
        assert mean_d.contiguous().data_ptr() == mean_d.data_ptr() and mean_d.data_ptr() % 16 == 8
    else:
        buf = torch.zeros((n + 1,), dtype=torch.float32, device=dev)
        buf[1:].copy_(std_d.reshape(-1))
        std_d = buf[1:].view(shape)
        assert std_d.contiguous().data_ptr() == std_d.data_ptr() and std_d.data_ptr() % 8 == 4
    _check_band(ops.band_stats(mean_d, std_d), mean, std, f"band offset {which}")


def test_band_stats_nan_inf_negative_zero(dev):
    """The rule of include/clair_hip.h: min / max are minNum / maxNum -- a NaN is skipped, +-inf is a number -- and the
    sums carry NaN and inf like any addition, so a NaN anywhere in a channel shows in that channel's sum."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(530)
    shape = (4, 6, 10)
    mean = rng.random(shape) + 0.5
    std = (rng.random(shape, dtype=np.float32) + np.float32(0.5)).astype(np.float32)
    mean[0, 2, 3], std[0, 4, 1] = np.nan, np.nan
    mean[1, 0, 0], std[1, 5, 9] = np.inf, np.inf
    mean[2, 3, 7], std[2, 1, 1] = -0.0, -0.0
    mean[3], std[3] = np.nan, np.nan                       # a channel without any number
    got = ops.band_stats(_to(mean, dev), _to(std, dev)).cpu().numpy()
    ref = sr.band_stats_f64(mean, std)
    assert np.array_equal(got[[0, 1, 3, 4]], ref[[0, 1, 3, 4]])
    for row, data in ((0, mean), (3, std)):
        rest = data[0][~np.isnan(data[0])].astype(np.float64)
        assert got[row, 0] == rest.min() and got[row + 1, 0] == rest.max() and math.isnan(got[row + 2, 0])
        assert got[row + 1, 1] == math.inf and got[row + 2, 1] == math.inf and got[row, 1] >= 0.5
        assert got[row, 2] == 0.0 and math.copysign(1.0, got[row, 2]) == -1.0     # every other value is >= 0.5
        assert got[row, 3] == math.inf and got[row + 1, 3] == -math.inf and math.isnan(got[row + 2, 3])
        assert abs(got[row + 2, 2] - ref[row + 2, 2]) <= sr.sum_tol(60, ref[row + 2, 2])


# ---- dark field ----------------------------------------------------------------------------------------------------
def _check_dark(xb, sig, ref_xb, ref_sig, what):
    assert_parity(xb.cpu().numpy(), ref_xb, rtol=sr.DARK_XB_TOL, norm_tol=sr.DARK_XB_TOL, what="side dark-field xb")
    assert_parity(sig.cpu().numpy(), ref_sig, rtol=sr.DARK_SIGMA_TOL, norm_tol=sr.DARK_SIGMA_TOL, what="side dark-field sigma_eff")


def _run_dark(dev, stored, sd, dark, dark_std, mode, value, max_code, **kw):
    from clair_torch_amd import ops
    return ops.dark_field_blur(_to(stored, dev), _to(dark, dev), _to(dark_std, dev), std=_to(sd, dev) if mode == "explicit" else None,
                               std_mode=mode, std_value=value, max_code=max_code, **kw)


@pytest.mark.parametrize("k", range(len(sr.DARK_CASES)), ids=[c[0] for c in sr.DARK_CASES])
def test_dark_blur_cases(dev, k):
    name, shape, dtype, max_code, mode, value = sr.DARK_CASES[k]
    stored, x, sd, dark, dark_std = sr.dark_inputs(400 + k, shape, dtype, max_code)
    m = 1.0 / (1.0 + np.exp(-50.0 * (dark.astype(np.float64) - 0.05)))
    assert m.min() < 0.2 and m.max() > 0.8 and np.mean((m > 0.1) & (m < 0.9)) > 0.2      # the mask is neither 0 nor 1
    xb, sig = _run_dark(dev, stored, sd, dark, dark_std, mode, value, max_code)
    ref_xb, ref_sig = sr.dark_blur_f64(x, dark, dark_std, sr.dark_sigma(mode, value, x, sd))
    _check_dark(xb, sig, ref_xb, ref_sig, name)


def _halo(x, r0, r1):
    b, c, h, w = x.shape
    halo = np.zeros((b, c, 2, w), dtype=x.dtype)
    if r0 > 0:
        halo[:, :, 0] = x[:, :, r0 - 1]
    if r1 < h:
        halo[:, :, 1] = x[:, :, r1]
    return halo


def test_dark_blur_bands_u16_halo(dev):
    """Row bands of uint16 codes with uint16 halo rows, one of them a single interior row: bit for bit the whole image,
    and the band the reference computes from the same halo."""
    from clair_torch_amd import ops
    seed, (_, shape, dtype, _, mode, value) = sr.DARK_EXTRA[0]
    assert (dtype, mode, value) == ("u16", "multiplier", 0.05)
    stored, x, sd, dark, dark_std = sr.dark_inputs(seed, shape, dtype)
    xb, sig = _run_dark(dev, stored, sd, dark, dark_std, "multiplier", 0.05, None)
    for r0, r1 in ((0, 5), (5, 6), (6, 13)):
        rows = slice(r0, r1)
        halo = _halo(stored, r0, r1)
        xt, st = _run_dark(dev, stored[:, :, rows], sd[:, :, rows], dark[:, :, rows], dark_std[:, :, rows], "multiplier", 0.05,
                           None, tile=ops.TileGeometry(h_global=13, row_offset=r0), halo=_to(halo, dev))
        assert torch.equal(xt, xb[:, :, rows]) and torch.equal(st, sig[:, :, rows])
        ref_xb, ref_sig = sr.dark_blur_f64(x[:, :, rows], dark[:, :, rows], dark_std[:, :, rows],
                                           sr.dark_sigma("multiplier", 0.05, x[:, :, rows], None), halo=_halo(x, r0, r1),
                                           h_global=13, row_offset=r0)
        _check_dark(xt, st, ref_xb, ref_sig, f"band rows {r0}:{r1}")


def test_dark_blur_refusals(dev):
    """A one-row band at the global top or bottom would reflect onto a row it does not hold (CT_ERR_UNSUPPORTED); a band
    that needs a neighbour's row and has no halo is an invalid call (CT_ERR_INVALID_ARGUMENT)."""
    from clair_torch_amd import _native as nv
    b, c, w, hg = 2, 3, 9, 13
    stored, _, _, dark, _ = sr.dark_inputs(451, (b, c, 1, w), "u16")
    stack, dark_d = _to(stored, dev), _to(dark, dev)
    halo = torch.zeros((b, c, 2, w), dtype=torch.uint16, device=dev)
    xb = torch.empty((b, c, 1, w), dtype=torch.float32, device=dev)

    def call(h_tile, r0, halo_t, stack_t=stack):
        geom = nv.Geometry(channels=c, h_tile=h_tile, width=w, h_global=hg, row_offset=r0, image_stride=c * h_tile * w,
                           layout=nv.LAYOUT_NCHW)
        return nv.load().ct_dark_field_blur(_ptr(stack_t), nv.DTYPE_U16, 65535.0, b, ctypes.byref(geom),
                                            None if halo_t is None else _ptr(halo_t), None, nv.STD_NONE, 0.0, _ptr(dark_d), None, b,
                                            0.05, 50.0, _ptr(xb), None, _stream(dev))
    assert call(1, 0, halo) == nv.ERR_UNSUPPORTED            # one row at the global top
    assert call(1, hg - 1, halo) == nv.ERR_UNSUPPORTED       # one row at the global bottom
    assert call(1, 5, None) == nv.ERR_INVALID_ARGUMENT            # interior band without its halo
    assert call(1, 5, halo) == 0             # the same band with it: accepted
    torch.cuda.synchronize(dev)


def test_dark_blur_grid_stride(dev):
    """4 x 3 x 300 x 300 float32 = 1 080 000 elements, more than 256 compute units x 16 workgroups x 256 threads."""
    seed, (_, shape, dtype, _, mode, _) = sr.DARK_EXTRA[1]
    assert (dtype, mode) == ("f32", "explicit")
    assert int(np.prod(shape)) > torch.cuda.get_device_properties(dev).multi_processor_count * 16 * 256
    stored, x, sd, dark, dark_std = sr.dark_inputs(seed, shape, dtype)
    xb, sig = _run_dark(dev, stored, sd, dark, dark_std, "explicit", 0.0, None)
    ref_xb, ref_sig = sr.dark_blur_f64(x, dark, dark_std, sd)
    _check_dark(xb, sig, ref_xb, ref_sig, "grid stride")
