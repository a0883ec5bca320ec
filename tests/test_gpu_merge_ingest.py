"""ct_hdr_merge_ingest_batch on the device: a recognised gpu_transforms chain and one batch of the HDR merge in one pass.
Its specification is one sentence -- state and outputs are bit for bit those of ct_ingest_transform (or _data) into a planar
float32 stack followed by ct_hdr_merge_batch on that stack -- so the comparisons with those two launches are exact bit
patterns (integer views of the mean, the std and the three state arrays; a NaN must sit at the same place).  That alone
would be self-referential, so one case goes to the float64 oracle on the chain run by the transform classes on the CPU,
with the tolerances the merge tests carry (tests/test_gpu_merge.py)."""
import ctypes

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from _util import assert_parity

pytestmark = pytest.mark.gpu

_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16}
PAIRS = {1: [(0.05, 0.9)], 3: [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)], 4: [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333), (0.01, 1.5)]}
SENTINEL = -7.25
INTERPS = ("lookup", "linear", "catmull", None)
STDS = ("none", "constant", "multiplier", "explicit")
FLAVOURS = [(torch.uint8, "nchw"), (torch.uint16, "nchw"), (torch.uint8, "nhwc"), (torch.uint16, "nhwc"),
            (torch.uint8, "nhwc_bgr"), (torch.uint16, "nhwc_bgr")]
# (5,3,7,13): a plane of 91 elements -- ragged, packets would cross planes; (3,3,8,16): whole packets; one and four
# channels (planar only); one exposure; one pixel
SHAPES = [(5, 3, 7, 13), (3, 3, 8, 16), (2, 1, 5, 7), (2, 4, 6, 9), (1, 3, 7, 13), (2, 3, 1, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _T():
    from clair_torch_amd.common import transforms
    return transforms


def _lut(channels, points=64):
    powers = (2.2, 2.4, 2.6, 1.8)[:channels]  # distinct rows: the p % C rule shows
    return np.stack([np.linspace(0, 1, points, dtype=np.float32) ** np.float32(p) for p in powers])


def _source(planar, layout):
    """(B,C,H,W) planes -> the stack in ``layout`` (BGR: what an OpenCV reader hands over)."""
    if layout == "nchw":
        return planar
    a = planar.numpy()
    return torch.from_numpy(np.ascontiguousarray((a[:, ::-1] if layout == "nhwc_bgr" else a).transpose(0, 2, 3, 1)))


def _stage_lists(dtype, channels):
    """The empty list (the codes act as pixels above 1: the gradient mask), a black level, a black level and a per-channel
    clamp, four stages with a target range whose low end is negative."""
    sub, div = (16.0, 184.0) if dtype == torch.uint8 else (64.0, 959.0)  # Normalize(200, 16) / Normalize(1023, 64)
    affine = ("affine", sub, div, 1.0, 0.0)
    pairs = ("clamp", PAIRS[channels])
    code_clamp = ("clamp", [(sub - 8.0, sub + div + 20.0)])
    return [[], [affine], [affine, pairs], [code_clamp, affine, pairs, ("affine", -0.125, 1.25, 1.5, -0.25)]]


def _draw(rng, shape, dtype, small=False):
    """Random codes below the black level, inside the range and above the maximum; ``small``: mostly 0 .. 2, for the empty
    list (a code is then the pixel: anything above 1 has no weight)."""
    top = 255 if dtype == torch.uint8 else 1100
    codes = rng.integers(0, top + 1, size=shape)
    if small:
        codes = np.where(rng.random(shape) < 0.75, rng.integers(0, 3, size=shape), codes)
    return torch.from_numpy(codes.astype(_NP[dtype]))


def _exposures(n):
    return torch.tensor([0.004 * 2.0 ** k for k in range(n)], dtype=torch.float64)


def _int_view(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def _same_bits(got, want):
    """Equal bit patterns; NaNs must sit at the same places (their payloads are not compared)."""
    if got is None or want is None:
        return got is None and want is None
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        return False
    zero = torch.zeros((), dtype=got.dtype)
    return torch.equal(_int_view(torch.where(nan, zero, got)), _int_view(torch.where(nan, zero, want)))


def _state_same(a, b):
    return _same_bits(a.mean, b.mean) and _same_bits(a.sumw, b.sumw) and _same_bits(a.var, b.var)


def _two_launches(x, stages, expo, layout="nchw", consts=None, **kw):
    """The comparand: the float32 stack of ct_ingest_transform(_data) through ct_hdr_merge_batch."""
    from clair_torch_amd import ops
    return ops.hdr_merge_batch(ops.ingest_transform(x, stages, layout=layout, consts=consts), expo, **kw)


def _fused(x, stages, expo, layout="nchw", consts=None, **kw):
    from clair_torch_amd import ops
    return ops.hdr_merge_ingest_batch(x, stages, expo, layout=layout, consts=consts, **kw)


def _mode_kw(dev, rng, shape, interp, gauss, std_name, lut_d):
    kw = dict(lut=None if interp is None else lut_d, interp=interp, gaussian_weight=gauss)
    if std_name == "explicit":
        sigma = (0.001 + 0.02 * rng.random(shape)).astype(np.float32)
        kw["std"] = torch.from_numpy(sigma).to(dev)   # planar, also for interleaved frames
    elif std_name != "none":
        kw.update(std_mode=std_name, std_value=0.01 if std_name == "constant" else 0.05)
    if interp in ("lookup", "catmull") and std_name != "none":
        kw["reference_order"] = False   # CT_MERGE_CLOSED_FORM: the reference-order kernel is not fused
    return kw


# ---- 1. two launches against one -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,layout", FLAVOURS)
def test_one_launch_equals_the_two(dev, dtype, layout):
    """Every interpolation x weight x uncertainty mode of this kernel flavour; stage lists and shapes cycle through the
    modes by a seeded draw, and each of them meets every flavour (asserted at the end); with and without a state, float64 and float32 mean."""
    from clair_torch_amd import ops
    from clair_torch_amd._native import NativeLibraryError
    rng, pick = np.random.default_rng(7), np.random.default_rng(3)
    shapes = [s for s in SHAPES if layout == "nchw" or s[1] == 3]
    combo, seen = 0, set()
    for interp in INTERPS:
        for gauss in (False, True):
            for std_name in STDS:
                combo += 1
                shape, which = shapes[int(pick.integers(len(shapes)))], int(pick.integers(4))
                b, c, h, w = shape
                stages = _stage_lists(dtype, c)[which]
                seen.add((shape, which))
                planar = _draw(rng, shape, dtype, small=which == 0)
                x = _source(planar, layout).to(dev)
                expo = _exposures(b)
                lut_d = torch.from_numpy(_lut(c)).to(dev)
                kw = _mode_kw(dev, rng, shape, interp, gauss, std_name, lut_d)
                kw["mean_dtype"] = torch.float32 if combo % 3 == 0 else torch.float64
                what = (interp, gauss, std_name, shape, which)
                if interp == "lookup" and not gauss and std_name != "none":
                    for run in (_two_launches, _fused):   # no gradient path: the reference's error on both routes
                        for order in (False, None):
                            with pytest.raises(RuntimeError, match="does not require grad"):
                                run(x, stages, expo, layout, **dict(kw, reference_order=order))
                    continue
                states = [ops.MergeState((c, h, w), dev, std_name != "none") if combo % 2 else None for _ in range(2)]
                want = _two_launches(x, stages, expo, layout, state=states[0], **kw)
                got = _fused(x, stages, expo, layout, state=states[1], **kw)
                assert got[0].dtype == kw["mean_dtype"] and tuple(got[0].shape) == (c, h, w), what
                assert _same_bits(got[0], want[0]), what
                assert _same_bits(got[1], want[1]), what
                if states[0] is not None:
                    assert _state_same(states[1], states[0]), what
                if interp in ("lookup", "catmull") and std_name != "none":
                    with pytest.raises(NativeLibraryError, match="code -2"):   # CT_ERR_UNSUPPORTED: not the reference-order kernel
                        _fused(x, stages, expo, layout, **dict(kw, reference_order=None))
    assert {w for _, w in seen} == {0, 1, 2, 3} and {s for s, _ in seen} == set(shapes)


# ---- 2. streaming ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
def test_streaming_batches(dev, layout):
    """Batches of 3, 2 and 3 exposures with the state carried along: equal to the two launches after every batch, and to
    one compute_hdr_image call on the same frames."""
    T = _T()
    from clair_torch_amd import ops
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    rng = np.random.default_rng(11)
    shape = (8, 3, 7, 13)
    planar = _draw(rng, shape, torch.uint16)
    host = _source(planar, layout)
    expo = _exposures(8)
    lut = _lut(3)
    lut_d = torch.from_numpy(lut).to(dev)
    stages = _stage_lists(torch.uint16, 3)[1]
    kw = dict(lut=lut_d, interp="linear", gaussian_weight=True, std_mode="multiplier", std_value=0.05)
    st_a, st_b = ops.MergeState(shape[1:], dev, True), ops.MergeState(shape[1:], dev, True)
    cuts = [(0, 3), (3, 5), (5, 8)]
    for a, b in cuts:
        x = host[a:b].contiguous().to(dev)
        want = _two_launches(x, stages, expo[a:b], layout, state=st_a, finalize=b == 8, **kw)
        got = _fused(x, stages, expo[a:b], layout, state=st_b, finalize=b == 8, **kw)
        assert _state_same(st_b, st_a), (a, b)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    assert st_b.batches == 3
    lead = [] if layout == "nchw" else [T.CvToTorch()]
    ds = _frames_dataset(host, expo.tolist(), MissingStdMode.MULTIPLIER, 0.05)
    loader = DataLoader(ds, batch_sampler=[list(range(a, b)) for a, b in cuts], collate_fn=custom_collate)
    model = ICRFModelDirect(icrf=torch.from_numpy(lut), interpolation_mode=InterpMode.LINEAR).to(dev)
    mean, std = compute_hdr_image(loader, "cuda", model, weight_fn=gaussian_value_weights,
                                  gpu_transforms=lead + [T.CastTo("float32"), T.Normalize(1023, 64)])
    assert _same_bits(mean, got[0]) and _same_bits(std, got[1])


def _frames_dataset(frames, times, std_mode=None, std_value=0.0, stds=None):
    """Raw frames of any layout ((H,W,3) BGR as an OpenCV reader hands them over; StackDataset itself insists on
    (N,C,H,W)), with the uncertainty hint of StackDataset or planar (C,H,W) uncertainty images."""
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import StackDataset

    class Frames(StackDataset):
        def __init__(self):
            self.values, self.stds, self.exposure_times = frames, stds, list(times)
            self.files = list(range(len(times)))
            self.missing_std_mode, self.materialize_std = std_mode or MissingStdMode.NONE, stds is not None
            self.std_hint = None if (std_mode is None or stds is not None) else (std_mode.name.lower(), float(std_value))

        def __len__(self):
            return len(self.exposure_times)

    return Frames()


# ---- 3. row bands ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "nhwc_bgr"])
def test_row_band_equals_its_rows_of_the_whole(dev, layout):
    from clair_torch_amd import ops
    rng = np.random.default_rng(13)
    planar = _draw(rng, (4, 3, 12, 13), torch.uint16)
    host = _source(planar, layout)
    band = (host[:, :, 5:9] if layout == "nchw" else host[:, 5:9]).contiguous().to(dev)
    expo = _exposures(4)
    lut_d = torch.from_numpy(_lut(3)).to(dev)
    stages = _stage_lists(torch.uint16, 3)[2]
    tile = ops.TileGeometry(h_global=12, row_offset=5)
    for interp in ("linear", "catmull"):
        kw = dict(lut=lut_d, interp=interp, gaussian_weight=True, std_mode="multiplier", std_value=0.05, reference_order=False)
        whole = _fused(host.to(dev), stages, expo, layout, **kw)
        got = _fused(band, stages, expo, layout, tile=tile, **kw)
        want = _two_launches(band, stages, expo, layout, tile=tile, **kw)
        for k in range(2):
            assert _same_bits(got[k], want[k]), (interp, k)
            assert _same_bits(got[k], whole[k][:, 5:9].contiguous()), (interp, k)
        untold = _fused(band, stages, expo, layout, **kw)
        assert not _same_bits(untold[0], got[0]), "the band would not need its position"


# ---- 4. an independent comparand -----------------------------------------------------------------------------------------------
def _consistent_codes(rng, n, c, h, w, t, black, span):
    """Exposures of one scene through a gamma curve, on a black level: what the oracle's closed form is well conditioned on."""
    e = rng.random((c, h, w)) * (2.0 / np.sqrt(t[0] * t[-1]))
    lin = np.clip(e[None] * t[:, None, None, None], 0.0, 1.0)
    return torch.from_numpy((black + np.rint(lin ** (1 / 2.2) * span)).astype(np.uint16))


@pytest.mark.parametrize("layout,interp,gauss,std_name", [("nchw", "linear", True, "multiplier"), ("nhwc_bgr", None, False, "constant")])
def test_against_the_float64_oracle(dev, layout, interp, gauss, std_name):
    """A black-level chain run by the transform classes on the CPU, then the float64 oracle of the merge tests."""
    T = _T()
    from oracle import ct_oracle as oc
    rng = np.random.default_rng(17)
    n, c, h, w = 6, 3, 9, 21
    t = 0.002 * 2.0 ** np.arange(n)
    planar = _consistent_codes(rng, n, c, h, w, t, 64, 959)
    planar[:, :, 0, :4] = 10   # below the black level: pixels below 0, clamped with a masked gradient
    chain = [T.CastTo("float32"), T.Normalize(1023, 64)]
    pixels = planar
    for tr in chain:
        pixels = tr(pixels)
    pixels = pixels.numpy()
    assert pixels.dtype == np.float32 and (pixels < 0).any()
    host = _source(planar, layout)
    plan = T.plan_staging(host, ([] if layout == "nchw" else [T.CvToTorch()]) + chain)
    assert plan.route == "ingest" and plan.source_layout == layout
    lut = _lut(c, 256)
    value = 0.05 if std_name == "multiplier" else 0.01
    sd = pixels * np.float32(value) if std_name == "multiplier" else np.full_like(pixels, np.float32(value))
    mean, std = _fused(host.to(dev), plan.stages, torch.from_numpy(t), layout, lut=None if interp is None else torch.from_numpy(lut).to(dev),
                       interp=interp, gaussian_weight=gauss, std_mode=std_name, std_value=value)
    mean_o, std_o = oc.hdr_merge(pixels, sd, t, None if interp is None else lut, interp or "none", gauss)
    assert_parity(mean.cpu().numpy(), mean_o, rtol=1e-5, norm_tol=1e-6, what=f"{layout} {interp} mean vs oracle")
    assert_parity(std.cpu().numpy(), std_o, rtol=1e-5, norm_tol=1e-5, what=f"{layout} {interp} std vs oracle")


# ---- 5. a data-dependent Normalize -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
def test_data_dependent_normalize(dev, layout):
    T = _T()
    from clair_torch_amd import ops
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    rng = np.random.default_rng(19)
    planar = torch.from_numpy(rng.integers(16, 1001, size=(4, 3, 7, 13)).astype(np.uint16))
    host = _source(planar, layout)
    x = host.to(dev)
    expo = _exposures(4)
    lut_d = torch.from_numpy(_lut(3)).to(dev)
    lead = [] if layout == "nchw" else [T.CvToTorch()]
    kw = dict(lut=lut_d, interp="linear", gaussian_weight=True, std_mode="multiplier", std_value=0.05)
    for norm in (T.Normalize(), T.Normalize(max_val=None, min_val=16)):
        plan = T.plan_staging(x, lead + [T.CastTo("float32"), norm])
        assert plan.route == "ingest_data" and plan.source_layout == layout
        consts = ops.ingest_extrema(x, plan.prefix, layout, plan.min_val, plan.max_val)
        want = _two_launches(x, plan.stages, expo, layout, consts=consts, **kw)
        got = _fused(x, plan.stages, expo, layout, consts=consts, **kw)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
        assert float(got[0].max()) > 0
    # a constant stack: the reference's ValueError, through the public entry point
    flat = torch.full_like(host, 77)
    loader = DataLoader(_frames_dataset(flat, expo.tolist(), MissingStdMode.MULTIPLIER, 0.05), batch_size=4, shuffle=False,
                        collate_fn=custom_collate)
    model = ICRFModelDirect(icrf=torch.from_numpy(_lut(3)), interpolation_mode=InterpMode.LINEAR).to(dev)
    with pytest.raises(ValueError, match="Normalization range is zero"):
        compute_hdr_image(loader, "cuda", model, gpu_transforms=lead + [T.CastTo("float32"), T.Normalize()])


# ---- 6. the repeat pass ------------------------------------------------------------------------------------------------------------
def _pivot_condition_ratio(pixels, t, lut, std_value=0.05):
    """Host evidence that a first batch trips the conditioning test of the pivoted float32 moments (LINEAR, Gaussian weights,
    sigma = std_value * x): per element (t1 + |t2| + t3) / (t1 + t2 + t3) of the kernels' epilogue, in float64, with the pivot
    from exposure B / 2.  The kernels repeat the batch where it exceeds kPivotCondLimit = 8."""
    b, c, h, w = pixels.shape
    x = pixels.astype(np.float64)
    top = lut.shape[1] - 1
    row = (np.arange(c * h * w).reshape(c, h, w) % c)[None].repeat(b, 0)   # the reference's flat index modulo C
    sraw = x * top
    ok = (sraw >= 0) & (sraw <= top)
    s = np.clip(sraw, 0, top)
    i0 = np.minimum(np.floor(s).astype(np.int64), top)
    i1 = np.minimum(i0 + 1, top)
    g0, g1 = lut.astype(np.float64)[row, i0], lut.astype(np.float64)[row, i1]
    lin, dfdx = g0 + (g1 - g0) * (s - i0), (g1 - g0) * top * ok
    tt = np.asarray(t, dtype=np.float64)[:, None, None, None]
    y, dy = lin / tt, dfdx / tt
    pivot = y[b // 2]
    wgt = np.exp(-30.0 * (x - 0.5) ** 2)
    dw = -60.0 * (x - 0.5) * wgt
    sigma = std_value * x
    a_n, c_n = dw * sigma, (dw * (y - pivot) + wgt * dy) * sigma
    W = wgt.sum(0)
    D = W + 1e-6
    qd = ((wgt * (y - pivot)).sum(0) - pivot * 1e-6) / D
    beta = 1.0 / D
    kap = -beta * qd
    t1, t2, t3 = beta * beta * (c_n * c_n).sum(0), 2 * beta * kap * (a_n * c_n).sum(0), kap * kap * (a_n * a_n).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (t1 + np.abs(t2) + t3) / (t1 + t2 + t3)


@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
def test_repeat_about_the_mean(dev, layout):
    """The stack of the merge tests' retry case (the first batch's pivot seed black or saturated, a second batch far from the
    running mean) on a black level, with a plateau-then-rise LUT and with a plain one: the conditioning test fires and the
    batch is repeated about the mean -- in both routes alike."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(123)
    n, c, h, w = 8, 3, 8, 32
    t = 0.001 * 2.0 ** np.arange(n)
    codes = _consistent_codes(rng, n, c, h, w, t, 64, 959).numpy()
    for probe in (n // 2, 5 // 2):
        codes[probe, :, :, : w // 2] = 64
        codes[probe, :, :, w // 2:] = 1023
    codes[5:] = (64 + np.rint((codes[5:].astype(np.float64) - 64) * 0.2)).astype(np.uint16)
    host = _source(torch.from_numpy(codes), layout)
    grid = np.linspace(0, 1, 256, dtype=np.float64)
    plateau = np.stack([np.where(grid < 100 / 255, 0.0, ((grid - 100 / 255) / (155 / 255)) ** p) for p in (3.0, 4.0, 5.0)]).astype(np.float32)
    stages = _stage_lists(torch.uint16, 3)[1]
    expo = torch.from_numpy(t)
    pixels = ((codes.astype(np.float32) - np.float32(64)) / np.float32(959))
    for lut in (plateau, _lut(3, 256)):
        # the repeat does run: in both first batches many elements are far beyond the conditioning limit of 8 (twice over,
        # so float32 rounding cannot decide it), and one such element makes its whole wavefront repeat the batch
        for first_batch in (pixels, pixels[:5]):
            ratio = _pivot_condition_ratio(first_batch, t[:len(first_batch)], lut)
            assert int((ratio > 16).sum()) >= 16, "this stack would not make the merge repeat a batch"
        kw = dict(lut=torch.from_numpy(lut).to(dev), interp="linear", gaussian_weight=True, std_mode="multiplier", std_value=0.05)
        for part in ([(0, 8)], [(0, 5), (5, 8)]):
            st_a, st_b = ops.MergeState((c, h, w), dev, True), ops.MergeState((c, h, w), dev, True)
            for a, b in part:
                x = host[a:b].contiguous().to(dev)
                want = _two_launches(x, stages, expo[a:b], layout, state=st_a, finalize=b == n, **kw)
                got = _fused(x, stages, expo[a:b], layout, state=st_b, finalize=b == n, **kw)
                assert _state_same(st_b, st_a), part
            assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), part
            assert bool(torch.isfinite(got[1]).all())


# ---- 7. guard margins ----------------------------------------------------------------------------------------------------------------
def _guarded(dev, n, dtype, lead, trail=29):
    buf = torch.full((lead + n + trail,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[lead:lead + n]


def _margins_untouched(buf, n, lead):
    flat = buf.cpu()
    return bool((flat[:lead] == SENTINEL).all()) and bool((flat[lead + n:] == SENTINEL).all())


@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
@pytest.mark.parametrize("leads", [(2, 4, 4, 2, 4), (1, 3, 2, 1, 1)])
def test_guard_margins_and_frames_untouched(dev, layout, leads):
    """State and outputs inside larger buffers, 16-byte aligned and not (element-wise accesses): nothing outside them is
    written, the frames are as they were, and the bits are those of the two launches."""
    from clair_torch_amd import _native as nv
    from clair_torch_amd import ops
    rng = np.random.default_rng(23)
    b, c, h, w = 5, 3, 7, 13
    q = c * h * w
    planar = _draw(rng, (b, c, h, w), torch.uint16)
    host = _source(planar, layout)
    x = host.to(dev)
    expo = _exposures(b).to(dev)
    lut_d = torch.from_numpy(_lut(c)).to(dev)
    stage_list = _stage_lists(torch.uint16, c)[3]
    arr, n_stages = ops._ingest_stages(stage_list, c)
    want_state = ops.MergeState((c, h, w), dev, True)
    kw = dict(lut=lut_d, interp="linear", gaussian_weight=True, std_mode="multiplier", std_value=0.05)
    _two_launches(x[:3].contiguous(), stage_list, expo[:3], layout, state=want_state, finalize=False, **kw)
    want = _two_launches(x[3:].contiguous(), stage_list, expo[3:], layout, state=want_state, **kw)
    dtypes = (torch.float64, torch.float32, torch.float32, torch.float64, torch.float32)  # mean, sumw, var, mean_out, std_out
    bufs = [_guarded(dev, q, dt, lead) for dt, lead in zip(dtypes, leads)]
    mean_s, sumw_s, var_s, mean_o, std_o = (v for _, v in bufs)
    icrf = nv.Icrf(lut_dev=lut_d.data_ptr(), n_points=lut_d.shape[1], interp=nv.INTERP_LINEAR)
    lay = {"nchw": nv.LAYOUT_NCHW, "nhwc_bgr": nv.LAYOUT_NHWC_BGR}[layout]
    geom = nv.Geometry(channels=c, h_tile=h, width=w, h_global=h, row_offset=0, image_stride=q, layout=lay)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for (a, e), flags in (((0, 3), nv.MERGE_FIRST_BATCH), ((3, 5), nv.MERGE_FINALIZE)):
        part = x[a:e].contiguous()
        rc = nv.load().ct_hdr_merge_ingest_batch(p(part), nv.DTYPE_U16, e - a, ctypes.byref(geom), arr, n_stages, None, None,
                                                 nv.STD_MULTIPLIER, 0.05, p(expo[a:e].contiguous()), ctypes.byref(icrf), nv.WEIGHT_GAUSS,
                                                 p(mean_s), p(sumw_s), p(var_s), p(mean_o), p(std_o), flags, stream)
        assert rc == 0
        if a == 0:  # not finalised: the outputs are not written
            torch.cuda.synchronize()
            assert bool((mean_o == SENTINEL).all()) and bool((std_o == SENTINEL).all())
    torch.cuda.synchronize()
    for (buf, _), lead in zip(bufs, leads):
        assert _margins_untouched(buf, q, lead)
    shape = (c, h, w)
    assert _same_bits(mean_o.view(shape), want[0]) and _same_bits(std_o.view(shape), want[1])
    assert _same_bits(mean_s.view(shape), want_state.mean) and _same_bits(sumw_s.view(shape), want_state.sumw)
    assert _same_bits(var_s.view(shape), want_state.var)
    assert torch.equal(x.cpu().view(torch.int16), host.view(torch.int16)), "the frames were written to"


# ---- 8. the public entry point, and proof of the route ------------------------------------------------------------------------------
def test_compute_hdr_image_takes_the_fused_route(dev, monkeypatch):
    T = _T()
    from clair_torch_amd import ops
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import ArtefactStack, custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    rng = np.random.default_rng(29)
    n, c, h, w = 6, 3, 9, 14
    t = 0.002 * 2.0 ** np.arange(n)
    frames = _source(_consistent_codes(rng, n, c, h, w, t, 64, 959), "nhwc_bgr")
    chain = [T.CvToTorch(), T.CastTo("float32"), T.Normalize(1023, 64)]
    ds = _frames_dataset(frames, t.tolist(), MissingStdMode.MULTIPLIER, 0.05)
    lut = torch.from_numpy(_lut(c, 256))

    def run(mode=InterpMode.LINEAR, **kw):
        loader = DataLoader(ds, batch_size=4, shuffle=False, collate_fn=custom_collate)
        model = ICRFModelDirect(icrf=lut.clone(), interpolation_mode=mode).to(dev)
        return compute_hdr_image(loader, "cuda", model, weight_fn=gaussian_value_weights, gpu_transforms=chain, **kw)

    fused, plain = run(fused_ingest=True), run(fused_ingest=False)
    assert fused[0].dtype == torch.float64 and tuple(fused[0].shape) == (c, h, w) and fused[1].dtype == torch.float32
    assert _same_bits(fused[0], plain[0]) and _same_bits(fused[1], plain[1])
    assert _same_bits(run()[0], fused[0])   # the default

    def refuse(*args, **kwargs):
        raise AssertionError("ct_ingest_transform ran: the float32 route was taken")

    monkeypatch.setattr(ops, "ingest_transform", refuse)
    again = run()
    assert _same_bits(again[0], fused[0]) and _same_bits(again[1], fused[1])
    closed = run(InterpMode.CATMULL, reference_order=False)   # closed form: fused as well
    assert bool(torch.isfinite(closed[1]).all())
    with pytest.raises(AssertionError, match="float32 route"):
        run(fused_ingest=False)
    with pytest.raises(AssertionError, match="float32 route"):   # LOOKUP with uncertainties: the reference-order kernel by default
        run(InterpMode.LOOKUP)
    with pytest.raises(AssertionError, match="float32 route"):   # a dark field works on the planar float32 batch
        dark = ArtefactStack(torch.zeros((c, h, w)), torch.zeros((c, h, w)))
        run(dark_field_dataset=dark)


# ---- 9. footprint --------------------------------------------------------------------------------------------------------------------
def test_no_float32_copy_of_the_batch(dev):
    T = _T()
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    rng = np.random.default_rng(31)
    shape = (8, 3, 256, 256)
    codes = torch.from_numpy(rng.integers(0, 1024, size=shape).astype(np.uint16))
    ds = StackDataset(codes, _exposures(8).tolist(), missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05,
                      materialize_std=False)
    model = ICRFModelDirect(icrf=torch.from_numpy(_lut(3, 256)), interpolation_mode=InterpMode.LINEAR).to(dev)
    float_stack = 4 * int(np.prod(shape))   # 6.3 MB

    def rise(fused):
        loader = DataLoader(ds, batch_size=8, shuffle=False, collate_fn=custom_collate)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = compute_hdr_image(loader, "cuda", model, weight_fn=gaussian_value_weights, fused_ingest=fused,
                                gpu_transforms=[T.CastTo("float32"), T.Normalize(1023, 64)])
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del out
        return peak

    rise(True)   # (warm-up: library load, the model's own buffers)
    fused, plain = rise(True), rise(False)
    print(f"peak rise: fused {fused} B, two launches {plain} B, float32 stack {float_stack} B")
    assert fused < float_stack
    assert plain >= float_stack


# ---- 10. graph capture ------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_bit_identically(dev):
    rng = np.random.default_rng(37)
    planar = _draw(rng, (4, 3, 17, 33), torch.uint16)
    frames = _source(planar, "nhwc_bgr").to(dev)
    expo = _exposures(4).to(dev)
    lut_d = torch.from_numpy(_lut(3)).to(dev)
    stages = _stage_lists(torch.uint16, 3)[2]
    kw = dict(lut=lut_d, interp="linear", gaussian_weight=True, std_mode="multiplier", std_value=0.05)
    eager = _fused(frames, stages, expo, "nhwc_bgr", **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        _fused(frames, stages, expo, "nhwc_bgr", **kw)  # warm-up on the capture stream
    side.synchronize()
    with torch.cuda.graph(graph, stream=side):  # one launch, one stream: a linear chain
        out = _fused(frames, stages, expo, "nhwc_bgr", **kw)
    for _ in range(2):
        out[0].zero_()
        out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out[0], eager[0]) and _same_bits(out[1], eager[1])
    want = _two_launches(frames, stages, expo, "nhwc_bgr", **kw)
    assert _same_bits(out[0], want[0]) and _same_bits(out[1], want[1])


# ---- the custom op -------------------------------------------------------------------------------------------------------------------
def test_custom_op(dev):
    from clair_torch_amd import ops, torch_ops
    rng = np.random.default_rng(41)
    planar = _draw(rng, (3, 3, 6, 10), torch.uint16)
    frames = _source(planar, "nhwc_bgr").to(dev)
    expo = _exposures(3)
    lut_d = torch.from_numpy(_lut(3)).to(dev)
    stages = _stage_lists(torch.uint16, 3)[2]
    flat = torch_ops.flatten_ingest_stages(stages, 3)
    want = _two_launches(frames, stages, expo, "nhwc_bgr", lut=lut_d, interp="linear", std_mode="multiplier", std_value=0.05)
    mean, sd = torch.ops.clair_hip.hdr_merge_ingest_batch(frames, flat, expo, lut_d, "linear", True, None, "multiplier", 0.05, "nhwc_bgr")
    assert _same_bits(mean, want[0]) and _same_bits(sd, want[1])
    data = [("affine_data", 1.0, 0.0)]
    consts = ops.ingest_extrema(frames, [], "nhwc_bgr")
    want = _two_launches(frames, data, expo, "nhwc_bgr", consts=consts, lut=lut_d, interp="catmull", gaussian_weight=False)
    mean, sd = torch.ops.clair_hip.hdr_merge_ingest_batch(frames, torch_ops.flatten_ingest_stages(data, 3), expo, lut_d, "catmull", False,
                                                          None, "none", 0.0, "nhwc_bgr", 0, 0, False, consts)
    assert _same_bits(mean, want[0]) and sd.numel() == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.hdr_merge_ingest_batch(planar, stages, expo, lut=lut_d)
    with pytest.raises(TypeError):
        ops.hdr_merge_ingest_batch(planar.to(dev).float(), stages, expo, lut=lut_d)
    with pytest.raises(ValueError):
        ops.hdr_merge_ingest_batch(planar.to(dev), stages, expo[:2], lut=lut_d)
    with pytest.raises(ValueError):   # an explicit std is planar
        ops.hdr_merge_ingest_batch(frames, stages, expo, lut=lut_d, layout="nhwc_bgr", std=torch.zeros(frames.shape, device=dev))
