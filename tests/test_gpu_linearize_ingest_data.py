"""The data-dependent Normalize of the streamed linearization on the device.  Every specification here is an equality of bit
patterns, with launches the project already had or with the CPU:
  1. ``ops.ingest_extrema_frames(x)[f]``  ==  ``ops.ingest_extrema(x[f:f+1])`` -- min, max and the NaN flag are exact and
     order-independent, so the partition of the work cannot show -- and, since both run one kernel, == the extrema of
     frame f behind the prefix as the transform classes give them on the CPU;
  2. ``ops.linearize_ingest_frames(frames, stages, ..., consts=K)[f]``  ==  ``ops.linearize_frames(ops.ingest_transform(
     frames[f:f+1], stages, consts=K[f]), ...)``;
  3. the pipelined route of linearize_dataset_generator  ==  its frame-by-frame route  ==  the CPU classes' chain applied
     frame by frame followed by ``oracle.ct_oracle.linearize_std``;
  4. the reference's zero-range ValueError arrives where the frame-by-frame route raises it;
  5. the two calls replay from one linear graph capture."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

F = 5
CLAMP3 = [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)]
_TORCH_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.float32: np.float32}
# the value of one uint8 code step in each dtype (float32 pixels are no whole numbers)
_SCALE = {torch.uint8: 1, torch.uint16: 257, torch.float32: 0.25}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _T():
    from clair_torch_amd.common import transforms
    return transforms


def _lut(channels, points):
    powers = (2.2, 1.8, 2.6, 1.4, 3.0)[:channels]
    return np.stack([np.linspace(0, 1, points, dtype=np.float32) ** np.float32(p) for p in powers])


def _bgr_frames(planar):
    """(B,3,H,W) RGB planes -> the (B,H,W,3) BGR frames an OpenCV reader hands over."""
    return torch.from_numpy(np.ascontiguousarray(planar.numpy()[:, ::-1].transpose(0, 2, 3, 1)))


def _interleave(planar, layout):
    if layout == "nchw":
        return planar
    if layout == "nhwc":
        return torch.from_numpy(np.ascontiguousarray(planar.numpy().transpose(0, 2, 3, 1)))
    return _bgr_frames(planar)


def _cpu_chain(host, transforms):
    x = host
    for t in transforms:
        x = t(x)
    assert x.dtype == torch.float32 and not x.is_cuda
    return x.contiguous()


def _bits(t):
    t = t.cpu() if t.is_cuda else t
    assert t.dtype == torch.float32
    return t.contiguous().view(torch.int32)


def _same_bits(got, want, nan_ok=False):
    """Equal bit patterns; ``nan_ok``: NaNs must sit at the same places, their payloads are not compared."""
    got = got.cpu() if got.is_cuda else got
    want = torch.from_numpy(want) if isinstance(want, np.ndarray) else (want.cpu() if want.is_cuda else want)
    if tuple(got.shape) != tuple(want.shape):
        return False
    if nan_ok:
        nan = torch.isnan(want)
        if not torch.equal(torch.isnan(got), nan):
            return False
        got, want = torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want)
    return torch.equal(_bits(got), _bits(want))


# ---- 1. extrema per frame ------------------------------------------------------------------------------------------------
def _bordered_frames(rng, shape, dtype):
    """(F,) + shape frames IN MEMORY ORDER (the caller names the layout): frame f's minimum lo_f sits in its first element
    and its maximum hi_f in its last, and both fall with f.  So the element behind frame f's last is lo_{f+1} < lo_f and
    the one in front of its first is hi_{f-1} > hi_f: a walk that crosses a frame border by one element changes a result.
    Returns the frames and the planted (lo_f, hi_f) in the frames' own unit."""
    n = int(np.prod(shape))
    lo = np.array([40 - 8 * f for f in range(F)], dtype=np.int64)
    hi = np.array([250 - 10 * f for f in range(F)], dtype=np.int64)
    flat = np.empty((F, n), dtype=np.int64)
    for f in range(F):
        flat[f] = rng.integers(lo[f] + 1, hi[f], size=n)
        flat[f, 0], flat[f, -1] = lo[f], hi[f]
        if n == 3:
            flat[f, 1] = (lo[f] + hi[f]) // 2 + f
    s = _SCALE[dtype]
    x = (flat * s).astype(_TORCH_NP[dtype]).reshape((F,) + tuple(shape))
    return torch.from_numpy(x), (lo * s).astype(np.float32), (hi * s).astype(np.float32)


def _prefixes(dtype):
    """The three prefix kinds in the frames' own unit: none (integer codes: the packed 16-bit reduction; float32: the
    uniform walk), a constant affine (the uniform walk), a per-channel clamp that cuts into planes 1 and 2 differently
    (planar: one span per plane; interleaved: the packed3 walk, whose channel phase is per frame)."""
    s = float(_SCALE[dtype])
    return {"none": [], "affine": [("affine", 3 * s, 201 * s, 2.0, -1.0)],
            "clamp": [("clamp", [(-1e30, 1e30), (60 * s, 200 * s), (50 * s, 190 * s)])]}


def _planar(mem, layout):
    """Host frames in memory order -> the planar (B,C,H,W) float32 tensor the chain receives."""
    x = mem.to(torch.float32)  # (exact for every code; torch flips no uint16)
    if layout != "nchw":
        x = x.permute(0, 3, 1, 2)
        x = x.flip(1) if layout == "nhwc_bgr" else x
    return x.contiguous()


def _cpu_extrema(planar, prefix):
    """x.min(), x.max() (0-dim float32) of ``planar`` behind the prefix stages, applied on the CPU by the project's own
    classes: ("affine", sub, div, mul, add) is Normalize(sub + div, sub, (add, add + mul)) -- every constant of _prefixes is
    exact in float32, so the class forms the same sub, div, mul and add -- and ("clamp", pairs) is ClampAlongDims(1, pairs)."""
    T = _T()
    classes = [T.Normalize(st[1] + st[2], st[1], (st[4], st[4] + st[3])) if st[0] == "affine" else T.ClampAlongDims(1, st[1])
               for st in prefix]
    x = _cpu_chain(planar, classes)
    return x.min(), x.max()


def _cpu_consts(lo, hi, mn, mx):
    """[sub, div = fl32(top - sub), data min, data max], formed in float32 as torch forms them."""
    sub = lo if mn is None else torch.tensor(mn, dtype=torch.float32)
    top = hi if mx is None else torch.tensor(mx, dtype=torch.float32)
    return torch.stack([sub, top - sub, lo, hi])


# 3x1x1: less than one packet; 3x5x7: 105 elements, so frame sizes are no multiples of 16 bytes and the heads differ per
# frame; 3x97x101: 29 391 elements, more than one workgroup trip per frame in every mode (the largest is 24 576 uint8
# elements for packed3)
_EXTREMA_SHAPES = [(3, 1, 1), (3, 5, 7), (3, 97, 101)]


@pytest.mark.parametrize("layout", ["nchw", "nhwc", "nhwc_bgr"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.float32])
def test_extrema_per_frame_equal_single_frame_calls(dev, dtype, layout):
    """Both calls run one kernel, so their equality checks the frame base, the per-frame head and the indexing of the
    partials; the values themselves are checked against the CPU, frame by frame."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(101)
    s = float(_SCALE[dtype])
    for chw in _EXTREMA_SHAPES:
        mem_shape = chw if layout == "nchw" else (chw[1], chw[2], chw[0])
        host, lo, hi = _bordered_frames(rng, mem_shape, dtype)
        x = host.to(dev)
        for kind, prefix in _prefixes(dtype).items():
            cpu = [_cpu_extrema(_planar(host[f:f + 1], layout), prefix) for f in range(F)]
            for mn, mx in ((None, None), (None, 300 * s), (-5 * s, None)):  # both, the minimum, the maximum from the data
                got = ops.ingest_extrema_frames(x, prefix, layout, mn, mx)
                assert tuple(got.shape) == (F, 4) and got.dtype == torch.float32 and got.device == x.device
                want = torch.stack([ops.ingest_extrema(x[f:f + 1], prefix, layout, mn, mx) for f in range(F)])
                assert _same_bits(got, want), (chw, kind, mn, mx, got.cpu(), want.cpu())
                ref = torch.stack([_cpu_consts(*cpu[f], mn, mx) for f in range(F)])
                assert _same_bits(got, ref), (chw, kind, mn, mx, got.cpu(), ref)
                if kind == "none":  # ... and what was planted
                    data = got.cpu().numpy()
                    assert np.array_equal(data[:, 2], lo) and np.array_equal(data[:, 3], hi), (chw, data)
                    if mn is None and mx is None:
                        assert np.array_equal(data[:, 0], lo) and np.array_equal(data[:, 1], hi - lo)


@pytest.mark.parametrize("layout,kind", [("nchw", "none"), ("nhwc_bgr", "clamp")])
def test_a_nan_stays_in_its_frame(dev, layout, kind):
    from clair_torch_amd import ops
    rng = np.random.default_rng(103)
    chw = (3, 5, 7)
    mem_shape = chw if layout == "nchw" else (chw[1], chw[2], chw[0])
    host, lo, hi = _bordered_frames(rng, mem_shape, torch.float32)
    host.view(F, -1)[2, 52] = float("nan")
    x = host.to(dev)
    prefix = _prefixes(torch.float32)[kind]
    got = ops.ingest_extrema_frames(x, prefix, layout)
    want = torch.stack([ops.ingest_extrema(x[f:f + 1], prefix, layout) for f in range(F)])
    assert _same_bits(got, want)
    data = got.cpu()
    assert torch.isnan(data[2]).all()  # sub = min and div = max - min come from the data here, so all four are NaN
    assert not torch.isnan(data[[0, 1, 3, 4]]).any()
    # a fixed bound is no NaN; the data extrema of that frame still are
    fixed = ops.ingest_extrema_frames(x, prefix, layout, -5.0, None).cpu()
    assert float(fixed[2, 0]) == -5.0 and torch.isnan(fixed[2, 1:]).all() and not torch.isnan(fixed[[0, 1, 3, 4]]).any()


def test_planes_of_a_second_image_take_their_channels_clamp(dev):
    """(2,3,5,7) uint16 planar behind the per-channel clamp: the whole-stack call walks six planes as one frame, and planes
    3 to 5 are channels 0 to 2 again (plane index % channels; the plane index alone would read pairs that are not there).
    The stack's extrema lie in the second image, where only its channel's pair cuts them.  Against the CPU, and the same
    stack through the per-frame call, where each image is a frame of three planes."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(163)
    s = _SCALE[torch.uint16]
    host = rng.integers(70, 181, size=(2, 3, 5, 7))
    host[1, 2, 2, 3], host[1, 1, 4, 6] = 10, 240  # below plane 2's lower bound 50, above plane 1's upper bound 200
    host = torch.from_numpy((host * s).astype(np.uint16))
    prefix = _prefixes(torch.uint16)["clamp"]
    x = host.to(dev)
    lo, hi = _cpu_extrema(_planar(host, "nchw"), prefix)
    assert float(lo) == 50 * s and float(hi) == 200 * s
    for mn, mx in ((None, None), (None, 300.0 * s), (-5.0 * s, None)):
        assert _same_bits(ops.ingest_extrema(x, prefix, "nchw", mn, mx), _cpu_consts(lo, hi, mn, mx)), (mn, mx)
        ref = torch.stack([_cpu_consts(*_cpu_extrema(_planar(host[f:f + 1], "nchw"), prefix), mn, mx) for f in range(2)])
        assert _same_bits(ops.ingest_extrema_frames(x, prefix, "nchw", mn, mx), ref), (mn, mx)


def test_extrema_front_end_buffers_and_custom_op(dev):
    from clair_torch_amd import ops, torch_ops
    rng = np.random.default_rng(107)
    host, _, _ = _bordered_frames(rng, (3, 5, 7), torch.uint16)
    x = host.to(dev)
    prefix = _prefixes(torch.uint16)["affine"]
    want = ops.ingest_extrema_frames(x, prefix)
    # caller-owned buffers: a workspace sized for more frames, an out slice of a larger tensor
    ws = ops.ingest_extrema_frames_workspace(16, dev)
    out = torch.full((16, 4), -7.25, device=dev)
    got = ops.ingest_extrema_frames(x, prefix, out=out[:F], workspace=ws)
    assert got.data_ptr() == out.data_ptr() and _same_bits(out[:F], want)
    assert bool((out[F:] == -7.25).all())
    assert _same_bits(ops.ingest_extrema_frames(x[:3], prefix, out=out[:3], workspace=ws), want[:3])
    with pytest.raises(ValueError):
        ops.ingest_extrema_frames(x, prefix, workspace=ws[:16])
    with pytest.raises(ValueError):
        ops.ingest_extrema_frames(x, prefix, out=out[:4])
    with pytest.raises((ValueError, TypeError)):
        ops.ingest_extrema_frames(x, prefix, out=out[:F].double())
    flat = torch_ops.flatten_ingest_stages(prefix, 3)
    assert _same_bits(torch.ops.clair_hip.ingest_extrema_frames(x, flat, "nchw"), want)
    assert _same_bits(torch.ops.clair_hip.ingest_extrema_frames(x, flat, "nchw", None, 70000.0),
                      ops.ingest_extrema_frames(x, prefix, "nchw", None, 70000.0))


# ---- 2. the fused pass -----------------------------------------------------------------------------------------------------
def _disjoint_frames(rng, chw, dtype, n=F):
    """Planar (n,) + chw codes, frame f within [f * R, (f + 1) * R): frame 0's constants fit no other frame."""
    r = 50 if dtype == torch.uint8 else 12000
    x = np.stack([rng.integers(f * r, (f + 1) * r, size=chw) for f in range(n)])
    return torch.from_numpy(x.astype(_TORCH_NP[dtype]))


def _stage_lists(dtype):
    s = 1.0 if dtype == torch.uint8 else 240.0
    black = ("affine", 2.0 * s, 1.0, 1.0, 0.0)  # a black level in code units in front of the data-dependent Normalize
    return [[("affine_data", 1.0, 0.0)], [black, ("affine_data", 1.25, -0.125), ("clamp", CLAMP3)]]


_MODES = [("linear", dict(std_mode="constant", std_value=0.01)), ("linear", dict(std_mode="multiplier", std_value=0.05)),
          ("linear", "explicit"), ("linear", dict(want_std=False)),
          ("catmull", dict(std_mode="constant", std_value=0.01)), ("catmull", dict(std_mode="multiplier", std_value=0.05)),
          ("catmull", "explicit"), ("catmull", dict(want_std=False)),
          ("lookup", dict(want_std=False)), ("lookup", dict(std_mode="none"))]


def _fused_equals_two_launches(dev, rng, chw, dtype, layout, modes, stage_lists):
    from clair_torch_amd import ops
    planar = _disjoint_frames(rng, chw, dtype)
    frames = _interleave(planar, layout).to(dev)
    lut_d = torch.from_numpy(_lut(3, 64)).to(dev)
    sigma = torch.from_numpy((0.001 + 0.02 * rng.random((F,) + tuple(chw))).astype(np.float32)).to(dev)
    for stages in stage_lists:
        K = ops.ingest_extrema_frames(frames, ops.data_stage_prefix(stages), layout)
        assert bool((K[:, 1] > 0).all())
        staged = [ops.ingest_transform(frames[f:f + 1], stages, layout, consts=K[f]) for f in range(F)]
        assert not _same_bits(staged[3], ops.ingest_transform(frames[3:4], stages, layout, consts=K[0])), "constants would not matter"
        for interp, kw in modes:
            explicit = kw == "explicit"
            kw = {} if explicit else kw
            got = ops.linearize_ingest_frames(frames, stages, lut_d, interp, std=sigma if explicit else None, layout=layout,
                                              consts=K, **kw)
            for f in range(F):
                want = ops.linearize_frames(staged[f], lut_d, interp, std=sigma[f:f + 1] if explicit else None, **kw)
                assert _same_bits(got[0][f:f + 1], want[0], nan_ok=True), (chw, interp, kw, f)
                if want[1] is None:
                    assert got[1] is None
                else:
                    assert _same_bits(got[1][f:f + 1], want[1], nan_ok=True), (chw, interp, kw, f)


@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16])
def test_fused_pass_equals_the_two_launches_per_frame(dev, dtype, layout):
    rng = np.random.default_rng(109)
    for chw in ((3, 5, 7), (3, 37, 41)):
        _fused_equals_two_launches(dev, rng, chw, dtype, layout, _MODES, _stage_lists(dtype))


@pytest.mark.parametrize("layout,dtype", [("nchw", torch.uint8), ("nhwc_bgr", torch.uint16)])
def test_fused_pass_on_more_than_one_workgroup_per_plane(dev, layout, dtype):
    """3x97x101: 9 797 pixels per plane, more than the 4 096 a workgroup owns."""
    rng = np.random.default_rng(113)
    _fused_equals_two_launches(dev, rng, (3, 97, 101), dtype, layout, [_MODES[1], _MODES[6]], _stage_lists(dtype)[1:])


@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
def test_a_row_band_with_the_whole_frames_constants(dev, layout):
    """Rows [2, 7) of 9: the fused pass applies the constants it is given, so a band that is handed the whole frame's
    constants (and told where it lies: the LINEAR / CATMULL row is the global flat index modulo C) equals those rows."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(127)
    planar = _disjoint_frames(rng, (3, 9, 13), torch.uint16)
    host = _interleave(planar, layout)
    rows = (lambda t: t[:, :, 2:7]) if layout == "nchw" else (lambda t: t[:, 2:7])
    stages = _stage_lists(torch.uint16)[1]
    lut_d = torch.from_numpy(_lut(3, 64)).to(dev)
    K = ops.ingest_extrema_frames(host.to(dev), ops.data_stage_prefix(stages), layout)
    for interp in ("linear", "catmull"):
        kw = dict(std_mode="multiplier", std_value=0.05, layout=layout, consts=K)
        whole = ops.linearize_ingest_frames(host.to(dev), stages, lut_d, interp, **kw)
        band = ops.linearize_ingest_frames(rows(host).contiguous().to(dev), stages, lut_d, interp,
                                           tile=ops.TileGeometry(h_global=9, row_offset=2), **kw)
        for k in range(2):
            assert _same_bits(band[k], whole[k][:, :, 2:7].contiguous()), (interp, k)
        for f in range(F):
            want = ops.linearize_frames(ops.ingest_transform(host[f:f + 1].to(dev), stages, layout, consts=K[f]), lut_d, interp,
                                        std_mode="multiplier", std_value=0.05)
            assert _same_bits(whole[0][f:f + 1], want[0]) and _same_bits(whole[1][f:f + 1], want[1]), (interp, f)


def test_more_plane_rows_than_one_grid_holds(dev):
    """F = 22 000 frames of 3x1x2 uint8: F * C = 66 000 workgroup rows, so the launch is chunked at row 65 535 = plane 0 of
    frame 21 845, and the chunk offset must be part of the frame index that selects the constants."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(131)
    n = 22000
    host = rng.integers(0, 256, size=(n, 3, 1, 2)).astype(np.uint8)
    host[:, 0, 0, 0] = rng.integers(0, 100, size=n)      # a range of at least 50 codes in every frame
    host[:, 2, 0, 1] = rng.integers(150, 256, size=n)
    x_host = torch.from_numpy(host)
    x = x_host.to(dev)
    stages = [("affine_data", 1.0, 0.0)]
    lut_d = torch.from_numpy(_lut(3, 64)).to(dev)
    K = ops.ingest_extrema_frames(x, (), "nchw")
    pix = x_host.to(torch.float32)
    lo, hi = pix.amin(dim=(1, 2, 3)), pix.amax(dim=(1, 2, 3))
    assert _same_bits(K, torch.stack([lo, hi - lo, lo, hi], dim=1))
    kw = dict(std_mode="multiplier", std_value=0.05)
    got = ops.linearize_ingest_frames(x, stages, lut_d, "linear", consts=K, **kw)
    # the chain as a float32 torch expression on the CPU (every operation rounded on its own, an IEEE division)
    chain = ((pix - lo.view(-1, 1, 1, 1)) / (hi - lo).view(-1, 1, 1, 1)) * 1.0 + 0.0
    want = ops.linearize_frames(chain.to(dev), lut_d, "linear", **kw)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    for f in (0, 21845, 21846, n - 1):
        two = ops.linearize_frames(ops.ingest_transform(x[f:f + 1], stages, consts=K[f]), lut_d, "linear", **kw)
        assert _same_bits(got[0][f:f + 1], two[0]) and _same_bits(got[1][f:f + 1], two[1]), f


def test_fused_front_end_and_custom_op(dev):
    from clair_torch_amd import ops, torch_ops
    rng = np.random.default_rng(137)
    planar = _disjoint_frames(rng, (3, 6, 10), torch.uint16)
    x, frames = planar.to(dev), _bgr_frames(planar).to(dev)
    lut_d = torch.from_numpy(_lut(3, 64)).to(dev)
    stages = _stage_lists(torch.uint16)[1]
    K = ops.ingest_extrema_frames(x, stages[:1])
    kw = dict(std_mode="multiplier", std_value=0.05)
    want = ops.linearize_ingest_frames(x, stages, lut_d, "linear", consts=K, **kw)
    flat = torch_ops.flatten_ingest_stages(stages, 3)
    for src, layout in ((x, "nchw"), (frames, "nhwc_bgr")):
        lin, sd = torch.ops.clair_hip.linearize_ingest_data(src, flat, K, lut_d, "linear", None, "multiplier", 0.05, layout)
        assert _same_bits(lin, want[0]) and _same_bits(sd, want[1]), layout
    # constants without a data stage are not read: the constant chain
    const = [("affine", 64, 4031, 1.0, 0.0), ("clamp", CLAMP3)]
    a = ops.linearize_ingest_frames(x, const, lut_d, "linear", consts=K, **kw)
    b = ops.linearize_ingest_frames(x, const, lut_d, "linear", **kw)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    # refusals
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x, stages, lut_d, "linear", **kw)                      # a data stage without constants
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x, stages, lut_d, "linear", consts=K[:4], **kw)
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x, stages, lut_d, "linear", consts=K[0], **kw)
    with pytest.raises((ValueError, TypeError)):
        ops.linearize_ingest_frames(x, stages, lut_d, "linear", consts=K.double(), **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linearize_ingest_frames(x, stages, lut_d, "linear", consts=K.cpu(), **kw)
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x, stages + [("affine_data", 1.0, 0.0)], lut_d, "linear", consts=K, **kw)
    with pytest.raises(RuntimeError, match="does not require grad"):
        ops.linearize_ingest_frames(x, stages, lut_d, "lookup", consts=K, **kw)


# ---- 3. the pipelined route ------------------------------------------------------------------------------------------------
def _raw_frames_dataset(frames, times, stds):
    """(H,W,3) BGR frames as an OpenCV reader hands them over, with planar (C,H,W) uncertainty images (StackDataset itself
    insists on (N,C,H,W) values)."""
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import StackDataset

    class RawFrames(StackDataset):
        def __init__(self):
            self.values, self.stds, self.exposure_times = frames, stds, times
            self.files, self.std_hint = list(range(len(times))), None
            self.missing_std_mode, self.materialize_std = MissingStdMode.NONE, True

        def __len__(self):
            return len(self.exposure_times)

    return RawFrames()


def _refuse(*args, **kwargs):
    raise AssertionError("the list took the frame-by-frame route")
    yield  # pragma: no cover - a generator, like the function it stands in for


def _model(dev, lut):
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.models import ICRFModelDirect
    return ICRFModelDirect(icrf=torch.from_numpy(lut), interpolation_mode=InterpMode.LINEAR).to(dev)


@pytest.mark.parametrize("pinned", [True, False])
@pytest.mark.parametrize("kind", ["planar_multiplier", "bgr_explicit_std", "planar_flat_field", "bgr_cv_output"])
def test_pipelined_route_equals_frame_by_frame(dev, monkeypatch, kind, pinned):
    """23 frames in groups of 3 (7 full groups + 2) through [CastTo, Normalize()] (planar_multiplier, bgr_cv_output behind
    CvToTorch) and through [(CvToTorch,) CastTo, Normalize(None, 64), ClampAlongDims] (the other two): the list takes the
    pipelined route (the frame-by-frame one is made to raise; on the parent commit it is the route these lists take), and
    every yielded frame, in order and with its own metadata, equals what the frame-by-frame route yields for the same
    dataset -- and the oracle on the CPU chain applied frame by frame, every frame normalised by its own extrema."""
    T = _T()
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import linearization, linearize_dataset_generator
    from oracle import ct_oracle as oc
    rng = np.random.default_rng(139)
    n, c, h, w = 23, 3, 37, 41
    lut = _lut(c, 256)
    model = _model(dev, lut)
    times = [float(k + 1) for k in range(n)]
    if kind in ("planar_multiplier", "bgr_cv_output"):
        chain = [T.CastTo("float32"), T.Normalize()]
    else:
        chain = [T.CastTo("float32"), T.Normalize(None, 64), T.ClampAlongDims(1, [(0.0, 1.0), (0.01, 0.95), (0.0, 0.9)])]
    # every frame has extrema of its own
    codes = torch.from_numpy(np.stack([rng.integers(3 * k, 3000 + 80 * k, size=(c, h, w)) for k in range(n)]).astype(np.uint16))
    pixels = torch.cat([_cpu_chain(codes[k:k + 1], chain) for k in range(n)]).numpy()
    pin = (lambda t: t.pin_memory()) if pinned else (lambda t: t)
    ff, cv = None, kind == "bgr_cv_output"
    if kind.startswith("planar"):
        ds = StackDataset(pin(codes), times, missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
        tf, sigma = chain, pixels * np.float32(0.05)
    else:
        sigma = (0.001 + 0.02 * rng.random((n, c, h, w))).astype(np.float32)
        ds = _raw_frames_dataset(pin(_bgr_frames(codes)), times, pin(torch.from_numpy(sigma)))
        tf = [T.CvToTorch()] + chain
    lin_o, sd_o = oc.linearize_std(pixels, sigma, lut, "linear")
    if kind == "planar_flat_field":
        flat = (0.6 + 0.4 * rng.random((c, h, w))).astype(np.float32)
        flat_std = (0.01 * rng.random((c, h, w))).astype(np.float32)
        ff = ArtefactStack(torch.from_numpy(flat), torch.from_numpy(flat_std))
        lin_o, sd_o = oc.flatfield_linearize(lin_o, sd_o, flat, flat_std)
    if cv:  # (H,W,C), channels reversed: what save_image writes
        lin_o, sd_o = (np.ascontiguousarray(a[:, ::-1].transpose(0, 2, 3, 1)) for a in (lin_o, sd_o))

    def run():
        loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
        return list(linearize_dataset_generator(loader, "cuda", model, flatfield_dataset=ff, gpu_transforms=tf,
                                                output_layout="cv" if cv else "planar"))

    monkeypatch.setattr(linearization, "_GROUP_BYTES", 2 * 4 * c * h * w * 3)  # groups of 3 frames
    with monkeypatch.context() as m:
        m.setattr(linearization, "_frame_by_frame", _refuse)
        got = run()
    with monkeypatch.context() as m:
        m.setattr(linearization, "pipeline_data_route", lambda probe, plan, has_dark: "frame_by_frame")
        slow = run()
    assert len(got) == len(slow) == n
    shape = (h, w, c) if cv else (c, h, w)
    for k in range(n):
        lin, sdv, meta = got[k]
        assert lin.device.type == "cpu" and tuple(lin.shape) == tuple(sdv.shape) == shape
        assert float(meta["exposure_time"]) == times[k] == float(slow[k][2]["exposure_time"])
        assert _same_bits(lin, slow[k][0]) and _same_bits(sdv, slow[k][1]), k
        assert _same_bits(lin, lin_o[k]) and _same_bits(sdv, sd_o[k]), k


# ---- 4. a zero range ---------------------------------------------------------------------------------------------------------
def _collect(gen):
    """What a consumer sees: the frames yielded in front of an exception, and the exception (or None)."""
    seen = []
    try:
        for item in gen:
            seen.append(item)
    except ValueError as e:
        return seen, e
    return seen, None


def test_zero_range_raises_where_the_frame_by_frame_route_raises(dev, monkeypatch):
    """7 frames in groups of 3, frame 4 constant: frames 0 to 3 arrive with the expected bits, then the reference's
    ValueError -- on both routes -- and nothing of frame 4's group is handed out behind it."""
    T = _T()
    from clair_torch_amd import ops
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import linearization, linearize_dataset_generator
    from oracle import ct_oracle as oc
    rng = np.random.default_rng(149)
    n, c, h, w = 7, 3, 11, 13
    lut = _lut(c, 256)
    model = _model(dev, lut)
    chain = [T.CastTo("float32"), T.Normalize()]
    codes = torch.from_numpy(rng.integers(0, 4000, size=(n, c, h, w)).astype(np.uint16))
    codes[4] = 777
    ds = StackDataset(codes, [float(k + 1) for k in range(n)], missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05,
                      materialize_std=False)
    pixels = torch.cat([_cpu_chain(codes[k:k + 1], chain) for k in range(4)]).numpy()
    lin_o, sd_o = oc.linearize_std(pixels, pixels * np.float32(0.05), lut, "linear")

    def run():
        loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
        return _collect(linearize_dataset_generator(loader, "cuda", model, gpu_transforms=chain))

    monkeypatch.setattr(linearization, "_GROUP_BYTES", 2 * 4 * c * h * w * 3)
    with monkeypatch.context() as m:
        m.setattr(linearization, "_frame_by_frame", _refuse)
        got, err = run()
    with monkeypatch.context() as m:
        m.setattr(linearization, "pipeline_data_route", lambda probe, plan, has_dark: "frame_by_frame")
        slow, slow_err = run()
    for seen, e in ((got, err), (slow, slow_err)):
        assert isinstance(e, ValueError) and str(e) == ops.ZERO_RANGE
        assert len(seen) == 4
        for k in range(4):
            assert float(seen[k][2]["exposure_time"]) == float(k + 1)
            assert _same_bits(seen[k][0], lin_o[k]) and _same_bits(seen[k][1], sd_o[k]), k


def test_a_nan_frame_raises_nothing(dev, monkeypatch):
    """float32 frames, frame 4 of 7 holds one NaN: its range is NaN, which is no zero (the reference's ``den == 0`` is
    false) -- NaN comes out for that frame only, its neighbours are untouched, on both routes."""
    T = _T()
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import linearization, linearize_dataset_generator
    rng = np.random.default_rng(151)
    n, c, h, w = 7, 3, 11, 13
    model = _model(dev, _lut(c, 256))
    chain = [T.Normalize()]
    frames = torch.from_numpy((0.1 + 0.8 * rng.random((n, c, h, w))).astype(np.float32))
    frames[4, 1, 5, 6] = float("nan")
    ds = StackDataset(frames, [float(k + 1) for k in range(n)], missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05,
                      materialize_std=False)

    def run():
        loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
        return _collect(linearize_dataset_generator(loader, "cuda", model, gpu_transforms=chain))

    monkeypatch.setattr(linearization, "_GROUP_BYTES", 2 * 4 * c * h * w * 3)
    with monkeypatch.context() as m:
        m.setattr(linearization, "_frame_by_frame", _refuse)
        got, err = run()
    with monkeypatch.context() as m:
        m.setattr(linearization, "pipeline_data_route", lambda probe, plan, has_dark: "frame_by_frame")
        slow, slow_err = run()
    assert err is None and slow_err is None and len(got) == len(slow) == n
    for k in range(n):
        # every pixel of frame 4 is NaN behind the chain, so every uncertainty |f'(x) * 0.05 x| of that frame is; the value
        # is what ct_linearize_std gives for a NaN pixel (its clamp to [0, L-1] takes NaN to LUT entry 0), on both routes
        assert bool(torch.isnan(got[k][1]).all()) == (k == 4) and bool(torch.isnan(got[k][1]).any()) == (k == 4), k
        assert not bool(torch.isnan(got[k][0]).any()) or k == 4, k
        assert _same_bits(got[k][0], slow[k][0], nan_ok=True) and _same_bits(got[k][1], slow[k][1], nan_ok=True), k


# ---- 5. graph capture --------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_on_fresh_frames(dev):
    """ingest_extrema_frames + linearize_ingest_frames(consts=) captured on ONE side stream (a linear graph: three kernel
    nodes in a chain, no parallel branches), replayed on fresh frames in the same buffers."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(157)
    first = _bgr_frames(_disjoint_frames(rng, (3, 17, 33), torch.uint16))
    fresh = _bgr_frames(_disjoint_frames(rng, (3, 17, 33), torch.uint16).flip(0))
    frames = first.to(dev)
    lut_d = torch.from_numpy(_lut(3, 64)).to(dev)
    stages = _stage_lists(torch.uint16)[1]
    prefix = ops.data_stage_prefix(stages)
    kw = dict(std_mode="multiplier", std_value=0.05, layout="nhwc_bgr")
    K = torch.empty((F, 4), device=dev)
    ws = ops.ingest_extrema_frames_workspace(F, dev)
    out = (torch.empty((F, 3, 17, 33), device=dev), torch.empty((F, 3, 17, 33), device=dev))

    def both():
        ops.ingest_extrema_frames(frames, prefix, "nhwc_bgr", out=K, workspace=ws)
        ops.linearize_ingest_frames(frames, stages, lut_d, "linear", out=out, consts=K, **kw)

    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        both()  # warm-up on the capture stream
    side.synchronize()
    with torch.cuda.graph(graph, stream=side):
        both()
    frames.copy_(fresh.to(dev))
    K.zero_()
    out[0].zero_()
    out[1].zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    eager_K = ops.ingest_extrema_frames(fresh.to(dev), prefix, "nhwc_bgr")
    eager = ops.linearize_ingest_frames(fresh.to(dev), stages, lut_d, "linear", consts=eager_K, **kw)
    assert _same_bits(K, eager_K) and _same_bits(out[0], eager[0]) and _same_bits(out[1], eager[1])
    stale = ops.linearize_ingest_frames(first.to(dev), stages, lut_d, "linear",
                                        consts=ops.ingest_extrema_frames(first.to(dev), prefix, "nhwc_bgr"), **kw)
    assert not _same_bits(out[0], stale[0]), "the replay would not have read the fresh frames"
