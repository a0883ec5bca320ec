"""ct_linearize_ingest on the device: a recognised gpu_transforms chain and the ICRF linearization in one pass.  Its
specification is one sentence -- the outputs are bit for bit those of ct_ingest_transform followed by ct_linearize_std on
its float32 result -- so every comparison here is an exact bit pattern, and the comparand is never the new kernel:
  (a) the two existing launches, ``ops.linearize_frames(ops.ingest_transform(x, stages, layout), lut, interp, ...)``;
  (b) the oracle, ``oracle.ct_oracle.linearize_std`` on the chain run with the project's transform classes on the CPU
      (LOOKUP / LINEAR, where the oracle is the reference bit for bit).
The pipelined route of linearize_dataset_generator is compared with the frame-by-frame route on the same dataset."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16}
CLAMP3 = [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)]
PAIRS = {1: [(0.05, 0.9)], 3: CLAMP3, 4: [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333), (0.01, 1.5)], 5: [(0.02, 0.95)]}
SENTINEL = -7.25


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


def _rgb_frames(planar):
    return torch.from_numpy(np.ascontiguousarray(planar.numpy().transpose(0, 2, 3, 1)))


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


def _two_launches(x, stages, lut, interp, layout="nchw", **kw):
    """Comparand (a): the float32 stack of ct_ingest_transform through ct_linearize_std."""
    from clair_torch_amd import ops
    return ops.linearize_frames(ops.ingest_transform(x, stages, layout=layout), lut, interp, **kw)


# ---- every code ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def all_codes():
    """uint16 (1,3,128,512): each plane holds all 65 536 codes (plane 0 in order); uint8 (1,3,16,16) likewise."""
    rng = np.random.default_rng(5)
    c16 = np.arange(65536, dtype=np.uint16)
    c8 = np.arange(256, dtype=np.uint8)
    u16 = np.stack([c16, rng.permutation(c16), c16[::-1]]).reshape(1, 3, 128, 512)
    u8 = np.stack([c8, rng.permutation(c8), c8[::-1]]).reshape(1, 3, 16, 16)
    return {torch.uint16: torch.from_numpy(np.ascontiguousarray(u16)), torch.uint8: torch.from_numpy(np.ascontiguousarray(u8))}


@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16])
def test_every_code(dev, all_codes, dtype, layout):
    """All codes through the chain [CastTo, Normalize(4095, 64) (, ClampAlongDims)] and the ICRF: equal to the two launches in
    every mode, and to the oracle on the CPU chain for LOOKUP / LINEAR."""
    T = _T()
    from clair_torch_amd import ops
    from oracle import ct_oracle as oc
    planar = all_codes[dtype]
    host = planar if layout == "nchw" else _bgr_frames(planar)
    lead = [] if layout == "nchw" else [T.CvToTorch()]
    x = host.to(dev)
    lut = _lut(3, 256)
    lut_d = torch.from_numpy(lut).to(dev)
    norms = [(4095, 64)] + ([(200, 16)] if dtype == torch.uint8 else [])  # uint8 codes reach x > 1 only with a smaller max
    for mx, mn in norms:
        chain = [T.CastTo("float32"), T.Normalize(mx, mn)]
        bare = _cpu_chain(planar, chain)
        # both sides of the clamp mask are exercised: codes below the black level, inside the range and above the maximum
        assert bool((bare < 0).any()) and bool(((bare >= 0) & (bare <= 1)).any())
        assert bool((bare > 1).any()) == (dtype == torch.uint16 or mx == 200)
        for ts in (chain + [T.ClampAlongDims(1, CLAMP3)], chain):
            plan = T.fusable_ingest(host, lead + ts)
            assert plan is not None and plan.layout == layout and plan.step == 1
            pixels = _cpu_chain(planar, ts).numpy()
            for interp in ("lookup", "linear", "catmull"):
                kw = dict(want_std=False) if interp == "lookup" else dict(std_mode="multiplier", std_value=0.05)
                lin, sd = ops.linearize_ingest_frames(x, plan.stages, lut_d, interp, layout=layout, **kw)
                lin_a, sd_a = _two_launches(x, plan.stages, lut_d, interp, layout, **kw)
                what = (mx, len(ts), interp)
                assert _same_bits(lin, lin_a), what
                if interp == "lookup":
                    assert sd is None and sd_a is None
                    lin_o, _ = oc.linearize_std(pixels, None, lut, interp)
                    assert _same_bits(lin, lin_o), what
                    continue
                assert _same_bits(sd, sd_a), what
                if interp == "linear":
                    lin_o, sd_o = oc.linearize_std(pixels, pixels * np.float32(0.05), lut, interp)
                    assert _same_bits(lin, lin_o) and _same_bits(sd, sd_o), what


# ---- ragged shapes ---------------------------------------------------------------------------------------------------
# (3,3,37,41): the plane is a multiple of neither 4 nor 3 -- heads, tails, unaligned planes 1 / 2 and the p % C quirk;
# one channel; four channels with four clamp pairs; five channels (one pair only); a single pixel
SHAPES = [(3, 3, 37, 41), (2, 1, 5, 7), (2, 4, 9, 10), (2, 5, 6, 6), (1, 3, 1, 1)]


def _draw(rng, shape, dtype):
    if dtype != torch.float32:
        top = 255 if dtype == torch.uint8 else 5000
        return torch.from_numpy(rng.integers(0, top + 1, size=shape).astype(_NP[dtype]))
    vals = (rng.random(shape, dtype=np.float32) * 5200.0 - 200.0).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, 64.0, 4095.0, 4096.0, 3.4028235e38],
                       dtype=np.float32)
    flat = vals.reshape(-1)
    at = rng.permutation(flat.size)[:min(special.size, flat.size)]
    flat[at] = special[:at.size]
    return torch.from_numpy(vals)


def _stage_lists(dtype, channels):
    sub, div = (16.0, 239.0) if dtype == torch.uint8 else (64.0, 4031.0)
    pairs = ("clamp", PAIRS[channels])
    code_clamp = ("clamp", [(sub + 4.0, sub + div - 40.0)])
    affine = ("affine", sub, div, 1.0, 0.0)
    return [[affine], [affine, pairs], [code_clamp, affine, pairs], [code_clamp, affine, pairs, ("affine", -0.125, 1.25, 0.9, 0.05)]]


def _guarded(dev, shape, lead, trail=37):
    n = int(np.prod(shape))
    buf = torch.full((lead + n + trail,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[lead:lead + n].view(shape)


def _margins_untouched(buf, shape, lead):
    n = int(np.prod(shape))
    flat = buf.cpu()
    return bool((flat[:lead] == SENTINEL).all()) and bool((flat[lead + n:] == SENTINEL).all())


@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.float32])
def test_ragged_shapes(dev, dtype):
    from clair_torch_amd import ops
    rng = np.random.default_rng(41)
    nan_ok = dtype == torch.float32
    combo = 0
    for shape in SHAPES:
        f, c, h, w = shape
        planar = _draw(rng, shape, dtype)
        sigma = (0.001 + 0.02 * rng.random(shape)).astype(np.float32)
        sigma.reshape(-1)[::7] = np.float32(3e-20)   # squares that underflow: the sqrtf branch
        sigma_d = torch.from_numpy(sigma).to(dev)
        sources = [("nchw", planar)] + ([("nhwc", _rgb_frames(planar)), ("nhwc_bgr", _bgr_frames(planar))] if c == 3 else [])
        luts = {n: torch.from_numpy(_lut(c, n)).to(dev) for n in (64, 257)}
        for layout, host in sources:
            x = host.to(dev)
            for stages in _stage_lists(dtype, c):
                for points, lut_d in luts.items():
                    for std_kw in (dict(std_mode="none"), dict(std_mode="constant", std_value=0.01),
                                   dict(std_mode="multiplier", std_value=0.05), dict(std=sigma_d), dict(want_std=False)):
                        combo += 1
                        interp = ("linear", "catmull")[combo % 2] if "want_std" not in std_kw else ("lookup", "linear", "catmull")[combo % 3]
                        lead = (4, 1, 2, 3)[combo % 4]  # aligned and unaligned outputs
                        what = (shape, layout, len(stages), points, sorted(std_kw), interp, lead)
                        lin_a, sd_a = _two_launches(x, stages, lut_d, interp, layout, **std_kw)
                        buf_l, out_l = _guarded(dev, shape, lead)
                        buf_s, out_s = _guarded(dev, shape, (lead + combo // 4) % 4 + 1)
                        want_std = std_kw.get("want_std", True)
                        lin, sd = ops.linearize_ingest_frames(x, stages, lut_d, interp, layout=layout,
                                                              out=(out_l, out_s if want_std else None), **std_kw)
                        assert lin is out_l and (sd is out_s if want_std else sd is None), what
                        assert _same_bits(lin, lin_a, nan_ok), what
                        assert _margins_untouched(buf_l, shape, lead), what
                        if want_std:
                            assert _same_bits(sd, sd_a, nan_ok), what
                        assert _margins_untouched(buf_s, shape, (lead + combo // 4) % 4 + 1), what
            back = x.cpu()
            same = back.view(torch.int16) == host.view(torch.int16) if dtype == torch.uint16 else \
                (back.view(torch.int32) == host.view(torch.int32) if dtype == torch.float32 else back == host)
            assert bool(same.all()), "the source frames were written to"


# ---- row bands -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
def test_row_bands_equal_the_whole(dev, layout):
    """(2,3,12,20) in bands of 5 and 7 rows: the LINEAR / CATMULL row is the GLOBAL flat index modulo C, so the bands must
    be told where they lie (band 2 starts at element 100 = 1 mod 3 of every plane)."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(43)
    planar = _draw(rng, (2, 3, 12, 20), torch.uint16)
    host = planar if layout == "nchw" else _bgr_frames(planar)
    stages = _stage_lists(torch.uint16, 3)[2]
    lut_d = torch.from_numpy(_lut(3, 64)).to(dev)
    rows = (lambda t, a, b: t[:, :, a:b]) if layout == "nchw" else (lambda t, a, b: t[:, a:b])
    for interp in ("linear", "catmull"):
        kw = dict(std_mode="multiplier", std_value=0.05, layout=layout)
        whole = ops.linearize_ingest_frames(host.to(dev), stages, lut_d, interp, **kw)
        want = _two_launches(host.to(dev), stages, lut_d, interp, layout, std_mode="multiplier", std_value=0.05)
        assert _same_bits(whole[0], want[0]) and _same_bits(whole[1], want[1]), interp
        bands = [ops.linearize_ingest_frames(rows(host, a, b).contiguous().to(dev), stages, lut_d, interp,
                                             tile=ops.TileGeometry(h_global=12, row_offset=a), **kw) for a, b in ((0, 5), (5, 12))]
        for k in range(2):
            assert _same_bits(torch.cat([bands[0][k], bands[1][k]], dim=2), whole[k]), (interp, k)
        untold = ops.linearize_ingest_frames(rows(host, 5, 12).contiguous().to(dev), stages, lut_d, interp, **kw)
        assert not _same_bits(untold[0], whole[0][:, :, 5:12].contiguous()), "the bands would not need their position"


# ---- front end, the custom op, graph capture ---------------------------------------------------------------------------
def test_front_end_checks_and_custom_op(dev):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from clair_torch_amd import ops, torch_ops
    rng = np.random.default_rng(47)
    planar = _draw(rng, (2, 3, 6, 10), torch.uint16)
    x, frames = planar.to(dev), _bgr_frames(planar).to(dev)
    lut_d = torch.from_numpy(_lut(3, 64)).to(dev)
    stages = [("affine", 64, 4031, 1.0, 0.0), ("clamp", CLAMP3)]
    kw = dict(std_mode="multiplier", std_value=0.05)
    want = _two_launches(x, stages, lut_d, "linear", **kw)
    got = ops.linearize_ingest_frames(x, stages, lut_d, "linear", **kw)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    # no stage at all is the cast alone
    pix = torch.from_numpy(rng.random((2, 3, 6, 10), dtype=np.float32)).to(dev)
    got = ops.linearize_ingest_frames(pix, [], lut_d, "catmull", **kw)
    want0 = ops.linearize_frames(pix, lut_d, "catmull", **kw)
    assert _same_bits(got[0], want0[0]) and _same_bits(got[1], want0[1])
    # the dispatcher-registered form, planar and interleaved, and its fake kernel
    flat = torch_ops.flatten_ingest_stages(stages, 3)
    for src, layout in ((x, "nchw"), (frames, "nhwc_bgr")):
        lin, sd = torch.ops.clair_hip.linearize_ingest(src, flat, lut_d, "linear", None, "multiplier", 0.05, layout)
        assert _same_bits(lin, want[0]) and _same_bits(sd, want[1]), layout
    sigma = torch.from_numpy((0.001 + 0.02 * rng.random((2, 3, 6, 10))).astype(np.float32)).to(dev)
    lin, sd = torch.ops.clair_hip.linearize_ingest(frames, flat, lut_d, "linear", sigma, "none", 0.0, "nhwc_bgr")
    want_e = _two_launches(x, stages, lut_d, "linear", std=sigma)
    assert _same_bits(lin, want_e[0]) and _same_bits(sd, want_e[1])
    with FakeTensorMode():
        lin, sd = torch.ops.clair_hip.linearize_ingest(torch.empty((2, 5, 7, 3), dtype=torch.uint16), flat, torch.empty((3, 64)),
                                                       "linear", None, "multiplier", 0.05, "nhwc_bgr")
        assert tuple(lin.shape) == tuple(sd.shape) == (2, 3, 5, 7) and lin.dtype == sd.dtype == torch.float32
    # empty frames: empty outputs, no call
    lin, sd = ops.linearize_ingest_frames(x[:0], stages, lut_d, "linear", **kw)
    assert tuple(lin.shape) == tuple(sd.shape) == (0, 3, 6, 10) and lin.dtype == torch.float32
    lin, sd = ops.linearize_ingest_frames(frames[:0], stages, lut_d, "linear", layout="nhwc_bgr", want_std=False)
    assert tuple(lin.shape) == (0, 3, 6, 10) and sd is None
    # refusals
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.linearize_ingest_frames(planar, stages, lut_d, "linear")
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x, [("affine_data", 1.0, 0.0)], lut_d, "linear")
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x, stages * 3, lut_d, "linear")
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x, stages, lut_d, "linear", layout="nhwc")      # (F,H,W,3) expected
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x.permute(0, 1, 3, 2), stages, lut_d, "linear")  # not contiguous
    with pytest.raises(TypeError):
        ops.linearize_ingest_frames(x.to(torch.float64), stages, lut_d, "linear")
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x, stages, lut_d[:2], "linear")                   # a LUT row per channel
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(frames, stages, lut_d, "linear", layout="nhwc_bgr", std=torch.zeros_like(frames, dtype=torch.float32))
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x, stages, lut_d, "linear", std=sigma.double())
    with pytest.raises(RuntimeError, match="does not require grad"):
        ops.linearize_ingest_frames(x, stages, lut_d, "lookup", **kw)
    good = torch.zeros((2, 3, 6, 10), device=dev)
    for bad in (torch.zeros((2, 3, 6, 9), device=dev), torch.zeros((2, 3, 6, 10), device=dev, dtype=torch.float64),
                torch.zeros((2, 3, 10, 6), device=dev).permute(0, 1, 3, 2), torch.zeros((2, 6, 10, 3), device=dev)):
        with pytest.raises(ValueError):
            ops.linearize_ingest_frames(x, stages, lut_d, "linear", out=(bad, good), **kw)
        with pytest.raises(ValueError):
            ops.linearize_ingest_frames(x, stages, lut_d, "linear", out=(good, bad), **kw)
    with pytest.raises(ValueError):
        ops.linearize_ingest_frames(x, stages, lut_d, "linear", out=(good, None), **kw)  # want_std needs out[1]
    with pytest.raises(RuntimeError):
        ops.linearize_ingest_frames(x, stages, lut_d, "linear", out=(torch.zeros((2, 3, 6, 10)), good), **kw)


def test_graph_capture_replays_bit_identically(dev):
    from clair_torch_amd import ops
    rng = np.random.default_rng(53)
    planar = _draw(rng, (2, 3, 17, 33), torch.uint16)
    frames = _bgr_frames(planar).to(dev)
    lut_d = torch.from_numpy(_lut(3, 64)).to(dev)
    stages = [("affine", 64, 4031, 2.0, -1.0), ("clamp", CLAMP3)]
    kw = dict(std_mode="multiplier", std_value=0.05, layout="nhwc_bgr")
    eager = ops.linearize_ingest_frames(frames, stages, lut_d, "linear", **kw)
    out = (torch.empty_like(eager[0]), torch.empty_like(eager[1]))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ops.linearize_ingest_frames(frames, stages, lut_d, "linear", out=out, **kw)  # warm-up on the capture stream
    side.synchronize()
    with torch.cuda.graph(graph, stream=side):  # one launch, one stream
        ops.linearize_ingest_frames(frames, stages, lut_d, "linear", out=out, **kw)
    out[0].zero_()
    out[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out[0], eager[0]) and _same_bits(out[1], eager[1])
    want = _two_launches(frames, stages, lut_d, "linear", "nhwc_bgr", std_mode="multiplier", std_value=0.05)
    assert _same_bits(out[0], want[0]) and _same_bits(out[1], want[1])


# ---- the pipelined route -----------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("pinned", [True, False])
@pytest.mark.parametrize("kind", ["planar_multiplier", "bgr_explicit_std", "planar_flat_field", "bgr_cv_output"])
def test_pipelined_route_equals_frame_by_frame(dev, monkeypatch, kind, pinned):
    """23 frames in groups of 3 (7 full groups + 2) through [CastTo, Normalize(4095, 64), ClampAlongDims]: the list takes
    the pipelined route (the frame-by-frame one is made to raise), and every yielded frame, in order and with its own
    metadata, equals what the frame-by-frame route yields for the same dataset -- and the oracle on the CPU chain."""
    T = _T()
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import linearization, linearize_dataset_generator
    from clair_torch_amd.models import ICRFModelDirect
    from oracle import ct_oracle as oc
    rng = np.random.default_rng(59)
    n, c, h, w = 23, 3, 37, 41
    lut = _lut(c, 256)
    model = ICRFModelDirect(icrf=torch.from_numpy(lut), interpolation_mode=InterpMode.LINEAR).to(dev)
    times = [float(k + 1) for k in range(n)]
    chain = [T.CastTo("float32"), T.Normalize(4095, 64), T.ClampAlongDims(1, [(0.0, 1.0), (0.01, 0.95), (0.0, 0.9)])]
    codes = torch.from_numpy(rng.integers(0, 5001, size=(n, c, h, w)).astype(np.uint16))
    pixels = _cpu_chain(codes, chain).numpy()
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

    def refuse(*args, **kwargs):
        raise AssertionError("the list took the frame-by-frame route")
        yield  # pragma: no cover - a generator, like the function it stands in for

    monkeypatch.setattr(linearization, "_GROUP_BYTES", 2 * 4 * c * h * w * 3)  # groups of 3 frames
    with monkeypatch.context() as m:
        m.setattr(linearization, "_frame_by_frame", refuse)
        got = run()
    with monkeypatch.context() as m:
        m.setattr(linearization, "pipeline_route", lambda probe, plan, has_dark: "frame_by_frame")
        slow = run()
    assert len(got) == len(slow) == n
    shape = (h, w, c) if cv else (c, h, w)
    for k in range(n):
        lin, sdv, meta = got[k]
        assert lin.device.type == "cpu" and tuple(lin.shape) == tuple(sdv.shape) == shape
        assert float(meta["exposure_time"]) == times[k] == float(slow[k][2]["exposure_time"])
        assert _same_bits(lin, slow[k][0]) and _same_bits(sdv, slow[k][1]), k
        assert _same_bits(lin, lin_o[k]) and _same_bits(sdv, sd_o[k]), k
