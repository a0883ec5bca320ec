"""ct_video_stats_batches / ct_video_stats_ingest_batches on the device: several consecutive batches of the streaming video
statistics in one launch, the running (mean, m2) in registers in between.  Their specification is one sentence -- the state
is bit for bit that of the single-batch entry point applied to the batches in turn -- so section A compares exact values
(torch.equal on mean and m2, states starting from a sentinel fill).  That alone would be self-referential, so section B goes
through compute_video_mean_and_std(batches_per_launch=...) to the reference's arithmetic: the transform classes' own
__call__ on the CPU, then oracle.eager_torch.video_mean_std, with the tolerances tests/test_gpu_video_ingest.py carries
against that oracle.  Section C: nothing outside the two state arrays is written."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from _util import assert_parity

pytestmark = pytest.mark.gpu

_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16}
PAIRS = {1: [(0.05, 0.9)], 3: [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)]}
INTERPS = (None, "lookup", "linear", "catmull")
LAYOUTS = (("nchw", 3), ("nchw", 1), ("nhwc", 3), ("nhwc_bgr", 3))
SHAPES = ((5, 7), (1, 3), (8, 16))   # Q = 105: packets and a tail of 1, interleaved planes no multiple of 4; 3 pixels; whole packets
# BMAX 16 / BMAX 32 (chosen from the largest batch) / the full argument block at the reference's batch size / an empty batch
PARTITIONS = ([1, 4, 3], [16, 17, 1], [4] * 16, [3, 0, 2])
FORMS = (("code", torch.uint8), ("code", torch.uint16), ("code", torch.float32), ("ingest", torch.uint8), ("ingest", torch.uint16))
FORM_IDS = ["code-u8", "code-u16", "code-f32", "ingest-u8", "ingest-u16"]
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
    powers = (2.2, 2.4, 2.6)[:channels]  # different rows: the flat-index-modulo-C rule shows
    return torch.from_numpy(np.stack([np.linspace(0, 1, points, dtype=np.float32) ** np.float32(p) for p in powers]))


def _source(planar, layout):
    """(B,C,H,W) planes -> the stack in ``layout`` (BGR: what an OpenCV reader hands over)."""
    if layout == "nchw":
        return planar
    a = planar.numpy()
    return torch.from_numpy(np.ascontiguousarray((a[:, ::-1] if layout == "nhwc_bgr" else a).transpose(0, 2, 3, 1)))


def _chains(dtype, channels):
    sub, div = (16.0, 184.0) if dtype == torch.uint8 else (64.0, 959.0)  # Normalize(200, 16) / Normalize(1023, 64)
    black, clamp = ("affine", sub, div, 1.0, 0.0), ("clamp", PAIRS[channels])
    return {"black": [black], "clamp": [black, clamp], "range": [black, clamp, ("affine", -0.125, 1.25, 1.5, -0.25)],
            "four": [("clamp", [(sub - 8.0, sub + div + 20.0)]), black, clamp, ("affine", -0.125, 1.25, 1.5, -0.25)], "empty": []}


def _draw(rng, shape, dtype, small=False):
    """Codes below the black level, inside the range and above the maximum (``small``: mostly 0 .. 2, for the empty list);
    float32 pixels from below 0 to above 1."""
    if dtype == torch.float32:
        return torch.from_numpy(rng.uniform(-0.1, 1.1, size=shape).astype(np.float32))
    codes = rng.integers(0, (255 if dtype == torch.uint8 else 1100) + 1, size=shape)
    if small:
        codes = np.where(rng.random(shape) < 0.75, rng.integers(0, 3, size=shape), codes)
    return torch.from_numpy(codes.astype(_NP[dtype]))


def _odd_view(host, dev):
    """The stack on the device as a view one element into a larger buffer: the frames are only element-aligned."""
    alias = torch.int16 if host.dtype == torch.uint16 else host.dtype  # torch has no uint16 fill / copy kernels
    buf = torch.zeros((host.numel() + 9,), dtype=alias, device=dev)
    buf[1:1 + host.numel()].copy_(host.view(alias).reshape(-1).to(dev))
    view = buf.view(host.dtype)[1:1 + host.numel()].view(host.shape)
    assert view.data_ptr() % (2 * host.element_size()) != 0 and view.is_contiguous()
    return view


def _run(dev, form, host, layout, partition, lut, interp, stages=None, tile=None, data=False, odd=(), states=None,
         frames_before=0, one_launch=True):
    """The batches of ``partition`` one launch each, and all of them in one call, from ``frames_before`` frames on: equality
    of the two states.  Every batch is an allocation of its own (``odd``: the batch positions that sit one element into a
    larger buffer).  Returns the grouped (mean, m2)."""
    from clair_torch_amd import ops
    chw = ops.ingest_shape(tuple(host.shape), layout)[1:]
    if states is None:
        states = [torch.full(chw, SENTINEL, dtype=torch.float32, device=dev) for _ in range(4)]
        if frames_before:  # a state that is read: the same in both
            for s in states[:2]:
                s.copy_(torch.rand(chw, generator=torch.Generator().manual_seed(frames_before)).to(dev))
            states[2].copy_(states[0]), states[3].copy_(states[1])
    mean_g, m2_g, mean_s, m2_s = states
    kw = dict(lut=None if interp is None else lut.to(dev), interp=interp, tile=tile, layout=layout)
    if form == "code":
        kw["max_code"] = None if host.dtype == torch.float32 else (200.0 if host.dtype == torch.uint8 else 1023.0)
    parts, consts, k = [], [], 0
    for i, b in enumerate(partition):
        part = host[k:k + b].contiguous()
        parts.append(_odd_view(part, dev) if (i in odd and b > 0) else part.to(dev))
        if data:  # an empty batch has no extrema: any constants stand in for it, as the single-batch entry point wants them
            consts.append(ops.ingest_extrema(parts[-1], ops.data_stage_prefix(stages), layout) if b > 0 else consts[-1])
        k += b
    assert k == host.shape[0]
    before = frames_before
    for i, x in enumerate(parts):
        if x.shape[0] == 0:
            continue
        if form == "code":
            ops.video_stats_batch(x, mean_s, m2_s, before, **kw)
        else:
            ops.video_stats_ingest_batch(x, stages, mean_s, m2_s, before, consts=consts[i] if data else None, **kw)
        before += x.shape[0]
    if form == "code":
        ops.video_stats_batches(parts, mean_g, m2_g, frames_before, require_one_launch=one_launch, **kw)
    else:
        ops.video_stats_ingest_batches(parts, stages, mean_g, m2_g, frames_before, consts=consts if data else None,
                                       require_one_launch=one_launch, **kw)
    assert torch.equal(mean_g, mean_s) and torch.equal(m2_g, m2_s), (form, partition)
    assert not torch.isnan(mean_g).any() and not torch.isnan(m2_g).any()
    return mean_g, m2_g


# ---- A. bit equality with one launch per batch -----------------------------------------------------------------------------
# The axes are not crossed in full.  Every test runs all four partitions; test_layouts_and_models crosses form x dtype x
# layout x interpolation at the ragged shape; test_chains chain x layout x dtype for the ingest form, the data-dependent
# chains with per-batch constants included; test_shapes the frame shapes and LUT sizes x layout x form; test_row_band the tile
# geometry.  Odd positions: one batch of the call is only element-aligned (the code form then takes the element-wise walk for
# all of them).
@pytest.mark.parametrize("form,dtype", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("layout,channels", LAYOUTS, ids=[f"{l}{c}" for l, c in LAYOUTS])
@pytest.mark.parametrize("interp", INTERPS, ids=[str(i) for i in INTERPS])
def test_layouts_and_models(dev, form, dtype, layout, channels, interp):
    rng = np.random.default_rng(3)
    stages = _chains(dtype, channels)["clamp"] if form == "ingest" else None
    for n, partition in enumerate(PARTITIONS):
        host = _source(_draw(rng, (sum(partition), channels, 5, 7), dtype), layout)
        _run(dev, form, host, layout, partition, _lut(channels, 16), interp, stages=stages, odd=(1,) if n % 2 else ())


@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("chain", ["black", "clamp", "range", "four", "empty", "data", "data_clamp"])
@pytest.mark.parametrize("layout,channels", LAYOUTS, ids=[f"{l}{c}" for l, c in LAYOUTS])
def test_chains(dev, dtype, chain, layout, channels):
    rng = np.random.default_rng(5)
    data = chain.startswith("data")
    if chain == "data":
        stages = [("affine_data", 1.0, 0.0)]
    elif chain == "data_clamp":  # a constant stage in front of the data-dependent one, a per-channel clamp behind it
        stages = [_chains(dtype, channels)["black"][0], ("affine_data", 1.0, 0.0), ("clamp", PAIRS[channels])]
    else:
        stages = _chains(dtype, channels)[chain]
    for partition in PARTITIONS:
        host = _source(_draw(rng, (sum(partition), channels, 5, 7), dtype, small=chain == "empty"), layout)
        for interp in ("linear", None):
            _run(dev, "ingest", host, layout, partition, _lut(channels, 256), interp, stages=stages, data=data,
                 odd=(0, 2) if chain in ("black", "data") else ())


@pytest.mark.parametrize("form", ["code", "ingest"])
@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("layout,channels", LAYOUTS, ids=[f"{l}{c}" for l, c in LAYOUTS])
@pytest.mark.parametrize("points", [16, 256])
def test_shapes(dev, form, hw, layout, channels, points):
    rng = np.random.default_rng(7)
    for dtype in (torch.uint8, torch.uint16) + ((torch.float32,) if form == "code" else ()):
        for data in (False, True) if form == "ingest" else (False,):
            stages = None if form == "code" else ([("affine_data", 2.0, -0.5)] if data else _chains(dtype, channels)["range"])
            for partition in PARTITIONS:
                host = _source(_draw(rng, (sum(partition), channels) + hw, dtype), layout)
                for interp in ("catmull", "lookup"):
                    _run(dev, form, host, layout, partition, _lut(channels, points), interp, stages=stages, data=data)


@pytest.mark.parametrize("form,dtype", FORMS, ids=FORM_IDS)
def test_consecutive_calls(dev, form, dtype):
    """[3, 2] then [4, 1] with the frame count carried along, against five single calls: the second call reads the state."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(11)
    for layout, channels in LAYOUTS:
        host = _source(_draw(rng, (10, channels, 5, 7), dtype), layout)
        stages = _chains(dtype, channels)["clamp"] if form == "ingest" else None
        chw = ops.ingest_shape(tuple(host.shape), layout)[1:]
        states = [torch.full(chw, SENTINEL, dtype=torch.float32, device=dev) for _ in range(4)]
        _run(dev, form, host[:5], layout, [3, 2], _lut(channels, 16), "linear", stages=stages, states=states)
        _run(dev, form, host[5:], layout, [4, 1], _lut(channels, 16), "linear", stages=stages, states=states, frames_before=5)
        # ... and a call that starts from a state it has not written itself
        _run(dev, form, host, layout, [2, 5, 3], _lut(channels, 16), "catmull", stages=stages, frames_before=7)


@pytest.mark.parametrize("form,dtype", FORMS, ids=FORM_IDS)
def test_fallback_and_its_refusal(dev, form, dtype):
    """A batch of 33 frames has no register-cached walk: one launch per batch, the same bits; refused where one launch is
    required.  So are, for the ingest form, batches with and without constants."""
    from clair_torch_amd import _native as nv
    rng = np.random.default_rng(13)
    host = _draw(rng, (35, 3, 5, 7), dtype)
    stages = _chains(dtype, 3)["clamp"] if form == "ingest" else None
    _run(dev, form, host, "nchw", [33, 2], _lut(3, 16), "linear", stages=stages, one_launch=False)
    with pytest.raises(nv.NativeLibraryError, match="_batches"):
        _run(dev, form, host, "nchw", [33, 2], _lut(3, 16), "linear", stages=stages, one_launch=True)
    if form == "ingest":
        from clair_torch_amd import ops
        parts = [host[:3].to(dev), host[3:5].to(dev)]
        consts = [ops.ingest_extrema(parts[0], (), "nchw"), None]
        states = [torch.full((3, 5, 7), SENTINEL, dtype=torch.float32, device=dev) for _ in range(4)]
        for k, x in zip((0, 3), parts):
            ops.video_stats_ingest_batch(x, stages, states[2], states[3], k)
        ops.video_stats_ingest_batches(parts, stages, states[0], states[1], 0, consts=consts)
        assert torch.equal(states[0], states[2]) and torch.equal(states[1], states[3])
        with pytest.raises(nv.NativeLibraryError, match="_batches"):
            ops.video_stats_ingest_batches(parts, stages, states[0], states[1], 0, consts=consts, require_one_launch=True)


@pytest.mark.parametrize("form,dtype", FORMS, ids=FORM_IDS)
def test_one_batch_with_frames_is_never_refused(dev, form, dtype):
    """A single batch with frames among empty ones is one launch of the single-batch kernels, so requiring one launch refuses
    nothing -- not even 33 frames, which no several-batches kernel takes.  (Only a launch tells the two apart: every status
    without one is the same.)"""
    rng = np.random.default_rng(17)
    host = _draw(rng, (33, 3, 5, 7), dtype)
    stages = _chains(dtype, 3)["clamp"] if form == "ingest" else None
    for partition in ([0, 5, 0], [0, 33]):
        _run(dev, form, host[:sum(partition)], "nchw", partition, _lut(3, 16), "linear", stages=stages, one_launch=True)
        _run(dev, form, host[:sum(partition)], "nchw", partition, _lut(3, 16), "linear", stages=stages, one_launch=True, frames_before=6)


@pytest.mark.parametrize("form,dtype", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "nhwc_bgr"])
def test_row_band(dev, form, dtype, layout):
    """Rows [2, 7) of a 9-row image: the LINEAR row follows the GLOBAL flat index (h_global > h_tile, row_offset > 0), as in
    one launch per batch and as in the whole image's statistics; with the band's own indices the result differs."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(9)
    partition = [4, 17, 3]
    whole = _draw(rng, (sum(partition), 3, 9, 7), dtype)
    stages = _chains(dtype, 3)["clamp"] if form == "ingest" else None
    lut = _lut(3, 16)
    band = _source(whole[:, :, 2:7].contiguous(), layout)
    mean_b, m2_b = _run(dev, form, band, layout, partition, lut, "linear", stages=stages, tile=ops.TileGeometry(h_global=9, row_offset=2))
    mean_w, m2_w = _run(dev, form, _source(whole, layout), layout, partition, lut, "linear", stages=stages)
    assert torch.equal(mean_b, mean_w[:, 2:7]) and torch.equal(m2_b, m2_w[:, 2:7])
    mean_l, _ = _run(dev, form, band, layout, partition, lut, "linear", stages=stages)
    assert not torch.equal(mean_l, mean_b)


# ---- B. the reference's arithmetic through the public interface ---------------------------------------------------------------
def _loader(frames, batch_sampler):
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate

    class Frames(StackDataset):  # raw frames of any layout (StackDataset itself insists on (N,C,H,W))
        def __init__(self):
            self.values, self.stds, self.exposure_times = frames, None, [1.0] * len(frames)
            self.files = list(range(len(frames)))
            self.missing_std_mode, self.materialize_std, self.std_hint = MissingStdMode.NONE, False, None

        def __len__(self):
            return len(self.exposure_times)

    ds = StackDataset(frames, [1.0] * len(frames)) if frames.shape[1] == 3 and frames.shape[-1] != 3 else Frames()
    return DataLoader(ds, batch_sampler=batch_sampler, collate_fn=custom_collate)


@pytest.fixture(scope="module")
def video():
    """The 12 uint16 frames 3x9x14 of tests/test_gpu_video_ingest.py: a black level of 64 and a white level of 1023 (959
    codes).  Every pixel has its own level and its frames lie in [level, level + 240]; the first frame of a pixel is its level
    and the second level + 240.  The clamp of test_public_interface cuts channel c at the code T_c (1023, 735, 383); the levels
    of that channel end at T_c - 160, so the brightest pixels saturate in some of their frames and none in its first one:
    every expected std is above 0.  That, and the share of saturated samples, are asserted there on the CPU."""
    rng = np.random.default_rng(21)
    level = np.stack([rng.integers(64, t - 160 + 1, size=(9, 14)) for t in (1023, 735, 383)])[None]
    offset = rng.integers(0, 241, size=(12, 3, 9, 14))
    offset[0], offset[1] = 0, 240
    return torch.from_numpy((level + offset).astype(np.uint16))


_EXPECTED = {}


def _expected(video, bs, chain):
    """The reference's result for one partition and chain, computed once: the classes' own __call__ on the CPU, batch by
    batch (a data-dependent Normalize sees one batch), then the eager reference with the same partition."""
    if (bs, chain) in _EXPECTED:
        return _EXPECTED[(bs, chain)]
    T = _T()
    from oracle import eager_torch as oe
    pairs = [(0.0, 1.0), (0.0, 0.7), (0.0, 0.3333)]
    tail = [T.CastTo("float32"), T.Normalize(1023, 64), T.ClampAlongDims(1, pairs)] if chain == "clamp" else \
        [T.CastTo("float32"), T.Normalize()]
    sampler = [list(range(k, min(k + bs, 12))) for k in range(0, 12, bs)]   # 4 4 4 / 5 5 2
    staged = []
    for idx in sampler:
        x = video[idx].to(torch.int32)   # (== CvToTorch of the raw frames; torch has few uint16 CPU kernels)
        for t in tail:
            x = t(x)
        staged.append(x)
    x = torch.cat(staged)
    assert x.dtype == torch.float32
    lut = _lut(3, 256)
    mean_o, std_o = oe.video_mean_std(x, lut, "linear", [len(i) for i in sampler])
    if chain == "clamp":   # the input conditions, on the CPU and with the reference alone
        hit = torch.zeros_like(x, dtype=torch.bool)
        for c, (lo, hi) in enumerate(pairs):
            hit[:, c] = (x[:, c] <= lo) | (x[:, c] >= hi)
        assert 0 < int(hit.sum()) < 0.10 * hit.numel() and not bool(hit.all(dim=0).any())
    assert bool((std_o > 0).all())
    _EXPECTED[(bs, chain)] = (tail, sampler, lut, mean_o, std_o)
    return _EXPECTED[(bs, chain)]


@pytest.mark.parametrize("per_launch", [3, 16])
@pytest.mark.parametrize("bs", [4, 5])
@pytest.mark.parametrize("raw", [False, True], ids=["planar", "cv"])
@pytest.mark.parametrize("chain", ["clamp", "data"])
def test_public_interface(dev, video, per_launch, bs, raw, chain):
    T = _T()
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.inference import compute_video_mean_and_std
    from clair_torch_amd.models import ICRFModelDirect
    tail, sampler, lut, mean_o, std_o = _expected(video, bs, chain)
    transforms = ([T.CvToTorch()] if raw else []) + tail
    frames = _source(video, "nhwc_bgr") if raw else video
    model = ICRFModelDirect(icrf=lut.clone(), interpolation_mode=InterpMode.LINEAR).to(dev)
    mean, std = compute_video_mean_and_std(_loader(frames, sampler), "cuda", model, gpu_transforms=transforms,
                                           batches_per_launch=per_launch)
    assert mean.dtype == torch.float32 and std.dtype == torch.float32 and tuple(mean.shape) == (3, 9, 14)
    assert_parity(mean.cpu().numpy(), mean_o.numpy(), rtol=1e-6, norm_tol=1e-7, what="video batches mean")
    assert_parity(std.cpu().numpy(), std_o.numpy(), rtol=1e-4, norm_tol=1e-6, what="video batches std")
    mean_1, std_1 = compute_video_mean_and_std(_loader(frames, sampler), "cuda", model, gpu_transforms=transforms, batches_per_launch=1)
    assert torch.equal(mean, mean_1) and torch.equal(std, std_1)
    mean_u, std_u = compute_video_mean_and_std(_loader(frames, sampler), "cuda", model, gpu_transforms=transforms, fused_ingest=False,
                                               batches_per_launch=per_launch)
    assert torch.equal(mean, mean_u) and torch.equal(std, std_u)


def test_public_interface_takes_the_grouped_routes(dev, video, monkeypatch):
    T = _T()
    from clair_torch_amd import ops
    from clair_torch_amd.inference import compute_video_mean_and_std
    seen = []
    for name in ("video_stats_ingest_batch", "video_stats_batch", "ingest_transform", "video_stats_ingest_batches", "video_stats_batches"):
        def spy(*a, _f=getattr(ops, name), _n=name, **kw):
            seen.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    sampler = [[0, 1, 2], [3, 4], [5, 6], [7, 8], [9, 10, 11]]
    compute_video_mean_and_std(_loader(video, sampler), "cuda", None, gpu_transforms=[T.CastTo("float32"), T.Normalize(1023, 64)],
                               batches_per_launch=4)
    assert seen == ["video_stats_ingest_batches"] * 2   # a black-level chain: 4 batches, then 1
    del seen[:]
    compute_video_mean_and_std(_loader(video, sampler), "cuda", None, gpu_transforms=[T.CastTo("float32"), T.Normalize(1023, 0)],
                               batches_per_launch=4)
    assert seen == ["video_stats_batches"] * 2          # route "code"


@pytest.mark.parametrize("fused", [True, False])
def test_zero_range_still_raises(dev, fused):
    """A data-dependent Normalize on a constant batch: the reference's ValueError, per batch, while the batch is staged."""
    T = _T()
    from clair_torch_amd.inference import compute_video_mean_and_std
    frames = torch.full((6, 3, 5, 7), 300, dtype=torch.int32)
    frames[:2, :, 0, 0] = 400   # the first batch has a range, the second has none
    frames = frames.to(torch.uint16)
    with pytest.raises(ValueError, match="Normalization range is zero"):
        compute_video_mean_and_std(_loader(frames, [[0, 1], [2, 3], [4, 5]]), "cuda", None,
                                   gpu_transforms=[T.CastTo("float32"), T.Normalize()], fused_ingest=fused, batches_per_launch=4)


# ---- C. nothing outside the state is touched -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["code", "ingest"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
@pytest.mark.parametrize("lead", [(64, 64), (3, 3), (1, 2)], ids=["aligned", "odd", "unequal"])
def test_state_margins_untouched(dev, form, layout, lead):
    """The two state arrays inside larger buffers filled with a sentinel, at equal and at unequal offsets from a 16-byte
    boundary (packets with scalar edges / element by element), Q = 105: whatever surrounds them stays, and so do the frames."""
    rng = np.random.default_rng(13)
    q, pad = 3 * 5 * 7, 64
    bufs = [torch.full((q + 2 * pad + 8,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(2)]
    views = [buf[lo:lo + q].view(3, 5, 7) for buf, lo in zip(bufs, lead)]
    plain = [torch.full((3, 5, 7), SENTINEL, dtype=torch.float32, device=dev) for _ in range(2)]
    stages = _chains(torch.uint16, 3)["clamp"] if form == "ingest" else None
    for partition in PARTITIONS:
        host = _source(_draw(rng, (sum(partition), 3, 5, 7), torch.uint16), layout)
        on_dev = host.view(torch.int16).to(dev)
        frames = on_dev.view(torch.uint16)
        before = on_dev.clone()
        for frames_before in (0, 6):   # a first call, and one that reads the state
            _run_resident(dev, form, frames, layout, partition, stages, views + plain, frames_before)
            assert torch.equal(on_dev, before)
            for buf, lo in zip(bufs, lead):
                assert bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + q:] == SENTINEL).all())


def _run_resident(dev, form, frames, layout, partition, stages, states, frames_before):
    """As _run, on frames that are already on the device (slices of one allocation), so that they can be compared after."""
    from clair_torch_amd import ops
    mean_g, m2_g, mean_s, m2_s = states
    kw = dict(lut=_lut(3, 16).to(dev), interp="linear", layout=layout)
    if form == "code":
        kw["max_code"] = 1023.0
    parts, k = [], 0
    for b in partition:
        parts.append(frames[k:k + b])
        k += b
    before = frames_before
    mean_s.copy_(mean_g), m2_s.copy_(m2_g)
    for x in parts:
        if x.shape[0] == 0:
            continue
        if form == "code":
            ops.video_stats_batch(x, mean_s, m2_s, before, **kw)
        else:
            ops.video_stats_ingest_batch(x, stages, mean_s, m2_s, before, **kw)
        before += x.shape[0]
    if form == "code":
        ops.video_stats_batches(parts, mean_g, m2_g, frames_before, require_one_launch=True, **kw)
    else:
        ops.video_stats_ingest_batches(parts, stages, mean_g, m2_g, frames_before, require_one_launch=True, **kw)
    assert torch.equal(mean_g, mean_s) and torch.equal(m2_g, m2_s)
