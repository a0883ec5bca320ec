"""A data-dependent Normalize (``max_val`` / ``min_val`` None) on the device: ct_ingest_extrema reduces the batch's own
extrema behind the constant prefix, ct_ingest_transform_data evaluates the chain with them
(clair_torch/common/general_functions.py:359-388, transforms.py:108-133).  The specification is the float32 arithmetic of
the project's classes on the CPU (tests/test_ingest_data_host.py pins them to the reference's recorded output), so every
comparison is one of bit patterns, NaN compared as NaN."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from test_gpu_ingest import PAIRS, SHAPES, _bgr_frames, _cpu_chain, _random, _raw_frames_dataset, _rgb_frames, _same_bits, _tensors

pytestmark = pytest.mark.gpu

ZERO = "Normalization range is zero"
CODE_CLAMPS = [(64.0, 4095.0), (100.0, 3000.5), (0.0, 2047.0)]
# (max_val, min_val): the four None / given combinations (both given is the constant chain of ct_ingest_transform)
BOUNDS = {torch.uint8: [(None, None), (None, 3), (251.5, None), (250, 2)],
          torch.uint16: [(None, None), (None, 64), (65000.5, None), (4095, 64)],
          torch.float32: [(None, None), (None, -150.25), (4700.5, None), (4095, 64)]}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _T():
    from clair_torch_amd.common import transforms
    return transforms


def _same(got, want):
    """Bit patterns, NaN compared as NaN (its payload is not specified)."""
    got = got.cpu() if got.is_cuda else got
    if tuple(got.shape) != tuple(want.shape) or got.dtype != torch.float32 or want.dtype != torch.float32:
        return False
    nan = torch.isnan(want)
    zero = torch.zeros_like(want)
    return torch.equal(torch.isnan(got), nan) and _same_bits(torch.where(nan, zero, got), torch.where(nan, zero, want))


def _cpu(host, transforms):
    """The classes on the CPU: the float32 result, or the ValueError they raise."""
    try:
        return _cpu_chain(host, transforms)
    except ValueError as e:
        return e


def _run(dev, host, transforms, layout=None, planar=None, check=True):
    """The recognised list through ``ops``: for ``host`` itself, or, with an explicit ``layout`` the recogniser has no list
    for (RGB frames), for the ``planar`` form of the same stack."""
    from clair_torch_amd import ops
    T = _T()
    probe = host if planar is None else planar
    plan = T.fusable_ingest_data(probe, transforms)
    if plan is None:  # both bounds given: the constant chain
        plan = T.fusable_ingest(probe, transforms)
        assert plan is not None and plan.step == 1
        return ops.ingest_transform(host.to(dev), plan.stages, layout=plan.layout if layout is None else layout)
    assert plan.step == 1 and T.fusable_ingest(probe, transforms) is None
    return ops.ingest_transform_data(host.to(dev), plan.stages, plan.layout if layout is None else layout, plan.min_val,
                                     plan.max_val, check=check)


def _agree(dev, host, transforms, want, layout=None, planar=None):
    if isinstance(want, ValueError):
        with pytest.raises(ValueError, match=ZERO):
            _run(dev, host, transforms, layout, planar)
        return True
    return _same(_run(dev, host, transforms, layout, planar), want)


# ---- shapes, dtypes, layouts, bounds ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.float32])
def test_shapes_layouts_and_bounds(dev, dtype):
    T = _T()
    rng = np.random.default_rng(41)
    cast = T.CastTo("float32")
    shapes = SHAPES + ([(4, 3, 256, 512)] if dtype == torch.uint8 else [])
    for shape in shapes:
        planar = _random(rng, shape, dtype)
        if shape == (1, 1, 1, 1):  # a value no given bound equals
            planar = torch.from_numpy(np.full(shape, 77, dtype=planar.numpy().dtype))
        for mx, mn in BOUNDS[dtype]:
            ts = [cast, T.Normalize(mx, mn, (-1.0, 1.0) if shape[3] % 2 else (0.0, 1.0))]
            want = _cpu(planar, ts)
            if shape == (1, 1, 1, 1):  # its own minimum is its own maximum
                assert isinstance(want, ValueError) == (mx is None and mn is None)
            assert _agree(dev, planar, ts, want), (shape, "nchw", mx, mn)
            if shape[1] == 3:
                assert _agree(dev, _rgb_frames(planar), ts, want, "nhwc", planar), (shape, "nhwc", mx, mn)
                assert _agree(dev, _bgr_frames(planar), ts, want, "nhwc_bgr", planar), (shape, "nhwc_bgr", mx, mn)
                if dtype != torch.float32:  # raw frames through the recogniser
                    assert _agree(dev, _bgr_frames(planar), [T.CvToTorch()] + ts, want), (shape, "CvToTorch", mx, mn)


def test_more_elements_than_one_pass_of_the_grid(dev):
    """The grid-stride loop and the fold: a stack of more 16-byte packets than the workgroups of one launch (one partial
    each in the workspace, 256 threads, 4 packets per thread and trip) cover in one trip, so that some workgroups make a
    second trip and some do not; planar codes reduced as integers, and interleaved frames behind a per-channel clamp
    (6 packets per thread and trip).  The extrema sit where only a second trip reaches them."""
    from clair_torch_amd import _native, ops
    groups = _native.load().ct_ingest_extrema_workspace() // 16
    one_pass = groups * 256 * 6 * 16
    rng = np.random.default_rng(43)
    n_pixels = one_pass // 3 + 300_000
    frames = rng.integers(20, 200, size=(1, n_pixels, 1, 3), dtype=np.uint8)
    assert frames.size > one_pass + 256 * 6 * 16
    flat = frames.reshape(-1)
    flat[one_pass + 12345] = 3       # memory channel 0: plane 2 of the planar result
    flat[flat.size - 2] = 250        # memory channel 1
    x = torch.from_numpy(frames).to(dev)
    got = ops.ingest_extrema(x.view(1, 1, 1, -1), (), "nchw").cpu()
    assert got.tolist() == [3.0, 247.0, 3.0, 250.0]
    pairs = [(30.0, 240.0), (10.0, 249.0), (5.0, 230.0)]  # of planes R, G, B = memory channels 2, 1, 0
    got = ops.ingest_extrema(x, [("clamp", pairs)], "nhwc_bgr", max_val=1000).cpu()
    assert got.tolist() == [5.0, 995.0, 5.0, 249.0]
    got = ops.ingest_extrema(x, [("clamp", pairs)], "nhwc").cpu()
    assert got.tolist() == [20.0, 229.0, 20.0, 249.0]  # the planted 3 is clamped to 30; planes 1 and 2 keep their 20s


# ---- where an element could be skipped -----------------------------------------------------------------------------------
def _interior(dev, host, lead):
    """``host`` on the device as an element-aligned interior slice of a larger buffer (torch's allocations are aligned)."""
    flat = host.reshape(-1)
    pad = torch.zeros(lead + flat.numel() + 19, dtype=host.dtype)
    pad[lead:lead + flat.numel()] = flat
    buf = pad.to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf[lead:lead + flat.numel()].view(host.shape)


@pytest.mark.parametrize("mode", ["codes", "uniform prefix", "planes", "bgr frames", "rgb frames"])
def test_extremum_at_every_kind_of_position(dev, mode):
    from clair_torch_amd import ops
    T = _T()
    rng = np.random.default_rng(47)
    shape, dtype, lead = (2, 3, 37, 53), torch.uint16, 3   # 11 766 elements, 5 of them in front of the first packet
    n = int(np.prod(shape))
    head = (16 - 2 * lead) // 2
    base = rng.integers(1000, 4000, size=shape).astype(np.uint16)
    prefix_ts = {"codes": [], "uniform prefix": [T.Normalize(4095, 64)]}.get(mode, [T.ClampAlongDims(1, [(9.0, 59990.0), (8.0, 59995.0), (0.0, 60030.0)])])  # what is planted depends on its channel
    layout = {"bgr frames": "nhwc_bgr", "rgb frames": "nhwc"}.get(mode, "nchw")
    prefix = T.fusable_ingest(torch.zeros(shape, dtype=torch.float32), prefix_ts).stages if prefix_ts else ()
    # first, last, around the first packet boundary, the ragged tail, the last workgroup's span, and three consecutive
    # elements (every memory channel of an interleaved pixel) in the middle and at both ends
    unit = 8 * (3 if "frames" in mode else 1)
    rest0 = head + (n - head) // unit * unit
    spots = sorted({0, 1, 2, head - 1, head, head + 1, head + 7, head + 8, n - 1, n - 2, n - 3, rest0 - 1, rest0, min(rest0 + 1, n - 1),
                    n - 300, n - 2048, n - 4097, n // 2, n // 2 + 1, n // 2 + 2, 37 * 53 - 1, 37 * 53, 3 * 37 * 53, 3 * 37 * 53 + 1})
    for k, lo_at in enumerate(spots):
        hi_at = spots[(k + 5) % len(spots)]
        planar = base.copy()
        host = planar if layout == "nchw" else np.ascontiguousarray(planar.transpose(0, 2, 3, 1)[..., ::-1] if layout == "nhwc_bgr" else planar.transpose(0, 2, 3, 1))
        host.reshape(-1)[lo_at] = 7          # in memory order: the kernel's own indexing
        host.reshape(-1)[hi_at] = 60000
        if layout != "nchw":
            planar = host[..., ::-1].transpose(0, 3, 1, 2) if layout == "nhwc_bgr" else host.transpose(0, 3, 1, 2)
        x = _cpu_chain(torch.from_numpy(np.ascontiguousarray(planar)), [T.CastTo("float32")] + prefix_ts)
        lo, hi = x.min(), x.max()
        want = torch.stack([lo, hi - lo, lo, hi])
        src = _interior(dev, torch.from_numpy(host), lead)
        got = ops.ingest_extrema(src, prefix, layout)
        assert _same_bits(got, want), (mode, lo_at, hi_at, got.tolist(), want.tolist())
        if k % 6 == 0:  # ... and the whole chain from the unaligned source, one bound given
            ts = [T.CastTo("float32")] + prefix_ts + [T.Normalize(None, 0.5, (-1.0, 1.0))]
            stages = tuple(prefix) + (("affine_data", 2.0, -1.0),)
            out = ops.ingest_transform_data(src, stages, layout, min_val=0.5)
            assert _same(out, _cpu_chain(torch.from_numpy(np.ascontiguousarray(planar)), ts)), (mode, lo_at)


# ---- prefix, suffix, stage count ------------------------------------------------------------------------------------------
def _staged(dev, host, transforms, planar=False):
    from clair_torch_amd.inference._staging import stage_images
    out = stage_images(host, dev, transforms, planar=planar)
    assert out[1] is None and out[0].dtype == torch.float32 and out[0].is_contiguous() and out[0].is_cuda
    assert out[2] == "nchw"
    return out[0]


def test_prefix_suffix_and_stage_count(dev):
    T = _T()
    rng = np.random.default_rng(53)
    planar = _random(rng, (2, 3, 9, 21), torch.uint16, top=5000)
    raw = _bgr_frames(planar)
    cast, cv, n1, free = T.CastTo("float32"), T.CvToTorch(), T.Normalize(4095, 64), T.Normalize()
    code_clamp, clamp = T.ClampAlongDims(1, CODE_CLAMPS), T.ClampAlongDims(1, PAIRS[3])
    lists = [[cast, n1, free],                                  # a constant Normalize in front
             [cast, code_clamp, free],                          # a per-channel clamp in front
             [cast, free, clamp],                               # a clamp behind
             [cast, code_clamp, n1, T.Normalize(None, 0.25, (-1.0, 1.0)), clamp],   # four stages
             [cast, n1, T.ClampAlongDims(0, (0.1, 0.8)), clamp, T.Normalize(0.75, None)]]
    for k, ts in enumerate(lists):
        assert T.fusable_ingest_data(planar, ts) is not None and T.fusable_ingest_data(raw, [cv] + ts).layout == "nhwc_bgr"
        want = _cpu_chain(planar, ts)
        assert _same(_staged(dev, planar, ts), want), (k, "planar")
        assert _same(_staged(dev, planar, ts, planar=True), want), (k, "planar, planar=True")
        assert _same(_staged(dev, raw, [cv] + ts), want), (k, "raw")
        assert _same(_staged(dev, raw, [cv] + ts, planar=True), want), (k, "raw, planar=True")
        assert _same(_run(dev, _rgb_frames(planar), ts, "nhwc", planar), want), (k, "nhwc")
    # five stages: the torch route, as before.  No bit-exactness is promised there: the extrema are exact, each of the 12
    # elementwise float32 operations is within 1 ulp (6e-8 of a magnitude below 8) of the CPU's, and the one stage behind
    # the first two normalisations that amplifies does so by 2.5
    n2 = T.Normalize(0.9, 0.1, (-1.0, 1.0))
    five = [cast, code_clamp, n1, free, clamp, n2]
    assert T.fusable_ingest_data(planar, five) is None and T.fusable_ingest(planar, five) is None
    assert torch.allclose(_staged(dev, planar, five).cpu(), _cpu_chain(planar, five), rtol=0, atol=12 * 8 * 6e-8 * 2.5)
    # two data-dependent stages decline as well
    two = [cast, free, T.Normalize(None, 0, (0.0, 2.0))]
    assert T.fusable_ingest_data(planar, two) is None
    assert torch.allclose(_staged(dev, planar, two).cpu(), _cpu_chain(planar, two), rtol=0, atol=8 * 8 * 6e-8 * 2.0)


# ---- the downscale on either side ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3])
def test_downscale_in_front_of_and_behind_the_normalize(dev, s):
    T = _T()
    from clair_torch_amd.inference._staging import stage_images
    rng = np.random.default_rng(59 + s)
    planar = _random(rng, (3, 3, 18, 34), torch.uint16, top=5000)
    flat = planar.view(torch.int16)
    flat[1, 2, 1, 1] = 30000  # the full-resolution maximum, on a pixel every stride skips
    flat[2, 0, 7, 5] = 0      # ... and the minimum (row 7, column 5: skipped by 2 and by 3)
    raw = _bgr_frames(planar)
    cast, free, clamp, sd, cv = T.CastTo("float32"), T.Normalize(), T.ClampAlongDims(1, PAIRS[3]), T.StridedDownscale(s), T.CvToTorch()
    first = _cpu_chain(planar, [sd, cast, free, clamp])
    behind = _cpu_chain(planar, [cast, free, clamp, sd])
    assert not torch.equal(first, behind), "the two orders must differ for this stack"
    cases = [([sd, cast, free, clamp], True, first), ([cast, sd, free, clamp], True, first),
             ([cast, free, sd, clamp], False, behind), ([cast, free, clamp, sd], False, behind)]
    for k, (ts, step_first, want) in enumerate(cases):
        plan = T.fusable_ingest_data(planar, ts)
        assert plan.step == s and plan.step_first == step_first and T.fusable_ingest_data(raw, [cv] + ts).layout == "nhwc_bgr"
        assert _same_bits(_cpu_chain(planar, ts), want)
        assert _same(_staged(dev, planar, ts), want), (k, "planar")
        assert _same(_staged(dev, raw, [cv] + ts), want), (k, "raw")
        assert _same(_staged(dev, raw, [cv] + ts, planar=True), want), (k, "raw, planar=True")
        again, max_code, layout = stage_images(raw, dev, [cv] + ts, planar=True)
        assert max_code is None and layout == "nchw" and _same(again, want), (k, "restaged")


# ---- special values, the zero range -----------------------------------------------------------------------------------
def test_nan_infinities_and_the_zero_range(dev):
    from clair_torch_amd import ops
    from clair_torch_amd.inference._staging import stage_images
    T = _T()
    rng = np.random.default_rng(61)
    cast, free = T.CastTo("float32"), T.Normalize()
    base = _random(rng, (2, 3, 7, 23), torch.float32)
    for at in (0, 5, 500, base.numel() - 1):
        x = base.clone()
        x.view(-1)[at] = float("nan")
        for ts in ([free], [T.Normalize(None, 0)], [T.Normalize(4095, None)], [T.Normalize(4095, 64), free, T.ClampAlongDims(1, PAIRS[3])]):
            want = _cpu_chain(x, ts)
            assert bool(torch.isnan(want).all())
            for layout, host in (("nchw", x), ("nhwc", _rgb_frames(x)), ("nhwc_bgr", _bgr_frames(x))):
                got = _run(dev, host, ts, layout, x)   # check=True: nothing is raised
                assert _same(got, want), (at, layout)
        consts = ops.ingest_extrema(x.to(dev)).cpu()
        assert bool(torch.isnan(consts).all())
    for value, ts in ((float("inf"), [free]), (float("-inf"), [free]), (float("inf"), [T.Normalize(None, 0)]),
                      (float("-inf"), [T.Normalize(4095, None, (-1.0, 1.0))]), (float("inf"), [T.Normalize(4095, None)])):
        x = base.clone()
        x.view(-1)[77] = value
        want = _cpu_chain(x, ts)
        assert _same(_run(dev, x, ts), want), (value, "nchw")
        assert _same(_run(dev, _bgr_frames(x), ts, "nhwc_bgr", x), want), (value, "nhwc_bgr")
    # a constant stack: the reference's message, through stage_images and through ops
    for dtype, fill in ((torch.uint8, 9), (torch.uint16, 4095), (torch.float32, 0.375)):
        const = torch.full((2, 3, 5, 7), fill, dtype=torch.float32).to(dtype) if dtype != torch.uint16 else \
            torch.from_numpy(np.full((2, 3, 5, 7), fill, dtype=np.uint16))
        with pytest.raises(ValueError, match=ZERO):
            _cpu_chain(const, [cast, free])
        with pytest.raises(ValueError, match=ZERO):
            stage_images(const, dev, [cast, free])
        with pytest.raises(ValueError, match=ZERO):
            stage_images(const, dev, [cast, T.Normalize(fill, None)], planar=True)
        with pytest.raises(ValueError, match=ZERO):
            ops.ingest_transform_data(const.to(dev), [("affine_data", 1.0, 0.0)], check=True)
        out, consts = ops.ingest_transform_data(const.to(dev), [("affine_data", 1.0, 0.0)], check=False)
        assert consts.cpu().tolist() == [float(fill), 0.0, float(fill), float(fill)]
        assert bool(torch.isnan(out).all())  # 0 / 0
    with pytest.raises(RuntimeError):
        ops.ingest_extrema(torch.zeros((0, 3, 4, 4), device=dev))
    with pytest.raises(ValueError):
        ops.ingest_extrema(base.to(dev), min_val=0.0, max_val=1.0)  # nothing depends on the data
    with pytest.raises(ValueError):
        ops.ingest_extrema(base.to(dev), [("affine", 0.0, 1.0, 1.0, 0.0)] * 4)  # at most three stages in front
    with pytest.raises(ValueError):
        ops.ingest_transform(base.to(dev), [("affine_data", 1.0, 0.0)])  # no constants
    with pytest.raises(ValueError):
        ops.ingest_transform(base.to(dev), [("affine_data", 1.0, 0.0)], consts=torch.zeros(3, device=dev))


def test_two_runs_give_identical_bits(dev):
    from clair_torch_amd import ops
    rng = np.random.default_rng(67)
    x = _random(rng, (4, 3, 96, 128), torch.float32).to(dev)
    stages = [("affine", 64, 4031, 1.0, 0.0), ("affine_data", 2.0, -1.0)]
    a, ca = ops.ingest_transform_data(x, stages, check=False)
    b, cb = ops.ingest_transform_data(x, stages, check=False)
    assert _same_bits(ca, cb.cpu()) and _same_bits(a, b.cpu())


# ---- graph capture -------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_with_new_data(dev):
    from clair_torch_amd import ops
    T = _T()
    rng = np.random.default_rng(71)
    first = _random(rng, (2, 3, 17, 33), torch.uint16, top=5000)
    second = torch.from_numpy((rng.integers(20000, 60000, size=(2, 17, 33, 3))).astype(np.uint16))  # BGR frames, another range
    static = _bgr_frames(first).to(dev)
    stages = [("affine_data", 2.0, -1.0), ("clamp", PAIRS[3])]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        ops.ingest_transform_data(static, stages, "nhwc_bgr", check=False)  # warm-up on the capture stream
    side.synchronize()
    with torch.cuda.graph(graph, stream=side):  # extrema, fold, ingest: one linear chain on one stream
        out, consts = ops.ingest_transform_data(static, stages, "nhwc_bgr", check=False)
    static.view(torch.int16).copy_(second.to(dev).view(torch.int16))
    graph.replay()
    torch.cuda.synchronize()
    eager, eager_consts = ops.ingest_transform_data(second.to(dev), stages, "nhwc_bgr", check=False)
    assert _same_bits(consts, eager_consts.cpu()) and _same_bits(out, eager.cpu())
    planar = torch.from_numpy(np.ascontiguousarray(second.numpy()[..., ::-1].transpose(0, 3, 1, 2)))
    assert _same_bits(out, _cpu_chain(planar, [T.CastTo("float32"), T.Normalize(None, None, (-1.0, 1.0)), T.ClampAlongDims(1, PAIRS[3])]))


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_entry_points_equal_the_cpu_staged_float_stack(dev):
    T = _T()
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image, linearize_dataset_generator
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    rng = np.random.default_rng(73)
    codes = _random(rng, (4, 3, 16, 24), torch.uint16, top=4500)
    t = [0.002 * 2.0 ** k for k in range(4)]
    model = ICRFModelDirect(icrf=torch.stack([torch.linspace(0, 1, 256) ** p for p in (2.2, 2.4, 2.6)]),
                            interpolation_mode=InterpMode.LINEAR).to(dev)
    std = dict(missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)

    def merge(dataset, transforms):
        return compute_hdr_image(DataLoader(dataset, batch_size=2, collate_fn=custom_collate), "cuda", model,
                                 weight_fn=gaussian_value_weights, gpu_transforms=transforms)

    def linearize(dataset, transforms):  # (linearization takes batch_size 1 only, as in the reference)
        loader = DataLoader(dataset, batch_size=1, collate_fn=custom_collate)
        return list(linearize_dataset_generator(loader, "cuda", model, gpu_transforms=transforms))

    def same_items(got, want):
        assert len(got) == len(want) >= 2
        for a, b in zip(got, want):
            ta, tb = _tensors(a), _tensors(b)
            assert len(ta) == len(tb) >= 2 and all(torch.equal(x, y) for x, y in zip(ta, tb))

    for ts, raw in (([T.CastTo("float32"), T.Normalize()], False), ([T.CvToTorch(), T.CastTo("float32"), T.Normalize(None, 0)], True)):
        tail = ts[1:] if raw else ts
        # every batch of two exposures normalises by its own extrema
        pixels = torch.cat([_cpu_chain(codes[0:2], tail), _cpu_chain(codes[2:4], tail)])
        source = _raw_frames_dataset(_bgr_frames(codes), t, ("multiplier", 0.05)) if raw else StackDataset(codes, t, **std)
        want = merge(StackDataset(pixels, t, **std), None)
        got = merge(source, ts)
        assert want[1] is not None and tuple(got[0].shape) == (3, 16, 24)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        frames = torch.cat([_cpu_chain(codes[k:k + 1], tail) for k in range(4)])  # ... and every frame by its own
        same_items(linearize(source, ts), linearize(StackDataset(frames, t, **std), None))


def test_custom_op_equals_ops(dev):
    from clair_torch_amd import ops, torch_ops
    rng = np.random.default_rng(79)
    planar = _random(rng, (2, 3, 6, 10), torch.uint16, top=5000)
    x, frames = planar.to(dev), _bgr_frames(planar).to(dev)
    prefix = [("clamp", CODE_CLAMPS), ("affine", 64, 4031, 1.0, 0.0)]
    flat = torch_ops.flatten_ingest_stages(prefix, 3)
    for mn, mx in ((None, None), (0.25, None), (None, 0.75)):
        want = ops.ingest_extrema(x, prefix, "nchw", mn, mx).cpu()
        assert _same_bits(torch.ops.clair_hip.ingest_extrema(x, flat, "nchw", mn, mx), want)
        assert _same_bits(torch.ops.clair_hip.ingest_extrema(frames, flat, "nhwc_bgr", mn, mx), want)
        assert _same_bits(ops.ingest_extrema(frames, prefix, "nhwc_bgr", mn, mx), want)
    assert _same_bits(torch.ops.clair_hip.ingest_extrema(x, [], "nchw"), ops.ingest_extrema(x).cpu())
    lo, hi = planar.to(torch.float32).min(), planar.to(torch.float32).max()
    assert _same_bits(ops.ingest_extrema(x), torch.stack([lo, hi - lo, lo, hi]))
