"""Device-side image export (clair_torch/common/data_io.py:228-234): ct_export_cv casts a planar result to the file's
dtype, interleaves it to (H, W, C) and reverses a 3-channel image to BGR.  A cast is defined bit for bit (IEEE round to
nearest even, as numpy's astype) and the rest is a permutation, so every comparison here is exact: the kernel against
the numpy expression, and the entry points' "cv" results against their own "planar" results permuted and flipped."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

_T = {"f32": torch.float32, "f64": torch.float64}
_N = {"f32": np.float32, "f64": np.float64}
_I = {np.dtype("float32"): np.uint32, np.dtype("float64"): np.uint64}

# (F, H, W): less than one packet; plane * C odd for C = 1, 3 (second image misaligned); heads and tails; whole packets
# only; one long odd row
_SHAPES = [(1, 1, 1), (1, 1, 3), (2, 3, 5), (3, 37, 53), (2, 16, 64), (1, 9, 131)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _data(rng, shape, dtype):
    """Normal deviates over many decades with planted specials; returns (array, flat index of the one NaN)."""
    n = int(np.prod(shape))
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-44, 39, size=n)
    specials = [0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1e-46, -1e-46, 3.5e38, -3.5e38, 1.0 + 2.0 ** -24,
                1.0 + 3.0 * 2.0 ** -24, -(1.0 + 2.0 ** -24), np.nan]
    where = rng.permutation(n)[:len(specials)]  # fewer positions than specials on the tiny shapes: the first ones win
    a[where] = specials[:len(where)]
    with np.errstate(over="ignore"):
        a = a.astype(dtype)
    nan = np.flatnonzero(np.isnan(a))
    assert len(nan) <= 1
    return a.reshape(shape), nan


def _reference(a, dt):
    """The array save_image writes (data_io.py:228-234), for one image or a stack of them."""
    with np.errstate(over="ignore"):
        b = a.astype(dt)
    if a.ndim == 2:
        return b
    b = np.moveaxis(b, -3, -1)
    return np.ascontiguousarray(b[..., ::-1] if a.shape[-3] == 3 else b)


def _assert_same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    gi, wi = got.view(_I[got.dtype]), want.view(_I[want.dtype])
    assert np.array_equal(gi[~nan], wi[~nan]), what


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("dst", ["f32", "f64"])
@pytest.mark.parametrize("src", ["f32", "f64"])
def test_kernel_equals_numpy_bit_for_bit(dev, src, dst, c):
    from clair_torch_amd import ops
    rng = np.random.default_rng(1000 * c + 10 * (src == "f64") + (dst == "f64"))
    cases = [(f, c, h, w) for f, h, w in _SHAPES] + [(c, 37, 53), (c, 2, 3), (37, 53), (1, 3)]
    for shape in cases:
        a, _ = _data(rng, shape, _N[src])
        want = _reference(a, _N[dst])
        x = torch.from_numpy(a).to(dev)
        got = ops.export_cv(x, _T[dst])
        assert got.dtype == _T[dst] and got.is_contiguous() and got.device == x.device, shape
        _assert_same_bits(got.cpu().numpy(), want, shape)
        assert np.array_equal(x.cpu().numpy().view(_I[a.dtype]), a.view(_I[a.dtype])), "the source was written to"
        if src == dst:
            keep = ops.export_cv(x)  # dtype=None keeps the input's
            assert keep.dtype == x.dtype and torch.equal(keep.view(torch.int64 if src == "f64" else torch.int32),
                                                         got.view(torch.int64 if src == "f64" else torch.int32))


def test_float64_to_float32_special_values(dev):
    """The cast alone, on values whose float32 image is a subnormal, a zero, an infinity or a tie."""
    from clair_torch_amd import ops
    v = np.array([1e-40, -1e-40, 1e-46, -1e-46, 3.5e38, -3.5e38, 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, 0.0, -0.0,
                  np.inf, -np.inf, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -150, 3.4028235677973366e38], dtype=np.float64)
    with np.errstate(over="ignore"):
        want = v.astype(np.float32)
    assert want[0] != 0 and want[2] == 0 and np.signbit(want[3]) and np.isinf(want[4]) and want[6] == 1.0
    assert want[7] == np.float32(1.0 + 2.0 ** -22) and want[13] == 0 and want[14] == np.float32(2.0 ** -149)
    for shape in [(1, 16), (4, 4), (1, 4, 4)]:  # one channel: the plain cast
        got = ops.export_cv(torch.from_numpy(v.reshape(shape)).to(dev), torch.float32).cpu().numpy()
        assert np.array_equal(got.view(np.uint32).ravel(), want.view(np.uint32)), shape
    # as the three planes of a (3, 4, 4) image: the regrouping route; and of a (2, 4, 4) image: the generic route
    for c in (3, 2):
        a = np.stack([np.roll(v, k) for k in range(c)]).reshape(c, 4, 4)
        got = ops.export_cv(torch.from_numpy(a).to(dev), torch.float32).cpu().numpy()
        _assert_same_bits(got, _reference(a, np.float32), c)


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("dst", ["f32", "f64"])
@pytest.mark.parametrize("src", ["f32", "f64"])
def test_bounds_with_misaligned_source_and_destination(dev, src, dst, c):
    from clair_torch_amd import ops
    rng = np.random.default_rng(7 + c)
    lead, trail, sentinel = 5, 37, -7.25
    for f, h, w in [(2, 3, 5), (3, 37, 53), (2, 16, 64)]:
        a = rng.standard_normal((f, c, h, w)).astype(_N[src])
        want = _reference(a, _N[dst])
        n = a.size
        # the source: a view starting at element 1 of a larger buffer (not 16-byte aligned)
        src_buf = torch.zeros(n + 3, dtype=_T[src], device=dev)
        src_buf[1:1 + n] = torch.from_numpy(a).reshape(-1).to(dev)
        x = src_buf[1:1 + n].view(f, c, h, w)
        assert x.data_ptr() % 16 != 0 and x.is_contiguous()
        _assert_same_bits(ops.export_cv(x, _T[dst]).cpu().numpy(), want, (f, h, w))
        # the destination: an interior slice of a sentinel-filled buffer; nothing outside the slice may change
        buf = torch.full((lead + n + trail,), sentinel, dtype=_T[dst], device=dev)
        out = buf[lead:lead + n].view(want.shape)
        assert out.data_ptr() % 16 != 0
        assert ops.export_cv(x, _T[dst], out=out) is out
        flat = buf.cpu().numpy()
        _assert_same_bits(flat[lead:lead + n].reshape(want.shape), want, (f, h, w))
        assert (flat[:lead] == sentinel).all() and (flat[lead + n:] == sentinel).all(), (f, h, w)


def test_front_end_checks(dev):
    from clair_torch_amd import ops, torch_ops  # noqa: F401 (torch_ops registers torch.ops.clair_hip.*)
    x = torch.randn(2, 3, 6, 10, device=dev)
    want = x.permute(0, 2, 3, 1).flip(-1)
    assert torch.equal(ops.export_cv(x), want)
    assert torch.equal(torch.ops.clair_hip.export_cv(x, False), ops.export_cv(x, torch.float32))
    assert torch.equal(torch.ops.clair_hip.export_cv(x, True), ops.export_cv(x, torch.float64))
    assert torch.ops.clair_hip.export_cv(x[0], True).dtype == torch.float64
    assert torch.equal(torch.ops.clair_hip.export_cv(x[0], True), want[0].double())
    with pytest.raises(TypeError):
        ops.export_cv(x.half())
    with pytest.raises(TypeError):
        ops.export_cv(x.to(torch.int32))
    with pytest.raises(TypeError):
        ops.export_cv(x, torch.float16)
    with pytest.raises(ValueError):
        ops.export_cv(x[0, 0, 0])                      # rank 1
    with pytest.raises(ValueError):
        ops.export_cv(x.unsqueeze(0))                  # rank 5
    with pytest.raises(ValueError):
        ops.export_cv(x.transpose(2, 3))               # not contiguous
    with pytest.raises(ValueError):
        ops.export_cv(x, out=torch.empty((2, 3, 6, 10), device=dev))                          # the input's shape
    with pytest.raises(ValueError):
        ops.export_cv(x, out=torch.empty((2, 6, 10, 3), dtype=torch.float64, device=dev))     # another dtype
    with pytest.raises(ValueError):
        ops.export_cv(x, out=torch.empty((2, 6, 3, 10), device=dev).transpose(2, 3))          # not contiguous
    with pytest.raises(RuntimeError):
        ops.export_cv(x.cpu())
    with pytest.raises(RuntimeError):
        ops.export_cv(x, out=torch.empty((2, 6, 10, 3)))
    for shape, result in [((0, 3, 4, 5), (0, 4, 5, 3)), ((3, 0, 5), (0, 5, 3)), ((4, 0), (4, 0)), ((2, 3, 4, 0), (2, 4, 0, 3))]:
        empty = ops.export_cv(torch.empty(shape, device=dev), torch.float64)
        assert tuple(empty.shape) == result and empty.dtype == torch.float64 and empty.numel() == 0


# ---- the entry points ---------------------------------------------------------------------------------------------
def _as_cv(planar):
    return planar.permute(1, 2, 0).flip(-1) if planar.ndim == 3 else planar


def _raw_frames_dataset(frames, times, std_hint):
    """(H,W,3) BGR frames as an OpenCV reader hands them over (StackDataset itself insists on (N,C,H,W))."""
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import StackDataset

    class RawFrames(StackDataset):
        def __init__(self):
            self.values, self.stds, self.exposure_times = frames, None, times
            self.files, self.std_hint = list(range(len(times))), std_hint
            self.missing_std_mode = MissingStdMode.MULTIPLIER
            self.materialize_std = False

        def __len__(self):
            return len(self.exposure_times)

    return RawFrames()


def _model(dev, channels=3):
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.models import ICRFModelDirect
    powers = (2.2, 2.4, 2.6)[:channels]
    return ICRFModelDirect(icrf=torch.stack([torch.linspace(0, 1, 256) ** p for p in powers]),
                           interpolation_mode=InterpMode.LINEAR).to(dev)


@pytest.fixture(scope="module")
def merge_cases(dev):
    """Every (label, planar result, cv result) of compute_hdr_image on one uint8 stack (8,3,18,34), computed once."""
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.common.transforms import BaseTransform, CastTo, CvToTorch, Normalize
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.training.losses import gaussian_value_weights
    rng = np.random.default_rng(11)
    planar = torch.from_numpy(rng.integers(0, 256, size=(8, 3, 18, 34)).astype(np.uint8))
    raw = torch.from_numpy(np.ascontiguousarray(planar.numpy()[:, ::-1].transpose(0, 2, 3, 1)))
    t = [0.002 * 2.0 ** k for k in range(8)]
    std = dict(missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
    pair = [CastTo("float32"), Normalize(255, 0)]
    flat = ArtefactStack(torch.from_numpy((0.6 + 0.4 * rng.random((3, 18, 34))).astype(np.float32)),
                         torch.from_numpy((0.01 * rng.random((3, 18, 34))).astype(np.float32)))

    class Identity(BaseTransform):
        def __call__(self, x):
            return x

    def both(dataset, transforms, channels=3, **kw):
        def run(layout):
            return compute_hdr_image(DataLoader(dataset, batch_size=4, collate_fn=custom_collate), "cuda",
                                     _model(dev, channels), weight_fn=gaussian_value_weights, gpu_transforms=transforms,
                                     output_layout=layout, **kw)
        return run("planar"), run("cv")

    return {
        "planar": both(StackDataset(planar, t, **std), pair),
        "flat field": both(StackDataset(planar, t, **std), pair, flat_field_dataset=flat),
        "raw frames": both(_raw_frames_dataset(raw, t, ("multiplier", 0.05)), [CvToTorch()] + pair),
        "generic list": both(StackDataset(planar, t, **std), pair + [Identity()]),
        "one channel": both(StackDataset(planar[:, :1].contiguous(), t, **std), pair, channels=1),
    }


@pytest.mark.parametrize("label", ["planar", "flat field", "raw frames", "generic list", "one channel"])
def test_compute_hdr_image_cv_layout(merge_cases, label):
    (mean, std), (cv_mean, cv_std) = merge_cases[label]
    if label == "one channel":
        assert mean.shape == (18, 34) and cv_mean.shape == (18, 34) and cv_std.shape == (18, 34)
    else:
        assert mean.shape == (3, 18, 34) and cv_mean.shape == (18, 34, 3) and cv_std.shape == (18, 34, 3)
    assert cv_mean.dtype == torch.float64 and cv_std.dtype == torch.float32
    assert cv_mean.is_cuda and cv_mean.is_contiguous() and cv_std.is_contiguous()
    assert torch.equal(cv_mean, _as_cv(mean)) and torch.equal(cv_std, _as_cv(std))
    assert bool(torch.isfinite(cv_mean).all()) and float(cv_mean.abs().max()) > 0


def test_compute_hdr_image_cv_layout_on_a_tile_and_bad_values(dev):
    from clair_torch_amd import ops
    from clair_torch_amd.common.transforms import CastTo, Normalize
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    kw = dict(gpu_transforms=[CastTo("float32"), Normalize(255, 0)])
    stack = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=(4, 3, 8, 16)).astype(np.uint8))
    loader = DataLoader(StackDataset(stack, [0.01, 0.02, 0.04, 0.08]), batch_size=4, collate_fn=custom_collate)
    tile = ops.TileGeometry(h_global=16, row_offset=8)
    mean, std = compute_hdr_image(loader, "cuda", _model(dev), tile=tile, **kw)
    cv_mean, cv_std = compute_hdr_image(loader, "cuda", _model(dev), tile=tile, output_layout="cv", **kw)
    assert std is None and cv_std is None  # no uncertainties asked for: nothing to export
    assert cv_mean.shape == (8, 16, 3) and torch.equal(cv_mean, _as_cv(mean))
    with pytest.raises(ValueError, match="output_layout"):
        compute_hdr_image(loader, "cuda", _model(dev), output_layout="hwc", **kw)


def _same_meta(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k]


@pytest.mark.parametrize("route", ["pipelined", "pipelined flat field", "frame by frame", "frame by frame flat field"])
def test_linearize_dataset_generator_cv_layout(dev, route):
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, Normalize, StridedDownscale
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import linearize_dataset_generator
    rng = np.random.default_rng(5)
    frames = torch.from_numpy(rng.integers(0, 65536, size=(3, 3, 17, 33)).astype(np.uint16))
    std = dict(missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
    transforms = [CastTo("float32"), Normalize(65535, 0)]
    h, w = 17, 33
    if route.startswith("frame by frame"):
        transforms = [StridedDownscale(2)] + transforms  # the pipelined route declines the list
        h, w = 9, 17
    flat = None
    if route.endswith("flat field"):
        flat = ArtefactStack(torch.from_numpy((0.6 + 0.4 * rng.random((3, h, w))).astype(np.float32)),
                             torch.from_numpy((0.01 * rng.random((3, h, w))).astype(np.float32)))

    def run(**kw):
        loader = DataLoader(StackDataset(frames, [0.01, 0.02, 0.04], **std), batch_size=1, collate_fn=custom_collate)
        return list(linearize_dataset_generator(loader, "cuda", _model(dev), flatfield_dataset=flat,
                                                gpu_transforms=transforms, **kw))

    ref, got = run(), run(output_layout="cv")
    assert len(ref) == len(got) == 3
    for (lin, lin_std, meta), (cv_lin, cv_std, cv_meta) in zip(ref, got):
        assert lin.shape == (3, h, w) and cv_lin.shape == (h, w, 3) and cv_std.shape == (h, w, 3)
        assert cv_lin.dtype == torch.float32 and cv_std.dtype == torch.float32 and not cv_lin.is_cuda
        assert cv_lin.is_contiguous() and cv_std.is_contiguous()
        assert torch.equal(cv_lin, _as_cv(lin)) and torch.equal(cv_std, _as_cv(lin_std))
        _same_meta(meta, cv_meta)
    assert not torch.equal(ref[0][0], ref[1][0])  # the frames differ, so the order is checked
    with pytest.raises(ValueError, match="output_layout"):
        run(output_layout="input")


@pytest.mark.parametrize("dt", ["float32", "float64"])
@pytest.mark.parametrize("label", ["planar", "one channel"])
def test_device_and_host_save_paths_agree(merge_cases, label, dt):
    from clair_torch_amd.common import image_to_cv_array
    for tensor in merge_cases[label][0]:
        on_device = image_to_cv_array(tensor, np.dtype(dt))
        on_host = image_to_cv_array(tensor.cpu(), np.dtype(dt))
        assert isinstance(on_device, np.ndarray) and on_device.dtype == np.dtype(dt) and on_device.flags.c_contiguous
        assert on_device.shape == on_host.shape == ((18, 34, 3) if tensor.ndim == 3 else (18, 34))
        assert np.array_equal(on_device.view(_I[np.dtype(dt)]), np.ascontiguousarray(on_host).view(_I[np.dtype(dt)]))


def test_save_image_from_the_device(dev, tmp_path, merge_cases):
    from clair_torch_amd.common import save_image
    mean = merge_cases["planar"][0][0]
    seen = []
    save_image(mean, tmp_path / "out" / "hdr.tif", writer=lambda p, a, k: seen.append((p, a, k)) or True)
    (path, array, params), = seen
    assert path == str(tmp_path / "out" / "hdr.tif") and params == [] and array.dtype == np.float64
    assert np.array_equal(array, mean.cpu().numpy().transpose(1, 2, 0)[:, :, ::-1])
