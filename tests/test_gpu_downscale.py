"""StridedDownscale on the device (clair_torch/common/transforms.py:194-216): ct_strided_downscale compacts the raw codes
in their own dtype and layout in front of the code-domain kernels.  Selecting pixels commutes with every per-pixel
operation of the hot path, so every comparison here is exact: the kernel against ``x.cpu()[..., ::s, ::s]``, and the
public entry points on a list holding the transform against the same entry point on a stack sliced on the host."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _random(rng, shape, dtype):
    if dtype == torch.float32:
        return torch.from_numpy(rng.random(shape, dtype=np.float32))
    return torch.from_numpy(rng.integers(0, np.iinfo(_NP[dtype]).max + 1, size=shape).astype(_NP[dtype]))


def _bits(t):
    """Same-width view torch can index and compare (it has no uint16 kernels for either)."""
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _shapes(s):
    # last row / column selected iff (n - 1) % s == 0; widths below one 16-byte packet; rows that are not 16-byte aligned;
    # more rows than one workgroup covers; whole packets only (16 x 64)
    return [(1, 1, 1), (2, 2, 3), (2, 5, s), (2, 7, s + 1), (3, 37, 53), (2, 16, 64), (1, 9, 131)]


@pytest.mark.parametrize("s", [2, 3, 4, 7, 9])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.float32])
def test_kernel_equals_host_slicing(dev, dtype, layout, s):
    from clair_torch_amd import ops
    rng = np.random.default_rng(100 * s + (layout == "nhwc"))
    for b, h, w in _shapes(s):
        planar = _random(rng, (b, 3, h, w), dtype)
        want = _bits(planar)[..., ::s, ::s]                        # the reference's expression, on the host
        host = planar if layout == "nchw" else planar.permute(0, 2, 3, 1).contiguous()
        if layout == "nhwc":
            want = want.permute(0, 2, 3, 1)
        x = host.to(dev)
        got = ops.strided_downscale(x, s, layout=layout)
        assert got.dtype == dtype and got.is_contiguous() and tuple(got.shape) == tuple(want.shape), (b, h, w)
        assert torch.equal(_bits(got).cpu(), want), (b, h, w)
        assert torch.equal(_bits(x).cpu(), _bits(host)), "the source stack was written to"
        # out= an interior slice (not 16-byte aligned) of a larger buffer: nothing outside the slice may change
        n, lead, trail = want.numel(), 5, 37
        sentinel = 0xA5 if dtype == torch.uint8 else (0xA5A5 - 65536 if dtype == torch.uint16 else -7.25)
        buf = torch.full((lead + n + trail,), sentinel, dtype=_bits(planar).dtype, device=dev)
        if dtype == torch.uint16:
            buf = buf.view(torch.uint16)
        out = buf[lead:lead + n].view(want.shape)
        assert ops.strided_downscale(x, s, layout=layout, out=out) is out
        flat = _bits(buf).cpu()
        assert torch.equal(flat[lead:lead + n].view(want.shape), want), (b, h, w)
        assert bool((flat[:lead] == sentinel).all()) and bool((flat[lead + n:] == sentinel).all()), (b, h, w)


def test_kernel_front_end_checks(dev):
    from clair_torch_amd import ops, torch_ops  # noqa: F401 (torch_ops registers torch.ops.clair_hip.*)
    x = (torch.arange(2 * 3 * 8 * 8) % 251).to(torch.uint8).view(2, 3, 8, 8).to(dev)
    assert ops.strided_downscale(x, 1) is x
    assert torch.equal(torch.ops.clair_hip.strided_downscale(x, 2, "nchw"), x[..., ::2, ::2])
    with pytest.raises(ValueError):
        ops.strided_downscale(x, 0)
    with pytest.raises(ValueError):
        ops.strided_downscale(x, 2, out=torch.zeros((2, 3, 4, 5), dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError):
        ops.strided_downscale(x.to(torch.float64), 2)
    with pytest.raises(RuntimeError):
        ops.strided_downscale(x.cpu(), 2)


# ---- the entry points on a list holding the transform -------------------------------------------------------------
def _host_sliced(stack, s, raw=False):
    a = stack.numpy()
    return torch.from_numpy(np.ascontiguousarray(a[:, ::s, ::s] if raw else a[..., ::s, ::s]))


def _raw_frames_dataset(frames, times, std_hint):
    """(H,W,3) BGR frames as an OpenCV reader hands them over (StackDataset itself insists on (N,C,H,W))."""
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import StackDataset

    class RawFrames(StackDataset):
        def __init__(self):
            self.values, self.stds, self.exposure_times = frames, None, times
            self.files, self.std_hint = list(range(len(times))), std_hint
            self.missing_std_mode = MissingStdMode.MULTIPLIER if std_hint else MissingStdMode.NONE
            self.materialize_std = False

        def __len__(self):
            return len(self.exposure_times)

    return RawFrames()


def _pair(dtype):
    from clair_torch_amd.common.transforms import CastTo, Normalize
    return [CastTo("float32"), Normalize(255 if dtype == torch.uint8 else 65535, 0)]


def _lists(dtype, s):
    """(transform lists for a planar stack, for raw frames): the downscale in every allowed position."""
    from clair_torch_amd.common.transforms import CvToTorch, StridedDownscale
    cast, norm = _pair(dtype)
    sd = StridedDownscale(s)
    return ([[sd, cast, norm], [cast, sd, norm], [cast, norm, sd]],
            [[CvToTorch(), sd, cast, norm], [CvToTorch(), cast, sd, norm], [CvToTorch(), cast, norm, sd]])


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16])
def test_stage_images_keeps_the_code_route(dev, dtype, s):
    from clair_torch_amd.common.transforms import BaseTransform
    from clair_torch_amd.inference._staging import stage_images
    rng = np.random.default_rng(s)
    planar = _random(rng, (4, 3, 18, 34), dtype)
    raw = planar.flip(1).permute(0, 2, 3, 1).contiguous() if dtype == torch.uint8 else \
        torch.from_numpy(np.ascontiguousarray(planar.numpy()[:, ::-1].transpose(0, 2, 3, 1)))
    planar_lists, raw_lists = _lists(dtype, s)
    max_code = 255.0 if dtype == torch.uint8 else 65535.0
    for ts in planar_lists:
        for need_planar in (True, False):
            out = stage_images(planar, dev, ts, planar=need_planar)
            assert out[0].dtype == dtype and out[1] == max_code and out[2] == "nchw"
            assert torch.equal(_bits(out[0]).cpu(), _bits(_host_sliced(planar, s)))
    for ts in raw_lists:
        images, mc, layout = stage_images(raw, dev, ts)
        assert images.dtype == dtype and mc == max_code and layout == "nhwc_bgr"
        assert torch.equal(_bits(images).cpu(), _bits(_host_sliced(raw, s, raw=True)))
        # a batch that has to be planar is staged on the generic route from the batch itself: the downscale is applied once
        again, mc2, layout2 = stage_images(raw, dev, ts, planar=True)
        generic, _, _ = stage_images(raw.to(dev), dev, ts, planar=True)  # ... whether it comes from the host or is there already
        assert mc2 is None and layout2 == "nchw" and again.dtype == torch.float32
        assert tuple(again.shape) == (4, 3, -(-18 // s), -(-34 // s)) and torch.equal(again, generic)

    class Identity(BaseTransform):
        def __call__(self, x):
            return x

    # any other list holding the transform runs its __call__ on the generic route
    images, mc, _ = stage_images(planar, dev, planar_lists[0] + [Identity()])
    assert mc is None and images.dtype == torch.float32 and tuple(images.shape) == (4, 3, -(-18 // s), -(-34 // s))


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("mode", ["linear", "lookup"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16])
def test_compute_hdr_image_equals_host_sliced_stack(dev, dtype, mode, s):
    """LINEAR: multiplier std, Gaussian weight (pivoted code-domain kernel, two batches in one launch); LOOKUP with
    uncertainties: the reference-order route.  Planar stacks and raw (H,W,3) BGR frames behind CvToTorch."""
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CvToTorch
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    rng = np.random.default_rng(7 * s + (mode == "lookup"))
    planar = _random(rng, (8, 3, 18, 34), dtype)
    raw = torch.from_numpy(np.ascontiguousarray(planar.numpy()[:, ::-1].transpose(0, 2, 3, 1)))
    t = [0.002 * 2.0 ** k for k in range(8)]
    model = ICRFModelDirect(icrf=torch.stack([torch.linspace(0, 1, 256) ** p for p in (2.2, 2.4, 2.6)]),
                            interpolation_mode=InterpMode.LINEAR if mode == "linear" else InterpMode.LOOKUP).to(dev)
    std = dict(missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)

    def merge(dataset, transforms, **kw):
        return compute_hdr_image(DataLoader(dataset, batch_size=4, collate_fn=custom_collate), "cuda", model,
                                 weight_fn=gaussian_value_weights, gpu_transforms=transforms, **kw)

    planar_lists, raw_lists = _lists(dtype, s)
    ref = merge(StackDataset(_host_sliced(planar, s), t, **std), _pair(dtype))
    assert ref[0].shape == (3, -(-18 // s), -(-34 // s)) and ref[1] is not None
    for ts in planar_lists:
        got = merge(StackDataset(planar, t, **std), ts)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    ref_raw = merge(_raw_frames_dataset(_host_sliced(raw, s, raw=True), t, ("multiplier", 0.05)), [CvToTorch()] + _pair(dtype))
    assert torch.equal(ref_raw[0], ref[0]) and torch.equal(ref_raw[1], ref[1])
    for ts in raw_lists:
        got = merge(_raw_frames_dataset(raw, t, ("multiplier", 0.05)), ts)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_measure_linearity_equals_host_sliced_stack(dev):
    from _util import golden
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import measure_linearity
    from clair_torch_amd.models import ICRFModelDirect
    g = golden("training")
    codes = torch.from_numpy(g["train_codes"])
    assert tuple(codes.shape) == (6, 3, 32, 32) and codes.dtype == torch.uint8
    t = g["train_exposures"].tolist()
    model = ICRFModelDirect(icrf=torch.from_numpy(g["train_lut0"]), interpolation_mode=InterpMode.LINEAR).to(dev)
    std = dict(missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)

    def measure(stack, transforms):
        loader = DataLoader(StackDataset(stack, t, **std), batch_size=6, shuffle=False, collate_fn=custom_collate)
        return measure_linearity(loader, "cuda", True, True, model, gpu_transforms=transforms)

    ref = measure(_host_sliced(codes, 2), _pair(torch.uint8))
    assert ref[1].shape[1] == 3 and ref[3] is not None
    for ts in _lists(torch.uint8, 2)[0]:
        got = measure(codes, ts)
        assert len(got) == 4
        for a, b in zip(got, ref):
            assert torch.equal(a, b)


def test_linearize_and_video_stats_equal_host_sliced_stack(dev):
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import compute_video_mean_and_std, linearize_dataset_generator
    from clair_torch_amd.models import ICRFModelDirect
    rng = np.random.default_rng(21)
    model = ICRFModelDirect(icrf=torch.stack([torch.linspace(0, 1, 256) ** p for p in (2.2, 2.4, 2.6)]),
                            interpolation_mode=InterpMode.LINEAR).to(dev)
    std = dict(missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
    s = 2
    frames = _random(rng, (2, 3, 17, 33), torch.uint16)

    def linearize(stack, transforms):
        loader = DataLoader(StackDataset(stack, [0.01, 0.02], **std), batch_size=1, collate_fn=custom_collate)
        return list(linearize_dataset_generator(loader, "cuda", model, gpu_transforms=transforms))

    ref = linearize(_host_sliced(frames, s), _pair(torch.uint16))
    for ts in _lists(torch.uint16, s)[0]:
        got = linearize(frames, ts)  # frame by frame: the pipelined route declines the list
        assert len(got) == len(ref) == 2
        for a, b in zip(got, ref):
            assert a[0].shape == (3, 9, 17) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    video = _random(rng, (5, 3, 17, 33), torch.uint16)

    def stats(stack, transforms):
        loader = DataLoader(StackDataset(stack, [1.0] * 5, missing_std_mode=MissingStdMode.NONE), batch_size=2,
                            collate_fn=custom_collate)
        return compute_video_mean_and_std(loader, "cuda", model, gpu_transforms=transforms)

    ref = stats(_host_sliced(video, s), _pair(torch.uint16))
    for ts in _lists(torch.uint16, s)[0]:
        got = stats(video, ts)
        assert got[0].shape == (3, 9, 17) and torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_tile_with_downscale_is_refused(dev):
    from clair_torch_amd import ops
    from clair_torch_amd.common.transforms import StridedDownscale
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image, measure_linearity
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training import train_icrf
    stack = _random(np.random.default_rng(0), (4, 3, 8, 16), torch.uint8)
    loader = DataLoader(StackDataset(stack, [0.01, 0.02, 0.04, 0.08]), batch_size=4, collate_fn=custom_collate)
    ts = [StridedDownscale(2)] + _pair(torch.uint8)
    tile = ops.TileGeometry(h_global=16, row_offset=8)
    with pytest.raises(ValueError, match="StridedDownscale"):
        compute_hdr_image(loader, "cuda", None, gpu_transforms=ts, tile=tile)
    with pytest.raises(ValueError, match="StridedDownscale"):
        measure_linearity(loader, "cuda", False, True, None, gpu_transforms=ts, tile=tile)
    with pytest.raises(ValueError, match="StridedDownscale"):
        train_icrf(loader, 4, "cuda", ICRFModelDirect(n_points=64, channels=3).to(dev), epochs=1, gpu_transforms=ts,
                   tile=tile, verbose=False)
    # without tile the same list is fine
    mean, _ = compute_hdr_image(loader, "cuda", None, gpu_transforms=ts)
    assert mean.shape == (3, 4, 8)
