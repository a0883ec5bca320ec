"""ct_linearize_dark_ingest on the device: a gpu_transforms chain, the dark-field conditional blur and the ICRF linearization of
independent raw frames in one pass.  Its specification is one sentence -- for every frame the outputs are bit for bit those of
ct_ingest_transform, ct_dark_field_blur on its result as a batch of one, and ct_linearize_std on (xb, sigma_eff) -- so everything
here is torch.equal against those three launches, through ops.linearize_dark_ingest_frames and through
linearize_dataset_generator(fused_dark_ingest=True / False).  No tolerance anywhere: the operations are the same, in the same
order, with contraction off."""
import functools

import pytest
import torch
from torch.utils.data import DataLoader

from _dark_cases import as_dtype as _as_dtype, scene

_scene = functools.partial(scene, period=8)     # 17 and 50 frames: the exposure times start over every 8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _bgr(planar):
    """(F,3,H,W) RGB planes -> the (F,H,W,3) BGR frames an OpenCV reader hands over."""
    return planar.flip(1).permute(0, 2, 3, 1).contiguous()


def _three(frames, stages, layout, darks, dark_stds, lut, interp, *, std=None, **kw):
    """The three launches the fused kernel replaces, the blur frame by frame."""
    from clair_torch_amd import ops
    x = ops.ingest_transform(frames, stages, layout)
    xbs, sigs = [], []
    for k in range(x.shape[0]):
        xb, sig = ops.dark_field_blur(x[k:k + 1], darks[k][None], dark_stds[k][None], std=None if std is None else std[k:k + 1], **kw)
        xbs.append(xb)
        sigs.append(sig)
    return ops.linearize_frames(torch.cat(xbs), lut, interp, std=torch.cat(sigs), want_std=True)


def _src(std_mode, sd):
    return dict(std=sd) if std_mode == "explicit" else dict(std_mode=std_mode, std_value=0.01 if std_mode == "constant" else 0.05)


CLAMPS = [(0.3, 0.6), (0.35, 0.55), (0.25, 0.65)]      # three DIFFERENT pairs, inside the scenes' range


def _chains(dtype, c):
    """name -> stage list, the constants scaled to the dtype's codes (float32 pixels lie in [0, 1])."""
    top = {torch.uint8: 255.0, torch.uint16: 65535.0}.get(dtype, 1.0)
    black = ("affine", top * 64 / 65535, top - top * 64 / 65535, 1, 0)
    pair = ("affine", 0, top, 1, 0)
    return {"black_level": [black],
            "code_pair": [pair],
            "per_channel_clamp": [pair, ("clamp", CLAMPS[:c]), ("affine", 0.25, 0.4, 0.8, 0.1)],
            "four_stages": [black, ("clamp", [(0.02, 0.97)]), ("affine", 0, 1, 0.9, 0.05), ("clamp", [(0.06, 0.9)])]}


STDS = ["constant", "multiplier", "explicit"]
# planar (F,C,H,W) -- (3,3,13,9): rows end inside a thread's group; (2,3,2,2): both reflections hit the same row and column;
# (1,1,5,6): one frame and channel; (5,2,3,130): more than one group walk per row, width no multiple of 4; (17,1,2,3): two
# launches; (2,1,3,5): one group and a one-element tail -- and interleaved (F,H,W,3), the same edges with 3 channels per pixel
PLANAR = [(3, 3, 13, 9), (2, 3, 2, 2), (1, 1, 5, 6), (5, 2, 3, 130), (17, 1, 2, 3), (2, 1, 3, 5)]
INTERLEAVED = [(3, 13, 9, 3), (2, 2, 2, 3), (17, 2, 3, 3), (2, 3, 130, 3), (1, 5, 6, 3)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint16, torch.uint8], ids=["f32", "u16", "u8"])
@pytest.mark.parametrize("shape", PLANAR + INTERLEAVED, ids=lambda s: ("hwc" if s in INTERLEAVED else "chw") + "x".join(map(str, s)))
def test_bit_equal_to_the_three_launches(dev, shape, dtype):
    from clair_torch_amd import ops
    raw = shape in INTERLEAVED
    n, c, h, w = (shape[0], 3, shape[1], shape[2]) if raw else shape
    x, sd, _, dark, dark_std, lut = _scene(11 + h, n, c, h, w)
    codes, _ = _as_dtype(x, dtype)
    layout = "nhwc_bgr" if raw else "nchw"
    frames = (_bgr(codes) if raw else codes).to(dev)
    assert tuple(frames.shape) == tuple(shape)
    # the mask is neither 0 nor 1 somewhere (here: everywhere), so blur and raw value both count
    m = torch.sigmoid((dark - 0.05) * 50.0)
    assert bool(((m > 0.01) & (m < 0.99)).any())
    sd, dark, dark_std, lut = sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    for name, stages in _chains(dtype, c).items():
        for std_mode in STDS:
            src = _src(std_mode, sd)
            for interp in ("linear", "catmull"):
                want = _three(frames, stages, layout, dark, dark_std, lut, interp, **src)
                assert bool(torch.isfinite(want[0]).all()) and bool(torch.isfinite(want[1]).all())
                got = ops.linearize_dark_ingest_frames(frames, stages, list(dark), list(dark_std), lut, interp, layout=layout, **src)
                assert got[0].shape == (n, c, h, w) and got[0].dtype == got[1].dtype == torch.float32
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, std_mode, interp)
        # (guards) the blur does something: the unblurred linearization of the same chain differs
        plain = ops.linearize_ingest_frames(frames, stages, lut, "linear", std_mode="multiplier", std_value=0.05, layout=layout)
        got = ops.linearize_dark_ingest_frames(frames, stages, dark, dark_std, lut, "linear", std_mode="multiplier", std_value=0.05,
                                               layout=layout)
        assert not torch.equal(got[0], plain[0]) and not torch.equal(got[1], plain[1]), name
        if raw:  # the dark field is read in plane (RGB) order: swapping its planes 0 and 2 changes the result
            swapped = ops.linearize_dark_ingest_frames(frames, stages, dark.flip(1), dark_std.flip(1), lut, "linear",
                                                       std_mode="multiplier", std_value=0.05, layout=layout)
            assert not torch.equal(swapped[0], got[0]), name
    # (guards) the per-channel clamp changes at least one sample in each channel
    stages = _chains(dtype, c)["per_channel_clamp"]
    before, after = ops.ingest_transform(frames, stages[:1], layout), ops.ingest_transform(frames, stages[:2], layout)
    for ch in range(c):
        assert not torch.equal(before[:, ch], after[:, ch]), ch


@pytest.mark.parametrize("raw", [False, True], ids=["planar", "bgr"])
def test_out_buffers_and_views(dev, raw):
    """``out=`` slices of a larger buffer at a frame offset whose address is not 16-byte aligned: the same bits as the whole
    stack gives, and nothing outside the slices is written."""
    from clair_torch_amd import ops
    n, c, h, w = 5, 3, 7, 9
    x, sd, _, dark, dark_std, lut = _scene(5, n, c, h, w)
    codes, _ = _as_dtype(x, torch.uint16)
    layout = "nhwc_bgr" if raw else "nchw"
    frames = (_bgr(codes) if raw else codes).to(dev)
    sd, dark, dark_std, lut = sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    stages = _chains(torch.uint16, c)["per_channel_clamp"]
    kw = dict(std_mode="multiplier", std_value=0.05, layout=layout)
    want = _three(frames, stages, layout, dark, dark_std, lut, "catmull", std_mode="multiplier", std_value=0.05)
    whole = ops.linearize_dark_ingest_frames(frames, stages, dark, dark_std, lut, "catmull", **kw)
    assert torch.equal(whole[0], want[0]) and torch.equal(whole[1], want[1])
    big_lin, big_std = torch.full((n + 3, c, h, w), -1.0, device=dev), torch.full((n + 3, c, h, w), -1.0, device=dev)
    assert big_lin[2:].data_ptr() % 16 != 0 and big_std[2:].data_ptr() % 16 != 0      # 2 * 189 floats into the buffer
    got = ops.linearize_dark_ingest_frames(frames, stages, dark, dark_std, lut, "catmull", out=(big_lin[2:2 + n], big_std[2:2 + n]), **kw)
    assert got[0].data_ptr() == big_lin[2:].data_ptr() and got[1].data_ptr() == big_std[2:].data_ptr()
    assert torch.equal(big_lin[2:2 + n], whole[0]) and torch.equal(big_std[2:2 + n], whole[1])
    for big in (big_lin, big_std):
        assert bool((big[:2] == -1).all()) and bool((big[2 + n:] == -1).all())
    # a range of the frames, as the pipeline hands a run of matched frames over, with explicit planar uncertainties
    big_lin.fill_(-1.0)
    big_std.fill_(-1.0)
    ops.linearize_dark_ingest_frames(frames[1:4], stages, dark[1:4], dark_std[1:4], lut, "linear", std=sd[1:4], layout=layout,
                                     out=(big_lin[3:6], big_std[3:6]))
    want = _three(frames, stages, layout, dark, dark_std, lut, "linear", std=sd)
    assert torch.equal(big_lin[3:6], want[0][1:4]) and torch.equal(big_std[3:6], want[1][1:4])
    for big in (big_lin, big_std):
        assert bool((big[:3] == -1).all()) and bool((big[6:] == -1).all())


def test_refusals_on_the_device(dev):
    """Everything below raises before any launch, with the exception types of linearize_dark_frames and
    linearize_ingest_frames."""
    from clair_torch_amd import ops
    x, sd, _, dark, dark_std, lut = [v.to(dev) for v in _scene(2, 3, 3, 6, 5)]
    pair = [("affine", 0, 1, 1, 0)]
    call = ops.linearize_dark_ingest_frames
    with pytest.raises(RuntimeError, match="does not require grad"):     # LOOKUP: sigma_eff always has the dark term
        call(x, pair, dark, dark_std, lut, "lookup", std=sd)
    with pytest.raises(RuntimeError, match="does not require grad"):
        call(x, pair, dark, dark_std, lut, "lookup")
    with pytest.raises(ValueError, match="stage 0"):                      # a data-dependent Normalize has no kernel here
        call(x, [("affine_data", 1, 0)], dark, dark_std, lut, "linear", std=sd)
    with pytest.raises(ValueError, match="at most 4 stages"):
        call(x, pair * 5, dark, dark_std, lut, "linear", std=sd)
    with pytest.raises(ValueError):                                       # the blur reflects: two columns at least
        call(x[:, :, :, :1].contiguous(), pair, dark[:, :, :, :1].contiguous(), dark_std[:, :, :, :1].contiguous(), lut, "linear")
    with pytest.raises(ValueError):                                       # ... and two rows
        call(x[:, :, :1].contiguous(), pair, dark[:, :, :1].contiguous(), dark_std[:, :, :1].contiguous(), lut, "linear")
    with pytest.raises(ValueError, match="takes \\(B, H, W, 3\\) frames"):  # an interleaved layout with C != 3
        call(x, pair, dark, dark_std, lut, "linear", layout="nhwc_bgr")
    with pytest.raises(ValueError, match="mask_map batch dimension"):    # dark fields of another shape
        call(x, pair, dark[:, :, :5], dark_std[:, :, :5], lut, "linear", std=sd)
    with pytest.raises(ValueError, match="mask_map batch dimension"):    # ... planar (C,H,W) also for interleaved frames
        call(_bgr(x), pair, _bgr(dark), _bgr(dark_std), lut, "linear", layout="nhwc_bgr")
    with pytest.raises(ValueError, match="dark_std shape"):
        call(x, pair, dark, dark_std[:, :, :, :4], lut, "linear", std=sd)
    with pytest.raises(ValueError, match="dark_stds is required"):
        call(x, pair, dark, None, lut, "linear", std=sd)
    with pytest.raises(ValueError, match="std must be a float32 tensor of shape"):     # explicit uncertainties are planar
        call(_bgr(x), pair, dark, dark_std, lut, "linear", std=_bgr(sd), layout="nhwc_bgr")
    lin, std = torch.empty((3, 3, 6, 5), device=dev), torch.empty((3, 3, 6, 5), device=dev)
    with pytest.raises(ValueError, match="contiguous float32 tensor of shape"):        # a wrong out dtype
        call(x, pair, dark, dark_std, lut, "linear", std=sd, out=(lin.double(), std))
    with pytest.raises(ValueError):
        call(x, pair, dark, dark_std, lut, "linear", std=sd, out=(lin, None))
    with pytest.raises(ValueError, match="stack must be contiguous"):
        call(x.transpose(2, 3), pair, dark, dark_std, lut, "linear")
    got = call(x, pair, dark, dark_std, lut, "linear", std=sd, out=(lin, std))         # (the arguments above are otherwise fine)
    assert got[0] is lin and bool(torch.isfinite(lin).all())


# ---- the generator ----------------------------------------------------------------------------------------------------
class _MatchesSome:
    """A dark-field dataset that has an image for the frames in ``frames`` only (the others: MissingValMode.SKIP_BATCH)."""

    def __init__(self, stack, frames):
        self.stack, self.frames = stack, set(frames)

    def get_matching_artefact_images(self, reference_frame_settings_list):
        if not set(reference_frame_settings_list) <= self.frames:
            return None, None, None, None
        return self.stack.get_matching_artefact_images(reference_frame_settings_list)


class _ByParity:
    """Two dark fields alternating by frame parity."""

    def __init__(self, even, odd):
        self.stacks = (even, odd)

    def get_matching_artefact_images(self, reference_frame_settings_list):
        return self.stacks[int(reference_frame_settings_list[0]) % 2].get_matching_artefact_images(reference_frame_settings_list)


class _NoStdAt:
    """A dark-field dataset that returns no dark std for one frame only."""

    def __init__(self, stack, frame):
        self.stack, self.frame = stack, frame

    def get_matching_artefact_images(self, reference_frame_settings_list):
        idx, value, std, meta = self.stack.get_matching_artefact_images(reference_frame_settings_list)
        return idx, value, (None if self.frame in reference_frame_settings_list else std), meta


def _run(loader, model, **kw):
    from clair_torch_amd.inference import linearize_dataset_generator
    return [(lin.clone(), sd.clone(), meta) for lin, sd, meta in linearize_dataset_generator(loader, "cuda", model, **kw)]


def _same(a, b):
    assert len(a) == len(b)
    for k, ((la, sa, ma), (lb, sb, mb)) in enumerate(zip(a, b)):
        assert torch.equal(la, lb) and torch.equal(sa, sb), k
        assert la.shape == lb.shape and la.dtype == lb.dtype, k
        assert ma.keys() == mb.keys() and all(torch.equal(torch.as_tensor(ma[key]), torch.as_tensor(mb[key])) for key in ma), k


def _collect_until_error(loader, model, **kw):
    from clair_torch_amd.inference import linearize_dataset_generator
    got, err = [], None
    try:
        for lin, sd, meta in linearize_dataset_generator(loader, "cuda", model, **kw):
            got.append((lin.clone(), sd.clone(), meta))
    except Exception as exc:  # noqa: BLE001 -- the type is what the caller asserts
        err = exc
    return got, err


def _case(dev, raw):
    """50 uint16 frames, MULTIPLIER uncertainties derived in the kernel, batch size 1: more than three groups of 16, so ring
    slots are re-used.  Planar 3x6x5 frames behind a black-level list, or 6x5x3 BGR frames behind CvToTorch + the code pair."""
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, CvToTorch, Normalize
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.models import ICRFModelDirect
    x, _, t, dark, dark_std, lut = _scene(43 if raw else 41, 50, 3, 6, 5)
    codes, _ = _as_dtype(x, torch.uint16)
    ds = StackDataset(_bgr(codes) if raw else codes, t.tolist(), missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05,
                      materialize_std=False)
    loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
    models = {m: ICRFModelDirect(icrf=lut, interpolation_mode=InterpMode[m.upper()]).to(dev) for m in ("linear", "catmull", "lookup")}
    tf = [CvToTorch(), CastTo("float32"), Normalize(65535, 0)] if raw else [CastTo("float32"), Normalize(65535, 64)]
    return dict(loader=loader, models=models, dark=dark, dark_std=dark_std, kw=dict(gpu_transforms=tf))


@pytest.fixture(scope="module")
def planar_case(dev):
    return _case(dev, False)


@pytest.fixture(scope="module")
def bgr_case(dev):
    return _case(dev, True)


@pytest.mark.parametrize("case_name", ["planar_case", "bgr_case"])
def test_generator_routes_are_bit_equal(dev, case_name, request, monkeypatch):
    from clair_torch_amd import ops
    from clair_torch_amd.datasets import ArtefactStack
    case = request.getfixturevalue(case_name)
    loader, kw, n = case["loader"], case["kw"], len(case["loader"].dataset)
    art = ArtefactStack(case["dark"][0], case["dark_std"][0])
    flat = ArtefactStack(0.8 + 0.4 * torch.rand((3, 6, 5), generator=torch.Generator().manual_seed(3)), 0.01 * torch.ones((3, 6, 5)))
    plain = {}
    for mode in ("linear", "catmull"):
        model = case["models"][mode]
        for extra in ({}, dict(flatfield_dataset=flat), dict(output_layout="cv")):
            want = _run(loader, model, dark_field_dataset=art, fused_dark_ingest=False, **kw, **extra)
            got = _run(loader, model, dark_field_dataset=art, fused_dark_ingest=True, **kw, **extra)
            assert len(got) == n and tuple(got[0][0].shape) == ((6, 5, 3) if extra.get("output_layout") else (3, 6, 5))
            _same(got, want)
            if not extra:
                plain[mode] = want
    model = case["models"]["linear"]
    # a dark field for some frames only: runs of matched and unmatched frames inside the groups, a whole unmatched group
    some = set(list(range(5)) + [9] + list(range(20, 37)) + [49])
    ds_some = _MatchesSome(art, some)
    want = _run(loader, model, dark_field_dataset=ds_some, fused_dark_ingest=False, **kw)
    got = _run(loader, model, dark_field_dataset=ds_some, fused_dark_ingest=True, **kw)
    _same(got, want)
    bare = _run(loader, model, **kw)      # no dark dataset at all
    for k in range(n):
        ref = plain["linear"] if k in some else bare
        assert torch.equal(got[k][0], ref[k][0]) and torch.equal(got[k][1], ref[k][1]), k
    assert any(not torch.equal(plain["linear"][k][0], bare[k][0]) for k in range(n))   # (the correction matters here)
    # two dark fields alternating by frame parity: the cache and the per-frame pointers
    parity = _ByParity(art, ArtefactStack(case["dark"][1], case["dark_std"][1]))
    want = _run(loader, model, dark_field_dataset=parity, fused_dark_ingest=False, **kw)
    got = _run(loader, model, dark_field_dataset=parity, fused_dark_ingest=True, **kw)
    _same(got, want)
    assert torch.equal(got[0][0], plain["linear"][0][0]) and not torch.equal(got[1][0], plain["linear"][1][0])

    # which route ran: the blur kernel of the frame-by-frame route is never called by the fused one
    def no_blur(*args, **kwargs):
        raise AssertionError("ct_dark_field_blur ran: the frame went frame by frame")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "dark_field_blur", no_blur)
        _same(_run(loader, model, dark_field_dataset=art, fused_dark_ingest=True, **kw), plain["linear"])
        with pytest.raises(AssertionError, match="frame by frame"):
            _run(loader, model, dark_field_dataset=art, fused_dark_ingest=False, **kw)
        with pytest.raises(AssertionError, match="frame by frame"):      # the keyword is read only with fused_dark=True
            _run(loader, model, dark_field_dataset=art, fused_dark=False, fused_dark_ingest=True, **kw)


@pytest.mark.parametrize("case_name", ["planar_case", "bgr_case"])
def test_generator_errors_surface_where_the_frame_by_frame_route_raises(dev, case_name, request):
    from clair_torch_amd.datasets import ArtefactStack
    case = request.getfixturevalue(case_name)
    loader, kw, model = case["loader"], case["kw"], case["models"]["linear"]
    art = ArtefactStack(case["dark"][0], case["dark_std"][0])
    full = _run(loader, model, dark_field_dataset=art, fused_dark_ingest=False, **kw)
    # no dark std for frame 5 only: exactly frames 0..4, then AttributeError; for frame 16: the first of the second group
    for frame in (5, 16):
        for flag in (True, False):
            got, err = _collect_until_error(loader, model, dark_field_dataset=_NoStdAt(art, frame), fused_dark_ingest=flag, **kw)
            assert isinstance(err, AttributeError) and len(got) == frame, (frame, flag, err)
            _same(got, full[:frame])
    # LOOKUP stays frame by frame and raises there, at the first frame
    for flag in (True, False):
        got, err = _collect_until_error(loader, case["models"]["lookup"], dark_field_dataset=art, fused_dark_ingest=flag, **kw)
        assert isinstance(err, RuntimeError) and "does not require grad" in str(err) and got == []


def test_declined_lists_stay_frame_by_frame(dev, planar_case, monkeypatch):
    """A data-dependent Normalize and a StridedDownscale with a dark field: today's route and values with the keyword on and
    off, and the fused front is never called."""
    from clair_torch_amd import ops
    from clair_torch_amd.common.transforms import CastTo, Normalize, StridedDownscale
    from clair_torch_amd.datasets import ArtefactStack
    loader, model = planar_case["loader"], planar_case["models"]["linear"]
    dark, dark_std = planar_case["dark"][0], planar_case["dark_std"][0]
    lists = (([CastTo("float32"), Normalize()], ArtefactStack(dark, dark_std)),
             ([StridedDownscale(2), CastTo("float32"), Normalize(65535, 64)], ArtefactStack(dark[:, ::2, ::2], dark_std[:, ::2, ::2])))
    wants = [_run(loader, model, gpu_transforms=tf, dark_field_dataset=art, fused_dark_ingest=False) for tf, art in lists]

    def no_fused(*args, **kwargs):
        raise AssertionError("ct_linearize_dark_ingest ran")

    monkeypatch.setattr(ops, "linearize_dark_ingest_frames", no_fused)
    for (tf, art), want in zip(lists, wants):
        assert len(want) == 50
        _same(_run(loader, model, gpu_transforms=tf, dark_field_dataset=art, fused_dark_ingest=True), want)
    with pytest.raises(AssertionError, match="ct_linearize_dark_ingest ran"):      # (the patch does bite on a black level)
        _run(loader, model, dark_field_dataset=ArtefactStack(dark, dark_std), fused_dark_ingest=True, **planar_case["kw"])
