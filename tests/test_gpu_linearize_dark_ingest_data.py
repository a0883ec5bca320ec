"""ct_linearize_dark_ingest_data on the device: a gpu_transforms chain with ONE data-dependent Normalize whose bounds are per frame,
the dark-field conditional blur and the ICRF linearization of independent raw frames in one pass.  Its specification is one
sentence -- for every frame the outputs are bit for bit those of ct_ingest_extrema_frames, ct_ingest_transform_data with that
frame's constants, ct_dark_field_blur on its result as a batch of one, and ct_linearize_std on (xb, sigma_eff) -- so everything
here is torch.equal against those four launches, through ops.linearize_dark_ingest_frames_data and through
linearize_dataset_generator(fused_dark_ingest_data=True / False).  No tolerance anywhere: the operations are the same, in the same
order, with contraction off."""
import functools

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from _dark_cases import as_dtype as _as_dtype, scene

_scene = functools.partial(scene, period=8)     # 17 and 50 frames: the exposure times start over every 8

pytestmark = pytest.mark.gpu

_TORCH_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _bgr(planar):
    """(F,3,H,W) RGB planes -> the (F,H,W,3) BGR frames an OpenCV reader hands over."""
    return planar.flip(1).permute(0, 2, 3, 1).contiguous()


def _disjoint_frames(rng, n, chw, dtype):
    """Planar (n,) + chw frames, frame f within [f * R, (f + 1) * R) of the dtype's codes and holding both ends of it: no two
    frames share a minimum or a range, so a kernel that reads another frame's constants cannot pass.  float32: the uint16
    codes over 65535."""
    top = 256 if dtype == torch.uint8 else 65536
    r = min(50 if dtype == torch.uint8 else 12000, top // n)
    x = np.stack([rng.integers(f * r, (f + 1) * r, size=chw) for f in range(n)])
    flat = x.reshape(n, -1)
    flat[:, 0], flat[:, -1] = np.arange(n) * r, (np.arange(n) + 1) * r - 1
    if dtype == torch.float32:
        return torch.from_numpy((x / 65535.0).astype(np.float32))
    return torch.from_numpy(x.astype(_TORCH_NP[dtype]))


def _four(frames, stages, layout, darks, dark_stds, lut, interp, *, std=None, **kw):
    """The four launches the fused pair replaces: the extrema of every frame, then chain and blur frame by frame with that
    frame's constants and dark field, then the linearization with std = sigma_eff, explicit."""
    from clair_torch_amd import ops
    K = ops.ingest_extrema_frames(frames, ops.data_stage_prefix(stages), layout)
    xbs, sigs = [], []
    for k in range(frames.shape[0]):
        x = ops.ingest_transform(frames[k:k + 1], stages, layout, consts=K[k])
        xb, sig = ops.dark_field_blur(x, darks[k][None], dark_stds[k][None], std=None if std is None else std[k:k + 1], **kw)
        xbs.append(xb)
        sigs.append(sig)
    return ops.linearize_frames(torch.cat(xbs), lut, interp, std=torch.cat(sigs), want_std=True), K


def _src(std_mode, sd):
    return dict(std=sd) if std_mode == "explicit" else dict(std_mode=std_mode, std_value=0.01 if std_mode == "constant" else 0.05)


CLAMPS = [(0.2, 0.8), (0.25, 0.7), (0.1, 0.9)]      # three DIFFERENT pairs, inside the normalised range


def _chains(dtype, c):
    """name -> stage list around the data stage; the black level in the dtype's own unit (it moves the extrema, not the result's
    range: the data stage behind it still maps each frame to [0, 1])."""
    black = ("affine", {torch.uint8: 2.0, torch.uint16: 480.0}.get(dtype, 480.0 / 65535), 1.0, 1.0, 0.0)
    return {"data_alone": [("affine_data", 1.0, 0.0)],
            "black_level_in_front": [black, ("affine_data", 1.0, 0.0)],
            "per_channel_clamp_behind": [("affine_data", 1.25, -0.125), ("clamp", CLAMPS[:c])]}


STDS = ["constant", "multiplier", "explicit"]
INTERPS = ["linear", "catmull", None]                  # None: no LUT
# planar (F,C,H,W) -- (3,3,13,9): rows end inside a thread's group; (2,3,2,2): both reflections hit the same row and column;
# (1,1,5,6): one frame and channel; (5,2,3,130): more than one group walk per row, width no multiple of 4; (17,1,2,3): two
# launches, so frame 16 reads row 16 of the constants through the second launch's pointer -- and interleaved (F,H,W,3), the same
# edges with 3 channels per pixel
PLANAR = [(3, 3, 13, 9), (2, 3, 2, 2), (1, 1, 5, 6), (5, 2, 3, 130), (17, 1, 2, 3)]
INTERLEAVED = [(3, 13, 9, 3), (2, 2, 2, 3), (17, 2, 3, 3), (2, 3, 130, 3)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint16, torch.uint8], ids=["f32", "u16", "u8"])
@pytest.mark.parametrize("shape", PLANAR + INTERLEAVED, ids=lambda s: ("hwc" if s in INTERLEAVED else "chw") + "x".join(map(str, s)))
def test_bit_equal_to_the_four_launches(dev, shape, dtype):
    from clair_torch_amd import ops
    raw = shape in INTERLEAVED
    n, c, h, w = (shape[0], 3, shape[1], shape[2]) if raw else shape
    rng = np.random.default_rng(211 + h)
    _, sd, _, dark2, dark_std2, lut = _scene(11 + h, max(n, 2), c, h, w)
    planar = _disjoint_frames(rng, n, (c, h, w), dtype)
    layout = "nhwc_bgr" if raw else "nchw"
    frames = (_bgr(planar) if raw else planar).to(dev)
    assert tuple(frames.shape) == tuple(shape)
    # two DIFFERENT dark fields, alternating by frame; the mask is neither 0 nor 1 somewhere, so blur and raw value both count
    assert not torch.equal(dark2[0], dark2[1])
    m = torch.sigmoid((dark2[:2] - 0.05) * 50.0)
    assert bool(((m > 0.01) & (m < 0.99)).any())
    sd, lut = sd[:n].to(dev), lut.to(dev)
    dark, dark_std = [dark2[k % 2].to(dev) for k in range(n)], [dark_std2[k % 2].to(dev) for k in range(n)]
    for name, stages in _chains(dtype, c).items():
        for std_mode in STDS:
            src = _src(std_mode, sd)
            for interp in INTERPS:
                table = None if interp is None else lut
                want, K = _four(frames, stages, layout, dark, dark_std, table, interp, **src)
                assert bool(torch.isfinite(want[0]).all()) and bool(torch.isfinite(want[1]).all()) and bool((K[:, 1] > 0).all())
                got = ops.linearize_dark_ingest_frames_data(frames, stages, dark, dark_std, table, interp, consts=K, layout=layout, **src)
                assert got[0].shape == (n, c, h, w) and got[0].dtype == got[1].dtype == torch.float32
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, std_mode, interp)
        # (guards) every frame has constants of its own, and they matter: frame n - 1 with frame 0's constants differs
        kw = dict(std_mode="multiplier", std_value=0.05, layout=layout)
        got = ops.linearize_dark_ingest_frames_data(frames, stages, dark, dark_std, lut, "linear", consts=K, **kw)
        if n > 1:
            assert len({tuple(row) for row in K[:, :2].cpu().tolist()}) == n
            shifted = ops.linearize_dark_ingest_frames_data(frames, stages, dark, dark_std, lut, "linear", consts=K.roll(1, 0).contiguous(), **kw)
            assert all(not torch.equal(shifted[0][k], got[0][k]) for k in range(n)), name
        # ... the blur does something: the unblurred linearization of the same chain differs
        plain = ops.linearize_ingest_frames(frames, stages, lut, "linear", consts=K, **kw)
        assert not torch.equal(got[0], plain[0]) and not torch.equal(got[1], plain[1]), name
        if n > 1:  # ... and each frame reads its own dark field: with the two swapped every frame changes
            swapped = ops.linearize_dark_ingest_frames_data(frames, stages, dark[1:] + dark[:1], dark_std[1:] + dark_std[:1], lut, "linear",
                                                            consts=K, **kw)
            assert all(not torch.equal(swapped[0][k], got[0][k]) for k in range(n - n % 2)), name
    # (guards) the per-channel clamp changes at least one sample in each channel
    stages = _chains(dtype, c)["per_channel_clamp_behind"]
    K = ops.ingest_extrema_frames(frames, (), layout)
    for ch in range(c):
        before = torch.cat([ops.ingest_transform(frames[k:k + 1], stages[:1], layout, consts=K[k]) for k in range(n)])
        after = torch.cat([ops.ingest_transform(frames[k:k + 1], stages, layout, consts=K[k]) for k in range(n)])
        assert not torch.equal(before[:, ch], after[:, ch]), ch


def test_constants_beside_a_constant_chain_are_not_read(dev):
    """consts without a data stage: the constant chain, bit for bit linearize_dark_ingest_frames -- whatever the constants hold."""
    from clair_torch_amd import ops
    x, _, _, dark, dark_std, lut = _scene(7, 3, 3, 7, 9)
    codes, _ = _as_dtype(x, torch.uint16)
    frames, dark, dark_std, lut = codes.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    stages = [("affine", 64, 65535 - 64, 1, 0), ("clamp", CLAMPS)]
    kw = dict(std_mode="multiplier", std_value=0.05)
    want = ops.linearize_dark_ingest_frames(frames, stages, dark, dark_std, lut, "catmull", **kw)
    K = torch.full((3, 4), float("nan"), device=dev)
    got = ops.linearize_dark_ingest_frames_data(frames, stages, dark, dark_std, lut, "catmull", consts=K, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bool(torch.isfinite(got[0]).all())


@pytest.mark.parametrize("raw", [False, True], ids=["planar", "bgr"])
def test_out_buffers_and_views(dev, raw):
    """``out=`` slices of a larger buffer at a frame offset whose address is not 16-byte aligned, and ``consts`` rows of a larger
    buffer: the same bits as the whole stack gives, and nothing outside the slices is written."""
    from clair_torch_amd import ops
    n, c, h, w = 5, 3, 7, 9
    rng = np.random.default_rng(223)
    _, sd, _, dark, dark_std, lut = _scene(5, n, c, h, w)
    planar = _disjoint_frames(rng, n, (c, h, w), torch.uint16)
    layout = "nhwc_bgr" if raw else "nchw"
    frames = (_bgr(planar) if raw else planar).to(dev)
    sd, dark, dark_std, lut = sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    stages = _chains(torch.uint16, c)["per_channel_clamp_behind"]
    kw = dict(std_mode="multiplier", std_value=0.05, layout=layout)
    want, K = _four(frames, stages, layout, dark, dark_std, lut, "catmull", std_mode="multiplier", std_value=0.05)
    whole = ops.linearize_dark_ingest_frames_data(frames, stages, dark, dark_std, lut, "catmull", consts=K, **kw)
    assert torch.equal(whole[0], want[0]) and torch.equal(whole[1], want[1])
    big_lin, big_std = torch.full((n + 3, c, h, w), -1.0, device=dev), torch.full((n + 3, c, h, w), -1.0, device=dev)
    assert big_lin[2:].data_ptr() % 16 != 0 and big_std[2:].data_ptr() % 16 != 0      # 2 * 189 floats into the buffer
    big_K = torch.full((16, 4), float("nan"), device=dev)                              # a ring slot's constants
    ops.ingest_extrema_frames(frames, ops.data_stage_prefix(stages), layout, out=big_K[:n])
    got = ops.linearize_dark_ingest_frames_data(frames, stages, dark, dark_std, lut, "catmull", consts=big_K[:n],
                                                out=(big_lin[2:2 + n], big_std[2:2 + n]), **kw)
    assert got[0].data_ptr() == big_lin[2:].data_ptr() and got[1].data_ptr() == big_std[2:].data_ptr()
    assert torch.equal(big_lin[2:2 + n], whole[0]) and torch.equal(big_std[2:2 + n], whole[1])
    for big in (big_lin, big_std):
        assert bool((big[:2] == -1).all()) and bool((big[2 + n:] == -1).all())
    # a range of the frames with its rows of the constants, as the pipeline hands a run of matched frames over, with explicit
    # planar uncertainties
    big_lin.fill_(-1.0)
    big_std.fill_(-1.0)
    ops.linearize_dark_ingest_frames_data(frames[1:4], stages, dark[1:4], dark_std[1:4], lut, "linear", consts=big_K[1:4], std=sd[1:4],
                                          layout=layout, out=(big_lin[3:6], big_std[3:6]))
    want, _ = _four(frames, stages, layout, dark, dark_std, lut, "linear", std=sd)
    assert torch.equal(big_lin[3:6], want[0][1:4]) and torch.equal(big_std[3:6], want[1][1:4])
    for big in (big_lin, big_std):
        assert bool((big[:3] == -1).all()) and bool((big[6:] == -1).all())


def test_refusals_on_the_device(dev):
    """Everything below raises before any launch, with the exception types of linearize_dark_ingest_frames and
    linearize_ingest_frames(consts=)."""
    from clair_torch_amd import ops
    x, sd, _, dark, dark_std, lut = [v.to(dev) for v in _scene(2, 3, 3, 6, 5)]
    data = [("affine_data", 1, 0)]
    K = ops.ingest_extrema_frames(x)
    call = ops.linearize_dark_ingest_frames_data
    with pytest.raises(RuntimeError, match="does not require grad"):     # LOOKUP: sigma_eff always has the dark term
        call(x, data, dark, dark_std, lut, "lookup", consts=K, std=sd)
    with pytest.raises(ValueError):                                       # two data stages
        call(x, data * 2, dark, dark_std, lut, "linear", consts=K, std=sd)
    with pytest.raises(ValueError):
        call(x, data, dark, dark_std, lut, "linear", consts=K[:2], std=sd)
    with pytest.raises(ValueError):
        call(x, data, dark, dark_std, lut, "linear", consts=K[0], std=sd)
    with pytest.raises((ValueError, TypeError)):
        call(x, data, dark, dark_std, lut, "linear", consts=K.double(), std=sd)
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(x, data, dark, dark_std, lut, "linear", consts=K.cpu(), std=sd)
    with pytest.raises(ValueError, match="takes \\(B, H, W, 3\\) frames"):  # an interleaved layout with C != 3
        call(x, data, dark, dark_std, lut, "linear", consts=K, layout="nhwc_bgr")
    with pytest.raises(ValueError, match="mask_map batch dimension"):    # dark fields of another shape
        call(x, data, dark[:, :, :5], dark_std[:, :, :5], lut, "linear", consts=K, std=sd)
    with pytest.raises(ValueError, match="stage 0"):                      # the sibling still has no kernel for the stage
        ops.linearize_dark_ingest_frames(x, data, dark, dark_std, lut, "linear", std=sd)
    lin, std = torch.empty((3, 3, 6, 5), device=dev), torch.empty((3, 3, 6, 5), device=dev)
    got = call(x, data, dark, dark_std, lut, "linear", consts=K, std=sd, out=(lin, std))   # (the arguments above are otherwise fine)
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


def _same(a, b, nan_ok=()):
    """Equal tensors, dtypes, shapes and metas, frame by frame; for the frames in ``nan_ok`` NaNs at the same places and equal
    values elsewhere."""
    assert len(a) == len(b)
    for k, ((la, sa, ma), (lb, sb, mb)) in enumerate(zip(a, b)):
        if k in nan_ok:
            for ta, tb in ((la, lb), (sa, sb)):
                assert torch.equal(torch.isnan(ta), torch.isnan(tb)) and torch.equal(torch.nan_to_num(ta), torch.nan_to_num(tb)), k
        else:
            assert torch.equal(la, lb) and torch.equal(sa, sb), k
        assert la.shape == lb.shape and la.dtype == lb.dtype and sa.shape == sb.shape and sa.dtype == sb.dtype, k
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


def _loader(values, times):
    from clair_torch_amd.common.enums import MissingStdMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    ds = StackDataset(values, times, missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
    return DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)


def _case(dev, raw):
    """50 uint16 frames, MULTIPLIER uncertainties derived in the kernel, batch size 1: more than three groups of 16, so ring
    slots are re-used.  Planar 3x6x5 frames behind [CastTo, Normalize()], or 6x5x3 BGR frames behind CvToTorch + that pair; every
    frame has extrema of its own (the exposure series).  ``loader_with(frame)``: the same run with that frame constant."""
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.common.transforms import CastTo, CvToTorch, Normalize
    from clair_torch_amd.models import ICRFModelDirect
    x, _, t, dark, dark_std, lut = _scene(43 if raw else 41, 50, 3, 6, 5)
    codes, _ = _as_dtype(x, torch.uint16)

    def loader_with(constant=None):
        values = codes.clone()
        if constant is not None:
            values[constant] = 777
        return _loader(_bgr(values) if raw else values, t.tolist())

    models = {m: ICRFModelDirect(icrf=lut, interpolation_mode=InterpMode[m.upper()]).to(dev) for m in ("linear", "catmull", "lookup")}
    tf = ([CvToTorch()] if raw else []) + [CastTo("float32"), Normalize()]
    return dict(loader=loader_with(), loader_with=loader_with, models=models, dark=dark, dark_std=dark_std, kw=dict(gpu_transforms=tf))


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
            want = _run(loader, model, dark_field_dataset=art, fused_dark_ingest_data=False, **kw, **extra)
            got = _run(loader, model, dark_field_dataset=art, fused_dark_ingest_data=True, **kw, **extra)
            assert len(got) == n and tuple(got[0][0].shape) == ((6, 5, 3) if extra.get("output_layout") else (3, 6, 5))
            _same(got, want)
            if not extra:
                plain[mode] = want
    model = case["models"]["linear"]
    assert any(not torch.equal(plain["linear"][k][0], plain["catmull"][k][0]) for k in range(n))
    # a dark field for some frames only: runs of matched and unmatched frames inside the groups 0, 1 and 3; group 2, frames
    # 32 to 47, wholly unmatched
    some = set(list(range(5)) + [9] + list(range(20, 32)) + [49])
    ds_some = _MatchesSome(art, some)
    want = _run(loader, model, dark_field_dataset=ds_some, fused_dark_ingest_data=False, **kw)
    got = _run(loader, model, dark_field_dataset=ds_some, fused_dark_ingest_data=True, **kw)
    _same(got, want)
    bare = _run(loader, model, **kw)      # no dark dataset at all
    for k in range(n):
        ref = plain["linear"] if k in some else bare
        assert torch.equal(got[k][0], ref[k][0]) and torch.equal(got[k][1], ref[k][1]), k
    assert all(not torch.equal(plain["linear"][k][0], bare[k][0]) for k in range(n))   # (the correction matters here)
    # ... and with a flat field applied inside the launches of the unmatched runs (fused_flat), behind those of the matched ones
    want = _run(loader, model, dark_field_dataset=ds_some, flatfield_dataset=flat, fused_dark_ingest_data=False, **kw)
    got = _run(loader, model, dark_field_dataset=ds_some, flatfield_dataset=flat, fused_flat=True, fused_dark_ingest_data=True, **kw)
    _same(got, want)
    # two dark fields alternating by frame parity: the cache and the per-frame pointers
    parity = _ByParity(art, ArtefactStack(case["dark"][1], case["dark_std"][1]))
    want = _run(loader, model, dark_field_dataset=parity, fused_dark_ingest_data=False, **kw)
    got = _run(loader, model, dark_field_dataset=parity, fused_dark_ingest_data=True, **kw)
    _same(got, want)
    assert torch.equal(got[0][0], plain["linear"][0][0]) and not torch.equal(got[1][0], plain["linear"][1][0])

    # which route ran: the blur kernel of the frame-by-frame route is never called by the fused one
    def no_blur(*args, **kwargs):
        raise AssertionError("ct_dark_field_blur ran: the frame went frame by frame")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "dark_field_blur", no_blur)
        _same(_run(loader, model, dark_field_dataset=art, fused_dark_ingest_data=True, **kw), plain["linear"])
        with pytest.raises(AssertionError, match="frame by frame"):
            _run(loader, model, dark_field_dataset=art, fused_dark_ingest_data=False, **kw)
        with pytest.raises(AssertionError, match="frame by frame"):      # the default
            _run(loader, model, dark_field_dataset=art, **kw)
        with pytest.raises(AssertionError, match="frame by frame"):      # the keyword is read only with fused_dark=True ...
            _run(loader, model, dark_field_dataset=art, fused_dark=False, fused_dark_ingest_data=True, **kw)
        with pytest.raises(AssertionError, match="frame by frame"):      # ... and fused_dark_ingest=True
            _run(loader, model, dark_field_dataset=art, fused_dark_ingest=False, fused_dark_ingest_data=True, **kw)

    # ... and the fused front is the one that ran: matched runs there, unmatched ones through linearize_ingest_frames(consts=)
    seen = []
    fused, unmatched = ops.linearize_dark_ingest_frames_data, ops.linearize_ingest_frames
    with monkeypatch.context() as mp:
        mp.setattr(ops, "linearize_dark_ingest_frames_data", lambda f, *a, **k: (seen.append(("dark", f.shape[0])), fused(f, *a, **k))[1])
        mp.setattr(ops, "linearize_ingest_frames", lambda f, *a, **k: (seen.append(("plain", f.shape[0], k["consts"] is not None)),
                                                                       unmatched(f, *a, **k))[1])
        _run(loader, model, dark_field_dataset=ds_some, fused_dark_ingest_data=True, **kw)
    assert seen == [("dark", 5), ("plain", 4, True), ("dark", 1), ("plain", 6, True), ("plain", 4, True), ("dark", 12), ("plain", 16, True),
                    ("plain", 1, True), ("dark", 1)]


@pytest.mark.parametrize("case_name", ["planar_case", "bgr_case"])
def test_generator_errors_surface_where_the_frame_by_frame_route_raises(dev, case_name, request):
    from clair_torch_amd import ops
    from clair_torch_amd.datasets import ArtefactStack
    case = request.getfixturevalue(case_name)
    loader, kw, model = case["loader"], case["kw"], case["models"]["linear"]
    art = ArtefactStack(case["dark"][0], case["dark_std"][0])
    full = _run(loader, model, dark_field_dataset=art, fused_dark_ingest_data=False, **kw)
    assert len(full) == 50
    # frame 5, and frame 16: the first of the second group
    for frame in (5, 16):
        constant = case["loader_with"](frame)
        for flag in (True, False):
            # a frame of constant value: exactly the frames in front, then the reference's ValueError
            got, err = _collect_until_error(constant, model, dark_field_dataset=art, fused_dark_ingest_data=flag, **kw)
            assert isinstance(err, ValueError) and str(err) == ops.ZERO_RANGE and len(got) == frame, (frame, flag, err)
            _same(got, full[:frame])
            # no dark std for that frame: AttributeError
            got, err = _collect_until_error(loader, model, dark_field_dataset=_NoStdAt(art, frame), fused_dark_ingest_data=flag, **kw)
            assert isinstance(err, AttributeError) and len(got) == frame, (frame, flag, err)
            _same(got, full[:frame])
            # both in one frame: it is staged before it is matched, so the zero range wins
            got, err = _collect_until_error(constant, model, dark_field_dataset=_NoStdAt(art, frame), fused_dark_ingest_data=flag, **kw)
            assert isinstance(err, ValueError) and str(err) == ops.ZERO_RANGE and len(got) == frame, (frame, flag, err)
            _same(got, full[:frame])
            # a constant frame BEHIND the one without a dark std is never reached
            got, err = _collect_until_error(case["loader_with"](frame + 2), model, dark_field_dataset=_NoStdAt(art, frame),
                                            fused_dark_ingest_data=flag, **kw)
            assert isinstance(err, AttributeError) and len(got) == frame, (frame, flag, err)
    # LOOKUP stays frame by frame and raises there, at the first frame
    for flag in (True, False):
        got, err = _collect_until_error(loader, case["models"]["lookup"], dark_field_dataset=art, fused_dark_ingest_data=flag, **kw)
        assert isinstance(err, RuntimeError) and "does not require grad" in str(err) and got == []


def test_a_nan_frame_raises_nothing(dev):
    """float32 frames behind [Normalize()], frame 5 of 20 holds one NaN: its range is NaN, which is no zero -- nothing is raised,
    NaN comes out for that frame only and the other frames are those of the clean run, on both routes."""
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.common.transforms import Normalize
    from clair_torch_amd.datasets import ArtefactStack
    from clair_torch_amd.models import ICRFModelDirect
    x, _, t, dark, dark_std, lut = _scene(47, 20, 3, 6, 5)
    model = ICRFModelDirect(icrf=lut, interpolation_mode=InterpMode.LINEAR).to(dev)
    art = ArtefactStack(dark[0], dark_std[0])
    dirty = x.clone()
    dirty[5, 1, 2, 3] = float("nan")
    kw = dict(gpu_transforms=[Normalize()], dark_field_dataset=art)
    clean = _run(_loader(x, t.tolist()), model, fused_dark_ingest_data=False, **kw)
    runs = {}
    for flag in (True, False):
        got, err = _collect_until_error(_loader(dirty, t.tolist()), model, fused_dark_ingest_data=flag, **kw)
        assert err is None and len(got) == 20, (flag, err)
        runs[flag] = got
        for k in range(20):
            assert bool(torch.isnan(got[k][1]).any()) == (k == 5), (flag, k)
            if k != 5:
                assert torch.equal(got[k][0], clean[k][0]) and torch.equal(got[k][1], clean[k][1]), (flag, k)
    _same(runs[True], runs[False], nan_ok=(5,))
    assert bool(torch.isnan(runs[True][5][1]).all())      # every pixel of the frame is NaN behind the chain
