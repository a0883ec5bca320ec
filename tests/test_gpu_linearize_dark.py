"""ct_linearize_dark on the device: the dark-field conditional blur and the ICRF linearization of independent frames in one
pass.  Its specification is one sentence -- for every frame the outputs are bit for bit those of ct_dark_field_blur on it as a
batch of one followed by ct_linearize_std on (xb, sigma_eff) -- so nearly everything here is torch.equal against that pair,
through ops.linearize_dark_frames and through linearize_dataset_generator(fused_dark=True / False); the generator is also held
against the eager restatement of the reference (oracle/eager_torch.py) at the tolerances of test_gpu_darkfield.py."""
import functools

import pytest
import torch
from torch.utils.data import DataLoader

from _dark_cases import as_dtype as _as_dtype, scene
from _util import assert_parity

_scene = functools.partial(scene, period=8)     # 17 and 50 frames: the exposure times start over every 8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _pair(frames, darks, dark_stds, lut, interp, *, std=None, **kw):
    """The two launches the fused kernel replaces, frame by frame."""
    from clair_torch_amd import ops
    lins, sds = [], []
    for k in range(frames.shape[0]):
        xb, sig = ops.dark_field_blur(frames[k][None], darks[k][None], dark_stds[k][None], std=None if std is None else std[k][None], **kw)
        lin, sd = ops.linearize_frames(xb, lut, interp, std=sig)
        lins.append(lin)
        sds.append(sd)
    return torch.cat(lins), torch.cat(sds)


STDS = ["explicit", "constant", "multiplier"]


def _src(std_mode, sd):
    return dict(std=sd) if std_mode == "explicit" else dict(std_mode=std_mode, std_value=0.01 if std_mode == "constant" else 0.05)


# (3,3,13,9): rows end inside a thread's group and the plane (117) is no multiple of it; (2,3,2,2): both reflections fold onto
# one row and column; (1,1,5,6): a single frame and channel; (5,2,3,130): more than one wavefront per row, a 2-column tail;
# (17,1,2,3): the 16-frame launch boundary; (2,1,2,4): a row of exactly one full group, whose right tap is the reflected W - 2;
# (1,2,3,8): full groups only, the last one at the right border; (2,1,3,5): one group and a one-element tail whose left tap lies
# in the group
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint16, torch.uint8], ids=["f32", "u16", "u8"])
@pytest.mark.parametrize("shape", [(3, 3, 13, 9), (2, 3, 2, 2), (1, 1, 5, 6), (5, 2, 3, 130), (17, 1, 2, 3), (2, 1, 2, 4), (1, 2, 3, 8), (2, 1, 3, 5)],
                         ids=lambda s: "x".join(map(str, s)))
def test_bit_equal_to_the_pair(dev, shape, dtype):
    from clair_torch_amd import ops
    n, c, h, w = shape
    x, sd, _, dark, dark_std, lut = _scene(11 + h, n, c, h, w)
    frames, max_code = _as_dtype(x, dtype)
    frames, sd, dark, dark_std, lut = frames.to(dev), sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    shared = [0] * n if n < 3 else [0, 1, 1] + list(range(3, n))       # frames 1 and 2 share one dark tensor
    for std_mode in STDS:
        src = _src(std_mode, sd)
        for interp in ("linear", "catmull"):
            want = _pair(frames, dark, dark_std, lut, interp, max_code=max_code, **src)
            assert bool(torch.isfinite(want[1]).all())
            # a distinct dark field per frame as a list of (C,H,W) tensors, and the (F,C,H,W) tensor form
            got = ops.linearize_dark_frames(frames, list(dark), list(dark_std), lut, interp, max_code=max_code, **src)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (std_mode, interp, "list")
            got = ops.linearize_dark_frames(frames, dark, dark_std, lut, interp, max_code=max_code, **src)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (std_mode, interp, "tensor")
        # a list in which frames share one dark tensor, (1,C,H,W) entries
        dl, sl = [dark[k][None] for k in range(n)], [dark_std[k][None] for k in range(n)]
        want = _pair(frames, dark[shared], dark_std[shared], lut, "linear", max_code=max_code, **src)
        got = ops.linearize_dark_frames(frames, [dl[k] for k in shared], [sl[k] for k in shared], lut, "linear", max_code=max_code, **src)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (std_mode, "shared")
    # no uncertainty of the raw image: sigma_eff is the dark term alone; no LUT: the identity model
    for lut_k, interp in ((lut, "linear"), (None, None)):
        want = _pair(frames, dark, dark_std, lut_k, interp, max_code=max_code)
        got = ops.linearize_dark_frames(frames, dark, dark_std, lut_k, interp, max_code=max_code)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if n > 1:     # the dark fields do differ between the frames (guards the test)
        straight = ops.linearize_dark_frames(frames, dark, dark_std, lut, "linear", max_code=max_code)
        swapped = ops.linearize_dark_frames(frames, dark.flip(0), dark_std.flip(0), lut, "linear", max_code=max_code)
        assert not torch.equal(swapped[0], straight[0]) and not torch.equal(swapped[1], straight[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint16], ids=["f32", "u16"])
def test_out_buffers_and_frame_views(dev, dtype):
    """``out=`` is written in place; frames that are a view of a larger buffer (image_stride larger than a frame) are read in
    place and give the same bits."""
    from clair_torch_amd import ops
    n, c, h, w = 5, 3, 7, 10
    x, sd, _, dark, dark_std, lut = _scene(5, n, c, h, w)
    frames, max_code = _as_dtype(x, dtype)
    frames, sd, dark, dark_std, lut = frames.to(dev), sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    kw = dict(std_mode="multiplier", std_value=0.05, max_code=max_code)
    want = _pair(frames, dark, dark_std, lut, "catmull", **kw)
    lin, std = torch.full((n, c, h, w), -1.0, device=dev), torch.full((n, c, h, w), -1.0, device=dev)
    got = ops.linearize_dark_frames(frames, dark, dark_std, lut, "catmull", out=(lin, std), **kw)
    assert got[0].data_ptr() == lin.data_ptr() and got[1].data_ptr() == std.data_ptr()
    assert torch.equal(lin, want[0]) and torch.equal(std, want[1])
    # slices of larger output buffers, as the pipeline's ring slots hand them over
    big_lin, big_std = torch.full((n + 3, c, h, w), -1.0, device=dev), torch.full((n + 3, c, h, w), -1.0, device=dev)
    ops.linearize_dark_frames(frames, dark, dark_std, lut, "catmull", out=(big_lin[2:2 + n], big_std[2:2 + n]), **kw)
    assert torch.equal(big_lin[2:2 + n], want[0]) and torch.equal(big_std[2:2 + n], want[1])
    assert bool((big_lin[:2] == -1).all()) and bool((big_lin[2 + n:] == -1).all()) and bool((big_std[2 + n:] == -1).all())
    # frames 2 * C*H*W + 8 elements apart, the first one 3 elements into its buffer (element-aligned only)
    wide = torch.zeros((n, 2 * c * h * w + 8), dtype=frames.dtype, device=dev)
    view = wide[:, 3:3 + c * h * w].view(n, c, h, w)
    view.copy_(frames)
    assert view.stride(0) == 2 * c * h * w + 8 and not view.is_contiguous()
    got = ops.linearize_dark_frames(view, dark, dark_std, lut, "catmull", **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    got = ops.linearize_dark_frames(view, dark, dark_std, lut, "linear", std=sd, max_code=max_code)   # explicit std: dense copies
    want = _pair(frames, dark, dark_std, lut, "linear", std=sd, max_code=max_code)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError, match="contiguous float32 tensor of shape"):
        ops.linearize_dark_frames(frames, dark, dark_std, lut, "linear", out=(lin[:, :, :, :5], std), **kw)
    with pytest.raises(ValueError):
        ops.linearize_dark_frames(frames, dark, dark_std, lut, "linear", out=(lin, None), **kw)


def test_refusals_on_the_device(dev):
    """The exceptions of the two fronts it replaces."""
    from clair_torch_amd import ops
    x, sd, _, dark, dark_std, lut = [v.to(dev) for v in _scene(2, 3, 3, 6, 5)]
    with pytest.raises(RuntimeError, match="does not require grad"):     # LOOKUP with uncertainties
        ops.linearize_dark_frames(x, dark, dark_std, lut, "lookup", std=sd)
    with pytest.raises(RuntimeError, match="does not require grad"):     # ... which the dark term always brings
        ops.linearize_dark_frames(x, dark, dark_std, lut, "lookup")
    with pytest.raises(ValueError, match="mask_map batch dimension"):    # a dark field of another shape
        ops.linearize_dark_frames(x, dark[:, :, :5], dark_std[:, :, :5], lut, "linear", std=sd)
    with pytest.raises(ValueError, match="mask_map batch dimension"):
        ops.linearize_dark_frames(x, [dark[0], dark[1], dark[2, :2]], list(dark_std), lut, "linear", std=sd)
    with pytest.raises(ValueError, match="dark_std shape"):
        ops.linearize_dark_frames(x, dark, dark_std[:, :, :, :4], lut, "linear", std=sd)
    with pytest.raises(ValueError, match="dark_stds is required"):       # a missing dark std
        ops.linearize_dark_frames(x, dark, None, lut, "linear", std=sd)
    with pytest.raises(TypeError):
        ops.linearize_dark_frames(x, list(dark), [dark_std[0], None, dark_std[2]], lut, "linear", std=sd)
    with pytest.raises(ValueError, match="std shape"):                   # _explicit_std
        ops.linearize_dark_frames(x, dark, dark_std, lut, "linear", std=sd[:2])
    with pytest.raises(ValueError, match="lut must be"):
        ops.linearize_dark_frames(x, dark, dark_std, lut[:2], "linear", std=sd)
    with pytest.raises(ValueError):       # the blur reflects: two columns at least (CT_ERR_INVALID_ARGUMENT)
        ops.linearize_dark_frames(x[:, :, :, :1].contiguous(), dark[:, :, :, :1].contiguous(), dark_std[:, :, :, :1].contiguous(), lut,
                                  "linear")


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


@pytest.fixture(scope="module")
def codes_case(dev):
    """50 frames of 3x6x5 uint16 behind CastTo + Normalize(65535, 0), MULTIPLIER uncertainties derived in the kernel, batch
    size 1: more than three groups of 16, so ring slots are re-used."""
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, Normalize
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.models import ICRFModelDirect
    x, _, t, dark, dark_std, lut = _scene(41, 50, 3, 6, 5)
    codes, _ = _as_dtype(x, torch.uint16)
    ds = StackDataset(codes, t.tolist(), missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
    loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
    models = {m: ICRFModelDirect(icrf=lut, interpolation_mode=InterpMode[m.upper()]).to(dev) for m in ("linear", "catmull", "lookup")}
    return dict(loader=loader, models=models, dark=dark, dark_std=dark_std, lut=lut, codes=codes, t=t,
                kw=dict(gpu_transforms=[CastTo("float32"), Normalize(65535, 0)]))


@pytest.fixture(scope="module")
def pixels_case(dev):
    """20 float32 frames with explicit uncertainty images, no transform list."""
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.datasets import StackDataset, custom_collate
    from clair_torch_amd.models import ICRFModelDirect
    x, sd, t, dark, dark_std, lut = _scene(42, 20, 3, 6, 5)
    loader = DataLoader(StackDataset(x, t.tolist(), stds=sd), batch_size=1, shuffle=False, collate_fn=custom_collate)
    models = {m: ICRFModelDirect(icrf=lut, interpolation_mode=InterpMode[m.upper()]).to(dev) for m in ("linear", "catmull")}
    return dict(loader=loader, models=models, dark=dark, dark_std=dark_std, lut=lut, x=x, sd=sd, kw={})


@pytest.mark.parametrize("case_name", ["codes_case", "pixels_case"])
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
            want = _run(loader, model, dark_field_dataset=art, fused_dark=False, **kw, **extra)
            got = _run(loader, model, dark_field_dataset=art, fused_dark=True, **kw, **extra)
            assert len(got) == n
            _same(got, want)
            if not extra:
                plain[mode] = want
    model = case["models"]["linear"]
    # a dark field for some frames only: runs of matched and unmatched frames inside the groups, a whole unmatched group
    some = {k for k in (list(range(5)) + [9] + list(range(20, 37)) + [49]) if k < n}
    ds_some = _MatchesSome(art, some)
    want = _run(loader, model, dark_field_dataset=ds_some, fused_dark=False, **kw)
    got = _run(loader, model, dark_field_dataset=ds_some, fused_dark=True, **kw)
    _same(got, want)
    bare = _run(loader, model, **kw)      # no dark dataset at all
    for k in range(n):
        ref = plain["linear"] if k in some else bare
        assert torch.equal(got[k][0], ref[k][0]) and torch.equal(got[k][1], ref[k][1]), k
    assert any(not torch.equal(plain["linear"][k][0], bare[k][0]) for k in range(n))   # (the correction matters here)
    # two dark fields alternating by frame parity: the cache and the per-frame pointers
    parity = _ByParity(art, ArtefactStack(case["dark"][1], case["dark_std"][1]))
    want = _run(loader, model, dark_field_dataset=parity, fused_dark=False, **kw)
    got = _run(loader, model, dark_field_dataset=parity, fused_dark=True, **kw)
    _same(got, want)
    assert torch.equal(got[0][0], plain["linear"][0][0]) and not torch.equal(got[1][0], plain["linear"][1][0])

    # the fused route is the one that ran: the blur kernel of the pair route is never called
    def no_blur(*args, **kwargs):
        raise AssertionError("ct_dark_field_blur ran: the frame took the pair route")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "dark_field_blur", no_blur)
        _same(_run(loader, model, dark_field_dataset=art, fused_dark=True, **kw), plain["linear"])
        with pytest.raises(AssertionError, match="pair route"):
            _run(loader, model, dark_field_dataset=art, fused_dark=False, **kw)


def test_generator_errors_surface_where_the_pair_route_raises(dev, codes_case, pixels_case):
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    loader, kw, model = codes_case["loader"], codes_case["kw"], codes_case["models"]["linear"]
    art = ArtefactStack(codes_case["dark"][0], codes_case["dark_std"][0])
    full = _run(loader, model, dark_field_dataset=art, fused_dark=False, **kw)
    # no dark std for frame 5 only: exactly frames 0..4, then AttributeError
    for flag in (True, False):
        got, err = _collect_until_error(loader, model, dark_field_dataset=_NoStdAt(art, 5), fused_dark=flag, **kw)
        assert isinstance(err, AttributeError) and len(got) == 5, (flag, err)
        _same(got, full[:5])
    # ... and for frame 16, the first of the second group
    got, err = _collect_until_error(loader, model, dark_field_dataset=_NoStdAt(art, 16), fused_dark=True, **kw)
    assert isinstance(err, AttributeError) and len(got) == 16
    _same(got, full[:16])
    # a main dataset without uncertainties: RuntimeError at the first matched frame (frame 3 here)
    bare = DataLoader(StackDataset(pixels_case["x"], [1.0] * 20), batch_size=1, shuffle=False, collate_fn=custom_collate)
    pmodel = pixels_case["models"]["linear"]
    part = _MatchesSome(ArtefactStack(pixels_case["dark"][0], pixels_case["dark_std"][0]), range(3, 20))
    seen = []
    for flag in (True, False):
        got, err = _collect_until_error(bare, pmodel, dark_field_dataset=part, fused_dark=flag)
        assert isinstance(err, RuntimeError) and "does not require grad" in str(err) and len(got) == 3, (flag, err)
        seen.append(got)
    _same(*seen)
    # LOOKUP stays frame by frame and raises there, at the first frame
    for flag in (True, False):
        got, err = _collect_until_error(loader, codes_case["models"]["lookup"], dark_field_dataset=art, fused_dark=flag, **kw)
        assert isinstance(err, RuntimeError) and "does not require grad" in str(err) and got == []


def test_black_level_chain_stays_frame_by_frame(dev, codes_case, monkeypatch):
    """A list ``fuses_with_linearize`` declines (route "ingest") with a dark field: today's route and result, whatever
    ``fused_dark`` says."""
    from clair_torch_amd import ops
    from clair_torch_amd.common.transforms import CastTo, Normalize
    from clair_torch_amd.datasets import ArtefactStack
    loader, model = codes_case["loader"], codes_case["models"]["linear"]
    art = ArtefactStack(codes_case["dark"][0], codes_case["dark_std"][0])
    kw = dict(gpu_transforms=[CastTo("float32"), Normalize(65535, 64)], dark_field_dataset=art)
    want = _run(loader, model, fused_dark=False, **kw)

    def no_fused(*args, **kwargs):
        raise AssertionError("ct_linearize_dark ran")

    monkeypatch.setattr(ops, "linearize_dark_frames", no_fused)
    _same(_run(loader, model, fused_dark=True, **kw), want)
    with pytest.raises(AssertionError, match="ct_linearize_dark ran"):      # (the patch does bite on the code pair)
        _run(loader, model, fused_dark=True, dark_field_dataset=art, **codes_case["kw"])


def test_fused_generator_against_the_eager_restatement(dev, pixels_case):
    """LINEAR only, at the tolerances tests/test_gpu_darkfield.py::test_linearize_generator_with_dark_field applies to the pair
    route (the fused route is bit-equal to it, so no new tolerance is introduced; CATMULL is held by bit-equality alone)."""
    from clair_torch_amd.datasets import ArtefactStack
    from oracle import eager_torch as oe
    x, sd, lut, dark, dark_std = (pixels_case[k] for k in ("x", "sd", "lut", "dark", "dark_std"))
    got = _run(pixels_case["loader"], pixels_case["models"]["linear"], dark_field_dataset=ArtefactStack(dark[0], dark_std[0]), fused_dark=True)
    assert len(got) == 20
    for k, (lin, lsd, _) in enumerate(got):
        lin_o, sd_o = oe.linearize_frame_dark(x[k], sd[k], lut, dark[0], dark_std[0], "linear")
        assert_parity(lin.numpy(), lin_o.numpy(), rtol=1e-5, norm_tol=1e-6, what="fused dark-field linearize value")
        assert_parity(lsd.numpy(), sd_o.numpy(), rtol=1e-5, norm_tol=1e-6, what="fused dark-field linearize std")
