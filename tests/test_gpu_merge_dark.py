"""ct_hdr_merge_dark_batch on the device: the dark-field conditional blur and one batch of the HDR merge in one pass.  Its
specification is one sentence -- state and outputs are bit for bit those of ct_dark_field_blur into float32 stacks followed
by ct_hdr_merge_batch on them (closed form) -- so nearly everything here is torch.equal against that pair; the public API is
also held against the eager restatement of the reference (oracle/eager_torch.py) at the tolerances of test_gpu_darkfield.py."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from _dark_cases import as_dtype as _as_dtype, scene as _scene
from _util import assert_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _pair(stack, t, dark, dark_std, *, std=None, std_mode="none", std_value=0.0, max_code=None, tile=None, halo=None, **merge):
    """The two launches the fused kernel replaces."""
    from clair_torch_amd import ops
    xb, sig = ops.dark_field_blur(stack, dark, dark_std, std=std, std_mode=std_mode, std_value=std_value, max_code=max_code,
                                  tile=tile, halo=halo)
    return ops.hdr_merge_batch(xb, t, std=sig, tile=tile, reference_order=False, **merge)


def _fused(stack, t, dark, dark_std, **kw):
    from clair_torch_amd import ops
    return ops.hdr_merge_dark_batch(stack, t, dark, dark_std, reference_order=False, **kw)


def _same_state(a, b):
    return torch.equal(a.mean, b.mean) and torch.equal(a.sumw, b.sumw) and (a.var is None or torch.equal(a.var, b.var))


MODES = [(None, False), (None, True), ("linear", False), ("linear", True), ("catmull", False), ("catmull", True), ("lookup", True)]
STDS = ["explicit", "constant", "multiplier"]


# (4,3,13,9): rows end inside a thread's group and the plane (117) is no multiple of it; (3,3,2,2): both reflections fold
# onto the same column and row; (1,1,5,6): B = 1, probe 0; (5,2,3,130): more than one wavefront per row band, a 2-column tail;
# (2,1,2,4): a row of exactly one full group, whose right tap is the reflected W - 2, B = 2 so the probe is exposure 1;
# (2,2,3,8): full groups only, the last one at the right border; (2,1,3,5): one group and a one-element tail whose left tap lies
# in the group
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint16, torch.uint8], ids=["f32", "u16", "u8"])
@pytest.mark.parametrize("shape", [(4, 3, 13, 9), (3, 3, 2, 2), (1, 1, 5, 6), (5, 2, 3, 130), (2, 1, 2, 4), (2, 2, 3, 8), (2, 1, 3, 5)],
                         ids=lambda s: "x".join(map(str, s)))
def test_bit_equal_to_the_pair(dev, shape, dtype):
    from clair_torch_amd import ops
    n, c, h, w = shape
    x, sd, t, dark, dark_std, lut = _scene(11 + h, n, c, h, w)
    stack, max_code = _as_dtype(x, dtype)
    stack, sd, dark, dark_std, lut = stack.to(dev), sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    checked = 0
    for std_mode in STDS:
        src = dict(std=sd) if std_mode == "explicit" else dict(std_mode=std_mode, std_value=0.01 if std_mode == "constant" else 0.05)
        for interp, gauss in MODES:
            for mean_dtype in (torch.float64, torch.float32):
                kw = dict(lut=None if interp is None else lut, interp=interp, gaussian_weight=gauss, mean_dtype=mean_dtype, max_code=max_code,
                          **src)
                st_a, st_b = ops.MergeState((c, h, w), dev, True), ops.MergeState((c, h, w), dev, True)
                # (finalize on a state: outputs AND every state array are written)
                want = _pair(stack, t, dark, dark_std, state=st_a, finalize=True, **{k: v for k, v in kw.items()})
                got = _fused(stack, t, dark, dark_std, state=st_b, finalize=True, **kw)
                what = (std_mode, interp, gauss, mean_dtype)
                assert got[0].dtype == mean_dtype and torch.equal(got[0], want[0]), what
                assert torch.equal(got[1], want[1]) and bool(torch.isfinite(got[1]).all()), what
                assert _same_state(st_b, st_a), what
                checked += 1
    assert checked == len(STDS) * len(MODES) * 2
    # without a state (one batch, first and final) the same outputs
    want = _pair(stack, t, dark, dark_std, lut=lut, interp="linear", gaussian_weight=True, max_code=max_code, std=sd)
    got = _fused(stack, t, dark, dark_std, lut=lut, interp="linear", gaussian_weight=True, max_code=max_code, std=sd)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # no uncertainty of the raw image: sigma_eff is the dark term alone
    want = _pair(stack, t, dark, dark_std, lut=lut, interp="linear", gaussian_weight=True, max_code=max_code)
    got = _fused(stack, t, dark, dark_std, lut=lut, interp="linear", gaussian_weight=True, max_code=max_code)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # no dark std: nothing is propagated, as the pair without one (one shared dark field is then allowed)
    for dk in (dark, dark[:1]):
        want = _pair(stack, t, dk, None, lut=lut, interp="catmull", gaussian_weight=True, max_code=max_code)
        got = _fused(stack, t, dk, None, lut=lut, interp="catmull", gaussian_weight=True, max_code=max_code)
        assert want[1] is None and got[1] is None and torch.equal(got[0], want[0])


def test_refusals_on_the_device(dev):
    """The exceptions of the two fronts it replaces."""
    from clair_torch_amd import _native as nv
    from clair_torch_amd import ops
    x, sd, t, dark, dark_std, lut = [v.to(dev) if i != 2 else v for i, v in enumerate(_scene(2, 3, 3, 6, 5))]
    kw = dict(lut=lut, interp="linear", std=sd)
    with pytest.raises(NotImplementedError, match="shared dark field"):
        ops.hdr_merge_dark_batch(x, t, dark[:1], dark_std[:1], **kw)
    with pytest.raises(ValueError, match="mask_map batch dimension"):
        ops.hdr_merge_dark_batch(x, t, dark[:2], dark_std[:2], **kw)
    with pytest.raises(ValueError, match="dark_std shape"):
        ops.hdr_merge_dark_batch(x, t, dark, dark_std[:, :, :3], **kw)
    with pytest.raises(ValueError, match="halo must be"):
        ops.hdr_merge_dark_batch(x, t, dark, dark_std, halo=torch.zeros((3, 3, 2, 4), device=dev), **kw)
    with pytest.raises(ValueError):       # a band without its halo (CT_ERR_INVALID_ARGUMENT)
        ops.hdr_merge_dark_batch(x, t, dark, dark_std, tile=ops.TileGeometry(h_global=20, row_offset=6), **kw)
    with pytest.raises(ValueError, match="exposure times"):
        ops.hdr_merge_dark_batch(x, t[:2], dark, dark_std, **kw)
    with pytest.raises(ValueError, match="needs a MergeState"):
        ops.hdr_merge_dark_batch(x, t, dark, dark_std, finalize=False, **kw)
    with pytest.raises(ValueError, match="without a variance buffer"):
        ops.hdr_merge_dark_batch(x, t, dark, dark_std, state=ops.MergeState((3, 6, 5), dev, False), **kw)
    with pytest.raises(RuntimeError, match="does not require grad"):     # LOOKUP, unit weights, uncertainties
        ops.hdr_merge_dark_batch(x, t, dark, dark_std, lut=lut, interp="lookup", gaussian_weight=False, std=sd, reference_order=False)
    for ro, interp in ((True, "linear"), (None, "catmull"), (None, "lookup")):   # the reference-order kernel is not fused
        with pytest.raises(nv.NativeLibraryError):
            ops.hdr_merge_dark_batch(x, t, dark, dark_std, lut=lut, interp=interp, std=sd, reference_order=ro)


def test_streaming_alternates_with_the_pair(dev):
    """Three batches [4, 2, 3] on one MergeState: fused and unfused batches in any alternation leave the pair's state and
    result, after every batch."""
    from clair_torch_amd import ops
    n, c, h, w = 9, 3, 7, 11
    x, sd, t, dark, dark_std, lut = _scene(21, n, c, h, w)
    stack, max_code = _as_dtype(x, torch.uint16)
    stack, sd, dark, dark_std, lut = stack.to(dev), sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    cuts = [(0, 4), (4, 6), (6, 9)]
    for interp, gauss in (("linear", True), ("catmull", True), (None, False)):
        kw = dict(lut=None if interp is None else lut, interp=interp, gaussian_weight=gauss, max_code=max_code)
        for routes in ((_fused, _pair, _fused), (_pair, _fused, _pair), (_fused, _fused, _fused)):
            st_a, st_b = ops.MergeState((c, h, w), dev, True), ops.MergeState((c, h, w), dev, True)
            for (a, b), route in zip(cuts, routes):
                args = (stack[a:b], t[a:b], dark[a:b], dark_std[a:b])
                want = _pair(*args, std=sd[a:b], state=st_a, finalize=b == n, **kw)
                got = route(*args, std=sd[a:b], state=st_b, finalize=b == n, **kw)
                assert _same_state(st_b, st_a) and st_b.batches == st_a.batches, (interp, a, b)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), interp


def _condition_ratio(xb, sig, t, lut):
    """Host evidence that a first batch trips the conditioning test of the pivoted float32 moments (LINEAR, Gaussian weights,
    explicit sigma): per element (t1 + |t2| + t3) / (t1 + t2 + t3) of the kernels' epilogue in float64, with the pivot from
    exposure B / 2.  The kernels repeat the batch where it exceeds kPivotCondLimit = 8."""
    b, c, h, w = xb.shape
    x, lut = xb.astype(np.float64), lut.astype(np.float64)
    top = lut.shape[1] - 1
    row = (np.arange(c * h * w).reshape(c, h, w) % c)[None].repeat(b, 0)   # the reference's flat index modulo C
    sraw = x * top
    ok = (sraw >= 0) & (sraw <= top)
    s = np.clip(sraw, 0, top)
    i0 = np.minimum(np.floor(s).astype(np.int64), top)
    i1 = np.minimum(i0 + 1, top)
    g0, g1 = lut[row, i0], lut[row, i1]
    lin, dfdx = g0 + (g1 - g0) * (s - i0), (g1 - g0) * top * ok
    tt = np.asarray(t, dtype=np.float64)[:, None, None, None]
    y, dy = lin / tt, dfdx / tt
    pivot = y[b // 2]
    wgt = np.exp(-30.0 * (x - 0.5) ** 2)
    dw = -60.0 * (x - 0.5) * wgt
    sigma = sig.astype(np.float64)
    a_n, c_n = dw * sigma, (dw * (y - pivot) + wgt * dy) * sigma
    D = wgt.sum(0) + 1e-6
    qd = ((wgt * (y - pivot)).sum(0) - pivot * 1e-6) / D
    beta = 1.0 / D
    kap = -beta * qd
    t1, t2, t3 = beta * beta * (c_n * c_n).sum(0), 2 * beta * kap * (a_n * c_n).sum(0), kap * kap * (a_n * a_n).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (t1 + np.abs(t2) + t3) / (t1 + t2 + t3)


def test_repeat_about_the_mean(dev):
    """The probe exposure saturated in one half of the image and black in the other, the rest of the series consistent: the
    conditioning test fires, the batch is repeated about the mean, and the result is still the pair's."""
    from clair_torch_amd import ops
    n, c, h, w = 8, 3, 8, 32
    x, sd, t, dark, dark_std, lut = _scene(31, n, c, h, w)
    for probe in (n // 2, 5 // 2):
        x[probe, :, :, : w // 2] = 0.0
        x[probe, :, :, w // 2:] = 1.0
    x[5:] = x[5:] * 0.2       # a second batch far from the running mean
    xd, sdd, dd, dsd, lutd = x.to(dev), sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    for first in (n, 5):      # the repeat does run: many elements far beyond the limit of 8, one makes its wavefront repeat
        xb, sig = ops.dark_field_blur(xd[:first], dd[:first], dsd[:first], std=sdd[:first])
        ratio = _condition_ratio(xb.cpu().numpy(), sig.cpu().numpy(), t[:first].numpy(), lut.numpy())
        assert int((ratio > 16).sum()) >= 16, "this stack would not make the merge repeat a batch"
    kw = dict(lut=lutd, interp="linear", gaussian_weight=True)
    for part in ([(0, 8)], [(0, 5), (5, 8)]):
        st_a, st_b = ops.MergeState((c, h, w), dev, True), ops.MergeState((c, h, w), dev, True)
        for a, b in part:
            args = (xd[a:b], t[a:b], dd[a:b], dsd[a:b])
            want = _pair(*args, std=sdd[a:b], state=st_a, finalize=b == n, **kw)
            got = _fused(*args, std=sdd[a:b], state=st_b, finalize=b == n, **kw)
            assert _same_state(st_b, st_a), part
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), part
        assert bool(torch.isfinite(got[1]).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint16], ids=["f32", "u16"])
def test_bands_with_halo_equal_whole(dev, dtype):
    """Row bands of a 17-row image with the neighbouring rows as halo, a one-row interior band among them, give the rows of
    the untiled result bit for bit (the LUT row comes from the GLOBAL flat index: 3 channels, 10 columns)."""
    from clair_torch_amd import ops
    n, c, h, w = 3, 3, 17, 10
    x, sd, t, dark, dark_std, lut = _scene(4, n, c, h, w)
    stack, max_code = _as_dtype(x, dtype)
    stack, sd, dark, dark_std, lut = stack.to(dev), sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    for interp, src in (("linear", dict(std=sd)), ("catmull", dict(std_mode="multiplier", std_value=0.05))):
        kw = dict(lut=lut, interp=interp, gaussian_weight=True, max_code=max_code)
        whole = _fused(stack, t, dark, dark_std, **kw, **src)
        for r0, r1 in ((0, 6), (6, 11), (11, 17), (8, 9)):
            halo = torch.zeros((n, c, 2, w), dtype=stack.dtype, device=dev)
            if r0 > 0:
                halo[:, :, 0] = stack[:, :, r0 - 1]
            if r1 < h:
                halo[:, :, 1] = stack[:, :, r1]
            band_src = {k: (v[:, :, r0:r1].contiguous() if k == "std" else v) for k, v in src.items()}
            args = (stack[:, :, r0:r1].contiguous(), t, dark[:, :, r0:r1].contiguous(), dark_std[:, :, r0:r1].contiguous())
            tile = ops.TileGeometry(h_global=h, row_offset=r0)
            got = _fused(*args, tile=tile, halo=halo, **kw, **band_src)
            assert torch.equal(got[0], whole[0][:, r0:r1]) and torch.equal(got[1], whole[1][:, r0:r1]), (interp, r0, r1)
            want = _pair(*args, tile=tile, halo=halo, **kw, **band_src)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (interp, r0, r1)


class _MatchesSome:
    """A dark-field dataset that has an image for the frames in ``frames`` only (the others: MissingValMode.SKIP_BATCH)."""

    def __init__(self, stack, frames):
        self.stack, self.frames = stack, set(frames)

    def get_matching_artefact_images(self, reference_frame_settings_list):
        if not set(reference_frame_settings_list) <= self.frames:
            return None, None, None, None
        return self.stack.get_matching_artefact_images(reference_frame_settings_list)


@pytest.mark.parametrize("mode", ["linear", "catmull"])
def test_compute_hdr_image_fused_dark(dev, mode, monkeypatch):
    from clair_torch_amd import ops
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    from oracle import eager_torch as oe
    x, sd, t, dark, dark_std, lut = _scene(5, 6, 3, 12, 10)
    dark, dark_std = dark[0], dark_std[0]
    model = ICRFModelDirect(icrf=lut, interpolation_mode=InterpMode[mode.upper()]).to(dev)
    ro = False if mode == "catmull" else None
    common = dict(weight_fn=gaussian_value_weights, reference_order=ro)

    def loader(batch_size, stds=sd):
        return DataLoader(StackDataset(x, t.tolist(), stds=stds), batch_size=batch_size, shuffle=False, collate_fn=custom_collate)

    art = ArtefactStack(dark, dark_std)
    plain = compute_hdr_image(loader(4), "cuda", model, dark_field_dataset=art, fused_dark=False, **common)
    fused = compute_hdr_image(loader(4), "cuda", model, dark_field_dataset=art, fused_dark=True, **common)
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1])
    mean_o, std_o = oe.merge_stack_dark(x, sd, t, lut, dark, dark_std, mode, True, [4, 2])
    for name, (mean, std) in (("fused", fused), ("pair", plain)):
        assert_parity(mean.cpu().numpy(), mean_o.numpy(), rtol=1e-5, norm_tol=1e-6, what=f"{name} dark-field merge mean {mode}")
        assert_parity(std.cpu().numpy(), std_o.numpy(), norm_tol=1e-5, elem_tol=4e-5 if mode == "catmull" else 1e-5,
                      what=f"{name} dark-field merge std {mode}")
    # a dark field for some batches only (batches of 2: the middle one, then the last one): the pair path's bits
    for frames in ((2, 3), (4, 5), (0, 1, 4, 5)):
        some = _MatchesSome(art, frames)
        want = compute_hdr_image(loader(2), "cuda", model, dark_field_dataset=some, fused_dark=False, **common)
        got = compute_hdr_image(loader(2), "cuda", model, dark_field_dataset=some, fused_dark=True, **common)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), frames
    second = _MatchesSome(art, (4, 5))
    want = compute_hdr_image(loader(4), "cuda", model, dark_field_dataset=second, fused_dark=False, **common)
    got = compute_hdr_image(loader(4), "cuda", model, dark_field_dataset=second, fused_dark=True, **common)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert float((got[0] - plain[0]).abs().max()) > 0        # (the first batch did go uncorrected)
    # the reference's error behaviour, as on the pair path
    with pytest.raises(AttributeError):
        compute_hdr_image(loader(4), "cuda", model, dark_field_dataset=ArtefactStack(dark), fused_dark=True, **common)
    with pytest.raises(RuntimeError, match="does not require grad"):
        compute_hdr_image(loader(4, stds=None), "cuda", model, dark_field_dataset=art, fused_dark=True, **common)

    # the fused route is the one that ran: the blur kernel of the pair path is never called
    def no_blur(*args, **kwargs):
        raise AssertionError("ct_dark_field_blur ran: the batch took the pair path")

    monkeypatch.setattr(ops, "dark_field_blur", no_blur)
    again = compute_hdr_image(loader(4), "cuda", model, dark_field_dataset=art, fused_dark=True, **common)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    with pytest.raises(AssertionError, match="pair path"):
        compute_hdr_image(loader(4), "cuda", model, dark_field_dataset=art, fused_dark=False, **common)
    if mode == "catmull":   # the library's default sends CATMULL with uncertainties to the reference-order kernel: not fused
        with pytest.raises(AssertionError, match="pair path"):
            compute_hdr_image(loader(4), "cuda", model, dark_field_dataset=art, fused_dark=True, weight_fn=gaussian_value_weights)


def test_compute_hdr_image_fused_dark_on_codes(dev, monkeypatch):
    """Planar uint16 codes behind CastTo + Normalize (route "code") with uncertainties derived in the kernel, and a flat
    field behind the merge: the fused route takes the codes themselves and leaves the pair path's bits."""
    from clair_torch_amd import ops
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, Normalize
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    x, _, t, dark, dark_std, lut = _scene(8, 7, 3, 9, 14)
    codes, _ = _as_dtype(x, torch.uint16)
    model = ICRFModelDirect(icrf=lut, interpolation_mode=InterpMode.LINEAR).to(dev)
    ds = StackDataset(codes, t.tolist(), missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
    loader = DataLoader(ds, batch_size=3, shuffle=False, collate_fn=custom_collate)
    art = ArtefactStack(dark[0], dark_std[0])
    flat = ArtefactStack(0.8 + 0.4 * torch.rand((3, 9, 14), generator=torch.Generator().manual_seed(3)),
                         0.01 * torch.ones((3, 9, 14)))
    kw = dict(weight_fn=gaussian_value_weights, gpu_transforms=[CastTo("float32"), Normalize(65535, 0)], dark_field_dataset=art)
    for extra in ({}, dict(flat_field_dataset=flat), dict(output_layout="cv")):
        want = compute_hdr_image(loader, "cuda", model, fused_dark=False, **kw, **extra)
        got = compute_hdr_image(loader, "cuda", model, fused_dark=True, **kw, **extra)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), extra
    seen = []
    real = ops.hdr_merge_dark_batch
    monkeypatch.setattr(ops, "hdr_merge_dark_batch", lambda stack, *a, **k: (seen.append(stack.dtype), real(stack, *a, **k))[1])
    compute_hdr_image(loader, "cuda", model, fused_dark=True, **kw)
    assert seen == [torch.uint16] * 3
