"""The flat-field correction inside the linearization launches, on the device: every fused launch (``flat=`` of
ops.linearize_frames, ops.linearize_ingest_frames and ops.linearize_ingest_frames_strided) against the same parent launch
followed by ct_flatfield_apply with the same flat-mean tensor, bit for bit (0 differing bits); the pair once against an
independent float64 restatement of the correction; and ``linearize_dataset_generator(fused_flat=True)`` against ``False`` on
every yielded pair.

Shapes where packets, heads and tails can go wrong: 3x5x7 (plane 35: unaligned heads and tails), 3x6x8 (every packet aligned),
1x1x3 (shorter than a packet), 1 and 5 frames per launch, 7x13 frames behind a step of 2 and 3, one row band.  The LUT rows
differ, so the reference's ``p % C`` row choice is live; the flat fields of the launch tests hold 0 and values near 1e-6, so
``den`` sits at its floor."""
import itertools

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 7), (3, 6, 8), (1, 1, 3)]
# (interp, std_mode): every std mode on LINEAR, CATMULL, and LOOKUP with STD_NONE (LOOKUP has no gradient path)
MODES = [("linear", "none"), ("linear", "constant"), ("linear", "multiplier"), ("linear", "explicit"), ("catmull", "multiplier"),
         ("catmull", "explicit"), ("lookup", "none")]
DTYPES = [torch.uint8, torch.uint16, torch.float32]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _lut(c, n=33):
    return torch.stack([torch.linspace(0, 1, n) ** p for p in (1.8, 2.2, 2.6)])[:c].contiguous()


def _frames(seed, f, chw, dtype):
    """(planar frames of ``dtype``, max_code | None, planar explicit uncertainties)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand((f,) + tuple(chw), generator=gen)
    sd = 0.002 + 0.03 * torch.rand((f,) + tuple(chw), generator=gen)
    if dtype == torch.float32:
        return x, None, sd
    top = 255 if dtype == torch.uint8 else 65535
    return torch.from_numpy(np.rint(x.numpy().astype(np.float64) * top).astype(np.uint8 if top == 255 else np.uint16)), float(top), sd


def _bgr(planar):
    """(F,3,H,W) RGB planes -> the (F,H,W,3) BGR frames an OpenCV reader hands over."""
    return planar.flip(1).permute(0, 2, 3, 1).contiguous()


def _flat(seed, chw, dev):
    """(flat, flat std, mean): a flat field around 1 with a 0, a 1e-6 and a 3e-7 in it, and a mean taken as given."""
    gen = torch.Generator().manual_seed(seed)
    flat = 0.5 + torch.rand(chw, generator=gen)
    edge = torch.tensor([0.0, 1e-6, 3e-7])
    n = flat[0].numel()
    flat.view(chw[0], -1)[:, :min(3, n)] = edge[:min(3, n)]
    flat.view(chw[0], -1)[:, n - 1] = 0.0
    flat_std = 0.001 + 0.02 * torch.rand(chw, generator=gen)
    mean = torch.tensor([0.96875, 1.0, 1.03125])[:chw[0]]
    return flat.to(dev), flat_std.to(dev), mean.to(dev)


def _front(ops, name, kw):
    """ops.<name>, or ops.<name>_flat for a call with ``flat``."""
    return getattr(ops, name + "_flat" if "flat" in kw else name)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _differing_bits(a, b):
    return int((_bits(a) ^ _bits(b)).ne(0).sum())


def _pair_and_fused(front, flat, flat_std, mean):
    """(lin, std) of ``front()`` followed by ct_flatfield_apply with ``mean``, and of ``front(flat=...)``."""
    from clair_torch_amd import ops
    lin, std = front()
    ops.flatfield_correct(lin, std, flat, flat_std, input_is_variance=False, through_mean=False, flat_mean=mean)
    return (lin, std), front(flat=(flat, flat_std, mean))


def _check(front, flat, flat_std, mean, what):
    want, got = _pair_and_fused(front, flat, flat_std, mean)
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    assert _differing_bits(got[0], want[0]) == 0, what
    assert _differing_bits(got[1], want[1]) == 0, what


def _std_kw(std_mode, sd):
    return dict(std=sd) if std_mode == "explicit" else dict(std_mode=std_mode, std_value=0.05)


@pytest.mark.parametrize("chw", SHAPES)
def test_linearize_std_flat(dev, chw):
    """ct_linearize_std_flat: planar frames (the packet kernel and the element tail) and (H,W,3) BGR frames (the pixel-owning
    kernel on 6x8, element by element on 5x7; explicit uncertainties in the frames' own layout: packets of 8)."""
    from clair_torch_amd import ops
    lut = _lut(chw[0]).to(dev)
    layouts = ["nchw", "nhwc_bgr"] if chw[0] == 3 else ["nchw"]
    for k, (f, dtype, layout, (interp, std_mode), with_fs) in enumerate(itertools.product((1, 5), DTYPES, layouts, MODES,
                                                                                          (True, False))):
        x, max_code, sd = _frames(100 + k, f, chw, dtype)
        if layout != "nchw":
            x, sd = _bgr(x), _bgr(sd)
        x, sd = x.to(dev), sd.to(dev)
        flat, flat_std, mean = _flat(7 + k, chw, dev)
        front = lambda **kw: _front(ops, "linearize_frames", kw)(x, lut, interp, max_code=max_code, layout=layout, **_std_kw(std_mode, sd), **kw)  # noqa: E731
        _check(front, flat, flat_std if with_fs else None, mean, (f, dtype, layout, interp, std_mode, with_fs))


def _chain(dtype):
    """A black level and a target range for the dtype."""
    return [("affine", 2.0, 250.0, 1.0, 0.0)] if dtype == torch.uint8 else (
        [("affine", 64.0, 4031.0, 1.0, 0.0)] if dtype == torch.uint16 else [("affine", 0.015625, 0.875, 1.0, 0.0)])


@pytest.mark.parametrize("chw", SHAPES)
def test_linearize_ingest_flat(dev, chw):
    """ct_linearize_ingest_flat behind a black-level chain, planar and raw BGR frames, and -- with per-frame constants -- behind
    one data-dependent Normalize."""
    from clair_torch_amd import ops
    lut = _lut(chw[0]).to(dev)
    layouts = ["nchw", "nhwc_bgr"] if chw[0] == 3 else ["nchw"]
    for k, (f, dtype, layout, (interp, std_mode), with_fs) in enumerate(itertools.product((1, 5), DTYPES, layouts, MODES,
                                                                                          (True, False))):
        x, _, sd = _frames(300 + k, f, chw, dtype)
        x, sd = (x if layout == "nchw" else _bgr(x)).to(dev), sd.to(dev)     # explicit uncertainties stay planar
        flat, flat_std, mean = _flat(11 + k, chw, dev)
        fs = flat_std if with_fs else None
        what = (f, dtype, layout, interp, std_mode, with_fs)
        front = lambda **kw: _front(ops, "linearize_ingest_frames", kw)(x, _chain(dtype), lut, interp, layout=layout, **_std_kw(std_mode, sd), **kw)  # noqa: E731
        _check(front, flat, fs, mean, what)
        if std_mode in ("none", "multiplier"):   # a data-dependent Normalize: sub and div of every frame from the device
            consts = ops.ingest_extrema_frames(x, (), layout)
            data = lambda **kw: _front(ops, "linearize_ingest_frames", kw)(x, [("affine_data", 1.0, 0.0)], lut, interp, layout=layout, consts=consts,  # noqa: E731
                                                            **_std_kw(std_mode, sd), **kw)
            _check(data, flat, fs, mean, what + ("data",))


@pytest.mark.parametrize("step,out_hw", [(2, (4, 7)), (3, (3, 5))])
def test_linearize_ingest_strided_flat(dev, step, out_hw):
    """ct_linearize_ingest_strided_flat on 7x13 frames: the flat field has the downscaled shape."""
    from clair_torch_amd import ops
    lut = _lut(3).to(dev)
    chw = (3,) + out_hw
    for k, (f, dtype, layout, (interp, std_mode), with_fs) in enumerate(itertools.product((1, 5), DTYPES, ("nchw", "nhwc_bgr"), MODES,
                                                                                          (True, False))):
        x, _, _ = _frames(500 + k, f, (3, 7, 13), dtype)
        _, _, sd = _frames(600 + k, f, chw, torch.float32)                    # uncertainties arrive at the downscaled shape
        x, sd = (x if layout == "nchw" else _bgr(x)).to(dev), sd.to(dev)
        flat, flat_std, mean = _flat(13 + k, chw, dev)
        what = (f, dtype, layout, interp, std_mode, with_fs)
        front = lambda **kw: _front(ops, "linearize_ingest_frames_strided", kw)(x, step, _chain(dtype), lut, interp, layout=layout,  # noqa: E731
                                                                 **_std_kw(std_mode, sd), **kw)
        _check(front, flat, flat_std if with_fs else None, mean, what)
        assert front()[0].shape == (f,) + chw
        if std_mode == "multiplier":
            consts = ops.ingest_extrema_frames(x, (), layout)
            data = lambda **kw: _front(ops, "linearize_ingest_frames_strided", kw)(x, step, [("affine_data", 1.0, 0.0)], lut, interp, layout=layout,  # noqa: E731
                                                                    consts=consts, **_std_kw(std_mode, sd), **kw)
            _check(data, flat, flat_std if with_fs else None, mean, what + ("data",))


def test_row_band(dev):
    """Rows [3, 7) of a 7-row image on the entries that take a band: the flat field holds the band's rows, the LINEAR / CATMULL
    row follows the GLOBAL index."""
    from clair_torch_amd import ops
    lut = _lut(3).to(dev)
    tile = ops.TileGeometry(h_global=7, row_offset=3)
    chw = (3, 4, 5)
    for k, (f, dtype, (interp, std_mode), with_fs) in enumerate(itertools.product((1, 5), DTYPES, MODES, (True, False))):
        x, max_code, sd = _frames(700 + k, f, chw, dtype)
        x, sd = x.to(dev), sd.to(dev)
        flat, flat_std, mean = _flat(17 + k, chw, dev)
        fs = flat_std if with_fs else None
        std_front = lambda **kw: _front(ops, "linearize_frames", kw)(x, lut, interp, max_code=max_code, tile=tile, **_std_kw(std_mode, sd), **kw)  # noqa: E731
        _check(std_front, flat, fs, mean, ("std", f, dtype, interp, std_mode, with_fs))
        ingest = lambda **kw: _front(ops, "linearize_ingest_frames", kw)(x, _chain(dtype), lut, interp, tile=tile, **_std_kw(std_mode, sd), **kw)  # noqa: E731
        _check(ingest, flat, fs, mean, ("ingest", f, dtype, interp, std_mode, with_fs))
        strided = lambda **kw: _front(ops, "linearize_ingest_frames_strided", kw)(x, 1, _chain(dtype), lut, interp, tile=tile,  # noqa: E731
                                                                   **_std_kw(std_mode, sd), **kw)
        _check(strided, flat, fs, mean, ("strided, step 1", f, dtype, interp, std_mode, with_fs))


def test_out_buffers_and_custom_ops(dev):
    """Caller-owned outputs are written in place, and the torch.ops registrations reach the same kernels."""
    import clair_torch_amd.torch_ops  # noqa: F401
    from clair_torch_amd import ops
    lut = _lut(3).to(dev)
    x, max_code, _ = _frames(900, 5, (3, 5, 7), torch.uint16)
    x = x.to(dev)
    flat, flat_std, mean = _flat(19, (3, 5, 7), dev)
    out = (torch.empty((5, 3, 5, 7), device=dev), torch.empty((5, 3, 5, 7), device=dev))
    want = ops.linearize_frames_flat(x, lut, "linear", std_mode="multiplier", std_value=0.05, flat=(flat, flat_std, mean))
    got = ops.linearize_frames_flat(x, lut, "linear", std_mode="multiplier", std_value=0.05, flat=(flat, flat_std, mean), out=out)
    assert got[0] is out[0] and got[1] is out[1] and torch.equal(_bits(out[0]), _bits(want[0])) and torch.equal(_bits(out[1]), _bits(want[1]))
    via = torch.ops.clair_hip.linearize_std_flat(x, lut, "linear", None, "multiplier", 0.05, 65535.0, flat, flat_std, mean)
    assert _differing_bits(via[0], want[0]) == 0 and _differing_bits(via[1], want[1]) == 0
    stages = [0.0, 64.0, 4031.0, 1.0, 0.0] + [0.0] * 8
    want = ops.linearize_ingest_frames_flat(x, _chain(torch.uint16), lut, "linear", std_mode="multiplier", std_value=0.05,
                                            flat=(flat, None, mean))
    via = torch.ops.clair_hip.linearize_ingest_flat(x, stages, lut, "linear", None, "multiplier", 0.05, flat, None, mean)
    assert _differing_bits(via[0], want[0]) == 0 and _differing_bits(via[1], want[1]) == 0
    exact = _exact_flat(5, (3, 5, 7)).to(dev)
    assert torch.equal(torch.ops.clair_hip.flatfield_mean(exact), ops.flatfield_mean(exact))
    assert torch.equal(ops.flatfield_mean(exact).cpu(), exact.double().mean(dim=(1, 2)).float().cpu())


# ---- the correction itself, against float64 ----------------------------------------------------------------------------------
# What five float32 roundings may cost: 1 ulp on lin' and 4 ulp on sd' bound them to first order.  The float32 formula itself --
# evaluated on the host with numpy's correctly rounded float32 operations on 4 million samples of these value ranges (lin in
# [0, 1), sd below 0.05, flat in [0.5, 1.5] and at the floor, flat std below 0.02) -- reaches 2.14 ulp on lin' (den, the quotient
# and the product each round, and an ulp halves across a power of two) and 4.18 ulp on sd'; the bounds are those plus one ulp.
LIN_ULP, SD_ULP = 3.14, 5.18


def test_pair_against_float64(dev):
    """The pair of launches -- and with it, bit for bit, the fused launch -- against a float64 numpy restatement of the six
    lines of the correction; M as given, results rounded to float32."""
    from clair_torch_amd import ops
    lut = _lut(3).to(dev)
    x, max_code, _ = _frames(1000, 5, (3, 5, 7), torch.uint16)
    x = x.to(dev)
    flat, flat_std, mean = _flat(23, (3, 5, 7), dev)
    for fs in (flat_std, None):
        lin0, sd0 = ops.linearize_frames(x, lut, "linear", max_code=max_code, std_mode="multiplier", std_value=0.05)
        front = lambda **kw: _front(ops, "linearize_frames", kw)(x, lut, "linear", max_code=max_code, std_mode="multiplier", std_value=0.05, **kw)  # noqa: E731
        want, got = _pair_and_fused(front, flat, fs, mean)
        assert _differing_bits(got[0], want[0]) == 0 and _differing_bits(got[1], want[1]) == 0
        lin, sd = lin0.cpu().numpy().astype(np.float64), sd0.cpu().numpy().astype(np.float64)
        m = mean.cpu().numpy().astype(np.float64)[None, :, None, None]
        den = flat.cpu().numpy().astype(np.float64)[None] + np.float64(np.float32(1e-6))
        lin_ref = (lin / den) * m
        grad = -(m * lin) / (den * den)
        var = sd * sd
        if fs is not None:
            var = var + (grad * fs.cpu().numpy().astype(np.float64)[None]) ** 2
        sd_ref = np.sqrt(var)
        for name, have, ref, bound in (("lin", want[0], lin_ref, LIN_ULP), ("sd", want[1], sd_ref, SD_ULP)):
            ulp = np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64)
            err = float(np.max(np.abs(have.cpu().numpy().astype(np.float64) - ref) / ulp))
            print(f"{name}' against float64, flat std {'given' if fs is not None else 'absent'}: {err:.3f} ulp (bound {bound})")
            assert err <= bound, (name, err)


# ---- the generator -----------------------------------------------------------------------------------------------------------
def _exact_flat(seed, chw):
    """Multiples of 2^-10 in [0.5, 1.5]: the float64 sums behind the mean are exact in any order of the atomics."""
    gen = torch.Generator().manual_seed(seed)
    return 0.5 + torch.randint(0, 1025, chw, generator=gen).float() / 1024.0


class _MatchesSome:
    """A dark-field dataset that has an image for the frames in ``frames`` only."""

    def __init__(self, stack, frames):
        self.stack, self.frames = stack, set(frames)

    def get_matching_artefact_images(self, reference_frame_settings_list):
        if not set(reference_frame_settings_list) <= self.frames:
            return None, None, None, None
        return self.stack.get_matching_artefact_images(reference_frame_settings_list)


def _run(loader, model, **kw):
    from clair_torch_amd.inference import linearize_dataset_generator
    return [(lin.clone(), sd.clone()) for lin, sd, _ in linearize_dataset_generator(loader, "cuda", model, **kw)]


def _fronts_called(monkeypatch, ops):
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda entry, *a: (calls.append(entry), real(entry, *a))[1])
    return calls


@pytest.mark.parametrize("case", ["code pair", "raw bgr", "downscale", "dark mix"])
@pytest.mark.parametrize("with_fs", [True, False])
def test_generator_fused_flat_is_bit_equal(dev, case, with_fs, monkeypatch):
    """21 frames in groups of 16: ``fused_flat=True`` yields what ``False`` yields, and the fused launches are the ones that ran."""
    from clair_torch_amd import ops
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, CvToTorch, Normalize, StridedDownscale
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.models import ICRFModelDirect
    n, chw = 21, ((3, 7, 13) if case == "downscale" else (3, 6, 5))
    dtype = torch.uint8 if case == "raw bgr" else torch.uint16
    codes, top, _ = _frames(2000, n, chw, dtype)
    tf = {"code pair": [CastTo("float32"), Normalize(top, 0)],
          "raw bgr": [CvToTorch(), CastTo("float32"), Normalize(top, 2)],
          "downscale": [CastTo("float32"), Normalize(4095, 64), StridedDownscale(2)],
          "dark mix": [CastTo("float32"), Normalize(top, 0)]}[case]
    out_chw = (3, 4, 7) if case == "downscale" else chw
    ds = StackDataset(_bgr(codes) if case == "raw bgr" else codes, [0.01 * (k + 1) for k in range(n)],
                      missing_std_mode=MissingStdMode.MULTIPLIER, missing_std_value=0.05, materialize_std=False)
    loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
    model = ICRFModelDirect(icrf=_lut(3), interpolation_mode=InterpMode.LINEAR).to(dev)
    gen = torch.Generator().manual_seed(5)
    flat = ArtefactStack(_exact_flat(31, out_chw), 0.001 + 0.02 * torch.rand(out_chw, generator=gen) if with_fs else None)
    kw = dict(gpu_transforms=tf, flatfield_dataset=flat)
    if case == "dark mix":   # runs of matched and unmatched frames inside the groups
        dark = ArtefactStack(0.1 * torch.rand(chw, generator=gen), 0.002 + 0.01 * torch.rand(chw, generator=gen))
        kw["dark_field_dataset"] = _MatchesSome(dark, set(range(3, 9)) | {12, 20})
    want = _run(loader, model, fused_flat=False, **kw)
    calls = _fronts_called(monkeypatch, ops)
    got = _run(loader, model, fused_flat=True, **kw)
    assert len(got) == len(want) == n and tuple(got[0][0].shape) == out_chw
    for k in range(n):
        assert _differing_bits(got[k][0], want[k][0]) == 0 and _differing_bits(got[k][1], want[k][1]) == 0, k
    fused = {"code pair": "ct_linearize_std_flat", "raw bgr": "ct_linearize_ingest_flat",
             "downscale": "ct_linearize_ingest_strided_flat", "dark mix": "ct_linearize_std_flat"}[case]
    assert fused in calls and calls.count("ct_flatfield_sums") == 1          # the mean: once per run
    assert ("ct_flatfield_apply" in calls) == (case == "dark mix")           # dark-matched runs keep the pair
