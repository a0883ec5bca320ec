"""ct_hdr_merge_ingest_batches on the device: several raw-frame batches behind one chain in ONE launch, the streaming state in
registers between them.  Its specification is one sentence -- exactly ct_hdr_merge_ingest_batch applied to the batches in
turn with the state carried along -- and that path is pinned to the float64 oracle and the golden vectors by
test_gpu_merge_ingest.py, so it is the comparand everywhere here and every comparison is on raw bits (integer views of the
mean, the std and the three state arrays; a NaN must sit at the same place).  There is no tolerance anywhere.  The new path
always passes ``require_one_launch=True``: a silent fall-back to one launch per batch would compare the comparand with itself.
"""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16}
PAIRS = {1: [(0.05, 0.9)], 3: [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)]}
INTERPS = ("lookup", "linear", "catmull", None)
STDS = ("none", "constant", "multiplier", "explicit")
# planar (3,5,7): a plane of 35, so planes 1 and 2 have a head of 1 and 2 elements and every plane a ragged tail;
# interleaved (5,7): odd H*W, planes 1 and 2 go element by element; interleaved (4,6): aligned packets; one pixel
FLAVOURS = [(torch.uint8, "nchw", (3, 5, 7)), (torch.uint16, "nchw", (3, 5, 7)), (torch.uint8, "nhwc", (3, 5, 7)),
            (torch.uint16, "nhwc_bgr", (3, 5, 7)), (torch.uint16, "nhwc", (3, 4, 6)), (torch.uint8, "nhwc_bgr", (3, 4, 6)),
            (torch.uint8, "nchw", (1, 1, 1)), (torch.uint16, "nchw", (1, 1, 1))]
# a single-exposure batch in the middle and a probe of B / 2; two equal batches; as many batches as a call takes
PARTITIONS = ([3, 1, 2, 2], [4, 4], [1] * 16)
CHAINS = ("black", "black_clamp", "data")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _T():
    from clair_torch_amd.common import transforms
    return transforms


def _lut(channels, points=64):
    powers = (2.2, 2.4, 2.6, 1.8)[:channels]  # distinct rows: the p % C rule shows
    return np.stack([np.linspace(0, 1, points, dtype=np.float32) ** np.float32(p) for p in powers])


def _source(planar, layout):
    """(B,C,H,W) planes -> the stack in ``layout`` (BGR: what an OpenCV reader hands over)."""
    if layout == "nchw":
        return planar
    a = planar.numpy()
    return torch.from_numpy(np.ascontiguousarray((a[:, ::-1] if layout == "nhwc_bgr" else a).transpose(0, 2, 3, 1)))


def _exposures(n):
    return torch.tensor([0.004 * 2.0 ** (k % 8) * (1.0 + 0.03 * (k // 8)) for k in range(n)], dtype=torch.float64)


def _int_view(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32)


def _same_bits(got, want):
    """Equal bit patterns; NaNs must sit at the same places (their payloads are not compared)."""
    if got is None or want is None:
        return got is None and want is None
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        return False
    zero = torch.zeros((), dtype=got.dtype)
    return torch.equal(_int_view(torch.where(nan, zero, got)), _int_view(torch.where(nan, zero, want)))


def _state_same(a, b):
    return _same_bits(a.mean, b.mean) and _same_bits(a.sumw, b.sumw) and _same_bits(a.var, b.var)


def _problem(dev, rng, dtype, layout, chw, sizes, chain):
    """The batches of one merge: (frames list on the device, stages, exposure list, consts list | None).  Batch b draws its
    codes from a range of its own -- below the black level, inside the range, above the maximum -- so the extrema of a
    data-dependent Normalize (the maximum from the data) differ from batch to batch: a kernel that reuses batch 0's constants fails."""
    from clair_torch_amd import ops
    c, h, w = chw
    top = 255 if dtype == torch.uint8 else 1100
    sub, div = (16.0, 184.0) if dtype == torch.uint8 else (64.0, 959.0)   # Normalize(200, 16) / Normalize(1023, 64)
    expo = _exposures(sum(sizes))
    frames, expos, n0 = [], [], 0
    for b, n in enumerate(sizes):
        lo, hi = (3 * b) % 40, top - (7 * b) % 60
        codes = rng.integers(lo, hi + 1, size=(n, c, h, w))
        codes.reshape(-1)[0], codes.reshape(-1)[-1] = lo, hi   # the extrema are attained (one pixel, one exposure: hi)
        frames.append(_source(torch.from_numpy(codes.astype(_NP[dtype])), layout).to(dev))
        expos.append(expo[n0:n0 + n])
        n0 += n
    affine = ("affine", sub, div, 1.0, 0.0)
    if chain == "black":
        return frames, [affine], expos, None
    if chain == "black_clamp":
        return frames, [affine, ("clamp", PAIRS[c])], expos, None
    # Normalize(max_val=None, min_val=0): a one-pixel batch of one exposure still has a range
    consts = [ops.ingest_extrema(f, (), layout, min_val=0.0) for f in frames]
    if frames[0].numel() > 1:
        assert any(not torch.equal(consts[0].cpu(), k.cpu()) for k in consts[1:]), "the batches share their extrema: a weak test"
    return frames, [("affine_data", 1.0, 0.0)], expos, consts


def _mode_kw(interp, gauss, std_name, lut_d):
    kw = dict(lut=None if interp is None else lut_d, interp=interp, gaussian_weight=gauss)
    if std_name not in ("none", "explicit"):
        kw.update(std_mode=std_name, std_value=0.01 if std_name == "constant" else 0.05)
    if interp in ("lookup", "catmull") and std_name != "none":
        kw["reference_order"] = False   # CT_MERGE_CLOSED_FORM: the reference-order kernel is not fused
    return kw


def _sigmas(dev, rng, frames, layout):
    """Explicit uncertainties: planar (B,C,H,W), also beside interleaved frames."""
    from clair_torch_amd import ops
    return [torch.from_numpy((0.001 + 0.02 * rng.random(ops.ingest_shape(tuple(f.shape), layout))).astype(np.float32)).to(dev)
            for f in frames]


def _per_batch(frames, stages, expos, consts=None, stds=None, state=None, finalize=True, **kw):
    """The comparand: ops.hdr_merge_ingest_batch once per batch, the MergeState carried along."""
    from clair_torch_amd import ops
    out = None
    for b, (f, e) in enumerate(zip(frames, expos)):
        out = ops.hdr_merge_ingest_batch(f, stages, e, consts=None if consts is None else consts[b], std=None if stds is None else stds[b],
                                         state=state, finalize=finalize and b == len(frames) - 1, **kw)
    return out


def _one_launch(frames, stages, expos, **kw):
    from clair_torch_amd import ops
    return ops.hdr_merge_ingest_batches(frames, stages, expos, require_one_launch=True, **kw)


# ---- 1. every mode -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,layout,chw", FLAVOURS)
def test_every_mode_equals_one_launch_per_batch(dev, dtype, layout, chw):
    """Every interpolation x weight x uncertainty mode of this kernel flavour; partitions and chains cycle through the modes
    so that each of them meets every flavour (asserted at the end).  Even combinations run as a whole merge without a state
    (first + finalize), odd ones with a MergeState whose bits are compared too; the mean is float64 and float32 in turn."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(41)
    lut_d = torch.from_numpy(_lut(chw[0])).to(dev)
    combo, seen, refused = 0, set(), 0
    for interp in INTERPS:
        for gauss in (False, True):
            for std_name in STDS:
                sizes, chain = PARTITIONS[combo % 3], CHAINS[(combo // 3) % 3]
                seen.add((len(sizes), chain))
                frames, stages, expos, consts = _problem(dev, rng, dtype, layout, chw, sizes, chain)
                stds = _sigmas(dev, rng, frames, layout) if std_name == "explicit" else None
                kw = dict(layout=layout, consts=consts, stds=stds, mean_dtype=torch.float32 if combo % 4 == 3 else torch.float64,
                          **_mode_kw(interp, gauss, std_name, lut_d))
                label = f"{interp} gauss={gauss} {std_name} {sizes} {chain}"
                has_std = std_name != "none"
                if interp == "lookup" and not gauss and has_std:   # nothing connects the mean to the image: both refuse
                    refused += 1
                    with pytest.raises(RuntimeError, match="does not require grad"):   # (torch.autograd.grad's text)
                        _per_batch(frames, stages, expos, state=ops.MergeState(chw, dev, True), **kw)
                    with pytest.raises(RuntimeError, match="does not require grad"):
                        _one_launch(frames, stages, expos, **kw)
                    combo += 1
                    continue
                want_state = ops.MergeState(chw, dev, has_std)
                want = _per_batch(frames, stages, expos, state=want_state, **kw)
                got_state = ops.MergeState(chw, dev, has_std) if combo % 2 else None
                got = _one_launch(frames, stages, expos, state=got_state, **kw)
                assert got[0].dtype == kw["mean_dtype"] and tuple(got[0].shape) == chw, label
                assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), label
                assert (got[1] is not None) == has_std, label
                if got_state is not None:
                    assert _state_same(got_state, want_state) and got_state.batches == len(sizes), label
                combo += 1
    assert combo == 32 and refused == 3 and len(seen) == 9


# ---- 2. every partition and chain on the headline mode and on the one that repeats batches ---------------------------------------
@pytest.mark.parametrize("dtype,layout,chw", FLAVOURS)
def test_every_partition_and_chain(dev, dtype, layout, chw):
    """LINEAR + Gauss + MULTIPLIER, and LOOKUP + Gauss + CONSTANT in closed form: its pivot test fails in every wavefront, so
    every batch -- the middle ones included -- runs its repeat pass inside the one launch."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(43)
    lut_d = torch.from_numpy(_lut(chw[0])).to(dev)
    for sizes in PARTITIONS:
        for chain in CHAINS:
            frames, stages, expos, consts = _problem(dev, rng, dtype, layout, chw, sizes, chain)
            for interp, std_name in (("linear", "multiplier"), ("lookup", "constant")):
                kw = dict(layout=layout, consts=consts, **_mode_kw(interp, True, std_name, lut_d))
                want_state, got_state = ops.MergeState(chw, dev, True), ops.MergeState(chw, dev, True)
                want = _per_batch(frames, stages, expos, state=want_state, **kw)
                got = _one_launch(frames, stages, expos, state=got_state, **kw)
                label = f"{interp} {std_name} {sizes} {chain}"
                assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and _state_same(got_state, want_state), label
                whole = _one_launch(frames, stages, expos, **kw)   # first + finalize, no state arrays at all
                assert _same_bits(whole[0], want[0]) and _same_bits(whole[1], want[1]), label


# ---- 3. the state: continued, left unfinalized, then finalized ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype,layout,chw", FLAVOURS[1:6])
@pytest.mark.parametrize("std_name", ["none", "multiplier", "explicit"])
def test_continues_a_merge_and_leaves_it_open(dev, dtype, layout, chw, std_name):
    from clair_torch_amd import ops
    rng = np.random.default_rng(47)
    lut_d = torch.from_numpy(_lut(chw[0])).to(dev)
    frames, stages, expos, _ = _problem(dev, rng, dtype, layout, chw, [2, 3, 1, 2, 2], "black_clamp")
    stds = _sigmas(dev, rng, frames, layout) if std_name == "explicit" else None
    kw = dict(layout=layout, **_mode_kw("linear", True, std_name, lut_d))
    has_std = std_name != "none"

    def part(a, b):
        return dict(stds=None if stds is None else stds[a:b])

    want_state, got_state = ops.MergeState(chw, dev, has_std), ops.MergeState(chw, dev, has_std)
    for st in (want_state, got_state):   # a non-empty state: the first batch, merged as ever
        assert _per_batch(frames[:1], stages, expos[:1], state=st, finalize=False, **part(0, 1), **kw) is None
    assert _state_same(got_state, want_state) and got_state.batches == 1
    # not FIRST_BATCH, not FINALIZE: three batches in one launch
    assert _per_batch(frames[1:4], stages, expos[1:4], state=want_state, finalize=False, **part(1, 4), **kw) is None
    assert _one_launch(frames[1:4], stages, expos[1:4], state=got_state, finalize=False, **part(1, 4), **kw) is None
    assert _state_same(got_state, want_state) and got_state.batches == want_state.batches == 4
    # ... then one more batch finalizes both
    want = _per_batch(frames[4:], stages, expos[4:], state=want_state, **part(4, 5), **kw)
    got = _per_batch(frames[4:], stages, expos[4:], state=got_state, **part(4, 5), **kw)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and _state_same(got_state, want_state)
    # a call that is not a whole merge needs the state
    with pytest.raises(ValueError, match="MergeState"):
        _one_launch(frames[1:4], stages, expos[1:4], finalize=False, **part(1, 4), **kw)


# ---- 4. row bands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "nhwc_bgr"])
def test_row_band_equals_its_rows_of_the_whole(dev, layout):
    """Rows 2..5 of 8: the LINEAR row is the global flat index modulo C, so a band must know where it lies."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(53)
    chw = (3, 8, 7)
    lut_d = torch.from_numpy(_lut(3)).to(dev)
    frames, stages, expos, _ = _problem(dev, rng, torch.uint16, layout, chw, [3, 1, 2, 2], "black_clamp")
    rows = slice(2, 6)
    band = [(f[:, :, rows] if layout == "nchw" else f[:, rows]).contiguous() for f in frames]
    stds = _sigmas(dev, rng, frames, layout)
    band_stds = [s[:, :, rows].contiguous() for s in stds]
    tile = ops.TileGeometry(h_global=8, row_offset=2)
    for interp, std_name in (("linear", "explicit"), ("catmull", "multiplier"), (None, "constant")):
        kw = dict(layout=layout, **_mode_kw(interp, True, std_name, lut_d))
        explicit = std_name == "explicit"
        whole = _one_launch(frames, stages, expos, stds=stds if explicit else None, **kw)
        got = _one_launch(band, stages, expos, stds=band_stds if explicit else None, tile=tile, **kw)
        want = _per_batch(band, stages, expos, stds=band_stds if explicit else None, tile=tile,
                          state=ops.MergeState((3, 4, 7), dev, True), **kw)
        for k in range(2):
            assert _same_bits(got[k], whole[k][:, rows].contiguous()) and _same_bits(got[k], want[k]), (interp, std_name, k)


# ---- 5. what cannot be one launch ------------------------------------------------------------------------------------------------------
def test_mixed_constants_fall_back_to_one_launch_per_batch(dev):
    """Batches with and without constants in one list (the chain has no data-dependent stage, so the constants are unused):
    one launch per batch with the state in memory -- the same bits -- unless one launch is required."""
    from clair_torch_amd import ops
    from clair_torch_amd._native import NativeLibraryError
    rng = np.random.default_rng(59)
    chw = (3, 5, 7)
    lut_d = torch.from_numpy(_lut(3)).to(dev)
    frames, stages, expos, _ = _problem(dev, rng, torch.uint16, "nhwc_bgr", chw, [3, 1, 2, 2], "black")
    consts = [ops.ingest_extrema(frames[0], (), "nhwc_bgr"), None, None, ops.ingest_extrema(frames[3], (), "nhwc_bgr")]
    kw = dict(layout="nhwc_bgr", **_mode_kw("linear", True, "multiplier", lut_d))
    want_state, got_state = ops.MergeState(chw, dev, True), ops.MergeState(chw, dev, True)
    want = _per_batch(frames, stages, expos, state=want_state, **kw)
    got = ops.hdr_merge_ingest_batches(frames, stages, expos, consts=consts, state=got_state, **kw)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and _state_same(got_state, want_state)
    stateless = ops.hdr_merge_ingest_batches(frames, stages, expos, consts=consts, **kw)   # the front end lends a state
    assert _same_bits(stateless[0], want[0]) and _same_bits(stateless[1], want[1])
    with pytest.raises(NativeLibraryError):
        _one_launch(frames, stages, expos, consts=consts, state=ops.MergeState(chw, dev, True), **kw)
    with pytest.raises(NativeLibraryError):
        _one_launch(frames, stages, expos, consts=consts, **kw)
    # one batch is the single-batch call
    one = ops.hdr_merge_ingest_batches(frames[:1], stages, expos[:1], **kw)
    assert _same_bits(one[0], _per_batch(frames[:1], stages, expos[:1], **kw)[0])


# ---- 6. the public entry point, and proof of the route -------------------------------------------------------------------------------------
def _frames_dataset(frames, times, std_mode, std_value):
    """Raw (H,W,3) BGR frames as an OpenCV reader hands them over (StackDataset itself insists on (N,C,H,W))."""
    from clair_torch_amd.datasets import StackDataset

    class Frames(StackDataset):
        def __init__(self):
            self.values, self.stds, self.exposure_times = frames, None, list(times)
            self.files = list(range(len(times)))
            self.missing_std_mode, self.materialize_std = std_mode, False
            self.std_hint = (std_mode.name.lower(), float(std_value))

        def __len__(self):
            return len(self.exposure_times)

    return Frames()


def _api(dev, n):
    """run(batch_size, **kw) -> compute_hdr_image over n raw BGR uint16 frames behind a black-level chain."""
    T = _T()
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    rng = np.random.default_rng(61)
    c, h, w = 3, 5, 7
    t = 0.002 * 1.5 ** np.arange(n)
    frames = _source(torch.from_numpy(rng.integers(40, 1101, size=(n, c, h, w)).astype(np.uint16)), "nhwc_bgr")
    chain = [T.CvToTorch(), T.CastTo("float32"), T.Normalize(1023, 64)]
    ds = _frames_dataset(frames, t.tolist(), MissingStdMode.MULTIPLIER, 0.05)
    model = ICRFModelDirect(icrf=torch.from_numpy(_lut(c, 256)), interpolation_mode=InterpMode.LINEAR).to(dev)

    def run(batch_size, **kw):
        loader = DataLoader(ds, batch_size=batch_size, shuffle=False, collate_fn=custom_collate)
        return compute_hdr_image(loader, "cuda", model, weight_fn=gaussian_value_weights, gpu_transforms=chain, **kw)

    return run


@pytest.mark.parametrize("batch_size", [2, 3])
def test_compute_hdr_image_queues_fused_batches(dev, monkeypatch, batch_size):
    from clair_torch_amd import ops
    run = _api(dev, 7)
    plain = run(batch_size, fused_ingest=False)
    fused = run(batch_size)
    assert fused[0].dtype == torch.float64 and tuple(fused[0].shape) == (3, 5, 7) and fused[1].dtype == torch.float32
    assert _same_bits(fused[0], plain[0]) and _same_bits(fused[1], plain[1])

    def refuse(*args, **kwargs):
        raise AssertionError("ct_hdr_merge_ingest_batch ran: a fused batch was launched on its own")

    calls, inner = [], ops.hdr_merge_ingest_batches

    def counted(frames_list, *args, **kwargs):
        calls.append(len(frames_list))
        return inner(frames_list, *args, **kwargs)

    monkeypatch.setattr(ops, "hdr_merge_ingest_batch", refuse)
    monkeypatch.setattr(ops, "hdr_merge_ingest_batches", counted)
    again = run(batch_size)
    assert calls == [-(-7 // batch_size)]   # one call takes every batch
    assert _same_bits(again[0], fused[0]) and _same_bits(again[1], fused[1])


def test_compute_hdr_image_hands_over_sixteen_batches_at_most(dev, monkeypatch):
    from clair_torch_amd import ops
    run = _api(dev, 20)
    plain = run(1, fused_ingest=False)
    calls, inner = [], ops.hdr_merge_ingest_batches

    def counted(frames_list, *args, **kwargs):
        calls.append(len(frames_list))
        return inner(frames_list, *args, **kwargs)

    monkeypatch.setattr(ops, "hdr_merge_ingest_batches", counted)
    fused = run(1)
    assert calls == [16, 4]
    assert _same_bits(fused[0], plain[0]) and _same_bits(fused[1], plain[1])
