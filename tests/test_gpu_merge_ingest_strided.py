"""ct_hdr_merge_ingest_strided_batches on the device: a StridedDownscale, a chain and 1 to 16 batches of the merge in ONE pass
over the raw full-size frames.  Its specification is one sentence -- ``ops.strided_downscale`` of every batch followed by
``ops.hdr_merge_ingest_batches`` on the compacted frames, bit for bit -- and that pair is pinned elsewhere
(test_gpu_downscale.py, test_gpu_merge_ingest.py, test_gpu_merge_ingest_batches.py), so it is the comparand here and every
comparison with it is on raw bits (integer views of the mean, the std and the three state arrays; a NaN must sit at the same
place).  The new path passes ``require_one_launch=True`` wherever the list can be one launch: a silent walk batch by batch
would hide the kernel's batch loop.  One scene is also checked against the float64 oracle on host-sliced frames.
"""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import _merge_views as mv
from _util import assert_parity

pytestmark = pytest.mark.gpu

_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16}
PAIRS = [(0.0, 1.0), (0.125, 0.7), (-0.25, 0.3333)]
INTERPS = ("lookup", "linear", "catmull", None)
STDS = ("none", "constant", "multiplier", "explicit")
SHAPES = [(7, 13), (8, 16), (5, 3)]
STEPS = (1, 2, 3, 5, 9)
PARTITIONS = ([6], [3, 2, 1], [1, 1, 4])
CHAINS = ("black_clamp", "data")
C = 3


def _down(n, step):
    return -(-n // step)


def test_the_shapes_cover_the_edges():
    """What the shapes and steps are chosen for, from the shapes alone: output planes that are no multiple of the 4 elements of
    a planar thread (a head, a tail, groups that straddle an output row), planes that are no multiple of 3 (the LINEAR row
    rotates from plane to plane), whole packets, a step that leaves one row, one that leaves one pixel, and rows narrower than
    a group."""
    planes = {(hw, s): _down(hw[0], s) * _down(hw[1], s) for hw in SHAPES for s in STEPS}
    assert any(p % 4 for p in planes.values()) and any(p % 4 == 0 and p > 4 for p in planes.values())
    assert any(p % 3 for p in planes.values()) and any(p % 3 == 0 for p in planes.values())
    assert any(_down(hw[0], s) == 1 and _down(hw[1], s) > 1 for hw in SHAPES for s in STEPS if s > 1)   # one row
    assert any(p == 1 for (hw, s), p in planes.items() if s > 1)                                       # one pixel
    assert any(1 < _down(hw[1], s) < 4 and _down(hw[0], s) > 1 for hw in SHAPES for s in STEPS)        # a group spans rows
    assert sum(PARTITIONS[0]) == sum(PARTITIONS[1]) == sum(PARTITIONS[2]) == 6


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


def _problem(dev, rng, dtype, layout, hw, sizes, chain):
    """The batches of one merge: (frames list on the device, stages, exposure list, consts list | None).  Batch b draws its codes
    from a range of its own, so the constants of a data-dependent Normalize -- taken from the FULL frames, in front of the
    downscale -- differ from batch to batch."""
    from clair_torch_amd import ops
    h, w = hw
    top = 255 if dtype == torch.uint8 else 1100
    sub, div = (16.0, 184.0) if dtype == torch.uint8 else (64.0, 959.0)   # a black level: Normalize(200, 16) / Normalize(1023, 64)
    expo = _exposures(sum(sizes))
    frames, expos, n0 = [], [], 0
    for b, n in enumerate(sizes):
        lo, hi = (3 * b) % 40, top - (7 * b) % 60
        codes = rng.integers(lo, hi + 1, size=(n, C, h, w))
        codes.reshape(-1)[0], codes.reshape(-1)[-1] = lo, hi
        frames.append(_source(torch.from_numpy(codes.astype(_NP[dtype])), layout).to(dev))
        expos.append(expo[n0:n0 + n])
        n0 += n
    if chain == "black_clamp":   # ... plus a clamp with a pair per channel
        return frames, [("affine", sub, div, 1.0, 0.0), ("clamp", PAIRS)], expos, None
    consts = [ops.ingest_extrema(f, (), layout, min_val=0.0) for f in frames]
    if len(frames) > 1:
        assert any(not torch.equal(consts[0].cpu(), k.cpu()) for k in consts[1:]), "the batches share their extrema: a weak test"
    return frames, [("affine_data", 1.0, 0.0)], expos, consts


def _mode_kw(interp, gauss, std_name, lut_d):
    kw = dict(lut=None if interp is None else lut_d, interp=interp, gaussian_weight=gauss)
    if std_name not in ("none", "explicit"):
        kw.update(std_mode=std_name, std_value=0.01 if std_name == "constant" else 0.05)
    if interp in ("lookup", "catmull") and std_name != "none":
        kw["reference_order"] = False   # CT_MERGE_CLOSED_FORM: the reference-order kernel is not fused
    return kw


def _sigmas(dev, rng, sizes, chw):
    """Explicit uncertainties: planar and of the DOWNSCALED shape, also beside interleaved frames."""
    return [torch.from_numpy((0.001 + 0.02 * rng.random((n,) + chw)).astype(np.float32)).to(dev) for n in sizes]


def _two_launches(frames, step, stages, expos, layout, **kw):
    """The comparand: ct_strided_downscale of every batch, then ct_hdr_merge_ingest_batches on the compacted copies."""
    from clair_torch_amd import ops
    return ops.hdr_merge_ingest_batches([ops.strided_downscale(f, step, layout) for f in frames], stages, expos, layout=layout, **kw)


def _fused(frames, step, stages, expos, layout, **kw):
    from clair_torch_amd import ops
    return ops.hdr_merge_ingest_batches_strided(frames, step, stages, expos, layout=layout, require_one_launch=True, **kw)


# ---- 1. bit-identity with the two launches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("dtype,layout", [(torch.uint8, "nchw"), (torch.uint16, "nchw"), (torch.uint8, "nhwc_bgr"), (torch.uint16, "nhwc_bgr")])
def test_equals_downscale_then_merge(dev, dtype, layout, hw):
    """Every step x interpolation x weight x uncertainty mode of this flavour and shape; partitions and chains cycle through
    them so that every step meets every partition and both chains (asserted at the end).  Even combinations run as a whole
    merge without a state, odd ones with a MergeState whose bits are compared too; the mean is float64 and float32 in turn."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(71)
    lut_d = torch.from_numpy(_lut(C)).to(dev)
    problems = {(p, chain): _problem(dev, rng, dtype, layout, hw, PARTITIONS[p], chain) for p in range(3) for chain in CHAINS}
    combo, seen, refused = 0, set(), 0
    for s_at, step in enumerate(STEPS):
        chw = (C, _down(hw[0], step), _down(hw[1], step))
        sigmas = {p: _sigmas(dev, rng, PARTITIONS[p], chw) for p in range(3)}
        for interp in INTERPS:
            for gauss in (False, True):
                for std_name in STDS:
                    p, chain = (combo + s_at) % 3, CHAINS[(combo // 3 + s_at) % 2]
                    seen.add((step, p, chain))
                    frames, stages, expos, consts = problems[p, chain]
                    kw = dict(consts=consts, stds=sigmas[p] if std_name == "explicit" else None,
                              mean_dtype=torch.float32 if combo % 4 == 3 else torch.float64, **_mode_kw(interp, gauss, std_name, lut_d))
                    label = f"step {step} {interp} gauss={gauss} {std_name} {PARTITIONS[p]} {chain}"
                    has_std = std_name != "none"
                    combo += 1
                    if interp == "lookup" and not gauss and has_std:   # nothing connects the mean to the image: both refuse
                        refused += 1
                        with pytest.raises(RuntimeError, match="does not require grad"):
                            _two_launches(frames, step, stages, expos, layout, **kw)
                        with pytest.raises(RuntimeError, match="does not require grad"):
                            _fused(frames, step, stages, expos, layout, **kw)
                        continue
                    want_state = ops.MergeState(chw, dev, has_std)
                    want = _two_launches(frames, step, stages, expos, layout, state=want_state, **kw)
                    got_state = ops.MergeState(chw, dev, has_std) if combo % 2 else None
                    got = _fused(frames, step, stages, expos, layout, state=got_state, **kw)
                    assert got[0].dtype == kw["mean_dtype"] and tuple(got[0].shape) == chw, label
                    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), label
                    assert (got[1] is not None) == has_std, label
                    if got_state is not None:
                        assert _state_same(got_state, want_state) and got_state.batches == len(PARTITIONS[p]), label
    assert combo == 32 * len(STEPS) and refused == 3 * len(STEPS)
    assert {(s, p) for s, p, _ in seen} == {(s, p) for s in STEPS for p in range(3)}
    assert {(s, ch) for s, _, ch in seen} == {(s, ch) for s in STEPS for ch in CHAINS}


@pytest.mark.parametrize("dtype,layout", [(torch.uint16, "nchw"), (torch.uint8, "nhwc_bgr"), (torch.uint16, "nhwc")])
def test_more_than_one_workgroup(dev, dtype, layout):
    """(75, 141) at step 2 is a plane of 38 x 71 = 2698: three workgroups of 256 threads x 4 elements per plane, six of 256 x 2
    pixels interleaved, an odd row length so that groups straddle rows at every phase, and a ragged last workgroup."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(97)
    hw, step = (75, 141), 2
    chw = (C, 38, 71)
    lut_d = torch.from_numpy(_lut(C)).to(dev)
    for chain, (interp, std_name) in zip(CHAINS, (("linear", "multiplier"), ("catmull", "explicit"))):
        frames, stages, expos, consts = _problem(dev, rng, dtype, layout, hw, [3, 2, 1], chain)
        kw = dict(consts=consts, stds=_sigmas(dev, rng, [3, 2, 1], chw) if std_name == "explicit" else None,
                  **_mode_kw(interp, True, std_name, lut_d))
        want_state, got_state = ops.MergeState(chw, dev, True), ops.MergeState(chw, dev, True)
        want = _two_launches(frames, step, stages, expos, layout, state=want_state, **kw)
        got = _fused(frames, step, stages, expos, layout, state=got_state, **kw)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and _state_same(got_state, want_state), (chain, interp)
        assert float(got[0].abs().max()) > 0


@pytest.mark.parametrize("layout", ["nchw", "nhwc_bgr"])
def test_outputs_four_bytes_behind_a_packet_boundary(dev, monkeypatch, layout):
    """The float32 mean, the std and the two float32 state arrays 4 bytes behind a 256-byte boundary: every packet of theirs is
    misaligned in memory and goes element by element.  Same bits, nothing outside the arrays written, every element written."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(73)
    hw, step = (7, 13), 2
    chw = (C, _down(hw[0], step), _down(hw[1], step))
    lut_d = torch.from_numpy(_lut(C)).to(dev)
    frames, stages, expos, _ = _problem(dev, rng, torch.uint16, layout, hw, [3, 2, 1], "black_clamp")
    kw = dict(mean_dtype=torch.float32, **_mode_kw("linear", True, "multiplier", lut_d))
    want_state = ops.MergeState(chw, dev, True)
    want = _two_launches(frames, step, stages, expos, layout, state=want_state, **kw)
    placed = {}
    inner = ops._merge_setup

    def setup(*args, **kwargs):
        flags, mean_out, std_out = inner(*args, **kwargs)
        placed["mean"], placed["mean_buf"] = mv.sentinel_like(tuple(mean_out.shape), torch.float32, 1, dev)
        placed["std"], placed["std_buf"] = mv.sentinel_like(tuple(std_out.shape), torch.float32, 1, dev)
        return flags, placed["mean"], placed["std"]

    got_state = ops.MergeState(chw, dev, True)
    got_state.sumw, sumw_buf = mv.sentinel_like(chw, torch.float32, 1, dev)
    got_state.var, var_buf = mv.sentinel_like(chw, torch.float32, 1, dev)
    monkeypatch.setattr(ops, "_merge_setup", setup)
    got = _fused(frames, step, stages, expos, layout, state=got_state, **kw)
    monkeypatch.undo()
    assert got[0].data_ptr() % 16 == 4 and got[1].data_ptr() % 16 == 4 and got_state.sumw.data_ptr() % 16 == 4
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and _state_same(got_state, want_state)
    n = int(np.prod(chw))
    for buf in (placed["mean_buf"], placed["std_buf"], sumw_buf, var_buf):
        assert mv.margins_untouched(buf, 1, n) and mv.fully_written(buf, 1, n)


def test_mixed_constants_walk_batch_by_batch(dev):
    """Batches with and without constants in one list cannot be one launch: the same kernels run once per batch with the state in
    memory -- the same bits -- unless one launch is required; a stateless call is lent a state by the front."""
    from clair_torch_amd import ops
    from clair_torch_amd._native import NativeLibraryError
    rng = np.random.default_rng(79)
    hw, step, layout = (7, 13), 3, "nhwc_bgr"
    chw = (C, _down(hw[0], step), _down(hw[1], step))
    lut_d = torch.from_numpy(_lut(C)).to(dev)
    frames, stages, expos, _ = _problem(dev, rng, torch.uint16, layout, hw, [3, 2, 1], "black_clamp")
    consts = [ops.ingest_extrema(frames[0], (), layout), None, ops.ingest_extrema(frames[2], (), layout)]   # unused by this chain
    kw = dict(**_mode_kw("linear", True, "multiplier", lut_d))
    want_state, got_state = ops.MergeState(chw, dev, True), ops.MergeState(chw, dev, True)
    want = _two_launches(frames, step, stages, expos, layout, state=want_state, **kw)
    got = ops.hdr_merge_ingest_batches_strided(frames, step, stages, expos, layout=layout, consts=consts, state=got_state, **kw)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and _state_same(got_state, want_state)
    stateless = ops.hdr_merge_ingest_batches_strided(frames, step, stages, expos, layout=layout, consts=consts, **kw)
    assert _same_bits(stateless[0], want[0]) and _same_bits(stateless[1], want[1])
    with pytest.raises(NativeLibraryError):
        _fused(frames, step, stages, expos, layout, consts=consts, state=ops.MergeState(chw, dev, True), **kw)
    # the single-batch form is the list of one
    one = ops.hdr_merge_ingest_batch_strided(frames[0], step, stages, expos[0], layout=layout, **kw)
    ref = ops.hdr_merge_ingest_batch(ops.strided_downscale(frames[0], step, layout), stages, expos[0], layout=layout, **kw)
    assert _same_bits(one[0], ref[0]) and _same_bits(one[1], ref[1])


# ---- 2. the state: continued, left unfinalized, then finalized ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype,layout", [(torch.uint16, "nchw"), (torch.uint8, "nhwc_bgr")])
@pytest.mark.parametrize("std_name", ["none", "multiplier", "explicit"])
def test_continues_a_merge_and_leaves_it_open(dev, dtype, layout, std_name):
    """State in, ``finalize=False``, then a second call that finalizes -- against one launch per (compacted) batch."""
    from clair_torch_amd import ops
    rng = np.random.default_rng(83)
    hw, step, sizes = (7, 13), 2, [2, 3, 1, 2, 2]
    chw = (C, _down(hw[0], step), _down(hw[1], step))
    lut_d = torch.from_numpy(_lut(C)).to(dev)
    frames, stages, expos, _ = _problem(dev, rng, dtype, layout, hw, sizes, "black_clamp")
    small = [ops.strided_downscale(f, step, layout) for f in frames]
    stds = _sigmas(dev, rng, sizes, chw) if std_name == "explicit" else None
    kw = dict(layout=layout, **_mode_kw("linear", True, std_name, lut_d))
    has_std = std_name != "none"

    def per_batch(a, b, state, finalize):
        out = None
        for k in range(a, b):
            out = ops.hdr_merge_ingest_batch(small[k], stages, expos[k], std=None if stds is None else stds[k], state=state,
                                             finalize=finalize and k == b - 1, **kw)
        return out

    def strided(a, b, state, finalize):
        return ops.hdr_merge_ingest_batches_strided(frames[a:b], step, stages, expos[a:b], stds=None if stds is None else stds[a:b],
                                                    state=state, finalize=finalize, require_one_launch=True, **kw)

    want_state, got_state = ops.MergeState(chw, dev, has_std), ops.MergeState(chw, dev, has_std)
    assert per_batch(0, 1, want_state, False) is None and strided(0, 1, got_state, False) is None   # starts the merge, leaves it open
    assert _state_same(got_state, want_state) and got_state.batches == 1
    assert per_batch(1, 4, want_state, False) is None and strided(1, 4, got_state, False) is None   # not FIRST_BATCH, not FINALIZE
    assert _state_same(got_state, want_state) and got_state.batches == want_state.batches == 4
    want, got = per_batch(4, 5, want_state, True), strided(4, 5, got_state, True)                   # ... and a second call finalizes
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]) and _state_same(got_state, want_state)
    with pytest.raises(ValueError, match="MergeState"):   # a call that is not a whole merge needs the state
        strided(1, 4, None, False)
    with pytest.raises(ValueError, match="MergeState has shape"):   # ... of the downscaled shape
        strided(1, 4, ops.MergeState((C,) + hw, dev, has_std), False)


# ---- 3. the float64 oracle -----------------------------------------------------------------------------------------------------------
def _consistent_codes(rng, n, c, h, w, t, black, span):
    """Exposures of one scene through a gamma curve, on a black level: what the oracle's closed form is well conditioned on."""
    e = rng.random((c, h, w)) * (2.0 / np.sqrt(t[0] * t[-1]))
    lin = np.clip(e[None] * t[:, None, None, None], 0.0, 1.0)
    return torch.from_numpy((black + np.rint(lin ** (1 / 2.2) * span)).astype(np.uint16))


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(17)
    n, c, h, w = 6, 3, 9, 21
    t = 0.002 * 2.0 ** np.arange(n)
    planar = _consistent_codes(rng, n, c, h, w, t, 64, 959)
    planar[:, :, 0, :4] = 10   # below the black level: pixels below 0, clamped with a masked gradient
    return planar, t


@pytest.mark.parametrize("step", [2, 3])
@pytest.mark.parametrize("layout,interp,gauss,std_name", [("nchw", "linear", True, "multiplier"), ("nhwc_bgr", None, False, "constant")])
def test_against_the_float64_oracle(dev, scene, layout, interp, gauss, std_name, step):
    """The frames sliced on the host, a black-level chain run by the transform classes on the CPU, then the float64 oracle of
    the merge tests.  Tolerances: those of test_gpu_merge_ingest.py::test_against_the_float64_oracle."""
    T = _T()
    from oracle import ct_oracle as oc
    planar, t = scene
    chain = [T.CastTo("float32"), T.Normalize(1023, 64)]
    pixels = planar[:, :, ::step, ::step]
    for tr in chain:
        pixels = tr(pixels)
    pixels = np.ascontiguousarray(pixels.numpy())
    assert pixels.dtype == np.float32 and (pixels < 0).any()
    host = _source(planar, layout)
    plan = T.plan_staging(host, ([] if layout == "nchw" else [T.CvToTorch()]) + chain + [T.StridedDownscale(step)], step_in_kernel=True)
    assert plan.route == "ingest" and plan.source_layout == layout and plan.step == step and plan.step_in_kernel
    lut = _lut(3, 256)
    value = 0.05 if std_name == "multiplier" else 0.01
    sd = pixels * np.float32(value) if std_name == "multiplier" else np.full_like(pixels, np.float32(value))
    x, expo = host.to(dev), torch.from_numpy(t)
    mean, std = _fused([x], step, plan.stages, [expo], layout, lut=None if interp is None else torch.from_numpy(lut).to(dev),
                       interp=interp, gaussian_weight=gauss, std_mode=std_name, std_value=value)
    mean_o, std_o = oc.hdr_merge(pixels, sd, t, None if interp is None else lut, interp or "none", gauss)
    assert tuple(mean.shape) == pixels.shape[1:]
    assert_parity(mean.cpu().numpy(), mean_o, rtol=1e-5, norm_tol=1e-6, what=f"{layout} {interp} step {step} mean vs oracle")
    assert_parity(std.cpu().numpy(), std_o, rtol=1e-5, norm_tol=1e-5, what=f"{layout} {interp} step {step} std vs oracle")


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from clair_torch_amd import ops
    lut_d = torch.from_numpy(_lut(C)).to(dev)
    stages = [("affine", 64.0, 959.0, 1.0, 0.0)]
    frames = [torch.zeros((2, C, 7, 13), dtype=torch.uint16, device=dev)] * 2
    expos = [torch.tensor([0.01, 0.02], dtype=torch.float64)] * 2
    kw = dict(lut=lut_d, interp="linear")
    for step in (0, -3, True, False, 2.0):
        with pytest.raises(ValueError, match="step must be an int >= 1"):
            ops.hdr_merge_ingest_batches_strided(frames, step, stages, expos, **kw)
        with pytest.raises(ValueError, match="step must be an int >= 1"):
            ops.hdr_merge_ingest_batch_strided(frames[0], step, stages, expos[0], **kw)
    with pytest.raises(ValueError, match="tile= cannot be combined with step > 1"):
        ops.hdr_merge_ingest_batches_strided(frames, 2, stages, expos, tile=ops.TileGeometry(h_global=14, row_offset=0), **kw)
    floats = [f.to(torch.float32) for f in frames]
    with pytest.raises(TypeError, match="takes uint8 / uint16 codes"):
        ops.hdr_merge_ingest_batches_strided(floats, 2, stages, expos, **kw)
    with pytest.raises(TypeError, match="takes uint8 / uint16 codes"):
        ops.hdr_merge_ingest_batch_strided(floats[0], 2, stages, expos[0], **kw)
    full = [torch.full((2, C, 7, 13), 0.01, dtype=torch.float32, device=dev)] * 2   # explicit stds of the full-size shape
    with pytest.raises(ValueError, match=r"std must be a float32 tensor of shape \(2, 3, 4, 7\)"):
        ops.hdr_merge_ingest_batches_strided(frames, 2, stages, expos, stds=full, **kw)
    with pytest.raises(ValueError, match=r"std must be a float32 tensor of shape \(2, 3, 4, 7\)"):
        ops.hdr_merge_ingest_batch_strided(frames[0], 2, stages, expos[0], std=full[0], **kw)
    with pytest.raises(ValueError, match="MergeState has shape"):
        ops.hdr_merge_ingest_batches_strided(frames, 2, stages, expos, state=ops.MergeState((C, 7, 13), dev, False), **kw)
    # the reference-order modes are not fused, behind a step as without one
    from clair_torch_amd._native import NativeLibraryError
    with pytest.raises(NativeLibraryError):
        ops.hdr_merge_ingest_batches_strided(frames, 2, stages, expos, lut=lut_d, interp="catmull", std_mode="constant", std_value=0.01)
    with pytest.raises(NativeLibraryError):
        ops.hdr_merge_ingest_batches_strided(frames, 2, stages, expos, reference_order=True, **kw)


# ---- 5. compute_hdr_image ---------------------------------------------------------------------------------------------------------------
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


def _api(dev, n, tail):
    """run(batch_size, **kw) -> compute_hdr_image over n raw BGR uint16 frames behind CvToTorch and the list ``tail``."""
    T = _T()
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.datasets import custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    rng = np.random.default_rng(89)
    c, h, w = 3, 7, 13
    t = 0.002 * 1.5 ** np.arange(n)
    frames = _source(torch.from_numpy(rng.integers(40, 1101, size=(n, c, h, w)).astype(np.uint16)), "nhwc_bgr")
    ds = _frames_dataset(frames, t.tolist(), MissingStdMode.MULTIPLIER, 0.05)
    model = ICRFModelDirect(icrf=torch.from_numpy(_lut(c, 256)), interpolation_mode=InterpMode.LINEAR).to(dev)

    def run(batch_size, **kw):
        loader = DataLoader(ds, batch_size=batch_size, shuffle=False, collate_fn=custom_collate)
        return compute_hdr_image(loader, "cuda", model, weight_fn=gaussian_value_weights, gpu_transforms=[T.CvToTorch()] + tail, **kw)

    return run


@pytest.mark.parametrize("batch_size", [2, 3])
@pytest.mark.parametrize("which", ["black_sd", "sd_black", "data_sd"])
def test_compute_hdr_image_fuses_the_downscale(dev, monkeypatch, batch_size, which):
    """A black level in front of and behind the downscale, and a data-dependent Normalize in FRONT of it: with
    ``fused_downscale=True`` ct_strided_downscale never runs and one strided call takes every batch."""
    T = _T()
    from clair_torch_amd import ops
    cast, sd = T.CastTo("float32"), T.StridedDownscale(2)
    tail = {"black_sd": [cast, T.Normalize(1023, 64), sd], "sd_black": [sd, cast, T.Normalize(1023, 64)], "data_sd": [cast, T.Normalize(), sd]}[which]
    run = _api(dev, 6, tail)
    plain = run(batch_size, fused_downscale=False)
    assert tuple(plain[0].shape) == (3, 4, 7) and plain[0].dtype == torch.float64 and plain[1].dtype == torch.float32
    default = run(batch_size)
    assert _same_bits(default[0], plain[0]) and _same_bits(default[1], plain[1])

    def refuse(*args, **kwargs):
        raise AssertionError("ct_strided_downscale ran: the batch was compacted")

    calls, inner = [], ops.hdr_merge_ingest_batches_strided

    def counted(frames_list, step, *args, **kwargs):
        calls.append((len(frames_list), step, tuple(frames_list[0].shape[1:])))
        return inner(frames_list, step, *args, **kwargs)

    monkeypatch.setattr(ops, "strided_downscale", refuse)
    monkeypatch.setattr(ops, "hdr_merge_ingest_batches_strided", counted)
    fused = run(batch_size, fused_downscale=True)
    assert calls == [(6 // batch_size, 2, (7, 13, 3))]   # one call, every batch, the raw full-size frames
    assert _same_bits(fused[0], plain[0]) and _same_bits(fused[1], plain[1])
    with pytest.raises(AssertionError, match="ct_strided_downscale ran"):   # (the proof proves: the other route does compact)
        run(batch_size, fused_downscale=False)


@pytest.mark.parametrize("batch_size", [2, 3])
def test_compute_hdr_image_falls_back_behind_the_downscale(dev, monkeypatch, batch_size):
    """The data-dependent Normalize BEHIND the downscale takes its extrema from the selected pixels: the staging compacts first,
    whatever the keyword says, and the results agree.  So do float32 frames' (materialised through the one helper)."""
    T = _T()
    from clair_torch_amd import ops
    run = _api(dev, 6, [T.StridedDownscale(2), T.CastTo("float32"), T.Normalize()])
    plain = run(batch_size, fused_downscale=False)
    calls, inner = [], ops.strided_downscale

    def counted(stack, step, *args, **kwargs):
        calls.append(step)
        return inner(stack, step, *args, **kwargs)

    def refuse(*args, **kwargs):
        raise AssertionError("the strided front ran behind a compaction")

    monkeypatch.setattr(ops, "strided_downscale", counted)
    monkeypatch.setattr(ops, "hdr_merge_ingest_batches_strided", refuse)
    fused = run(batch_size, fused_downscale=True)
    assert calls == [2] * (6 // batch_size)
    assert tuple(fused[0].shape) == (3, 4, 7) and _same_bits(fused[0], plain[0]) and _same_bits(fused[1], plain[1])
    # the reference-order modes get the float32 stack: downscale, chain, then the float32 merge
    del calls[:]
    run2 = _api(dev, 6, [T.CastTo("float32"), T.Normalize(1023, 64), T.StridedDownscale(2)])
    want = run2(batch_size, fused_downscale=False, reference_order=True)
    assert calls == [2] * (6 // batch_size)
    got = run2(batch_size, fused_downscale=True, reference_order=True)
    assert calls == [2] * (2 * (6 // batch_size))
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
