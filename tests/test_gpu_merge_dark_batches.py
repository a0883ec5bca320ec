"""ct_hdr_merge_dark_batches on the device: several dark-field batches in ONE launch, the streaming state in registers in between.
Its specification is one sentence -- state and outputs are bit for bit those of ct_hdr_merge_dark_batch applied to the batches in
turn on the same state -- so every comparison here is torch.equal on mean state, sum of weights, variance, mean_out and std_out
against that loop (which test_gpu_merge_dark.py holds to ct_dark_field_blur + the float32 merge)."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from _dark_cases import as_dtype as _as_dtype, scene as _scene
from test_merge_dark_batches_host import LDS_EDGE_POINTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _cuts(parts):
    edges = np.cumsum([0] + list(parts))
    return [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def _split(t, cuts):
    return None if t is None else [t[c] for c in cuts]


def _loop(stacks, ts, darks, dark_stds, *, state, finalize=True, stds=None, halos=None, **kw):
    """One ct_hdr_merge_dark_batch launch per batch on ``state``; FINALIZE on the last one."""
    from clair_torch_amd import ops
    out = None
    for i, stack in enumerate(stacks):
        out = ops.hdr_merge_dark_batch(stack, ts[i], darks[i], None if dark_stds is None else dark_stds[i],
                                       std=None if stds is None else stds[i], halo=None if halos is None else halos[i], state=state,
                                       finalize=finalize and i == len(stacks) - 1, reference_order=False, **kw)
    return out


def _multi(stacks, ts, darks, dark_stds, **kw):
    from clair_torch_amd import ops
    kw.setdefault("require_one_launch", True)
    return ops.hdr_merge_dark_batches(stacks, ts, darks, dark_stds, reference_order=False, **kw)


def _assert_same(got, want, st_got, st_want, what):
    if st_got is not None:
        assert torch.equal(st_got.mean, st_want.mean) and torch.equal(st_got.sumw, st_want.sumw), what
        assert (st_got.var is None) == (st_want.var is None) and (st_got.var is None or torch.equal(st_got.var, st_want.var)), what
        assert st_got.batches == st_want.batches, what
    assert (got is None) == (want is None), what
    if got is not None:
        assert got[0].dtype == want[0].dtype and torch.equal(got[0], want[0]), what
        assert (got[1] is None) == (want[1] is None) and (got[1] is None or torch.equal(got[1], want[1])), what
        assert bool(torch.isfinite(got[0]).all()) and (got[1] is None or bool(torch.isfinite(got[1]).all())), what


# (8,3,13,9): rows end inside a thread's group and the plane is no multiple of it; (5,2,3,130): more than one wavefront per
# row band and a 2-column tail; (4,1,2,4): a row of exactly one aligned packet; (6,1,3,5): one group and a one-element tail, each
# with its own walk over the batches; (3,3,2,2): every row is an edge, both reflections fold onto the same row and column.
# The modes are a covering set: every dtype, interpolation, weight, raw std mode and "no dark std" appears at least once.
CASES = [
    # shape, partition, dtype, interp, gauss, raw std, dark std, dark fields per batch (None: one per frame)
    ((8, 3, 13, 9), [4, 4], torch.uint16, "linear", True, "multiplier", True, None),
    ((8, 3, 13, 9), [3, 3, 2], torch.float32, "catmull", True, "explicit", True, None),
    ((8, 3, 13, 9), [1] * 8, torch.uint8, "lookup", True, "constant", True, None),
    ((5, 2, 3, 130), [2, 3], torch.uint16, None, False, "explicit", True, None),
    ((4, 1, 2, 4), [2, 2], torch.float32, "linear", False, "multiplier", True, None),
    ((6, 1, 3, 5), [1, 2, 3], torch.uint8, "linear", True, "multiplier", False, ["shared", "shared", "frames"]),
    ((6, 1, 3, 5), [1, 2, 3], torch.uint16, "catmull", False, "none", False, None),
    ((3, 3, 2, 2), [1, 2], torch.uint16, "catmull", True, "constant", True, None),
]


def _case_id(case):
    shape, parts, dtype, interp, gauss, std_mode, has_dark_std, shared = case
    return "-".join(["x".join(map(str, shape)), "+".join(map(str, parts)) if len(parts) < 8 else "1x8", str(dtype).split(".")[1], str(interp),
                     "gauss" if gauss else "unit", std_mode, "darkstd" if has_dark_std else "nodarkstd"] + (["mixed"] if shared else []))


def _inputs(dev, case, seed=7):
    """The batches of a case as the fronts take them, and the merge keywords."""
    shape, parts, dtype, interp, gauss, std_mode, has_dark_std, shared = case
    n, c, h, w = shape
    x, sd, t, dark, dark_std, lut = _scene(seed + h, n, c, h, w)
    stack, max_code = _as_dtype(x, dtype)
    cuts = _cuts(parts)
    stacks, ts = _split(stack.to(dev), cuts), _split(t, cuts)
    darks, dark_stds = _split(dark.to(dev), cuts), (_split(dark_std.to(dev), cuts) if has_dark_std else None)
    if shared is not None:   # one shared dark field (only without a dark std) for some batches, one per frame for the others
        darks = [d[:1] if kind == "shared" else d for d, kind in zip(darks, shared)]
    kw = dict(lut=None if interp is None else lut.to(dev), interp=interp, gaussian_weight=gauss, max_code=max_code)
    stds = None
    if std_mode == "explicit":
        stds = _split(sd.to(dev), cuts)
    elif std_mode != "none":
        kw.update(std_mode=std_mode, std_value=0.01 if std_mode == "constant" else 0.05)
    return stacks, ts, darks, dark_stds, stds, kw, (c, h, w)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_partitions_and_modes_equal_the_loop(dev, case):
    from clair_torch_amd import ops
    stacks, ts, darks, dark_stds, stds, kw, chw = _inputs(dev, case)
    has_var = dark_stds is not None
    if case[7] is not None:
        assert sorted({int(d.shape[0]) for d in darks}) == [1, 3]       # a shared dark field and one per frame in one call
    st_a, st_b = ops.MergeState(chw, dev, has_var), ops.MergeState(chw, dev, has_var)
    want = _loop(stacks, ts, darks, dark_stds, state=st_a, stds=stds, **kw)
    got = _multi(stacks, ts, darks, dark_stds, state=st_b, stds=stds, **kw)
    _assert_same(got, want, st_b, st_a, _case_id(case))
    # the float32 mean output of the same call
    st_a, st_b = ops.MergeState(chw, dev, has_var), ops.MergeState(chw, dev, has_var)
    want = _loop(stacks, ts, darks, dark_stds, state=st_a, stds=stds, mean_dtype=torch.float32, **kw)
    got = _multi(stacks, ts, darks, dark_stds, state=st_b, stds=stds, mean_dtype=torch.float32, **kw)
    assert got[0].dtype == torch.float32
    _assert_same(got, want, st_b, st_a, _case_id(case))


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[5]], ids=_case_id)
def test_state_before_between_and_none(dev, case):
    from clair_torch_amd import ops
    stacks, ts, darks, dark_stds, stds, kw, chw = _inputs(dev, case, seed=19)
    has_var = dark_stds is not None
    part = lambda v, s: None if v is None else v[s]   # noqa: E731
    # a call without FIRST on a state an earlier (single-batch) call left
    st_a, st_b = ops.MergeState(chw, dev, has_var), ops.MergeState(chw, dev, has_var)
    head, rest = slice(0, 1), slice(1, None)
    for st in (st_a, st_b):
        _loop(stacks[head], ts[head], darks[head], part(dark_stds, head), state=st, finalize=False, stds=part(stds, head), **kw)
    want = _loop(stacks[rest], ts[rest], darks[rest], part(dark_stds, rest), state=st_a, stds=part(stds, rest), **kw)
    if len(stacks[rest]) > 1:
        got = _multi(stacks[rest], ts[rest], darks[rest], part(dark_stds, rest), state=st_b, stds=part(stds, rest), **kw)
        _assert_same(got, want, st_b, st_a, "continues a state")
    # FIRST and no FINALIZE: nothing is returned, the state is the loop's; then a finalising call (also several batches where
    # the partition has them)
    st_a, st_b = ops.MergeState(chw, dev, has_var), ops.MergeState(chw, dev, has_var)
    k = len(stacks)
    a, b = slice(0, max(2, k - 2)), slice(max(2, k - 2), None)
    if k > 2:
        want = _loop(stacks[a], ts[a], darks[a], part(dark_stds, a), state=st_a, finalize=False, stds=part(stds, a), **kw)
        got = _multi(stacks[a], ts[a], darks[a], part(dark_stds, a), state=st_b, finalize=False, stds=part(stds, a), **kw)
        assert got is None and want is None
        _assert_same(got, want, st_b, st_a, "first, not final")
        want = _loop(stacks[b], ts[b], darks[b], part(dark_stds, b), state=st_a, stds=part(stds, b), **kw)
        got = _multi(stacks[b], ts[b], darks[b], part(dark_stds, b), state=st_b, stds=part(stds, b), require_one_launch=False, **kw)
        _assert_same(got, want, st_b, st_a, "the finalising call")
    # FIRST + FINALIZE without state arrays: the same outputs
    st_a = ops.MergeState(chw, dev, has_var)
    want = _loop(stacks, ts, darks, dark_stds, state=st_a, stds=stds, **kw)
    got = _multi(stacks, ts, darks, dark_stds, state=None, stds=stds, **kw)
    _assert_same(got, want, None, None, "no state arrays")
    # exposure times that live on the device already are concatenated there
    got = _multi(stacks, [t.to(dev) for t in ts], darks, dark_stds, state=None, stds=stds, **kw)
    _assert_same(got, want, None, None, "device exposures")


def _condition_ratio(xb, sig, t, lut, w_state=None, mean_state=None):
    """Host evidence, in float64, that a batch trips the conditioning test of the pivoted float32 moments (LINEAR, Gaussian
    weights, a dark std): per element (t1 + |t2| + t3) / (t1 + t2 + t3) of the kernels' epilogue.  The pivot is exposure B / 2
    on a first batch (no state given), else the running mean.  The kernels repeat the batch where it exceeds 8."""
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
    first = w_state is None
    pivot = y[b // 2] if first else mean_state.astype(np.float32).astype(np.float64)
    wgt = np.exp(-30.0 * (x - 0.5) ** 2)
    dw = -60.0 * (x - 0.5) * wgt
    sigma = sig.astype(np.float64)
    a_n, c_n = dw * sigma, (dw * (y - pivot) + wgt * dy) * sigma
    wb = wgt.sum(0)
    D = wb + 1e-6
    qd = ((wgt * (y - pivot)).sum(0) - pivot * 1e-6) / D
    wa = 0.0 if first else w_state.astype(np.float64)
    wt = wa + wb
    gam = 0.0 if first else wa / (wt * wt) * ((pivot - mean_state) + qd)
    beta = (wb / wt) / D
    kap = gam - beta * qd
    t1, t2, t3 = beta * beta * (c_n * c_n).sum(0), 2 * beta * kap * (a_n * c_n).sum(0), kap * kap * (a_n * a_n).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (t1 + np.abs(t2) + t3) / (t1 + t2 + t3)


def test_repeat_about_the_mean_in_the_second_batch(dev):
    """One short exposure (a batch of one: its pivot is its own sample), then seven well-weighted frames that contradict it: the first batch of the launch is well
    conditioned, the second one (pivot: the running mean, which the new frames outweigh) trips the conditioning test
    and is repeated about its own mean -- inside the launch, with the state in registers.  Still the loop's bits."""
    from clair_torch_amd import ops
    n, c, h, w = 8, 3, 8, 32
    x, sd, t, dark, dark_std, lut = _scene(31, n, c, h, w)
    gen = torch.Generator().manual_seed(5)
    x[1:] = 0.4 + 0.2 * torch.rand(x[1:].shape, generator=gen)
    xd, sdd, dd, dsd, lutd = x.to(dev), sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    cuts = _cuts([1, 7])
    kw = dict(lut=lutd, interp="linear", gaussian_weight=True)
    args = [_split(v, cuts) for v in (xd, t, dd, dsd)]
    stds = _split(sdd, cuts)
    st_a, st_b = ops.MergeState((c, h, w), dev, True), ops.MergeState((c, h, w), dev, True)
    # the evidence: batch 0 alone, then batch 1 on the state batch 0 left
    xb, sig = ops.dark_field_blur(args[0][0], args[2][0], args[3][0], std=stds[0])
    ratio0 = _condition_ratio(xb.cpu().numpy(), sig.cpu().numpy(), t[:1].numpy(), lut.numpy())
    _loop(args[0][:1], args[1][:1], args[2][:1], args[3][:1], state=st_a, finalize=False, stds=stds[:1], **kw)
    xb, sig = ops.dark_field_blur(args[0][1], args[2][1], args[3][1], std=stds[1])
    ratio1 = _condition_ratio(xb.cpu().numpy(), sig.cpu().numpy(), t[1:].numpy(), lut.numpy(), st_a.sumw.cpu().numpy(), st_a.mean.cpu().numpy())
    print("condition ratio: first batch max", float(np.nanmax(ratio0)), "second batch: elements > 16:", int((ratio1 > 16).sum()),
          "of", ratio1.size)
    assert float(np.nanmax(ratio0)) < 8, "the first batch would repeat as well"
    assert int((ratio1 > 16).sum()) >= 16, "this stack would not make the merge repeat its second batch"
    want = _loop(args[0][1:], args[1][1:], args[2][1:], args[3][1:], state=st_a, stds=stds[1:], **kw)
    got = _multi(*args, state=st_b, stds=stds, **kw)
    _assert_same(got, want, st_b, st_a, "repeat in the second batch")


def test_bands_with_halo_equal_whole(dev):
    """One image as two row bands, the halo rows taken from the whole image on the host: several batches per launch on the
    bands == one launch per batch on the bands == several batches per launch on the whole image."""
    from clair_torch_amd import ops
    n, c, h, w = 5, 3, 9, 10
    x, sd, t, dark, dark_std, lut = _scene(4, n, c, h, w)
    stack, max_code = _as_dtype(x, torch.uint16)
    stack, sd, dark, dark_std, lut = stack.to(dev), sd.to(dev), dark.to(dev), dark_std.to(dev), lut.to(dev)
    cuts = _cuts([2, 3])
    kw = dict(lut=lut, interp="linear", gaussian_weight=True, max_code=max_code)
    whole = _multi(_split(stack, cuts), _split(t, cuts), _split(dark, cuts), _split(dark_std, cuts), stds=_split(sd, cuts), state=None, **kw)
    for r0, r1 in ((0, 4), (4, 9)):
        halo = torch.zeros((n, c, 2, w), dtype=stack.dtype, device=dev)
        if r0 > 0:
            halo[:, :, 0] = stack[:, :, r0 - 1]
        if r1 < h:
            halo[:, :, 1] = stack[:, :, r1]
        band = [_split(v[:, :, r0:r1].contiguous(), cuts) for v in (stack, dark, dark_std, sd)]
        tile = ops.TileGeometry(h_global=h, row_offset=r0)
        st_a, st_b = ops.MergeState((c, r1 - r0, w), dev, True), ops.MergeState((c, r1 - r0, w), dev, True)
        want = _loop(band[0], _split(t, cuts), band[1], band[2], state=st_a, stds=band[3], halos=_split(halo, cuts), tile=tile, **kw)
        got = _multi(band[0], _split(t, cuts), band[1], band[2], state=st_b, stds=band[3], halos=_split(halo, cuts), tile=tile, **kw)
        _assert_same(got, want, st_b, st_a, (r0, r1))
        assert torch.equal(got[0], whole[0][:, r0:r1]) and torch.equal(got[1], whole[1][:, r0:r1]), (r0, r1)


def test_lds_fallback_walks_the_batches(dev):
    """A LUT that leaves room for the scales of one batch of 4 but not of 16 of them: the call still succeeds, one launch per
    batch, and equals the loop; asked for one launch it is refused."""
    from clair_torch_amd import _native as nv
    from clair_torch_amd import ops
    n, c, h, w = 64, 1, 2, 4
    x, sd, t, dark, dark_std, _ = _scene(3, n, c, h, w, period=4)
    lut = (torch.linspace(0, 1, LDS_EDGE_POINTS) ** 2.2).reshape(1, -1).to(dev)
    cuts = _cuts([4] * 16)
    args = [_split(v.to(dev) if i != 1 else v, cuts) for i, v in enumerate((x, t, dark, dark_std))]
    stds = _split(sd.to(dev), cuts)
    kw = dict(lut=lut, interp="linear", gaussian_weight=True)
    st_a, st_b = ops.MergeState((c, h, w), dev, True), ops.MergeState((c, h, w), dev, True)
    want = _loop(*args, state=st_a, stds=stds, **kw)
    got = _multi(*args, state=st_b, stds=stds, require_one_launch=False, **kw)
    _assert_same(got, want, st_b, st_a, "one launch per batch")
    got = _multi(*args, state=None, stds=stds, require_one_launch=False, **kw)     # the front lends the walk a state
    _assert_same(got, want, None, None, "no state given")
    with pytest.raises(nv.NativeLibraryError):
        _multi(*args, state=ops.MergeState((c, h, w), dev, True), stds=stds, require_one_launch=True, **kw)
    got = _multi(args[0][:2], args[1][:2], args[2][:2], args[3][:2], state=None, stds=stds[:2], require_one_launch=True, **kw)
    want = _loop(args[0][:2], args[1][:2], args[2][:2], args[3][:2], state=ops.MergeState((c, h, w), dev, True), stds=stds[:2], **kw)
    _assert_same(got, want, None, None, "two batches fit one launch")


class _MatchesAllBut:
    """A dark-field dataset that has an image for every frame except ``frames`` (those: MissingValMode.SKIP_BATCH)."""

    def __init__(self, stack, frames):
        self.stack, self.frames = stack, set(frames)

    def get_matching_artefact_images(self, reference_frame_settings_list):
        if set(reference_frame_settings_list) & self.frames:
            return None, None, None, None
        return self.stack.get_matching_artefact_images(reference_frame_settings_list)


@pytest.fixture(scope="module")
def api(dev):
    """20 exposures served one per batch, frame 17 without a dark field, and the one-launch-per-batch results (computed once)."""
    from clair_torch_amd.common.enums import InterpMode
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.inference import compute_hdr_image
    from clair_torch_amd.models import ICRFModelDirect
    from clair_torch_amd.training.losses import gaussian_value_weights
    x, sd, t, dark, dark_std, lut = _scene(5, 20, 3, 6, 10, period=10)
    ds = StackDataset(x, t.tolist(), stds=sd)
    model = ICRFModelDirect(icrf=lut, interpolation_mode=InterpMode.LINEAR).to(dev)
    art = _MatchesAllBut(ArtefactStack(dark[0], dark_std[0]), [ds.files[17]])
    flat = ArtefactStack(0.8 + 0.4 * torch.rand((3, 6, 10), generator=torch.Generator().manual_seed(3)), 0.01 * torch.ones((3, 6, 10)))

    def run(**kw):
        loader = DataLoader(ds, batch_size=1, shuffle=False, collate_fn=custom_collate)
        return compute_hdr_image(loader, "cuda", model, weight_fn=gaussian_value_weights, dark_field_dataset=art, **kw)

    return dict(run=run, flat=flat, per_batch=run(dark_batches_per_launch=1), per_batch_flat=run(dark_batches_per_launch=1, flat_field_dataset=flat))


def _record_calls(monkeypatch):
    from clair_torch_amd import ops
    seen = []
    real = ops.hdr_merge_dark_batches
    monkeypatch.setattr(ops, "hdr_merge_dark_batches", lambda stacks, *a, **k: (seen.append(len(stacks)), real(stacks, *a, **k))[1])
    return seen


def test_api_twenty_batches(dev, api, monkeypatch):
    """Queue full (16), key change at the unmatched frame 17 (1), end of the stream (2)."""
    seen = _record_calls(monkeypatch)
    got = api["run"](dark_batches_per_launch=16)
    assert seen == [16, 1, 2]
    assert torch.equal(got[0], api["per_batch"][0]) and torch.equal(got[1], api["per_batch"][1])
    del seen[:]
    got = api["run"](dark_batches_per_launch=5)
    assert seen == [5, 5, 5, 2, 2]
    assert torch.equal(got[0], api["per_batch"][0]) and torch.equal(got[1], api["per_batch"][1])
    del seen[:]
    api["run"](dark_batches_per_launch=1)
    assert seen == []                                            # one launch per matched batch, as before


def test_api_byte_bound(dev, api, monkeypatch):
    from clair_torch_amd.inference import hdr_merge
    one = 3 * 6 * 10 * (4 + 4 + 4 + 4)                           # a float32 frame, its std, a dark field and a dark std
    monkeypatch.setattr(hdr_merge, "DARK_QUEUE_BYTES", 2 * one - 1)
    seen = _record_calls(monkeypatch)
    got = api["run"](dark_batches_per_launch=16)
    assert seen == [1] * 19
    assert torch.equal(got[0], api["per_batch"][0]) and torch.equal(got[1], api["per_batch"][1])
    del seen[:]
    monkeypatch.setattr(hdr_merge, "DARK_QUEUE_BYTES", 3 * one)
    api["run"](dark_batches_per_launch=16)
    assert seen == [3, 3, 3, 3, 3, 2, 2]


def test_api_flat_field(dev, api, monkeypatch):
    """The state is kept and ``finalize`` deferred to the flat-field epilogue."""
    seen = _record_calls(monkeypatch)
    got = api["run"](dark_batches_per_launch=16, flat_field_dataset=api["flat"])
    assert seen == [16, 1, 2]
    assert torch.equal(got[0], api["per_batch_flat"][0]) and torch.equal(got[1], api["per_batch_flat"][1])
