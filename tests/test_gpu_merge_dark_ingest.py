"""ct_hdr_merge_dark_ingest_batches on the device: a gpu_transforms chain, the dark-field conditional blur and 1 to 16 batches of
the HDR merge in ONE pass over the raw frames.  Its specification is one sentence -- for every batch the state and the outputs
are bit for bit those of ct_ingest_transform (with constants: ct_ingest_transform_data) into a planar float32 stack followed by
ct_hdr_merge_dark_batch on that stack, batch after batch on the same state -- so every comparison here is torch.equal on mean
state, sum of weights, variance, mean_out (float64 and float32) and std_out against that loop (which test_gpu_merge_dark.py holds
to ct_dark_field_blur + the float32 merge), through ops.hdr_merge_dark_ingest_batches and through
compute_hdr_image(fused_dark_ingest=True / False).  No tolerance anywhere: the operations are the same, in the same order."""
import pytest
import torch
from torch.utils.data import DataLoader

from _dark_cases import as_dtype as _as_dtype, scene as _scene
from test_gpu_merge_dark_batches import _assert_same, _cuts, _split
from test_merge_dark_batches_host import LDS_EDGE_POINTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _interleave(planar, layout):
    """(B,3,H,W) RGB planes -> the raw (B,H,W,3) frames of ``layout`` (BGR: what an OpenCV reader hands over)."""
    if layout == "nchw":
        return planar
    return (planar.flip(1) if layout == "nhwc_bgr" else planar).permute(0, 2, 3, 1).contiguous()


def _chain(name, dtype, c):
    """The stage list of a chain on raw frames of ``dtype`` (codes up to ``top``, float32 pixels up to 1)."""
    top = {torch.uint8: 255.0, torch.uint16: 65535.0, torch.float32: 1.0}[dtype]
    black = top / 1024.0 if dtype != torch.float32 else 0.0625          # 64 of 65535: Normalize(65535, 64)
    per_channel = [(0.10 + 0.05 * k, 0.90 - 0.07 * k) for k in range(c)]   # different pairs per channel
    return {
        "black": [("affine", black, top - black, 1.0, 0.0)],
        "range": [("affine", 0.0, top, 1.5, -0.25)],                    # a target range (-0.25, 1.25): values leave [0, 1]
        "clamp": [("affine", 0.0, top, 1.0, 0.0), ("clamp", per_channel)],
        "cast": [],                                                     # the cast alone (float32 pixels: codes would stay codes)
        "four": [("affine", black, top - black, 1.0, 0.0), ("clamp", [(0.02, 0.98)]), ("affine", 0.0, 1.0, 1.1, -0.05), ("clamp", per_channel)],
        "data": [("affine_data", 1.0, 0.0)],                            # a data-dependent Normalize(): min and max of every batch
        "black+data": [("affine", black, 1.0, 1.0, 0.0), ("affine_data", 1.0, 0.0)],
    }[name]


def _consts(frames, stages, layout):
    """Per batch the constants of ``ingest_extrema`` behind the stages in front of the data-dependent one, or None."""
    from clair_torch_amd import ops
    kinds = [st[0] for st in stages]
    if "affine_data" not in kinds:
        return None
    prefix = stages[:kinds.index("affine_data")]
    return [ops.ingest_extrema(f, prefix, layout, None, None) for f in frames]


# planar: (8,3,13,9) rows end inside a thread's group; (5,2,3,130) more than one wavefront per row and a 2-column tail;
# (4,1,2,4) a row of exactly one aligned packet; (6,1,3,5) one group and a one-element tail; (3,3,2,2) every row and column is
# a reflected edge.  interleaved, as raw (B,H,W,3): (6,7,9,3) a one-pixel tail behind four pairs; (4,2,2,3) one pair per row,
# every tap reflected; (5,3,131,3) more than one wavefront per row and a one-pixel tail.  The modes are a covering set: every
# dtype, interpolation, weight, raw std mode, "no dark std", a shared dark field mixed with one per frame, every chain and the
# three layouts appear at least once.
CASES = [
    # planar shape (B,C,H,W), layout, partition, dtype, interp, gauss, raw std, dark std, dark fields per batch, chain
    ((8, 3, 13, 9), "nchw", [4, 4], torch.uint16, "linear", True, "multiplier", True, None, "black"),
    ((8, 3, 13, 9), "nchw", [3, 3, 2], torch.float32, "catmull", True, "explicit", True, None, "clamp"),
    ((8, 3, 13, 9), "nchw", [1] * 8, torch.uint8, "lookup", True, "constant", True, None, "range"),
    ((5, 2, 3, 130), "nchw", [2, 3], torch.uint16, None, False, "explicit", True, None, "four"),
    ((4, 1, 2, 4), "nchw", [2, 2], torch.float32, "linear", False, "multiplier", True, None, "data"),
    ((6, 1, 3, 5), "nchw", [1, 2, 3], torch.uint8, "linear", True, "multiplier", False, ["shared", "shared", "frames"], "black"),
    ((6, 1, 3, 5), "nchw", [1, 2, 3], torch.uint16, "catmull", False, "none", False, None, "black+data"),
    ((3, 3, 2, 2), "nchw", [1, 2], torch.uint16, "catmull", True, "constant", True, None, "clamp"),
    ((8, 3, 13, 9), "nchw", [4, 4], torch.float32, "linear", True, "multiplier", True, None, "cast"),
    ((6, 3, 7, 9), "nhwc_bgr", [1, 2, 3], torch.uint16, "linear", True, "multiplier", True, None, "clamp"),
    ((4, 3, 2, 2), "nhwc", [1, 3], torch.uint8, "catmull", False, "explicit", True, None, "data"),
    ((5, 3, 3, 131), "nhwc_bgr", [2, 3], torch.float32, None, True, "constant", True, None, "four"),
    ((6, 3, 7, 9), "nhwc", [1, 2, 3], torch.float32, "lookup", True, "multiplier", False, ["shared", "shared", "frames"], "range"),
    ((8, 3, 7, 9), "nhwc_bgr", [3, 3, 2], torch.uint16, "catmull", True, "explicit", True, None, "black+data"),
]


def _case_id(case):
    shape, layout, parts, dtype, interp, gauss, std_mode, has_dark_std, shared, chain = case
    return "-".join(["x".join(map(str, shape)), layout, "+".join(map(str, parts)) if len(parts) < 8 else "1x8", str(dtype).split(".")[1],
                     str(interp), "gauss" if gauss else "unit", std_mode, "darkstd" if has_dark_std else "nodarkstd", chain] +
                    (["mixed"] if shared else []))


def _inputs(dev, case, seed=7):
    """The batches of a case as the front takes them, and the merge keywords."""
    from clair_torch_amd import ops
    shape, layout, parts, dtype, interp, gauss, std_mode, has_dark_std, shared, chain = case
    n, c, h, w = shape
    x, sd, t, dark, dark_std, lut = _scene(seed + h, n, c, h, w)
    raw, _ = _as_dtype(x, dtype)
    cuts = _cuts(parts)
    frames, ts = _split(_interleave(raw, layout).to(dev), cuts), _split(t, cuts)
    darks, dark_stds = _split(dark.to(dev), cuts), (_split(dark_std.to(dev), cuts) if has_dark_std else None)
    if shared is not None:   # one shared dark field (only without a dark std) for some batches, one per frame for the others
        darks = [d[:1] if kind == "shared" else d for d, kind in zip(darks, shared)]
    stages = _chain(chain, dtype, c)
    kw = dict(lut=None if interp is None else lut.to(dev), interp=interp, gaussian_weight=gauss)
    stds = None
    if std_mode == "explicit":
        stds = _split(sd.to(dev), cuts)
    elif std_mode != "none":
        kw.update(std_mode=std_mode, std_value=0.01 if std_mode == "constant" else 0.05)
    del ops
    return dict(frames=frames, ts=ts, darks=darks, dark_stds=dark_stds, stds=stds, stages=stages, layout=layout,
                consts=_consts(frames, stages, layout), kw=kw, chw=(c, h, w))


def _loop(inp, *, state, finalize=True, which=None, halos=None, **extra):
    """The yardstick: per batch ct_ingest_transform into the float32 stack (the raw halo rows likewise), then one
    ct_hdr_merge_dark_batch launch on ``state``; FINALIZE on the last one."""
    from clair_torch_amd import ops
    out = None
    which = list(range(len(inp["frames"]))) if which is None else which
    for pos, i in enumerate(which):
        consts = None if inp["consts"] is None else inp["consts"][i]
        x32 = ops.ingest_transform(inp["frames"][i], inp["stages"], inp["layout"], consts=consts)
        halo = None if halos is None else ops.ingest_transform(halos[i], inp["stages"], "nchw", consts=consts)
        out = ops.hdr_merge_dark_batch(x32, inp["ts"][i], inp["darks"][i], None if inp["dark_stds"] is None else inp["dark_stds"][i],
                                       std=None if inp["stds"] is None else inp["stds"][i], halo=halo, state=state,
                                       finalize=finalize and pos == len(which) - 1, reference_order=False, **inp["kw"], **extra)
    return out


def _fused(inp, *, which=None, halos=None, **extra):
    from clair_torch_amd import ops
    which = list(range(len(inp["frames"]))) if which is None else which
    pick = lambda v: None if v is None else [v[i] for i in which]   # noqa: E731
    extra.setdefault("require_one_launch", True)
    return ops.hdr_merge_dark_ingest_batches(pick(inp["frames"]), inp["stages"], pick(inp["ts"]), pick(inp["darks"]), pick(inp["dark_stds"]),
                                             consts=pick(inp["consts"]), stds=pick(inp["stds"]), halos=pick(halos), layout=inp["layout"],
                                             reference_order=False, **inp["kw"], **extra)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_partitions_modes_and_chains_equal_the_composition(dev, case):
    from clair_torch_amd import ops
    inp = _inputs(dev, case)
    has_var = inp["dark_stds"] is not None
    if case[8] is not None:
        assert sorted({int(d.shape[0]) for d in inp["darks"]}) == [1, 3]   # a shared dark field and one per frame in one call
    for mean_dtype in (torch.float64, torch.float32):
        st_a, st_b = ops.MergeState(inp["chw"], dev, has_var), ops.MergeState(inp["chw"], dev, has_var)
        want = _loop(inp, state=st_a, mean_dtype=mean_dtype)
        got = _fused(inp, state=st_b, mean_dtype=mean_dtype)
        assert got[0].dtype == mean_dtype
        _assert_same(got, want, st_b, st_a, _case_id(case))


def test_per_channel_clamp_hits_the_plane_channel_on_bgr(dev):
    """The clamp pairs differ per channel and the frames are BGR: the result depends on which pair a tap gets (feeding the
    pairs in memory order gives other bits), and it is the composition's."""
    from clair_torch_amd import ops
    inp = _inputs(dev, CASES[9])
    want = _loop(inp, state=ops.MergeState(inp["chw"], dev, True))
    got = _fused(inp, state=None)
    _assert_same(got, want, None, None, "plane channel")
    swapped = dict(inp, stages=[inp["stages"][0], ("clamp", list(reversed(inp["stages"][1][1])))])
    other = _fused(swapped, state=None)
    assert not torch.equal(other[0], got[0])


@pytest.mark.parametrize("case", [CASES[0], CASES[6], CASES[13]], ids=_case_id)
def test_carried_state_and_not_final(dev, case):
    """``first=False`` on a state an earlier call left, ``finalize=False``, no state arrays at all, one batch as a list of one."""
    from clair_torch_amd import ops
    inp = _inputs(dev, case, seed=19)
    has_var = inp["dark_stds"] is not None
    k = len(inp["frames"])
    st_a, st_b = ops.MergeState(inp["chw"], dev, has_var), ops.MergeState(inp["chw"], dev, has_var)
    want = _loop(inp, state=st_a, which=[0], finalize=False)
    got = _fused(inp, state=st_b, which=[0], finalize=False)            # one batch: the same kernel with a list of one
    assert got is None and want is None
    _assert_same(got, want, st_b, st_a, "first, not final, a list of one")
    rest = list(range(1, k))
    want = _loop(inp, state=st_a, which=rest)
    st_b.batches = 0                                                   # a state filled elsewhere: ``first`` says so
    got = _fused(inp, state=st_b, which=rest, first=False)
    st_b.batches += 1
    _assert_same(got, want, st_b, st_a, "continues a state")
    want = _loop(inp, state=ops.MergeState(inp["chw"], dev, has_var))
    got = _fused(inp, state=None)
    _assert_same(got, want, None, None, "no state arrays")


def test_two_row_bands_with_raw_halo_rows(dev):
    """One planar image as two row bands, the RAW halo rows cut from the whole image by hand: each band equals the composition
    on the band and the rows of the untiled result."""
    from clair_torch_amd import ops
    n, c, h, w = 5, 3, 9, 10
    case = ((n, c, h, w), "nchw", [2, 3], torch.uint16, "linear", True, "explicit", True, None, "clamp")
    inp = _inputs(dev, case, seed=4)
    whole = _fused(inp, state=None)
    cuts = _cuts(case[2])
    raw = torch.cat(inp["frames"])
    for r0, r1 in ((0, 4), (4, 9)):
        halo = torch.zeros((n, c, 2, w), dtype=raw.dtype, device=dev)
        if r0 > 0:
            halo[:, :, 0] = raw[:, :, r0 - 1]
        if r1 < h:
            halo[:, :, 1] = raw[:, :, r1]
        rows = lambda v: None if v is None else [t[:, :, r0:r1].contiguous() for t in v]   # noqa: E731
        band = dict(inp, frames=rows(inp["frames"]), darks=rows(inp["darks"]), dark_stds=rows(inp["dark_stds"]), stds=rows(inp["stds"]),
                    chw=(c, r1 - r0, w))
        tile = ops.TileGeometry(h_global=h, row_offset=r0)
        st_a, st_b = ops.MergeState(band["chw"], dev, True), ops.MergeState(band["chw"], dev, True)
        want = _loop(band, state=st_a, halos=_split(halo, cuts), tile=tile)
        got = _fused(band, state=st_b, halos=_split(halo, cuts), tile=tile)
        _assert_same(got, want, st_b, st_a, (r0, r1))
        assert torch.equal(got[0], whole[0][:, r0:r1]) and torch.equal(got[1], whole[1][:, r0:r1]), (r0, r1)
    with pytest.raises(ValueError, match="planar frames"):             # no bands on interleaved frames
        bgr = _inputs(dev, CASES[9])
        _fused(bgr, state=None, tile=ops.TileGeometry(h_global=20, row_offset=0))


def test_lds_edge_walks_the_batches(dev):
    """A LUT that leaves room for the scales of one batch of 4 but not of 16 of them: the call still succeeds, one launch per
    batch, and equals the loop; asked for one launch it is refused."""
    from clair_torch_amd import ops
    n, c, h, w = 64, 1, 2, 4
    x, sd, t, dark, dark_std, _ = _scene(3, n, c, h, w, period=4)
    raw, _ = _as_dtype(x, torch.uint16)
    lut = (torch.linspace(0, 1, LDS_EDGE_POINTS) ** 2.2).reshape(1, -1).to(dev)
    cuts = _cuts([4] * 16)
    stages = _chain("black", torch.uint16, c)
    inp = dict(frames=_split(raw.to(dev), cuts), ts=_split(t, cuts), darks=_split(dark.to(dev), cuts), dark_stds=_split(dark_std.to(dev), cuts),
               stds=_split(sd.to(dev), cuts), stages=stages, layout="nchw", consts=None, chw=(c, h, w),
               kw=dict(lut=lut, interp="linear", gaussian_weight=True))
    st_a, st_b = ops.MergeState((c, h, w), dev, True), ops.MergeState((c, h, w), dev, True)
    want = _loop(inp, state=st_a)
    got = _fused(inp, state=st_b, require_one_launch=False)
    _assert_same(got, want, st_b, st_a, "one launch per batch")
    got = _fused(inp, state=None, require_one_launch=False)             # the front lends the walk a state
    _assert_same(got, want, None, None, "no state given")
    with pytest.raises(ValueError, match="too large"):                  # CT_ERR_TOO_LARGE
        _fused(inp, state=ops.MergeState((c, h, w), dev, True), require_one_launch=True)
    got = _fused(inp, state=None, which=[0, 1], require_one_launch=True)
    want = _loop(inp, state=ops.MergeState((c, h, w), dev, True), which=[0, 1])
    _assert_same(got, want, None, None, "two batches fit one launch")


# ---- compute_hdr_image --------------------------------------------------------------------------------------------------------
class _MatchesSome:
    """A dark-field dataset that has an image for the frames in ``frames`` only (the others: MissingValMode.SKIP_BATCH)."""

    def __init__(self, stack, frames):
        self.stack, self.frames = stack, set(frames)

    def get_matching_artefact_images(self, reference_frame_settings_list):
        if not set(reference_frame_settings_list) <= self.frames:
            return None, None, None, None
        return self.stack.get_matching_artefact_images(reference_frame_settings_list)


def _api_case(dev, kind):
    """10 uint16 frames of 3x6x10 in batches of 2, MULTIPLIER uncertainties derived in the kernel: planar frames behind a black
    level, BGR frames behind CvToTorch, or planar frames behind a data-dependent list."""
    from clair_torch_amd.common.enums import InterpMode, MissingStdMode
    from clair_torch_amd.common.transforms import CastTo, CvToTorch, Normalize
    from clair_torch_amd.datasets import ArtefactStack, StackDataset, custom_collate
    from clair_torch_amd.models import ICRFModelDirect
    x, _, t, dark, dark_std, lut = _scene({"black": 41, "bgr": 43, "data": 47}[kind], 10, 3, 6, 10, period=5)
    codes, _ = _as_dtype(x, torch.uint16)
    ds = StackDataset(_interleave(codes, "nhwc_bgr") if kind == "bgr" else codes, t.tolist(), missing_std_mode=MissingStdMode.MULTIPLIER,
                      missing_std_value=0.05, materialize_std=False)
    tf = {"black": [CastTo("float32"), Normalize(65535, 64)], "bgr": [CvToTorch(), CastTo("float32"), Normalize(65535, 0)],
          "data": [CastTo("float32"), Normalize()]}[kind]
    model = ICRFModelDirect(icrf=lut, interpolation_mode=InterpMode.LINEAR).to(dev)
    art = ArtefactStack(dark[0], dark_std[0])
    flat = ArtefactStack(0.8 + 0.4 * torch.rand((3, 6, 10), generator=torch.Generator().manual_seed(3)), 0.01 * torch.ones((3, 6, 10)))

    def run(dark_ds=art, **kw):
        from clair_torch_amd.inference import compute_hdr_image
        from clair_torch_amd.training.losses import gaussian_value_weights
        loader = DataLoader(ds, batch_size=2, shuffle=False, collate_fn=custom_collate)
        return compute_hdr_image(loader, "cuda", model, weight_fn=gaussian_value_weights, gpu_transforms=tf, dark_field_dataset=dark_ds, **kw)

    return dict(run=run, art=art, flat=flat, files=ds.files)


def _equal(got, want, what):
    assert got[0].shape == want[0].shape and got[0].dtype == want[0].dtype, what
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all()), what


@pytest.mark.parametrize("kind", ["black", "bgr", "data"])
def test_compute_hdr_image_routes_are_bit_equal(dev, kind, monkeypatch):
    from clair_torch_amd import ops
    api = _api_case(dev, kind)
    run = api["run"]
    want = run(fused_dark_ingest=False)
    for k in (1, 3):
        _equal(run(fused_dark_ingest=True, dark_batches_per_launch=k), want, (kind, k))
    # a flat field behind the merge (the state is kept, ``finalize`` deferred) and the OpenCV-order export
    for extra in (dict(flat_field_dataset=api["flat"]), dict(output_layout="cv")):
        _equal(run(fused_dark_ingest=True, dark_batches_per_launch=3, **extra), run(fused_dark_ingest=False, **extra), (kind, extra))
    # a dark field for some batches only (SKIP_BATCH for the others): the key changes mid-stream, unmatched batches take the
    # chain + merge queue
    some = _MatchesSome(api["art"], [api["files"][i] for i in (2, 3, 4, 5, 8, 9)])
    want_some = run(some, fused_dark_ingest=False)
    for k in (1, 3):
        _equal(run(some, fused_dark_ingest=True, dark_batches_per_launch=k), want_some, (kind, "some", k))
    assert not torch.equal(want_some[0], want[0])                      # (the correction matters here)
    seen = []
    real = ops.hdr_merge_dark_ingest_batches
    monkeypatch.setattr(ops, "hdr_merge_dark_ingest_batches", lambda frames, *a, **k: (seen.append(len(frames)), real(frames, *a, **k))[1])
    run(some, fused_dark_ingest=True, dark_batches_per_launch=3)
    assert seen == [2, 1]
    del seen[:]
    run(fused_dark_ingest=True, dark_batches_per_launch=3)
    assert seen == [3, 2]
    del seen[:]
    run(fused_dark_ingest=True, fused_dark=False)
    run(fused_dark_ingest=False)
    assert seen == []

    # the fused route is the one that ran: the float32 stack of a batch is never made
    def no_stack(*args, **kwargs):
        raise AssertionError("ct_ingest_transform ran: the batch was materialised")

    monkeypatch.setattr(ops, "ingest_transform", no_stack)
    _equal(run(fused_dark_ingest=True, dark_batches_per_launch=3), want, (kind, "no float32 stack"))
    with pytest.raises(AssertionError, match="materialised"):
        run(fused_dark_ingest=False)
