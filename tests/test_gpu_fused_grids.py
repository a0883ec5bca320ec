"""The fused kernel families beyond their first workgroup in x.

Every fused kernel finds its work as ``slot = blockIdx.x * 256 + threadIdx.x`` (the linearize families walk four slots per
thread).  The families' own test files cross modes, dtypes, layouts, alignments and partitions at shapes of ONE workgroup in
x; this module runs every family at the smallest shapes with three or more workgroups, a ragged last one and an odd row
length, so that a wrong multiplier on blockIdx.x, a ragged-end guard off by one group, a row carry that holds for the first
256 slots only or a per-workgroup preamble only workgroup 0 gets right shows.  tests/_grid_cases.py restates the grids;
tests/test_grid_cases_host.py proves the conditions below on the CPU.

family (kernel files)                              grid in x (host function)                    shape    slots -> workgroups
merge ingest (ct_merge_ingest[_multi].hip)         1 + ceil(plane / 4 | 2) slots / 256 (mi_grid)  38x71    676 -> 3 planar, 1350 -> 6 packed
merge dark (ct_merge_dark[_multi].hip)             ceil(W / 4) H slots / 256 (md_grid)            38x71    684 -> 3
merge dark ingest (ct_merge_dark_ingest*.hip)      as md_grid; packed ceil(W / 2) H               38x71    684 -> 3, 1368 -> 6
statistics ingest (ct_stats_ingest[_multi].hip)    plane / 4 | plane threads / 256 (si_layout)    38x71    674 -> 3 (+ edge launch), 2698 -> 11
statistics, code form (ct_stats_multi.hip)         Q / 4 threads / 256 (stats_grid, V = 4)        3x40x71  2130 -> 9
  ... its V = 1 instantiation                      Q threads / 256                                3x38x71  8094 -> 32
linearize dark (ct_linearize_dark.hip)             ceil(W / 4) H slots / 1024 (ld_launch)         67x131   2211 -> 3
linearize dark ingest, also DATA                   as ld_launch (ldi_launch)                      67x131   2211 -> 3
linearize ingest (ct_linearize_ingest.hip)         1 + ceil(plane / 4) slots / 1024               67x131   2196 -> 3
FLAT forms of _ingest, _strided                    as linearize ingest                            67x131   2196 -> 3
FLAT form of ct_linearize.hip (lin_typed)          Q / 3072 planar, plane / 4 / 256 RGB, Q / 2048   72x131   28296 -> 10, 2358 -> 10, -> 14
  ... its element kernel                           Q / 256                                        67x131   26331 -> 103

Tests, in the order of the rows: test_merge_ingest (+ _against_the_float64_oracle); test_merge_dark and test_merge_dark_ingest
(+ test_dark_merges_against_the_eager_restatement); test_video_stats (forms "ingest" and "code"); test_linearize_dark (forms
"dark", "dark_ingest", "dark_ingest_data"); test_linearize_ingest; test_flat_forms.

The code-form statistics read packets of 4 only where image_stride = C H W is a multiple of 4 (stats_frames_vec_ok), so contiguous
batches never have a vector body AND a V = 1 tail: 3x38x71 (Q = 8094) runs entirely on the V = 1 kernel.  The V = 4 kernel -- the
one of every real frame size -- is therefore taken at 40x71, the next shape with an odd width whose Q is a multiple of 4, in
every design, reference and band case; two "scalar" cases keep 3x38x71 for the V = 1 grid.

Row bands take rows [5, 33) of 38x71 and [9, 58) of 67x131: two workgroups where the whole image has three (the band is
compared with those rows of the whole-image run, which has all of them).

What a case asserts: (1) the family's specification at this shape -- state and outputs bit for bit those of the unfused route
its own test file compares with; (2) nothing outside the outputs is written and all of them are: every output and state array
is a view inside a sentinel-filled buffer (tests/_merge_views.py; the merge fronts allocate their outputs themselves, so
``_merge_setup`` is wrapped for the fused call and hands out such views), the raw frames are unchanged; (3) a mismatch names the
first differing flat index, its (frame, channel, row, column) and the x-workgroup that owns it.  Per family and layout one
case goes to an independent reference at the tolerances of the family's own file, labelled "grid ...": oracle.ct_oracle for
the merge, oracle.eager_torch.merge_stack_dark for the dark merges, _side_refs.video_stats_f64 over _linearize_refs.linearize_f64
for the statistics, _linearize_refs for linearize ingest, eager_torch.linearize_frame_dark for the dark linearize forms.

The axes (dtype, layout, interpolation, std) are not crossed in full -- the families' own files do that at one workgroup:
``_grid_cases.pairwise`` keeps every PAIR of values (the host test checks it).  Beyond pairs the axes do not interact with the
grid: dtype, interpolation and std act on one sample, the layout alone decides the ownership.  Left out because a family does
not take it: float32 frames on merge ingest and statistics ingest (codes only); LOOKUP with uncertainties on the linearize
forms (no gradient path) and LOOKUP at all on the dark linearize forms (no kernel); interleaved frames on merge dark and
linearize dark (planar only) and on a dark row band (no halo is built for them); ``tile=`` on the dark linearize forms (not
taken).  The weights alternate between Gaussian and unit from case to case (LOOKUP: Gaussian, unit weights with
uncertainties are refused).  The FLAT forms: the parent launch goes to _linearize_refs.linearize_f64 at that file's tolerances
("grid flat ... parent"), and the fused launch to the float64 restatement of the correction on the parent's float32 pair at the
ulp bounds of tests/test_gpu_linearize_flat.py (LIN_ULP, SD_ULP, imported; recorded as "grid flat ... ulp")."""
import contextlib
from unittest import mock

import numpy as np
import pytest
import torch

import _grid_cases as gc
import _linearize_refs as lr
import _merge_views as mv
from _side_refs import video_stats_f64
from _util import OBSERVED, assert_parity
from test_gpu_linearize_flat import LIN_ULP, SD_ULP

pytestmark = pytest.mark.gpu

C = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


def _ids(case):
    return "-".join(str(v) for v in case)


# ---- sentinels and the comparison ---------------------------------------------------------------------------------------------
class _Sentinels:
    """The output / state views of one case and the buffers around them."""

    def __init__(self, dev, lead):
        self.dev, self.lead, self.made = dev, lead, []

    def like(self, shape, dtype, name):
        view, buf = mv.sentinel_like(tuple(shape), dtype, self.lead, self.dev)
        self.made.append((name, view, buf))
        return view

    def check(self, what):
        for name, view, buf in self.made:
            assert mv.margins_untouched(buf, self.lead, view.numel()), f"{what}: {name} was written outside the array"
            assert mv.fully_written(buf, self.lead, view.numel()), f"{what}: {name} was not written everywhere"

    def state(self, chw, has_var):
        from clair_torch_amd import ops
        st = ops.MergeState((1, 1, 1), self.dev, has_var)
        st.mean = self.like(chw, torch.float64, "mean state")
        st.sumw = self.like(chw, torch.float32, "sumw state")
        st.var = self.like(chw, torch.float32, "var state") if has_var else None
        return st

    @contextlib.contextmanager
    def merge_outputs(self):
        """While active, the merge fronts' own (mean_out, std_out) are such views too."""
        from clair_torch_amd import ops
        real = ops._merge_setup

        def setup(*args, **kw):
            flags, mean_out, std_out = real(*args, **kw)
            swap = lambda t, name: None if t is None else self.like(t.shape, t.dtype, name)   # noqa: E731
            return flags, swap(mean_out, "mean_out"), swap(std_out, "std_out")

        with mock.patch.object(ops, "_merge_setup", setup):
            yield


def _same(got, want, family, layout, what, lead=0, owner_of=None):
    if got is None or want is None:
        assert got is None and want is None, what
        return
    msg = gc.where_differs(got.detach().cpu().numpy(), want.detach().cpu().numpy(), family, layout, lead, owner_of)
    assert msg is None, f"{what}: {msg}"


def _same_state(a, b, family, layout, what):
    _same(a.mean, b.mean, family, layout, what + " mean state")
    _same(a.sumw, b.sumw, family, layout, what + " sumw state")
    _same(a.var, b.var, family, layout, what + " var state")


def _raw(planar, layout, dev):
    """(the raw stack of ``layout`` on the device, a copy kept to show that the kernels only read it)"""
    host = torch.from_numpy(gc.to_layout(planar, layout))
    x = host.to(dev)
    return x, host


def _unchanged(frames, what):
    for x, host in frames:
        alias = torch.int16 if host.dtype == torch.uint16 else host.dtype
        assert torch.equal(x.cpu().view(alias), host.view(alias)), f"{what}: the raw frames were written"


def _merge_kw(dev, interp, std, gauss, sigma):
    """The merge keywords of a mode; ``sigma``: per batch the explicit planar uncertainties (device)."""
    kw = dict(lut=None if interp is None else torch.from_numpy(gc.lut()).to(dev), interp=interp, gaussian_weight=gauss)
    if std not in ("none", "explicit"):
        kw.update(std_mode=std, std_value=0.01 if std == "constant" else 0.05)
    if interp in ("lookup", "catmull") and std != "none":
        kw["reference_order"] = False      # CT_MERGE_CLOSED_FORM: the reference-order kernel is not fused
    return kw, (sigma if std == "explicit" else [None] * len(sigma))


def _gauss(k, interp):
    return True if interp == "lookup" else k % 2 == 0


PARTS = ((0, 3), (3, 5), (5, 7))     # [3, 2] in one launch, then a call of one batch of 2 that continues from its state


# ---- merge ingest -------------------------------------------------------------------------------------------------------------
MERGE_INGEST = [(k,) + t + ("plain",) for k, t in enumerate(gc.merge_ingest_design())] + [
    (100, "u16", "nchw", "linear", "multiplier", "consts"), (101, "u8", "nhwc_bgr", "catmull", "none", "consts"),
    (102, "u16", "nchw", "linear", "explicit", "band"), (103, "u8", "nhwc", "catmull", "multiplier", "band"),
    (104, "u16", "nhwc_bgr", None, "constant", "band")]


@pytest.mark.parametrize("case", MERGE_INGEST, ids=_ids)
def test_merge_ingest(dev, case):
    """ct_hdr_merge_ingest_batches ([3, 2], one launch) and ct_hdr_merge_ingest_batch continuing from its state, against
    ct_ingest_transform + ct_hdr_merge_batch batch by batch."""
    from clair_torch_amd import ops
    k, dtype, layout, interp, std, variant = case
    h, w = gc.S1
    planar = gc.random_codes(300 + k, (7, C, h, w), dtype)
    sigma = gc.explicit_sigma(300 + k, planar.shape)
    r0, r1 = gc.BAND1 if variant == "band" else (0, h)
    tile = ops.TileGeometry(h_global=h, row_offset=r0) if variant == "band" else None
    whole, _ = _raw(planar, layout, dev)
    frames = [_raw(planar[a:b, :, r0:r1], layout, dev) for a, b in PARTS]
    sig = [torch.from_numpy(np.ascontiguousarray(sigma[a:b, :, r0:r1])).to(dev) for a, b in PARTS]
    t = [torch.tensor([0.004 * 2.0 ** j for j in range(a, b)], dtype=torch.float64) for a, b in PARTS]
    stages = [("affine_data", 1.0, 0.0)] if variant == "consts" else gc.black_level_stages(dtype)
    consts = [ops.ingest_extrema(x, (), layout) for x, _ in frames] if variant == "consts" else None
    kw, sig = _merge_kw(dev, interp, std, _gauss(k, interp), sig)
    kw["mean_dtype"] = torch.float32 if k % 3 == 0 else torch.float64
    chw, has_var, lead = (C, r1 - r0, w), std != "none", k % 2
    what = _ids(case)

    st_u = ops.MergeState(chw, dev, has_var)
    for i in range(3):
        x32 = ops.ingest_transform(frames[i][0], stages, layout, consts=None if consts is None else consts[i])
        want = ops.hdr_merge_batch(x32, t[i], std=sig[i], state=st_u, finalize=i == 2, tile=tile, **kw)

    sen = _Sentinels(dev, lead)
    st_f = sen.state(chw, has_var)
    first = ops.hdr_merge_ingest_batches([f[0] for f in frames[:2]], stages, t[:2], stds=None if sig[0] is None else sig[:2], state=st_f,
                                         finalize=False, tile=tile, layout=layout, consts=None if consts is None else consts[:2],
                                         require_one_launch=True, **kw)
    assert first is None and st_f.batches == 2
    sen.check(what + " after [3, 2]")
    with sen.merge_outputs():
        got = ops.hdr_merge_ingest_batch(frames[2][0], stages, t[2], std=sig[2], state=st_f, finalize=True, tile=tile, layout=layout,
                                         consts=None if consts is None else consts[2], **kw)
    _same(got[0], want[0], "merge_ingest", layout, what + " mean")
    _same(got[1], want[1], "merge_ingest", layout, what + " std")
    _same_state(st_f, st_u, "merge_ingest", layout, what)
    sen.check(what)
    assert len(sen.made) == (3 if has_var else 2) + (2 if has_var else 1)
    _unchanged(frames, what)
    if variant == "band":      # the band is those rows of the whole image, bit for bit
        tw = torch.cat(t)
        sw = None if sig[0] is None else torch.from_numpy(sigma).to(dev)
        full = ops.hdr_merge_ingest_batch(whole, stages, tw, std=sw, layout=layout, **kw)
        part = ops.hdr_merge_ingest_batch(torch.cat([f[0] for f in frames]), stages, tw, std=None if sw is None else sw[:, :, r0:r1].contiguous(),
                                          tile=tile, layout=layout, **kw)
        for j in range(2):
            _same(part[j], None if full[j] is None else full[j][:, r0:r1].contiguous(), "merge_ingest", layout, what + " band of the whole")


@pytest.mark.parametrize("layout,interp,gauss,std", [("nchw", "linear", True, "multiplier"), ("nhwc", "linear", False, "constant"),
                                                     ("nhwc_bgr", None, False, "constant")])
def test_merge_ingest_against_the_float64_oracle(dev, layout, interp, gauss, std):
    """The tolerances of tests/test_gpu_merge_ingest.py::test_against_the_float64_oracle."""
    from clair_torch_amd import ops
    from oracle import ct_oracle as oc
    h, w = gc.S1
    planar, t = gc.scene_codes(17, 5, (C, h, w), "u16")
    stages = gc.black_level_stages("u16")
    pixels = gc.chain_f32(planar, stages)
    sd = gc.sigma_of(std, pixels, None)
    x, host = _raw(planar, layout, dev)
    kw, _ = _merge_kw(dev, interp, std, gauss, [None])
    sen = _Sentinels(dev, 1)
    with sen.merge_outputs():
        mean, sdev = ops.hdr_merge_ingest_batch(x, stages, torch.from_numpy(t), layout=layout, **kw)
    sen.check(layout)
    assert [name for name, _, _ in sen.made] == ["mean_out", "std_out"]      # (the wrapper of _merge_setup was used)
    _unchanged([(x, host)], layout)
    mean_o, std_o = oc.hdr_merge(pixels, sd, t, None if interp is None else gc.lut(), interp or "none", gauss)
    assert_parity(mean.cpu().numpy(), mean_o, rtol=1e-5, norm_tol=1e-6, what=f"grid merge ingest {layout} {interp} mean vs oracle")
    assert_parity(sdev.cpu().numpy(), std_o, rtol=1e-5, norm_tol=1e-5, what=f"grid merge ingest {layout} {interp} std vs oracle")


# ---- the dark merges ----------------------------------------------------------------------------------------------------------
def _halos(planar, r0, r1, dev):
    """Per batch the RAW rows above and below the band (B,C,2,W); rows outside the image stay 0 (they are reflected)."""
    n, c, h, w = planar.shape
    halo = np.zeros((n, c, 2, w), dtype=planar.dtype)
    if r0 > 0:
        halo[:, :, 0] = planar[:, :, r0 - 1]
    if r1 < h:
        halo[:, :, 1] = planar[:, :, r1]
    return [torch.from_numpy(np.ascontiguousarray(halo[a:b])).to(dev) for a, b in PARTS]


MERGE_DARK = [(k,) + t + ("plain",) for k, t in enumerate(gc.merge_dark_design())] + [(100, "u16", "linear", "explicit", "band"),
                                                                                      (101, "f32", "catmull", "multiplier", "band")]


@pytest.mark.parametrize("case", MERGE_DARK, ids=_ids)
def test_merge_dark(dev, case):
    """ct_hdr_merge_dark_batches ([3, 2], one launch) and ct_hdr_merge_dark_batch continuing from its state, against
    ct_dark_field_blur + ct_hdr_merge_batch (closed form) batch by batch."""
    from clair_torch_amd import ops
    k, dtype, interp, std, variant = case
    h, w = gc.S1
    planar = gc.random_codes(400 + k, (7, C, h, w), dtype)
    sigma = gc.explicit_sigma(400 + k, planar.shape)
    dark, dark_std = gc.dark_fields(400 + k, planar.shape)
    r0, r1 = gc.BAND1 if variant == "band" else (0, h)
    tile = ops.TileGeometry(h_global=h, row_offset=r0) if variant == "band" else None
    halos = _halos(planar, r0, r1, dev) if variant == "band" else [None] * 3
    cut = lambda a: [torch.from_numpy(np.ascontiguousarray(a[i:j, :, r0:r1])).to(dev) for i, j in PARTS]   # noqa: E731
    frames = [_raw(planar[a:b, :, r0:r1], "nchw", dev) for a, b in PARTS]
    sig, darks, dark_stds = cut(sigma), cut(dark), cut(dark_std)
    t = [torch.tensor([0.004 * 2.0 ** j for j in range(a, b)], dtype=torch.float64) for a, b in PARTS]
    kw, sig = _merge_kw(dev, interp, std, _gauss(k, interp), sig)
    kw["reference_order"] = False
    lead, chw, what = k % 2, (C, r1 - r0, w), _ids(case)
    mean_dtype = torch.float32 if k % 3 == 0 else torch.float64
    blur_kw = {q: kw[q] for q in ("std_mode", "std_value") if q in kw}
    merge_kw = {q: v for q, v in kw.items() if q not in ("std_mode", "std_value")}

    st_u = ops.MergeState(chw, dev, True)
    for i in range(3):
        xb, se = ops.dark_field_blur(frames[i][0], darks[i], dark_stds[i], std=sig[i], tile=tile, halo=halos[i], **blur_kw)
        want = ops.hdr_merge_batch(xb, t[i], std=se, state=st_u, finalize=i == 2, tile=tile, mean_dtype=mean_dtype, **merge_kw)

    sen = _Sentinels(dev, lead)
    st_f = sen.state(chw, True)
    first = ops.hdr_merge_dark_batches([f[0] for f in frames[:2]], t[:2], darks[:2], dark_stds[:2], stds=None if sig[0] is None else sig[:2],
                                       state=st_f, finalize=False, tile=tile, halos=None if halos[0] is None else halos[:2],
                                       require_one_launch=True, mean_dtype=mean_dtype, **kw)
    assert first is None and st_f.batches == 2
    sen.check(what + " after [3, 2]")
    with sen.merge_outputs():
        got = ops.hdr_merge_dark_batch(frames[2][0], t[2], darks[2], dark_stds[2], std=sig[2], state=st_f, finalize=True, tile=tile,
                                       halo=halos[2], mean_dtype=mean_dtype, **kw)
    _same(got[0], want[0], "merge_dark", "nchw", what + " mean")
    _same(got[1], want[1], "merge_dark", "nchw", what + " std")
    _same_state(st_f, st_u, "merge_dark", "nchw", what)
    sen.check(what)
    assert len(sen.made) == 3 + 2      # three state arrays, and the front's own two outputs through the wrapper of _merge_setup
    _unchanged(frames, what)
    if variant == "band":
        every = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
        sw = every(sigma) if sig[0] is not None else None
        full = ops.hdr_merge_dark_batch(every(planar), torch.cat(t), every(dark), every(dark_std), std=sw, mean_dtype=mean_dtype, **kw)
        part = ops.hdr_merge_dark_batch(torch.cat([f[0] for f in frames]), torch.cat(t), torch.cat(darks), torch.cat(dark_stds),
                                        std=None if sw is None else torch.cat(sig), tile=tile, halo=torch.cat(halos), mean_dtype=mean_dtype, **kw)
        for j in range(2):
            _same(part[j], full[j][:, r0:r1].contiguous(), "merge_dark", "nchw", what + " band of the whole")


MERGE_DARK_INGEST = [(k,) + t + ("plain",) for k, t in enumerate(gc.merge_dark_ingest_design())] + [
    (100, "u16", "nchw", "linear", "multiplier", "consts"), (101, "f32", "nhwc_bgr", "catmull", "explicit", "consts"),
    (102, "u8", "nhwc", None, "constant", "consts"), (103, "u16", "nchw", "linear", "explicit", "band")]


@pytest.mark.parametrize("case", MERGE_DARK_INGEST, ids=_ids)
def test_merge_dark_ingest(dev, case):
    """ct_hdr_merge_dark_ingest_batches ([3, 2] in one launch, then a list of one on the same state) against
    ct_ingest_transform + ct_hdr_merge_dark_batch batch by batch."""
    from clair_torch_amd import ops
    k, dtype, layout, interp, std, variant = case
    h, w = gc.S1
    planar = gc.random_codes(500 + k, (7, C, h, w), dtype)
    sigma = gc.explicit_sigma(500 + k, planar.shape)
    dark, dark_std = gc.dark_fields(500 + k, planar.shape)
    r0, r1 = gc.BAND1 if variant == "band" else (0, h)
    tile = ops.TileGeometry(h_global=h, row_offset=r0) if variant == "band" else None
    halos = _halos(planar, r0, r1, dev) if variant == "band" else None
    cut = lambda a: [torch.from_numpy(np.ascontiguousarray(a[i:j, :, r0:r1])).to(dev) for i, j in PARTS]   # noqa: E731
    frames = [_raw(planar[a:b, :, r0:r1], layout, dev) for a, b in PARTS]
    sig, darks, dark_stds = cut(sigma), cut(dark), cut(dark_std)
    t = [torch.tensor([0.004 * 2.0 ** j for j in range(a, b)], dtype=torch.float64) for a, b in PARTS]
    stages = [("affine_data", 1.0, 0.0)] if variant == "consts" else gc.black_level_stages(dtype)
    consts = [ops.ingest_extrema(x, (), layout) for x, _ in frames] if variant == "consts" else None
    kw, sig = _merge_kw(dev, interp, std, _gauss(k, interp), sig)
    kw.update(reference_order=False, mean_dtype=torch.float32 if k % 3 == 0 else torch.float64)
    lead, chw, what = k % 2, (C, r1 - r0, w), _ids(case)

    st_u = ops.MergeState(chw, dev, True)
    for i in range(3):
        ci = None if consts is None else consts[i]
        x32 = ops.ingest_transform(frames[i][0], stages, layout, consts=ci)
        halo = None if halos is None else ops.ingest_transform(halos[i], stages, "nchw", consts=ci)
        want = ops.hdr_merge_dark_batch(x32, t[i], darks[i], dark_stds[i], std=sig[i], halo=halo, state=st_u, finalize=i == 2, tile=tile, **kw)

    def fused(which, **extra):
        pick = lambda v: None if v is None or v[0] is None else [v[i] for i in which]   # noqa: E731
        return ops.hdr_merge_dark_ingest_batches([frames[i][0] for i in which], stages, pick(t), pick(darks), pick(dark_stds), consts=pick(consts),
                                                 stds=pick(sig), halos=pick(halos), tile=tile, layout=layout, require_one_launch=True, **kw, **extra)

    sen = _Sentinels(dev, lead)
    st_f = sen.state(chw, True)
    assert fused([0, 1], state=st_f, finalize=False) is None and st_f.batches == 2
    sen.check(what + " after [3, 2]")
    with sen.merge_outputs():
        got = fused([2], state=st_f, finalize=True)
    family = "merge_dark_ingest"
    _same(got[0], want[0], family, layout, what + " mean")
    _same(got[1], want[1], family, layout, what + " std")
    _same_state(st_f, st_u, family, layout, what)
    sen.check(what)
    assert len(sen.made) == 3 + 2      # three state arrays, and the front's own two outputs through the wrapper of _merge_setup
    _unchanged(frames, what)
    if variant == "band":
        every = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
        stds = None if sig[0] is None else [every(sigma)]
        full = ops.hdr_merge_dark_ingest_batches([every(planar)], stages, [torch.cat(t)], [every(dark)], [every(dark_std)], stds=stds, **kw)
        part = ops.hdr_merge_dark_ingest_batches([torch.cat([f[0] for f in frames])], stages, [torch.cat(t)], [torch.cat(darks)],
                                                 [torch.cat(dark_stds)], stds=None if stds is None else [torch.cat(sig)],
                                                 halos=[torch.cat(halos)], tile=tile, **kw)
        for j in range(2):
            _same(part[j], full[j][:, r0:r1].contiguous(), family, layout, what + " band of the whole")


@pytest.mark.parametrize("family,layout", [("merge_dark", "nchw"), ("merge_dark_ingest", "nchw"), ("merge_dark_ingest", "nhwc"),
                                           ("merge_dark_ingest", "nhwc_bgr")])
def test_dark_merges_against_the_eager_restatement(dev, family, layout):
    """LINEAR, Gaussian weights, explicit uncertainties, one dark field matched to every frame, batches [3, 2]: the
    tolerances of tests/test_gpu_merge_dark.py::test_compute_hdr_image_fused_dark."""
    from clair_torch_amd import ops
    from oracle import eager_torch as oe
    h, w = gc.S1
    dtype = "f32" if family == "merge_dark" else "u16"
    planar, t = gc.scene_codes(23, 5, (C, h, w), dtype)
    stages = gc.black_level_stages(dtype) if family == "merge_dark_ingest" else []
    pixels = gc.chain_f32(planar, stages)
    sigma = gc.explicit_sigma(23, planar.shape)
    dark, dark_std = (a[0] for a in gc.dark_fields(23, (1, C, h, w)))
    parts = ((0, 3), (3, 5))
    every = lambda a, i, j: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (j - i, C, h, w)))).to(dev)   # noqa: E731
    frames = [_raw(planar[i:j], layout, dev) for i, j in parts]
    ts = [torch.from_numpy(t[i:j]) for i, j in parts]
    darks, dark_stds = [every(dark, i, j) for i, j in parts], [every(dark_std, i, j) for i, j in parts]
    stds = [torch.from_numpy(sigma[i:j]).to(dev) for i, j in parts]
    lut = torch.from_numpy(gc.lut())
    kw = dict(lut=lut.to(dev), interp="linear", gaussian_weight=True, stds=stds, require_one_launch=True)
    sen = _Sentinels(dev, 1)
    with sen.merge_outputs():
        if family == "merge_dark":
            mean, sdev = ops.hdr_merge_dark_batches([f[0] for f in frames], ts, darks, dark_stds, **kw)
        else:
            mean, sdev = ops.hdr_merge_dark_ingest_batches([f[0] for f in frames], stages, ts, darks, dark_stds, layout=layout, **kw)
    sen.check(family)
    assert [name for name, _, _ in sen.made] == ["mean_out", "std_out"]
    _unchanged(frames, family)
    mean_o, std_o = oe.merge_stack_dark(torch.from_numpy(pixels), torch.from_numpy(sigma), torch.from_numpy(t), lut, torch.from_numpy(dark),
                                        torch.from_numpy(dark_std), "linear", True, [3, 2])
    assert_parity(mean.cpu().numpy(), mean_o.numpy(), rtol=1e-5, norm_tol=1e-6, what=f"grid {family} {layout} mean linear")
    assert_parity(sdev.cpu().numpy(), std_o.numpy(), norm_tol=1e-5, elem_tol=1e-5, what=f"grid {family} {layout} std linear")


# ---- the statistics -----------------------------------------------------------------------------------------------------------
STATS = [("ingest", k) + t + ("plain",) for k, t in enumerate(gc.stats_design("ingest"))] + [
    ("ingest", 100, "u16", "nchw", "linear", "consts"), ("ingest", 101, "u8", "nhwc_bgr", "catmull", "consts"),
    ("ingest", 102, "u16", "nchw", "catmull", "band"), ("ingest", 103, "u8", "nhwc", "linear", "band")] + [
    ("code", k) + t + ("plain",) for k, t in enumerate(gc.stats_design("code"))] + [
    ("code", 100, "u16", "nchw", "linear", "band"), ("code", 101, "f32", "nhwc_bgr", "catmull", "band"),
    ("code", 200, "u16", "nchw", "linear", "scalar"), ("code", 201, "u8", "nhwc", "catmull", "scalar")]
# the first case of every form and layout also goes to float64
STATS_REFERENCE = {(form, min(k for k, t in enumerate(gc.stats_design(form)) if t[1] == layout)) for form in ("ingest", "code")
                   for layout in gc.LAYOUTS}
CODE_PARTS = ((0, 3), (3, 5), (5, 6), (6, 7))     # the code form continues with a second LIST: [1, 1]


@pytest.mark.parametrize("case", STATS, ids=_ids)
def test_video_stats(dev, case):
    """ct_video_stats_ingest_batches / ct_video_stats_batches on [3, 2] in one launch, then the continuation (ingest: the
    single-batch kernel; code form: a second list) against one launch per batch on the unfused route (ingest:
    ct_ingest_transform + ct_video_stats_batch).  The first cases of every layout also go to float64."""
    from clair_torch_amd import ops
    form, k, dtype, layout, interp, variant = case
    h, w = gc.S1_CODE if form == "code" and variant != "scalar" else gc.S1
    if form == "code":      # (which instantiation runs: packets of 4, or single elements at 3x38x71)
        assert gc.stats_frames_vec_ok(C, h, w) == (variant != "scalar")
    planar = gc.random_codes(600 + k, (7, C, h, w), dtype)
    r0, r1 = gc.BAND1 if variant == "band" else (0, h)
    tile = ops.TileGeometry(h_global=h, row_offset=r0) if variant == "band" else None
    frames = [_raw(planar[a:b, :, r0:r1], layout, dev) for a, b in (PARTS if form == "ingest" else CODE_PARTS)]
    stages = [("affine_data", 1.0, 0.0)] if variant == "consts" else gc.black_level_stages(dtype)
    consts = [ops.ingest_extrema(x, (), layout) for x, _ in frames] if variant == "consts" else None
    lut = gc.lut()
    kw = dict(lut=None if interp is None else torch.from_numpy(lut).to(dev), interp=interp, tile=tile)
    chw, family, what = (C, r1 - r0, w), "stats_" + ("ingest" if form == "ingest" else "multi"), _ids(case)
    lead = k % 2 if form == "ingest" else 0      # (the code form's packets need 16-byte aligned states: stats_split)
    mean_u, m2_u = (torch.full(chw, mv.SENTINEL, dtype=torch.float32, device=dev) for _ in range(2))
    before = 0
    for i, (x, _) in enumerate(frames):
        if form == "ingest":
            x32 = ops.ingest_transform(x, stages, layout, consts=None if consts is None else consts[i])
            ops.video_stats_batch(x32, mean_u, m2_u, before, **kw)
        else:
            ops.video_stats_batch(x, mean_u, m2_u, before, layout=layout, **kw)
        before += x.shape[0]

    sen = _Sentinels(dev, lead)
    mean_f, m2_f = sen.like(chw, torch.float32, "mean state"), sen.like(chw, torch.float32, "m2 state")
    xs = [f[0] for f in frames]
    if form == "ingest":
        ops.video_stats_ingest_batches(xs[:2], stages, mean_f, m2_f, 0, layout=layout, consts=None if consts is None else consts[:2],
                                       require_one_launch=True, **kw)
        sen.check(what + " after [3, 2]")
        ops.video_stats_ingest_batch(xs[2], stages, mean_f, m2_f, 5, layout=layout, consts=None if consts is None else consts[2], **kw)
    else:
        ops.video_stats_batches(xs[:2], mean_f, m2_f, 0, layout=layout, require_one_launch=True, **kw)
        sen.check(what + " after [3, 2]")
        ops.video_stats_batches(xs[2:], mean_f, m2_f, 5, layout=layout, require_one_launch=True, **kw)
    _same(mean_f, mean_u, family, layout, what + " mean", lead)
    _same(m2_f, m2_u, family, layout, what + " m2", lead)
    sen.check(what)
    _unchanged(frames, what)
    if (form, k) in STATS_REFERENCE:
        pixels = gc.chain_f32(planar, stages) if form == "ingest" else lr.to_pixels(planar, dtype, gc.TOP[dtype])
        x_lin = lr.linearize_f64(pixels, None, lut, interp)[0]
        mean_o, std_o = video_stats_f64(x_lin, [7])
        std = np.sqrt(m2_f.cpu().numpy().astype(np.float64) / 6.0) / np.sqrt(7.0)
        assert_parity(mean_f.cpu().numpy(), mean_o, rtol=1e-6, norm_tol=1e-7, what=f"grid video {form} {layout} {interp} mean")
        assert_parity(std, std_o, rtol=1e-4, norm_tol=1e-6, what=f"grid video {form} {layout} {interp} std")
    if variant == "band":
        whole, _ = _raw(planar, layout, dev)
        mean_w, m2_w = (torch.zeros((C, h, w), dtype=torch.float32, device=dev) for _ in range(2))
        if form == "ingest":
            ops.video_stats_ingest_batch(whole, stages, mean_w, m2_w, 0, layout=layout, **dict(kw, tile=None))
        else:
            ops.video_stats_batches([whole[:3].contiguous(), whole[3:].contiguous()], mean_w, m2_w, 0, layout=layout, **dict(kw, tile=None))
        mean_b, m2_b = (torch.zeros(chw, dtype=torch.float32, device=dev) for _ in range(2))
        band = torch.cat(xs)
        if form == "ingest":
            ops.video_stats_ingest_batch(band, stages, mean_b, m2_b, 0, layout=layout, **kw)
        else:
            ops.video_stats_batches([band[:3].contiguous(), band[3:].contiguous()], mean_b, m2_b, 0, layout=layout, **kw)
        _same(mean_b, mean_w[:, r0:r1].contiguous(), family, layout, what + " band of the whole, mean")
        _same(m2_b, m2_w[:, r0:r1].contiguous(), family, layout, what + " band of the whole, m2")


# ---- linearize ----------------------------------------------------------------------------------------------------------------
F = 3


def _lin_std(std, sigma_dev):
    if std == "explicit":
        return dict(std=sigma_dev)
    return dict(std_mode=std, std_value=lr.STD_CONSTANT if std == "constant" else (lr.STD_MULTIPLIER if std == "multiplier" else 0.0))


LIN_INGEST = [(k,) + t + ("plain",) for k, t in enumerate(gc.linearize_ingest_design())] + [
    (100, "u16", "nchw", "linear", "multiplier", "band"), (101, "u8", "nhwc_bgr", "catmull", "explicit", "band"),
    (102, "f32", "nhwc", "lookup", "none", "band")]


@pytest.mark.parametrize("case", LIN_INGEST, ids=_ids)
def test_linearize_ingest(dev, case):
    """ct_linearize_ingest (the constant chain) against ct_ingest_transform + ct_linearize_std, and against float64 at the
    tolerances of tests/_linearize_refs.py."""
    from clair_torch_amd import ops
    k, dtype, layout, interp, std, variant = case
    h, w = gc.S2
    planar = gc.random_codes(700 + k, (F, C, h, w), dtype)
    sigma = gc.explicit_sigma(700 + k, planar.shape)
    r0, r1 = gc.BAND2 if variant == "band" else (0, h)
    tile = ops.TileGeometry(h_global=h, row_offset=r0) if variant == "band" else None
    x, host = _raw(planar[:, :, r0:r1], layout, dev)
    sg = torch.from_numpy(np.ascontiguousarray(sigma[:, :, r0:r1])).to(dev)
    stages = gc.black_level_stages(dtype)
    lut = gc.lut()
    lut_d = None if interp is None else torch.from_numpy(lut).to(dev)
    skw, lead, what = _lin_std(std, sg), k % 4, _ids(case)
    want = ops.linearize_frames(ops.ingest_transform(x, stages, layout), lut_d, interp, tile=tile, **skw)
    sen = _Sentinels(dev, lead)
    shape = (F, C, r1 - r0, w)
    out = (sen.like(shape, torch.float32, "lin"), sen.like(shape, torch.float32, "std"))
    got = ops.linearize_ingest_frames(x, stages, lut_d, interp, tile=tile, layout=layout, out=out, **skw)
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    _same(got[0], want[0], "linearize_ingest", layout, what + " lin", lead)
    _same(got[1], want[1], "linearize_ingest", layout, what + " std", lead)
    sen.check(what)
    _unchanged([(x, host)], what)
    pixels = gc.chain_f32(planar, stages)
    lin_o, std_o = lr.linearize_f64(pixels, gc.sigma_of(std, pixels, sigma), lut, interp)
    if variant == "band":
        whole = ops.linearize_ingest_frames(_raw(planar, layout, dev)[0], stages, lut_d, interp, layout=layout,
                                            **_lin_std(std, torch.from_numpy(sigma).to(dev)))
        for j in range(2):
            _same(got[j], whole[j][:, :, r0:r1].contiguous(), "linearize_ingest", layout, what + " band of the whole", lead)
    lr.check(got[0].cpu().numpy(), lin_o[:, :, r0:r1], ("lin", interp), f"grid linearize ingest {what} lin")
    lr.check(got[1].cpu().numpy(), std_o[:, :, r0:r1], ("std", interp), f"grid linearize ingest {what} std")


LIN_DARK = [("dark", k) + t for k, t in enumerate(gc.linearize_dark_design(("nchw",)))] + [
    ("dark_ingest", k) + t for k, t in enumerate(gc.linearize_dark_design(gc.LAYOUTS))] + [
    ("dark_ingest_data", 100, "u16", "nchw", "linear", "multiplier"), ("dark_ingest_data", 101, "u8", "nhwc_bgr", "catmull", "explicit"),
    ("dark_ingest_data", 102, "f32", "nhwc", None, "constant")]
# the first LINEAR case of every form and layout also goes to the eager restatement
LIN_DARK_REFERENCE = {(form, layout): min(c[1] for c in LIN_DARK if c[0] == form and c[3] == layout and c[4] == "linear")
                      for form, layout in [("dark", "nchw")] + [("dark_ingest", lay) for lay in gc.LAYOUTS]}


@pytest.mark.parametrize("case", LIN_DARK, ids=_ids)
def test_linearize_dark(dev, case):
    """ct_linearize_dark / ct_linearize_dark_ingest / ct_linearize_dark_ingest_data against, frame by frame,
    (ct_ingest_transform +) ct_dark_field_blur + ct_linearize_std; the first LINEAR case of every form and layout also against the
    eager restatement at the tolerances of tests/test_gpu_linearize_dark.py."""
    from clair_torch_amd import ops
    from oracle import eager_torch as oe
    form, k, dtype, layout, interp, std = case
    h, w = gc.S2
    planar = gc.random_codes(800 + k, (F, C, h, w), dtype)
    sigma = gc.explicit_sigma(800 + k, planar.shape)
    dark, dark_std = gc.dark_fields(800 + k, planar.shape)
    x, host = _raw(planar, layout, dev)
    sg, dk, ds = (torch.from_numpy(a).to(dev) for a in (sigma, dark, dark_std))
    lut = gc.lut()
    lut_d = None if interp is None else torch.from_numpy(lut).to(dev)
    skw = _lin_std(std, sg)
    stages = [] if form == "dark" else ([("affine_data", 1.0, 0.0)] if form == "dark_ingest_data" else gc.black_level_stages(dtype))
    consts = ops.ingest_extrema_frames(x, (), layout) if form == "dark_ingest_data" else None
    lead, what, family = k % 4, _ids(case), "linearize_dark" if form == "dark" else "linearize_dark_ingest"
    want = [[], []]
    for f in range(F):
        one = dict(std=sg[f:f + 1]) if std == "explicit" else skw
        if form == "dark":
            src = x[f:f + 1]
        else:
            src = ops.ingest_transform(x[f:f + 1], stages, layout, consts=None if consts is None else consts[f])
        xb, se = ops.dark_field_blur(src, dk[f:f + 1], ds[f:f + 1], **one)
        pair = ops.linearize_frames(xb, lut_d, interp, std=se)
        want[0].append(pair[0]), want[1].append(pair[1])
    want = [torch.cat(v) for v in want]
    sen = _Sentinels(dev, lead)
    out = (sen.like((F, C, h, w), torch.float32, "lin"), sen.like((F, C, h, w), torch.float32, "std"))
    if form == "dark":
        got = ops.linearize_dark_frames(x, dk, ds, lut_d, interp, out=out, **skw)
    elif form == "dark_ingest":
        got = ops.linearize_dark_ingest_frames(x, stages, dk, ds, lut_d, interp, layout=layout, out=out, **skw)
    else:
        got = ops.linearize_dark_ingest_frames_data(x, stages, dk, ds, lut_d, interp, consts=consts, layout=layout, out=out, **skw)
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    _same(got[0], want[0], family, layout, what + " lin")
    _same(got[1], want[1], family, layout, what + " std")
    sen.check(what)
    _unchanged([(x, host)], what)
    if LIN_DARK_REFERENCE.get((form, layout)) == k:
        pix = gc.chain_f32(planar, stages) if form != "dark" else lr.to_pixels(planar, dtype, gc.TOP[dtype])
        sig = gc.sigma_of(std, pix, sigma)
        sig = np.zeros_like(pix) if sig is None else sig
        pixels = torch.from_numpy(pix)
        for f in range(F):
            lin_o, sd_o = oe.linearize_frame_dark(pixels[f], torch.from_numpy(sig[f]), torch.from_numpy(lut), torch.from_numpy(dark[f]),
                                                  torch.from_numpy(dark_std[f]), "linear")
            assert_parity(got[0][f].cpu().numpy(), lin_o.numpy(), rtol=1e-5, norm_tol=1e-6, what=f"grid linearize {form} {layout} value")
            assert_parity(got[1][f].cpu().numpy(), sd_o.numpy(), rtol=1e-5, norm_tol=1e-6, what=f"grid linearize {form} {layout} std")


# ---- the FLAT forms -----------------------------------------------------------------------------------------------------------
# ct_linearize_std_flat goes through lin_typed, whose packet kernels need whole packets per frame (Q, image and output strides
# multiples of 4, of 8 for packet8): 3x67x131 runs element by element whatever the addresses.  The first three "std" cases
# therefore take 72x131 (gc.S2_STD) with aligned outputs -- the planar, the RGB and the packet8 kernel -- the fourth 67x131.
FLAT_STD_PATH = {"nchw": "planar", "nhwc_bgr": "rgb", "nhwc": "packet8"}
FLAT = [("std", "u16", "nchw", "linear", "multiplier"), ("std", "f32", "nhwc_bgr", "catmull", "constant"), ("std", "u8", "nhwc", "linear", "explicit"),
        ("std", "u8", "nhwc", "lookup", "none"),
        ("ingest", "u8", "nchw", "catmull", "explicit"), ("ingest", "u16", "nhwc", "linear", "constant"), ("ingest", "f32", "nhwc_bgr", None, "multiplier"),
        ("strided", "u16", "nchw", "linear", "explicit"), ("strided", "u8", "nhwc_bgr", "catmull", "multiplier"), ("strided", "f32", "nhwc", "lookup", "none")]


@pytest.mark.parametrize("case", FLAT, ids=_ids)
def test_flat_forms(dev, case):
    """ct_linearize_std_flat, ct_linearize_ingest_flat and ct_linearize_ingest_strided_flat (step 2, a 67x131 OUTPUT) against the
    parent launch followed by ct_flatfield_apply with the same flat-mean tensor, bit for bit; the parent against
    _linearize_refs.linearize_f64, the fused pair against the float64 correction of the parent's pair (every form in every layout)."""
    from clair_torch_amd import ops
    form, dtype, layout, interp, std = case
    k = FLAT.index(case)
    packets = form == "std" and std != "none"
    h, w = gc.S2_STD if packets else gc.S2
    src_hw = (2 * h - 1, 2 * w - 1) if form == "strided" else (h, w)
    planar = gc.random_codes(900 + k, (F, C) + src_hw, dtype)
    x, host = _raw(planar, layout, dev)
    sigma = torch.from_numpy(gc.explicit_sigma(900 + k, (F, C, h, w)))
    rng = np.random.default_rng(950 + k)
    flat = torch.from_numpy((0.5 + rng.random((C, h, w))).astype(np.float32)).to(dev)
    flat_std = torch.from_numpy((0.001 + 0.02 * rng.random((C, h, w))).astype(np.float32)).to(dev) if k % 2 == 0 else None
    mean = ops.flatfield_mean(flat)
    lut_d = None if interp is None else torch.from_numpy(gc.lut()).to(dev)
    stages = gc.black_level_stages(dtype)
    if form == "std":   # explicit uncertainties in the frames' own layout
        skw = _lin_std(std, torch.from_numpy(gc.to_layout(sigma.numpy(), layout)).to(dev))
        front = lambda **kw: (ops.linearize_frames_flat if "flat" in kw else ops.linearize_frames)(x, lut_d, interp, layout=layout, **skw, **kw)   # noqa: E731
    elif form == "ingest":
        skw = _lin_std(std, sigma.to(dev))
        front = lambda **kw: (ops.linearize_ingest_frames_flat if "flat" in kw else ops.linearize_ingest_frames)(   # noqa: E731
            x, stages, lut_d, interp, layout=layout, **skw, **kw)
    else:
        skw = _lin_std(std, sigma.to(dev))
        front = lambda **kw: (ops.linearize_ingest_frames_strided_flat if "flat" in kw else ops.linearize_ingest_frames_strided)(   # noqa: E731
            x, 2, stages, lut_d, interp, layout=layout, **skw, **kw)
    want = front()
    assert tuple(want[0].shape) == (F, C, h, w)
    parent = [v.cpu().numpy() for v in want]          # (the correction below is in place)
    ops.flatfield_correct(want[0], want[1], flat, flat_std, input_is_variance=False, through_mean=False, flat_mean=mean)
    lead, what = 0 if packets else 1 + k % 3, _ids(case)
    sen = _Sentinels(dev, lead)
    out = (sen.like((F, C, h, w), torch.float32, "lin"), sen.like((F, C, h, w), torch.float32, "std"))
    got = front(flat=(flat, flat_std, mean), out=out)
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    if form == "std":       # lin_typed's own grids: which of them runs depends on the addresses
        path = lr.linearize_path_of(dtype, layout, C, h * w, C * h * w, F, std, {"lin": (4 * lead) % 32, "std_out": (4 * lead) % 32},
                                    (C * h * w, C * h * w))
        assert path == (FLAT_STD_PATH[layout] if packets else "scalar"), path
        owner_of = lambda chw, c, row, col: f"{gc.lin_typed_owner(path, chw, layout, c, row, col)} ({path})"   # noqa: E731
    else:
        owner_of = None
    _same(got[0], want[0], "linearize_ingest", layout, what + " lin", lead, owner_of)
    _same(got[1], want[1], "linearize_ingest", layout, what + " std", lead, owner_of)
    sen.check(what)
    _unchanged([(x, host)], what)
    # the parent launch against float64 ...
    picked = planar[:, :, ::2, ::2] if form == "strided" else planar
    pixels = lr.to_pixels(picked, dtype, gc.TOP[dtype]) if form == "std" else gc.chain_f32(picked, stages)
    lin_o, std_o = lr.linearize_f64(pixels, gc.sigma_of(std, pixels, sigma.numpy()), gc.lut(), interp)
    lr.check(parent[0], lin_o, ("lin", interp), f"grid flat {what} parent lin")
    lr.check(parent[1], std_o, ("std", interp), f"grid flat {what} parent std")
    # ... and the fused launch against the float64 restatement of the correction on the parent's pair (the six lines and the
    # bounds of test_gpu_linearize_flat.py::test_pair_against_float64)
    lin, sd = parent[0].astype(np.float64), parent[1].astype(np.float64)
    m = mean.cpu().numpy().astype(np.float64)[None, :, None, None]
    den = flat.cpu().numpy().astype(np.float64)[None] + np.float64(np.float32(1e-6))
    var = sd * sd
    if flat_std is not None:
        var = var + (-(m * lin) / (den * den) * flat_std.cpu().numpy().astype(np.float64)[None]) ** 2
    for name, have, ref, bound in (("lin", got[0], (lin / den) * m, LIN_ULP), ("sd", got[1], np.sqrt(var), SD_ULP)):
        ulp = np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64)
        err = float(np.max(np.abs(have.cpu().numpy().astype(np.float64) - ref) / ulp))
        OBSERVED.append({"test": "test_flat_forms", "what": f"grid flat {what} {name}' ulp", "norm": 0.0, "norm_tol": 0.0, "elem": err,
                         "elem_tol": bound, "n": int(ref.size)})
        assert err <= bound, f"grid flat {what} {name}': {err:.3f} ulp > {bound}"
