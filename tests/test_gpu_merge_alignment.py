"""The HDR merge on pointers that are only element-aligned, and what lies beside its outputs.

Which launch a merge takes depends on the addresses it is given (packets of V elements where every pointer and the image stride
allow them, one-element launches otherwise), and every other merge test hands it allocations of their own, which are aligned to
256 bytes and more.  Here every tensor is a view into a larger buffer (tests/_merge_views.py): ``lead`` elements behind a 256-byte
boundary, the rest of the buffer holding a sentinel.  One pointer at a time is moved off the boundary -- by one element, and by
half a packet, which a check made at half the width would still accept -- then all at once, on (3, 4, 8) (Q = 96: whole packets
of 4 and 8, plane 32) and on the control (3, 5, 7) (Q = 105, odd stride and plane: one-element launches whatever the address).
Five exposures, as one batch and streamed as 3 + 2.  For every case:

  (a) the result equals the all-aligned run of the same data BIT FOR BIT, on every route.  ct::merge_pivot_kernel says so of
      itself (merge_typed: "not a single bit").  ct::merge_kernel and ct::merge_reference_order_kernel: V only says which thread
      owns an element -- every sum, pivot, retry decision and store is per element e of the packet, in the same order, the library
      is built with -ffp-contract=off and without SLP vectorisation (every FMA is spelled out), and a wavefront's repeat about the
      mean recomputes the elements that did not ask for it bit-identically -- so torch.equal is asserted there as well;
  (b) the result meets the comparand the route has in tests/test_gpu_merge.py at that file's tolerances: the float64 closed-form
      oracle with the same batch composition (mean rtol 1e-5 / norm 1e-6, std rtol 1e-5 / norm 1e-5), for the reference-order
      route the float32-order emulation, evaluated so that every column lies in one of torch.sum's vectorised blocks (see
      _comparand) and held to that file's figures for such columns everywhere (std 1e-6 / norm 1e-6, mean 1e-13 / norm 1e-14;
      the 1e-5 it grants the differently summed tail columns is not used).  Labels "merge align ..." in parity_observed.json.
      A state is compared through its mean and the root of its variance;
  (c) every margin of every written buffer (outputs; the state arrays when streamed) still holds the sentinel bit for bit, and
      no element of the view does.

Address condition -> the test that makes it false:

| condition | test |
|---|---|
| packets_aligned: ``stack`` at sizeof(T) * V -- generic V = 4 (float32, uint16) and 8 (uint8), pivot V = 4 | test_one_batch_leads[*-3x4x8], lead "stack" (one element; half a packet: 8 B float32, 4 B uint16 and uint8 V = 8, 2 B uint8 V = 4) |
| packets_aligned: ``std_stack`` at 4 V (16 B, 32 B for uint8 V = 8) | test_one_batch_leads, std mode "explicit", lead "std" (4 B, 8 B, 16 B for V = 8) |
| packets_aligned: ``mean_out`` at 8 V (32 B, 64 B for V = 8) | test_one_batch_leads, lead "mean_out" (8 B, 16 B, 32 B for V = 8) |
| packets_aligned: ``std_out`` at 4 V | test_one_batch_leads, lead "std_out" |
| packets_aligned: ``image_stride % V`` | the control shape 3x5x7 of every test (stride 105) |
| packets_aligned(with_state): ``mean_state`` at 8 V, ``sumw_state`` and ``var_state`` at 4 V (generic kernel) | test_streamed_state_leads[generic-*], leads "mean_state", "sumw_state", "var_state" |
| pivoted kernel: state addressed element by element at any lead, stack of a later batch (state-carrying instantiations) | test_streamed_state_leads[pivot-*], the same leads and "stack1" |
| ``fast`` of ct_hdr_merge_batches: packets_aligned per batch -- batch 0's stack, batch 1's stack, batch 1's explicit std; ``Ql % 4`` | test_batch_lists[pivot-*]: CT_ERR_UNSUPPORTED under CT_MERGE_REQUIRE_ONE_LAUNCH with nothing written; the loop's bits without it; 3x5x7 refused all-aligned |
| ``vec_ok`` of exact_typed: ``a.stack``, ``a.std_stack``, stride | test_one_batch_leads[reforder-*] |
| ``vec_ok`` of exact_typed: ``batch_ptr[b]``, ``std_ptr[b]`` | test_batch_lists[reforder-*]: still one launch, the loop's bits |
| ``rgb252`` of launch_pivot: aligned(mean_out, 16), aligned(std_out, 16) (implied by packets_aligned at V = 4) | test_rgb252_outputs: outputs aligned, ``std_out`` 8 B in, ``mean_out`` 8 B and 16 B in |
| ``rgb252``: not with CT_MERGE_MEAN_OUT_F32, not with CT_MERGE_OUT_AS_INPUT | test_rgb252_outputs, the float32 mean and out_layout "input" |
| ``rgb252``: the workgroup's regrouped packet stores of a full tile, the ragged ends one by one | test_rgb252_outputs[3x16x24] (Q = 1152: one full tile and a ragged one), margins |
| fused dark-field merges: stack, dark, dark std, explicit std, state arrays one element in | test_dark_batch_leads, test_dark_ingest_leads |
| ct_dark_field_blur: inputs one element in (ops front), outputs one element in (the entry point itself: the front has no ``out``) | test_dark_field_blur_leads |

A pointer that is not a multiple of its own element is refused before any launch: tests/test_malformed_calls_host.py.
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

import _merge_views as mv
from _dark_cases import as_dtype as _as_dtype, scene as _scene
from _util import assert_parity

pytestmark = pytest.mark.gpu

N, PART = 5, (3, 2)
SHAPES = [(3, 4, 8), (3, 5, 7)]
T = 0.002 * 2.0 ** (np.arange(N) / 2.0)
STD_VALUE = 0.05
FIRST, FINALIZE, MEAN_F32, F64_MOMENTS, REFERENCE_ORDER, STD_HINT, ONE_LAUNCH, OUT_AS_INPUT = 1, 2, 4, 8, 16, 64, 128, 256
OK, UNSUPPORTED = 0, -2
CLOSED_STDS = ("none", "multiplier", "explicit")

# route -> (stored dtype, max_code, interpolation, route flags, V of its packet launch, what ct_hdr_merge_kernel_name says, std modes)
ROUTES = {
    "generic-f32": ("f32", None, "linear", 0, 4, "ct::merge_kernel (float32 moments about a per-pixel pivot, float32 pixels", CLOSED_STDS),
    "generic-u8-200": ("u8", 200.0, "linear", 0, 8, "ct::merge_kernel (float32 moments about a per-pixel pivot, integer codes", CLOSED_STDS),
    "generic-f64-u16": ("u16", 65535.0, "linear", F64_MOMENTS, 4, "ct::merge_kernel (float64 moments, integer codes)", CLOSED_STDS),
    "pivot-u8": ("u8", 255.0, "linear", 0, 4, "ct::merge_pivot_kernel", CLOSED_STDS),
    "pivot-u16": ("u16", 65535.0, "linear", 0, 4, "ct::merge_pivot_kernel", CLOSED_STDS),
    "pivot-u16-4095": ("u16", 4095.0, "linear", 0, 4, "ct::merge_pivot_kernel", CLOSED_STDS),
    "reforder-catmull-u16": ("u16", 65535.0, "catmull", 0, 4, "ct::merge_reference_order_kernel", ("multiplier",)),
    "reforder-catmull-f32": ("f32", None, "catmull", 0, 4, "ct::merge_reference_order_kernel", ("multiplier",)),
    "reforder-linear-u16": ("u16", 65535.0, "linear", REFERENCE_ORDER, 4, "ct::merge_reference_order_kernel", ("explicit",)),
}
CLOSED = [r for r in ROUTES if not r.startswith("reforder")]
_ID = lambda s: "x".join(map(str, s))   # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from clair_torch_amd import _native
    _native.load()
    return torch.device("cuda:0")


# ---- data and comparands (computed once, shared, never modified) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lut():
    return np.stack([np.linspace(0, 1, 256, dtype=np.float32) ** np.float32(p) for p in (2.2, 2.4, 2.6)])


@functools.lru_cache(maxsize=None)
def _data(kind, max_code, shape):
    """(stored stack, its float32 pixels as the reference's Normalize forms them, explicit uncertainties), planar (N, C, H, W)."""
    from oracle import ct_oracle as oc
    rng = np.random.default_rng(zlib.crc32(repr((kind, max_code, shape)).encode()))
    full = (N,) + tuple(shape)
    if kind == "f32":
        stored = rng.random(full, dtype=np.float32)
        x = stored
    else:
        hi, npdt = (256, np.uint8) if kind == "u8" else (65536, np.uint16)
        top = int(max_code)
        stored = rng.integers(0, top + 1, size=full).astype(npdt)
        if top < hi - 1:   # codes above max_code: the model clamps them to the top of the LUT (never in exposure 0, so that
            above = rng.random(full) < 0.15   # every pixel keeps a sample whose weight is not negligible)
            above[0] = False
            stored[above] = rng.integers(top + 1, min(hi, top + top // 3), size=int(above.sum())).astype(npdt)
            x = (stored.astype(np.float32) / np.float32(top)).astype(np.float32)
        else:
            x = oc.normalize_codes(stored)
    sd = (0.001 + 0.05 * rng.random(full)).astype(np.float32)
    for a in (stored, x, sd):
        a.setflags(write=False)
    return stored, x, sd


@functools.lru_cache(maxsize=None)
def _comparand(route, shape, std_mode, part):
    """(mean, std | None), flat, of the batches ``part`` (sizes, from exposure 0 on): the comparand of (b)."""
    from oracle import ct_oracle as oc
    from oracle import eager_torch as oe
    kind, max_code, interp = ROUTES[route][:3]
    _, x, sd = _data(kind, max_code, shape)
    k = sum(part)
    sdo = {"none": None, "multiplier": x * np.float32(STD_VALUE), "explicit": sd}[std_mode]
    sdo = None if sdo is None else sdo[:k].copy()
    x = x[:k].copy()
    if route.startswith("reforder"):
        torch.set_num_threads(1)  # the reference's column blocks start at the beginning of each thread's chunk
        batches, n0 = [], 0
        for b in part:
            batches.append(list(range(n0, n0 + b)))
            n0 += b
        # torch.sum on the CPU associates the last Q % 32 flattened columns differently from its vectorised blocks, and the
        # kernel follows the vectorised order in every column (tests/test_gpu_merge.py holds those tail columns to 1e-5 only,
        # on shapes where they are a fraction of a per cent; of Q = 105 they are 9).  So the emulation runs on the same columns
        # followed by padding up to a multiple of 32 (and of C = 3: the LUT row, flat index % C, stays), which puts every
        # real column into a vectorised block; the padding's results are dropped.
        q = int(np.prod(shape))
        qp = -(-q // 96) * 96

        def padded(a, fill):
            flat = np.full((k, qp), fill, dtype=np.float32)
            flat[:, :q] = a.reshape(k, q)
            return torch.from_numpy(flat.reshape(k, 3, qp // 24, 8))

        mean, std = oe.merge_stack_reference_order(padded(x, 0.5), padded(sdo, 0.01), torch.from_numpy(T[:k].copy()),
                                                   torch.from_numpy(_lut()), interp, True, batches, exp=lambda v: torch.exp(v.double()).float())
        return mean.numpy().reshape(-1)[:q].copy(), std.numpy().reshape(-1)[:q].copy()
    mean, std = oc.hdr_merge(x, sdo, T[:k].copy(), _lut(), interp, True, list(part))
    return np.asarray(mean).reshape(-1), (None if std is None else np.asarray(std).reshape(-1))


def _check_b(route, shape, std_mode, part, mean, std, what):
    """(b): ``mean`` / ``std`` (device tensors in planar order, std None without uncertainties) against the route's comparand."""
    mean_o, std_o = _comparand(route, tuple(shape), std_mode, tuple(part))
    gm = mean.double().cpu().numpy().reshape(-1)
    label = f"merge align {route} {_ID(shape)} {std_mode} {what}"
    if route.startswith("reforder"):
        # every column lies in one of torch.sum's vectorised blocks (_comparand): that file's tolerances for such columns
        assert_parity(std.cpu().numpy().reshape(-1), std_o, rtol=1e-6, norm_tol=1e-6, what=label + " std")
        assert_parity(gm, mean_o, rtol=1e-13, norm_tol=1e-14, what=label + " mean")
        return
    assert_parity(gm, mean_o, rtol=1e-5, norm_tol=1e-6, what=label + " mean")
    if std is not None:
        assert_parity(std.double().cpu().numpy().reshape(-1), std_o, rtol=1e-5, norm_tol=1e-5, what=label + " std")


# ---- placing the tensors -----------------------------------------------------------------------------------------------------
_DEVICE_CONSTANTS = {}


def _constants(dev):
    if dev not in _DEVICE_CONSTANTS:
        _DEVICE_CONSTANTS[dev] = (torch.from_numpy(_lut()).to(dev), torch.from_numpy(T.copy()).to(dev))
    return _DEVICE_CONSTANTS[dev]


def _interleave(planar, layout):
    """(B,3,H,W) planes -> the raw (B,H,W,3) frames of ``layout`` (BGR: what an OpenCV reader hands over)."""
    if layout == "nchw":
        return planar
    return np.ascontiguousarray((planar[:, ::-1] if layout == "nhwc_bgr" else planar).transpose(0, 2, 3, 1))


class _Placed:
    """An array a kernel writes, ``lead`` elements behind a 256-byte boundary of a buffer full of the sentinel."""

    def __init__(self, shape, dtype, lead, dev):
        self.view, self.buf = mv.sentinel_like(shape, dtype, lead, dev)
        self.lead, self.n = lead, self.view.numel()

    def check(self, what):
        """(c)"""
        assert mv.margins_untouched(self.buf, self.lead, self.n), f"{what}: a margin was written"
        assert mv.fully_written(self.buf, self.lead, self.n), f"{what}: elements of the view were left unwritten"

    def check_untouched(self, what):
        assert mv.all_sentinel(self.buf), f"{what}: written by a refused call"


class _State:
    def __init__(self, shape, has_var, leads, dev):
        self.mean = _Placed(shape, torch.float64, leads.get("mean_state", 0), dev)
        self.sumw = _Placed(shape, torch.float32, leads.get("sumw_state", 0), dev)
        self.var = _Placed(shape, torch.float32, leads.get("var_state", 0), dev) if has_var else None
        self.arrays = [a for a in (self.mean, self.sumw, self.var) if a is not None]

    def pointers(self):
        return self.mean.view, self.sumw.view, None if self.var is None else self.var.view

    def check(self, what):
        for a, name in zip(self.arrays, ("mean state", "sumw state", "var state")):
            a.check(f"{what} {name}")

    def check_untouched(self, what):
        for a in self.arrays:
            a.check_untouched(what)

    def snapshot(self):
        return [a.view.clone() for a in self.arrays]


def _inputs(dev, route, shape, std_mode, frames, leads, suffix="", layout="nchw"):
    """(stack view, explicit std view | None) of the exposures ``frames`` = (first, end)."""
    kind, max_code = ROUTES[route][:2]
    stored, _, sd = _data(kind, max_code, tuple(shape))
    a, b = frames
    stack, _ = mv.interior(torch.from_numpy(_interleave(stored[a:b], layout).copy()), leads.get("stack" + suffix, 0), dev)
    std = None
    if std_mode == "explicit":
        std, _ = mv.interior(torch.from_numpy(_interleave(sd[a:b], layout).copy()), leads.get("std" + suffix, 0), dev)
    return stack, std


def _merge_kw(dev, route, std_mode):
    lut, _ = _constants(dev)
    _, max_code, interp = ROUTES[route][:3]
    kw = dict(max_code=max_code, lut=lut, interp=interp, gaussian_weight=True)
    if std_mode != "explicit":
        kw.update(std_mode=std_mode, std_value=STD_VALUE)
    return kw


def _assert_route(route, std_mode, first=True):
    from clair_torch_amd import _native as nv
    from clair_torch_amd import ops
    kind, max_code, interp, flags, _, name = ROUTES[route][:6]
    dtype = {"u8": nv.DTYPE_U8, "u16": nv.DTYPE_U16, "f32": nv.DTYPE_F32}[kind]
    word = flags | FINALIZE | (FIRST if first else 0) | (STD_HINT if std_mode != "none" else 0)
    got = nv.load().ct_hdr_merge_kernel_name(dtype, float(max_code or 1.0), ops._INTERP[interp], 256, word).decode()
    assert got.startswith(name), (route, std_mode, got)


def _lead_cases(pointers, v):
    """One pointer at a time by one element and by half a packet of V elements, then all at once."""
    widths = sorted({1, v // 2})
    for p in pointers:
        for lead in widths:
            yield {p: lead}
    for lead in widths:
        yield {p: lead for p in pointers}


def _one_batch(dev, route, shape, std_mode, leads, *, layout="nchw", extra_flags=0, what=""):
    """The five exposures as one batch without a state -> (mean, std | None), after (c)."""
    has_std = std_mode != "none"
    _, exposures = _constants(dev)
    stack, std = _inputs(dev, route, shape, std_mode, (0, N), leads, layout=layout)
    out_shape = tuple(stack.shape[1:]) if extra_flags & OUT_AS_INPUT else tuple(shape)
    mean_out = _Placed(out_shape, torch.float32 if extra_flags & MEAN_F32 else torch.float64, leads.get("mean_out", 0), dev)
    std_out = _Placed(out_shape, torch.float32, leads.get("std_out", 0), dev) if has_std else None
    rc = mv.merge_batch(stack, exposures, std=std, layout=layout, mean_out=mean_out.view, std_out=None if std_out is None else std_out.view,
                        flags=FIRST | FINALIZE | ROUTES[route][3] | extra_flags, **_merge_kw(dev, route, std_mode))
    assert rc == OK, (what, leads, rc)
    mean_out.check(f"{what} {leads} mean_out")
    if has_std:
        std_out.check(f"{what} {leads} std_out")
    return mean_out.view.clone(), (std_out.view.clone() if has_std else None)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---- one batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
@pytest.mark.parametrize("route", list(ROUTES))
def test_one_batch_leads(dev, route, shape):
    """Stack, explicit std, mean_out and std_out of a one-batch merge (no state), one at a time and all at once: (a), (b), (c)."""
    v, stds = ROUTES[route][4], ROUTES[route][6]
    for std_mode in stds:
        _assert_route(route, std_mode)
        base = _one_batch(dev, route, shape, std_mode, {}, what=route)
        _check_b(route, shape, std_mode, (N,), base[0], base[1], "aligned")
        pointers = ["stack"] + (["std"] if std_mode == "explicit" else []) + ["mean_out"] + (["std_out"] if std_mode != "none" else [])
        for leads in _lead_cases(pointers, v):
            got = _one_batch(dev, route, shape, std_mode, leads, what=route)
            assert _same(got, base), (route, std_mode, leads)
            _check_b(route, shape, std_mode, (N,), got[0], got[1], "one batch")


# ---- streamed: the second batch merges into a state the first one wrote at a lead ----------------------------------------------
def _streamed(dev, route, shape, std_mode, leads):
    """3 + 2 exposures through ct_hdr_merge_batch on one state -> [state after batch 0, state after batch 1, outputs], after (c)."""
    has_std = std_mode != "none"
    _, exposures = _constants(dev)
    state = _State(shape, has_std, leads, dev)
    mean_out = _Placed(shape, torch.float64, leads.get("mean_out", 0), dev)
    std_out = _Placed(shape, torch.float32, leads.get("std_out", 0), dev) if has_std else None
    kw = _merge_kw(dev, route, std_mode)
    snaps, n0 = [], 0
    for k, b in enumerate(PART):
        stack, std = _inputs(dev, route, shape, std_mode, (n0, n0 + b), leads, suffix=str(k))
        last = k == len(PART) - 1
        rc = mv.merge_batch(stack, exposures[n0:n0 + b], std=std, state=state.pointers(), mean_out=mean_out.view if last else None,
                            std_out=std_out.view if last and has_std else None,
                            flags=(FIRST if k == 0 else 0) | (FINALIZE if last else 0) | ROUTES[route][3], **kw)
        assert rc == OK, (route, leads, k, rc)
        state.check(f"{route} {leads} batch {k}")
        if not last:   # a launch without FINALIZE stores no result
            mean_out.check_untouched("mean_out of a non-final batch")
        snaps.append(state.snapshot())
        n0 += b
    mean_out.check(f"{route} {leads} mean_out")
    if has_std:
        std_out.check(f"{route} {leads} std_out")
    snaps.append([mean_out.view.clone()] + ([std_out.view.clone()] if has_std else []))
    return snaps


def _check_b_streamed(route, shape, std_mode, snaps, what):
    has_std = std_mode != "none"
    for k in range(len(PART)):   # the state after batch k: its mean, and the root of its variance
        var = snaps[k][2] if has_std else None
        _check_b(route, shape, std_mode, PART[:k + 1], snaps[k][0], None if var is None else var.double().sqrt(), f"{what} state {k}")
    _check_b(route, shape, std_mode, PART, snaps[-1][0], snaps[-1][1] if has_std else None, what)


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
@pytest.mark.parametrize("route", CLOSED)
def test_streamed_state_leads(dev, route, shape):
    """The three state arrays (and the later batch's stack, both outputs) of the closed-form routes, with and without
    uncertainties: the state after each batch and the final outputs, (a), (b), (c)."""
    v = ROUTES[route][4]
    for std_mode in ("none", "multiplier"):
        _assert_route(route, std_mode, first=False)
        base = _streamed(dev, route, shape, std_mode, {})
        _check_b_streamed(route, shape, std_mode, base, "streamed aligned")
        one_at_a_time = ["stack1", "mean_state", "sumw_state"] + (["var_state"] if std_mode != "none" else [])
        everything = ["stack0"] + one_at_a_time + ["mean_out"] + (["std_out"] if std_mode != "none" else [])
        cases = [c for c in _lead_cases(one_at_a_time, v) if len(c) == 1] + [{p: 1 for p in everything}, {p: v // 2 for p in everything}]
        for leads in cases:
            got = _streamed(dev, route, shape, std_mode, leads)
            for a, b in zip(got, base):
                assert _same(a, b), (route, std_mode, leads)
            _check_b_streamed(route, shape, std_mode, got, "streamed")


# ---- batch lists ---------------------------------------------------------------------------------------------------------------
def _list_call(dev, route, shape, std_mode, views, flags, loop):
    """ct_hdr_merge_batches on the two batches ``views`` (or the loop of ct_hdr_merge_batch calls it stands for) with a fresh state and
    fresh outputs -> (status, state, mean_out, std_out)."""
    has_std = std_mode != "none"
    _, exposures = _constants(dev)
    state = _State(shape, has_std, {}, dev)
    mean_out = _Placed(shape, torch.float64, 0, dev)
    std_out = _Placed(shape, torch.float32, 0, dev) if has_std else None
    kw = _merge_kw(dev, route, std_mode)
    outs = dict(mean_out=mean_out.view, std_out=None if std_out is None else std_out.view)
    if loop:
        rc, n0 = OK, 0
        for k, (stack, std) in enumerate(views):
            b, last = stack.shape[0], k == len(views) - 1
            rc = mv.merge_batch(stack, exposures[n0:n0 + b], std=std, state=state.pointers(), **(outs if last else {}),
                                flags=(FIRST if k == 0 else 0) | (FINALIZE if last else 0) | ROUTES[route][3], **kw)
            assert rc == OK
            n0 += b
    else:
        stds = [s for _, s in views] if std_mode == "explicit" else None
        rc = mv.merge_batches([s for s, _ in views], exposures, stds=stds, state=state.pointers(), flags=FIRST | FINALIZE | ROUTES[route][3] | flags,
                              **outs, **kw)
    return rc, state, mean_out, std_out


LIST_ROUTES = {"pivot-u8": "explicit", "pivot-u16": "explicit", "pivot-u16-4095": "explicit", "reforder-linear-u16": "explicit",
               "reforder-catmull-f32": "multiplier"}


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
@pytest.mark.parametrize("route", list(LIST_ROUTES))
def test_batch_lists(dev, route, shape):
    """ct_hdr_merge_batches on 3 + 2 exposures: the second batch's stack, its explicit std, the first batch's stack off the packet,
    one at a time.  The pivoted one-launch route must step aside (CT_ERR_UNSUPPORTED when one launch is required, nothing
    written; otherwise the bits of the loop of ct_hdr_merge_batch calls on the same views); the reference-order route stays one
    launch and only drops its packets."""
    std_mode = LIST_ROUTES[route]
    pivot, packets = route.startswith("pivot"), shape == (3, 4, 8)
    _assert_route(route, std_mode)

    def views_for(leads):
        out, n0 = [], 0
        for k, b in enumerate(PART):
            out.append(_inputs(dev, route, shape, std_mode, (n0, n0 + b), leads, suffix=str(k)))
            n0 += b
        return out

    def finished(rc, state, mean_out, std_out, what):
        assert rc == OK, (what, rc)
        state.check(what)
        mean_out.check(what)
        std_out.check(what)
        return state.snapshot() + [mean_out.view.clone(), std_out.view.clone()]

    aligned = views_for({})
    base = finished(*_list_call(dev, route, shape, std_mode, aligned, 0, loop=True), "aligned loop")
    _check_b(route, shape, std_mode, PART, base[-2], base[-1], "batch list aligned")
    # all aligned: one launch where there are whole packets (and for the reference-order route anyway) ...
    rc, state, mean_out, std_out = _list_call(dev, route, shape, std_mode, aligned, ONE_LAUNCH, loop=False)
    if pivot and not packets:   # ... Q = 105 is no multiple of the packet: refused before anything is written
        assert rc == UNSUPPORTED
        state.check_untouched("refused"), mean_out.check_untouched("refused"), std_out.check_untouched("refused")
    else:
        assert _same(finished(rc, state, mean_out, std_out, "aligned one launch"), base)
    pointers = ["stack1"] + (["std1"] if std_mode == "explicit" else []) + ["stack0"]
    for leads in (c for c in _lead_cases(pointers, ROUTES[route][4]) if len(c) == 1):
        views = views_for(leads)
        rc, state, mean_out, std_out = _list_call(dev, route, shape, std_mode, views, ONE_LAUNCH, loop=False)
        if pivot:
            assert rc == UNSUPPORTED, (route, leads, rc)
            state.check_untouched(leads), mean_out.check_untouched(leads), std_out.check_untouched(leads)
        else:
            assert _same(finished(rc, state, mean_out, std_out, f"one launch {leads}"), base), (route, leads)
        want = finished(*_list_call(dev, route, shape, std_mode, views, 0, loop=True), f"loop {leads}")
        got = finished(*_list_call(dev, route, shape, std_mode, views, 0, loop=False), f"list {leads}")
        assert _same(got, want) and _same(got, base), (route, leads)
        _check_b(route, shape, std_mode, PART, got[-2], got[-1], "batch list")


# ---- interleaved frames with regrouped packet stores ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 4, 8), (3, 16, 24)], ids=_ID)
@pytest.mark.parametrize("layout", ["nhwc", "nhwc_bgr"])
def test_rgb252_outputs(dev, layout, shape):
    """uint16 RGB / BGR frames, one batch, no state: launch_pivot's ``rgb252`` route (interleaved input, planar outputs aligned to
    16 bytes) and what switches it off -- an output 8 bytes in (then no packets at all: packets_aligned asks 32 bytes of
    mean_out), a float32 mean, outputs in the input's order -- give the bits of the planar-input run of the same data, and
    leave the margins alone.  3x16x24 has one full tile of 1024 elements, whose results are regrouped through LDS and stored
    as packets, and a ragged one."""
    route = "pivot-u16"
    for std_mode in ("multiplier", "none"):
        _assert_route(route, std_mode)
        planar = _one_batch(dev, route, shape, std_mode, {}, what="planar")
        _check_b(route, shape, std_mode, (N,), planar[0], planar[1], "rgb252 planar")
        cases = [{}, {"std_out": 2}, {"mean_out": 1}, {"mean_out": 2}, {"mean_out": 4, "std_out": 4}, {"mean_out": 1, "std_out": 1}, {"stack": 1}]
        for leads in cases:
            if std_mode == "none":
                leads = {k: lead for k, lead in leads.items() if k != "std_out"}
            got = _one_batch(dev, route, shape, std_mode, leads, layout=layout, what=layout)
            assert _same(got, planar), (layout, std_mode, leads)
        _check_b(route, shape, std_mode, (N,), got[0], got[1], "rgb252 " + layout)
        planar32 = _one_batch(dev, route, shape, std_mode, {}, extra_flags=MEAN_F32, what="planar float32 mean")
        assert planar32[0].dtype == torch.float32 and torch.equal(planar32[0], planar[0].float())
        for leads in ({}, {"mean_out": 1}, {"mean_out": 2}):
            assert _same(_one_batch(dev, route, shape, std_mode, leads, layout=layout, extra_flags=MEAN_F32, what=layout + " float32 mean"), planar32)
        for leads in ({}, {"mean_out": 1}, {"mean_out": 2, "std_out": 2}):
            if std_mode == "none":
                leads = {k: lead for k, lead in leads.items() if k != "std_out"}
            as_input = _one_batch(dev, route, shape, std_mode, leads, layout=layout, extra_flags=OUT_AS_INPUT, what=layout + " input order")
            back = [None if x is None else (x.permute(2, 0, 1).flip(0) if layout == "nhwc_bgr" else x.permute(2, 0, 1)) for x in as_input]
            assert _same(back, planar), (layout, std_mode, leads)


# ---- the dark-field forms, through the ops fronts (which accept views) ---------------------------------------------------------
DARK_N, DARK_CUTS = 4, ((0, 2), (2, 4))
DARK_LEADS = {"aligned": (), "stack": ("stack",), "dark": ("dark",), "dark_std": ("dark_std",), "std": ("std",),
              "states": ("mean_state", "sumw_state", "var_state"), "all": ("stack", "dark", "dark_std", "std", "mean_state", "sumw_state", "var_state")}
_BLACK = 65535.0 / 1024.0
DARK_STAGES = [("affine", _BLACK, 65535.0 - _BLACK, 1.0, 0.0)]


@functools.lru_cache(maxsize=None)
def _dark_data(shape):
    c, h, w = shape
    x, sd, t, dark, dark_std, lut = _scene(5 + h, DARK_N, c, h, w)
    codes, max_code = _as_dtype(x, torch.uint16)
    return codes, max_code, sd, t, dark, dark_std, lut


def _dark_batches(dev, shape, leads):
    """Per batch (stack, exposure times, dark, dark std, explicit std), every device tensor its own view."""
    codes, _, sd, t, dark, dark_std, _ = _dark_data(tuple(shape))
    place = lambda host, key: mv.interior(host.contiguous(), leads.get(key, 0), dev)[0]   # noqa: E731
    return [(place(codes[a:b], "stack"), t[a:b], place(dark[a:b], "dark"), place(dark_std[a:b], "dark_std"), place(sd[a:b], "std"))
            for a, b in DARK_CUTS]


def _placed_merge_state(dev, shape, leads):
    from clair_torch_amd import ops
    placed = _State(shape, True, leads, dev)
    state = ops.MergeState(tuple(shape), dev, True)
    state.mean, state.sumw, state.var = placed.pointers()
    return state, placed


def _dark_stream(dev, shape, leads, merge_one):
    """The batches through ``merge_one(state, finalize, stack, t, dark, dark_std, sd)`` on a state placed by ``leads`` ->
    [state after every batch ..., outputs]; the state's margins after every batch."""
    state, placed = _placed_merge_state(dev, shape, leads)
    snaps, res = [], None
    batches = _dark_batches(dev, shape, leads)
    for k, args in enumerate(batches):
        res = merge_one(state, k == len(batches) - 1, *args)
        placed.check(f"dark {leads} batch {k}")
        snaps.append(placed.snapshot())
    return snaps + [[res[0], res[1]]]


def _leads_of(which):
    return {name: 1 for name in DARK_LEADS[which]}


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
@pytest.mark.parametrize("which", list(DARK_LEADS))
def test_dark_batch_leads(dev, which, shape):
    """ops.hdr_merge_dark_batch, two batches on one MergeState: stack, dark field, its std, the explicit std and the state arrays one
    element in -- the bits of the aligned run and of the unfused pair (ct_dark_field_blur, then ct_hdr_merge_batch), state margins."""
    from clair_torch_amd import ops
    _, max_code, _, _, _, _, lut = _dark_data(tuple(shape))
    kw = dict(lut=lut.to(dev), interp="linear", gaussian_weight=True, reference_order=False)

    def fused(state, finalize, stack, t, dark, dark_std, sd):
        return ops.hdr_merge_dark_batch(stack, t, dark, dark_std, std=sd, max_code=max_code, state=state, finalize=finalize, **kw)

    def pair(state, finalize, stack, t, dark, dark_std, sd):
        xb, sig = ops.dark_field_blur(stack, dark, dark_std, std=sd, max_code=max_code)
        return ops.hdr_merge_batch(xb, t, std=sig, state=state, finalize=finalize, **kw)

    want = _dark_stream(dev, shape, {}, pair)
    base = _dark_stream(dev, shape, {}, fused)
    got = _dark_stream(dev, shape, _leads_of(which), fused)
    for g, b, w in zip(got, base, want):
        assert _same(g, b) and _same(g, w), which


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
@pytest.mark.parametrize("which", list(DARK_LEADS))
def test_dark_ingest_leads(dev, which, shape):
    """ops.hdr_merge_dark_ingest_batches (one batch per call, two calls on one MergeState) on raw uint16 frames behind a chain: the
    same leads, against the aligned run and ct_ingest_transform + ct_hdr_merge_dark_batch."""
    from clair_torch_amd import ops
    lut = _dark_data(tuple(shape))[6]
    kw = dict(lut=lut.to(dev), interp="linear", gaussian_weight=True, reference_order=False)

    def fused(state, finalize, frames, t, dark, dark_std, sd):
        return ops.hdr_merge_dark_ingest_batches([frames], DARK_STAGES, [t], [dark], [dark_std], stds=[sd], state=state, finalize=finalize, **kw)

    def unfused(state, finalize, frames, t, dark, dark_std, sd):
        x32 = ops.ingest_transform(frames, DARK_STAGES, "nchw")
        return ops.hdr_merge_dark_batch(x32, t, dark, dark_std, std=sd, state=state, finalize=finalize, **kw)

    want = _dark_stream(dev, shape, {}, unfused)
    base = _dark_stream(dev, shape, {}, fused)
    got = _dark_stream(dev, shape, _leads_of(which), fused)
    for g, b, w in zip(got, base, want):
        assert _same(g, b) and _same(g, w), which


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
@pytest.mark.parametrize("which", ["stack", "dark", "dark_std", "std", "xb", "sig", "all"])
def test_dark_field_blur_leads(dev, which, shape):
    """ct_dark_field_blur: inputs one element in through ops.dark_field_blur; outputs one element in through the entry point
    itself (the front allocates its own) -- the aligned run's bits, output margins untouched, every output element written."""
    from clair_torch_amd import _native as nv
    from clair_torch_amd import ops
    names = ("stack", "dark", "dark_std", "std", "xb", "sig") if which == "all" else (which,)
    leads = {name: 1 for name in names}
    _, max_code, _, _, _, _, _ = _dark_data(tuple(shape))
    c, h, w = shape
    (stack0, _, dark0, dark_std0, sd0), _ = _dark_batches(dev, shape, {})
    want = ops.dark_field_blur(stack0, dark0, dark_std0, std=sd0, max_code=max_code)
    (stack, _, dark, dark_std, sd), _ = _dark_batches(dev, shape, leads)
    got = ops.dark_field_blur(stack, dark, dark_std, std=sd, max_code=max_code)
    assert _same(got, want), which
    b = stack.shape[0]
    xb = _Placed((b, c, h, w), torch.float32, leads.get("xb", 0), dev)
    sig = _Placed((b, c, h, w), torch.float32, leads.get("sig", 0), dev)
    geom = ops._geometry(stack, None)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    with torch.cuda.device(dev):
        rc = nv.load().ct_dark_field_blur(ptr(stack), nv.DTYPE_U16, float(max_code), b, ctypes.byref(geom), None, ptr(sd), nv.STD_EXPLICIT, 0.0,
                                          ptr(dark), ptr(dark_std), dark.shape[0], 0.05, 50.0, ptr(xb.view), ptr(sig.view), ops._stream(dev))
    assert rc == OK
    xb.check(f"blur {which} xb"), sig.check(f"blur {which} sig")
    assert torch.equal(xb.view, want[0]) and torch.equal(sig.view, want[1]), which
