"""Helpers of tests/test_gpu_fused_grids.py (importable without a GPU; tests/test_grid_cases_host.py covers them).

The fused kernels find their work from ``blockIdx.x``.  This module restates, per family, how the HOST sizes the grid in x and
which x-workgroup owns an output element, so that the GPU tests can (a) prove on the CPU that their shapes reach a third,
ragged workgroup and a group that meets a row end, and (b) name the owning workgroup when a value differs.  Every formula
names the host function it mirrors; none of them is read by the library.

``pairwise`` thins a product of axes to a design that still holds every PAIR of values (tests/_pair_refs.py's matrix_cases by
hand; here greedy and checked by the host test); ``chain_f32`` is the float32 arithmetic of a constant stage list on the CPU
and ``scene_codes`` / ``random_codes`` are the seeded inputs, the same on the host and in the GPU tests."""
import itertools

import numpy as np

K_BLOCK = 256            # ct_device.hpp kBlock
S1 = (38, 71)            # merge and statistics-ingest families (plane 2698)
S1_CODE = (40, 71)       # code-form statistics: Q = 3 * 2840 is a multiple of 4, so the V = 4 kernel runs (stats_frames_vec_ok)
S2 = (67, 131)           # linearize families: four slots per thread (plane 8777)
S2_STD = (72, 131)       # ct_linearize_std_flat: lin_typed's packet kernels need Q = 3 * plane a multiple of 8 (packet8: of the strides)
BAND1 = (5, 33)          # rows of S1 / S2 the row-band cases take
BAND2 = (9, 58)

# family -> (kernel files, host function mirrored, planar group, interleaved group | None, slots per thread, rule)
#   rule "packets": one slot for what precedes a plane's first aligned packet, then one per packet of G plane elements
#                   (mi_grid, li_launch_rows);  "rows": ceil(W / G) groups per row, no group crosses a row (md_grid, ld_launch,
#                   ldi_launch);  "threads": plane / G threads, the edges in a launch of their own (si_layout);  "flat": Q / 4
#                   threads over the frame's memory order where every batch can be read as packets (stats_frames_vec_ok:
#                   image_stride = C * plane a multiple of 4 -- so contiguous batches never have a vector body AND a V = 1
#                   tail), else Q threads of the V = 1 kernel (stats_split / stats_grid)
FAMILIES = {
    "merge_ingest": ("ct_merge_ingest.hip, ct_merge_ingest_multi.hip", "mi_grid", 4, 2, 1, "packets"),
    "merge_dark": ("ct_merge_dark.hip, ct_merge_dark_multi.hip", "md_grid", 4, None, 1, "rows"),
    "merge_dark_ingest": ("ct_merge_dark_ingest*.hip", "md_grid", 4, 2, 1, "rows"),
    "stats_ingest": ("ct_stats_ingest.hip, ct_stats_ingest_multi.hip", "si_layout / si_grid", 4, 1, 1, "threads"),
    "stats_multi": ("ct_stats_multi.hip", "stats_split / stats_grid", 4, 4, 1, "flat"),
    "linearize_dark": ("ct_linearize_dark.hip", "ld_launch", 4, None, 4, "rows"),
    "linearize_dark_ingest": ("ct_linearize_dark_ingest.hip", "ldi_launch", 4, 4, 4, "rows"),
    "linearize_ingest": ("ct_linearize_ingest.hip, ct_linearize_ingest_strided.hip", "li_launch_rows", 4, 4, 4, "packets"),
}
LAYOUTS = ("nchw", "nhwc", "nhwc_bgr")


def layouts_of(family):
    return LAYOUTS if FAMILIES[family][3] is not None else ("nchw",)


def stats_frames_vec_ok(channels, h, w, frames_lead=0, state_lead=0):
    """stats_frames_vec_ok and stats_split's vec_ok restated for the contiguous batches of ct_video_stats_batches, whose
    image_stride is C * H * W: packets of 4 need that stride, the frames' pointers and both state pointers on a packet
    boundary (``*_lead``: elements behind one)."""
    return (channels * h * w) % 4 == 0 and frames_lead % 4 == 0 and state_lead % 4 == 0


def _group(family, layout, chw=None):
    _, _, g_planar, g_packed, per_thread, rule = FAMILIES[family]
    g = g_planar if layout == "nchw" else g_packed
    if rule == "flat" and chw is not None and not stats_frames_vec_ok(*chw):
        g = 1
    return g, per_thread, rule


def slots_x(family, layout, h, w, channels=3):
    """(slots or threads along x, slots per workgroup) of the family's main launch for one (h, w) plane."""
    g, per_thread, rule = _group(family, layout, (channels, h, w))
    plane = h * w
    per_block = K_BLOCK * per_thread
    if rule == "packets":
        return 1 + -(-plane // g), per_block
    if rule == "rows":
        return -(-w // g) * h, per_block
    if rule == "threads":
        return plane // g, per_block
    return (channels * plane) // g, per_block          # "flat": the vector body over Q = C * plane


def grid_x(family, layout, h, w, channels=3):
    n, per_block = slots_x(family, layout, h, w, channels)
    return -(-n // per_block)


def last_fill(family, layout, h, w, channels=3):
    """Slots the last x-workgroup holds (of ``slots per workgroup``)."""
    n, per_block = slots_x(family, layout, h, w, channels)
    return n - (grid_x(family, layout, h, w, channels) - 1) * per_block, per_block


def meets_row_end(family, layout, h, w, head=0, channels=3):
    """Does some thread's group cross a row end (packets of a plane, or of the frame's memory order) or end short at one
    (row groups)?  None where a thread owns ONE element or pixel: there is no group."""
    g, _, rule = _group(family, layout, (channels, h, w))
    if g == 1:
        return None
    if rule == "rows":
        return w % g != 0
    plane = h * w
    if rule == "flat":   # packets of the memory order: q over C * plane (planar: row q // w), or pixel q // C of an interleaved frame
        row_of = (lambda q: q // w) if layout == "nchw" else (lambda q: q // channels // w)
        return any(row_of(q0) != row_of(q0 + g - 1) for q0 in range(0, (channels * plane // g) * g, g))
    return any(p0 // w != (min(p0 + g, plane) - 1) // w for p0 in range(head, plane, g))


def conditions(family, layout, h, w, channels=3):
    """The three conditions of the GPU module's shapes: >= 3 workgroups in x, a partly filled last one, a group at a row end
    (``row_end`` None: a thread owns single elements or pixels, the condition does not apply)."""
    fill, per_block = last_fill(family, layout, h, w, channels)
    return dict(workgroups=grid_x(family, layout, h, w, channels), ragged=0 < fill < per_block,
                row_end=meets_row_end(family, layout, h, w, 0, channels))


def head_of(lead, plane_index, plane, group=4):
    """Elements in front of the first aligned packet of plane ``plane_index`` of an array whose first element lies ``lead``
    elements behind a packet boundary (merge ingest: ``lead`` 0, the index space; statistics / linearize ingest: the pointer)."""
    return (-(lead + plane_index * plane)) % group


def owner(family, layout, chw, c, row, col, frame=0, lead=0):
    """The x-workgroup of the family's main launch that owns element (c, row, col) of planar frame ``frame`` of the outputs
    (``lead``: see ``head_of``), or a string for what a launch of its own handles (the statistics ingest's edges).  The code-form
    statistics are taken with aligned frames and states (what the GPU tests hand over)."""
    channels, h, w = chw
    g, per_thread, rule = _group(family, layout, chw)
    plane, p = h * w, row * w + col
    per_block = K_BLOCK * per_thread
    if rule == "rows":
        return (row * -(-w // g) + col // g) // per_block
    if rule == "packets":
        if layout == "nchw":
            index = (frame * channels + c) if family == "linearize_ingest" else c
            head = head_of(lead, index, plane, g)
        else:
            head = head_of(lead, frame * channels, plane, g) if family == "linearize_ingest" else 0
        return 0 if p < head else (1 + (p - head) // g) // per_block
    if rule == "threads":
        if layout != "nchw":
            return p // per_block
        head = min(head_of(lead, c, plane, g), plane)
        body_end = head + ((plane - head) // g) * g
        return (p - head) // g // per_block if head <= p < body_end else "edge launch"
    q = (c * plane + p) if layout == "nchw" else p * channels + (c if layout == "nhwc" else channels - 1 - c)
    return q // g // per_block      # (V = 4 or V = 1 for the whole frame: see stats_frames_vec_ok)


LIN_TYPED = {"rgb": 3072, "planar": 3072, "packet8": 2048, "scalar": 256}   # elements of a frame per workgroup (lin_launch)


def lin_typed_owner(path, chw, layout, c, row, col):
    """The x-workgroup of lin_typed's launch (ct_linearize.hip; ``path`` as _linearize_refs.linearize_path_of names it) that owns
    an output element: the kernels walk the frame's MEMORY order q; what a "+tail" launch handles is named as such."""
    channels, h, w = chw
    p, q_all = row * w + col, channels * h * w
    q = (c * h * w + p) if layout == "nchw" else p * channels + (c if layout == "nhwc" else channels - 1 - c)
    body, _, tail = path.partition("+")
    if body == "rgb":               # a thread owns 4 pixels of the three planes: 12 elements
        return (p // 4) // K_BLOCK
    packet = {"planar": 4, "packet8": 8, "scalar": 1}[body]
    if tail and q >= (q_all // packet) * packet:
        return "tail launch"
    return q // LIN_TYPED[body]


def where_differs(got, want, family, layout, lead=0, owner_of=None):
    """None when the two arrays ((C,H,W) or (F,C,H,W), any float / int dtype) hold the same bits; else the message of the
    first difference: flat index, (frame,) channel, row, column and the owning x-workgroup (``owner_of(chw, c, row, col)``
    where the family's rule is not one of ``owner``'s)."""
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / dtype {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    bits = {4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize]
    diff = np.flatnonzero(a.reshape(-1).view(bits) != b.reshape(-1).view(bits))
    if diff.size == 0:
        return None
    at = int(diff[0])
    idx = np.unravel_index(at, a.shape)
    frame = int(idx[0]) if a.ndim == 4 else 0
    c, row, col = (int(v) for v in idx[-3:])
    wg = owner_of(a.shape[-3:], c, row, col) if owner_of else owner(family, layout, a.shape[-3:], c, row, col, frame, lead)
    return (f"{diff.size} of {a.size} differ, first at flat index {at} = (frame {frame}, channel {c}, row {row}, column {col}), "
            f"x-workgroup {wg} of {family} {layout}: got {a.reshape(-1)[at]!r}, want {b.reshape(-1)[at]!r}")


# ---- reduced designs -----------------------------------------------------------------------------------------------------------
def pairwise(*axes, allowed=None):
    """A list of tuples, one value per axis, in which every pair of values of two axes that some ``allowed`` tuple holds
    appears: greedy, deterministic.  ``allowed(tuple) -> bool`` removes combinations a family does not take."""
    full = [t for t in itertools.product(*axes) if allowed is None or allowed(t)]
    pairs = lambda t: {(i, t[i], j, t[j]) for i in range(len(t)) for j in range(i + 1, len(t))}   # noqa: E731
    todo = set().union(*(pairs(t) for t in full)) if full else set()
    out = []
    while todo:
        best = max(full, key=lambda t: len(pairs(t) & todo))
        out.append(best)
        todo -= pairs(best)
    return out


def pairs_covered(cases, *axes, allowed=None):
    full = [t for t in itertools.product(*axes) if allowed is None or allowed(t)]
    want = {(i, t[i], j, t[j]) for t in full for i in range(len(t)) for j in range(i + 1, len(t))}
    have = {(i, t[i], j, t[j]) for t in cases for i in range(len(t)) for j in range(i + 1, len(t))}
    return want <= have


DTYPES = ("u8", "u16", "f32")
INTERPS = (None, "lookup", "linear", "catmull")
STDS = ("none", "constant", "multiplier", "explicit")


def merge_ingest_design():
    """(dtype, layout, interp, std): codes only (the family refuses float32 pixels)."""
    return pairwise(("u8", "u16"), LAYOUTS, INTERPS, STDS)


def merge_dark_design():
    """(dtype, interp, std): planar only."""
    return pairwise(DTYPES, INTERPS, STDS)


def merge_dark_ingest_design():
    return pairwise(DTYPES, LAYOUTS, INTERPS, STDS)


def stats_design(form):
    """(dtype, layout, interp); the statistics carry no uncertainty.  The ingest form takes codes only."""
    return pairwise(DTYPES if form == "code" else ("u8", "u16"), LAYOUTS, INTERPS)


def _no_lookup_std(t):
    return not (t[-2] == "lookup" and t[-1] != "none")      # LOOKUP with uncertainties: no gradient path, refused


def linearize_ingest_design():
    return pairwise(DTYPES, LAYOUTS, INTERPS, STDS, allowed=_no_lookup_std)


def linearize_dark_design(layouts):
    """(dtype, layout, interp, std): the dark forms always propagate an uncertainty and have no LOOKUP kernel."""
    return pairwise(DTYPES, layouts, (None, "linear", "catmull"), STDS)


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------
NP_DTYPE = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
TOP = {"u8": 255.0, "u16": 65535.0, "f32": 1.0}


def lut(channels=3, points=256):
    """(C, L) float32, one distinct gamma curve per row: a wrong row or plane shows."""
    g = np.linspace(0.0, 1.0, points, dtype=np.float64)
    return np.stack([g ** p for p in (1.8, 2.2, 2.6, 2.0)[:channels]]).astype(np.float32)


def random_codes(seed, shape, dtype):
    """Planar (N,C,H,W) samples drawn over the whole range of ``dtype`` (float32: [0, 1))."""
    rng = np.random.default_rng(seed)
    if dtype == "f32":
        return rng.random(shape, dtype=np.float32)
    return rng.integers(0, int(TOP[dtype]) + 1, size=shape).astype(NP_DTYPE[dtype])


def scene_codes(seed, n, chw, dtype):
    """A consistent exposure series through a gamma curve (what the merge oracles are well conditioned on), stored as
    ``dtype`` over its whole range -> (stored (N,C,H,W), exposure times float64 (N))."""
    rng = np.random.default_rng(seed)
    t = 0.002 * 2.0 ** np.arange(n)
    e = rng.random(chw) * (2.0 / np.sqrt(t[0] * t[-1]))
    x = np.clip(e[None] * t[:, None, None, None], 0.0, 1.0) ** (1 / 2.2)
    if dtype == "f32":
        return x.astype(np.float32), t
    return np.rint(x * TOP[dtype]).astype(NP_DTYPE[dtype]), t


def to_layout(planar, layout):
    """Planar (N,C,H,W) -> the raw stack of ``layout`` ((N,H,W,C); BGR: memory channel k holds plane C - 1 - k)."""
    if layout == "nchw":
        return np.ascontiguousarray(planar)
    return np.ascontiguousarray((planar[:, ::-1] if layout == "nhwc_bgr" else planar).transpose(0, 2, 3, 1))


def black_level_stages(dtype):
    """One constant Normalize with a black level: [("affine", sub, div, 1, 0)] over the range of ``dtype``."""
    top = TOP[dtype]
    black = top / 16.0 if dtype != "f32" else 0.0625
    return [("affine", float(np.float32(black)), float(np.float32(top - black)), 1.0, 0.0)]


def chain_f32(planar, stages, consts=None):
    """The float32 arithmetic of ct_ingest_transform on planar (N,C,H,W) samples: every operation rounded on its own.
    ``consts``: (sub, div) of an ("affine_data", mul, add) stage."""
    x = np.asarray(planar).astype(np.float32)
    f = np.float32
    for st in stages:
        if st[0] == "clamp":
            pairs = list(st[1]) * (x.shape[1] if len(st[1]) == 1 else 1)
            for c, (lo, hi) in enumerate(pairs[:x.shape[1]]):
                x[:, c] = np.minimum(np.maximum(x[:, c], f(lo)), f(hi))
            continue
        sub, div, mul, add = (consts[0], consts[1], st[1], st[2]) if st[0] == "affine_data" else st[1:]
        x = (((x - f(sub)) / f(div)).astype(np.float32) * f(mul)).astype(np.float32) + f(add)
    return x.astype(np.float32)


def sigma_of(std, pixels, explicit):
    """The float32 per-sample uncertainty of a std mode (0.01 constant, 0.05 multiplier), None for "none"."""
    if std == "none":
        return None
    if std == "constant":
        return np.full_like(pixels, np.float32(0.01))
    if std == "multiplier":
        return (pixels * np.float32(0.05)).astype(np.float32)
    return explicit


def explicit_sigma(seed, shape):
    rng = np.random.default_rng(seed + 7000)
    return (np.float32(0.002) + np.float32(0.03) * rng.random(shape, dtype=np.float32)).astype(np.float32)


def dark_fields(seed, shape):
    """One dark field per frame straddling the 0.05 threshold, and its std, float32 (N,C,H,W)."""
    rng = np.random.default_rng(seed + 9000)
    dark = (np.float32(0.1) * rng.random(shape, dtype=np.float32)).astype(np.float32)
    return dark, (np.float32(0.002) + np.float32(0.01) * rng.random(shape, dtype=np.float32)).astype(np.float32)
