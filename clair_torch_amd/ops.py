"""Tensor-level front-end of the HIP kernels (thin: validation, pointer plumbing, stream selection).

PyTorch is used here only for device memory, streams and dtype bookkeeping; all arithmetic on image
data happens inside the C-ABI library (include/clair_hip.h).  Every function requires CUDA (ROCm) tensors
and raises otherwise -- there is no CPU implementation in this package.
"""
import ctypes
from dataclasses import dataclass
from typing import Optional

import torch

from . import _native as nv

_INTERP = {"lookup": nv.INTERP_LOOKUP, "linear": nv.INTERP_LINEAR, "catmull": nv.INTERP_CATMULL, None: nv.INTERP_NONE}
_STD = {"none": nv.STD_NONE, "constant": nv.STD_CONSTANT, "multiplier": nv.STD_MULTIPLIER, "explicit": nv.STD_EXPLICIT}
_DTYPE = {torch.uint8: nv.DTYPE_U8, torch.uint16: nv.DTYPE_U16, torch.float32: nv.DTYPE_F32}
# input stack layouts: planar (N,C,H,W) as the reference's tensors, or interleaved (N,H,W,C) as OpenCV decodes
# (optionally BGR: the kernels then fold cv_to_torch's channel reversal into the load).  Outputs are always (C,H,W).
_LAYOUT = {"nchw": nv.LAYOUT_NCHW, "nhwc": nv.LAYOUT_NHWC, "nhwc_bgr": nv.LAYOUT_NHWC_BGR}


@dataclass
class TileGeometry:
    """Rows [row_offset, row_offset + h_tile) of a global (C, h_global, W) image (include/clair_hip.h ct_geometry)."""
    h_global: int
    row_offset: int = 0


def _require_device(t: torch.Tensor, name: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: clair_torch_amd kernels run on MI355X (cuda/ROCm) tensors only; "
                           "there is no CPU path in this package")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _chw(stack: torch.Tensor, layout: str):
    if layout not in _LAYOUT:
        raise ValueError(f"unknown layout {layout!r} (nchw, nhwc, nhwc_bgr)")
    if layout == "nchw":
        return stack.shape[1], stack.shape[2], stack.shape[3]
    return stack.shape[3], stack.shape[1], stack.shape[2]


def _out_shape(stack: torch.Tensor, layout: str, out_layout: str):
    """Shape of the merge's state / outputs: planar (C,H,W), or the stack's own per-image shape with out_layout "input"."""
    if out_layout not in ("planar", "input"):
        raise ValueError(f"unknown out_layout {out_layout!r} (planar, input)")
    return tuple(stack.shape[1:]) if out_layout == "input" else tuple(_chw(stack, layout))


def _tile_rows(h: int, tile: Optional[TileGeometry]):
    """(h_global, row_offset) of a band of ``h`` rows: the band itself without ``tile``."""
    hg, r0 = (h, 0) if tile is None else (tile.h_global, tile.row_offset)
    if r0 < 0 or r0 + h > hg:
        raise ValueError(f"tile rows [{r0}, {r0 + h}) do not fit a global height of {hg}")
    return hg, r0


def _geometry(stack: torch.Tensor, tile: Optional[TileGeometry], layout: str = "nchw") -> nv.Geometry:
    c, h, w = _chw(stack, layout)
    hg, r0 = _tile_rows(h, tile)
    return nv.Geometry(channels=c, h_tile=h, width=w, h_global=hg, row_offset=r0, image_stride=stack.stride(0),
                       layout=_LAYOUT[layout])


def _ingest_geometry(shape, tile: Optional[TileGeometry], layout: str) -> nv.Geometry:
    """Geometry of a contiguous stack the ingest fronts take, from its planar shape (B, C, H, W) (``ingest_shape``)."""
    _, c, h, w = shape
    hg, r0 = _tile_rows(h, tile)
    return nv.Geometry(channels=c, h_tile=h, width=w, h_global=hg, row_offset=r0, image_stride=c * h * w, layout=_LAYOUT[layout])


def _check_4d(stack: torch.Tensor, name: str, dims: str):
    """A 4-dimensional device tensor of a dtype the kernels read; ``dims``: how the caller words the four dimensions."""
    _require_device(stack, name)
    if stack.ndim != 4:
        raise ValueError(f"{name} must be {dims}, got shape {tuple(stack.shape)}")
    if stack.dtype not in _DTYPE:
        raise TypeError(f"{name} dtype {stack.dtype} unsupported (uint8, uint16 codes or float32 pixels)")


def _check_stack(stack: torch.Tensor, name="stack"):
    _check_4d(stack, name, "(N, C, H, W)")
    if stack.shape[0] > 0 and not stack[0].is_contiguous():
        raise ValueError(f"every image of {name} must be contiguous (C, H, W)")


def _default_max_code(t: torch.Tensor, max_code):
    """``max_code`` as given; for integer codes None means the dtype's full range (float32 pixels carry none)."""
    if t.dtype != torch.float32 and max_code is None:
        return 255.0 if t.dtype == torch.uint8 else 65535.0
    return max_code


def _explicit_std(std: torch.Tensor, stack: torch.Tensor, name: str = "stack", shapes: bool = False):
    """Explicit uncertainties in the stack's own layout as the kernels read them: float32, contiguous.  ``shapes``: the
    merge fronts' message, which names the two shapes."""
    _require_device(std, "std")
    if std.shape != stack.shape:
        raise ValueError(f"std shape {tuple(std.shape)} != stack shape {tuple(stack.shape)}" if shapes else f"std shape != {name} shape")
    return std.to(torch.float32).contiguous()


def _planar_std(std: torch.Tensor, shape, device, like: str):
    """Explicit uncertainties of an ingest front: float32 and planar ``shape`` like the ``like`` (outputs / state)."""
    _require_device(std, "std")
    if std.dtype != torch.float32 or tuple(std.shape) != shape or std.device != device:
        raise ValueError(f"std must be a float32 tensor of shape {shape} (planar, like the {like}) on {device}")
    return std.contiguous()


def _exposures_to_device(exposures: torch.Tensor, batch: int, device):
    """The ``batch`` exposure times as float64 on ``device``."""
    if exposures.is_cuda or device.type != "cuda":
        exposure_dev = exposures.to(device=device, dtype=torch.float64).contiguous()
    else:
        # A copy from pageable host memory blocks the host until the stream reaches it -- i.e. until the previous merge
        # kernel has finished -- which serialises this call's host work with the device (measured: 1.18 ms per
        # compute_hdr_image call against a 0.95 ms kernel).  Staged through pinned memory the copy is asynchronous.
        exposure_dev = exposures.to(torch.float64).contiguous().pin_memory().to(device, non_blocking=True)
    if exposure_dev.numel() != batch:
        raise ValueError(f"{exposure_dev.numel()} exposure times for a batch of {batch}")
    return exposure_dev


def _exposure_list_to_device(exposures, sizes, device):
    """The exposure times of several batches of ``sizes`` frames, one after the other, as float64 on ``device``.  Lists that
    live on the device already are concatenated there (no copy back to the host, which would wait for the stream); host lists
    are staged through pinned memory (see ``_exposures_to_device``)."""
    for e, n in zip(exposures, sizes):
        if e.numel() != n:
            raise ValueError(f"{e.numel()} exposure times for a batch of {n}")
    if all(e.is_cuda for e in exposures):
        return torch.cat([e.detach().to(device=device, dtype=torch.float64).reshape(-1) for e in exposures])
    host_exp = torch.cat([e.detach().to("cpu", torch.float64).reshape(-1) for e in exposures])
    return host_exp.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host_exp


def _pointers(tensors):
    """The HOST array of the tensors' device pointers (NULL for a None among them); None for no list at all."""
    if tensors is None:
        return None
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _lin_std_out(out, shape, device, want_std: bool, lin_required: bool):
    """The (lin, std | None) float32 outputs of a linearization: fresh ones, or the caller's ``out`` pair checked.
    ``lin_required``: refuse a pair without out[0] here (else the library does)."""
    if out is None:
        lin = torch.empty(shape, dtype=torch.float32, device=device)
        return lin, (torch.empty_like(lin) if want_std else None)
    lin, std_out = out
    for name, t in (("out[0]", lin), ("out[1]", std_out)):
        if t is None:
            continue
        _require_device(t, name)
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape}")
    if lin_required and lin is None:
        raise ValueError("out[0] is required")
    if want_std and std_out is None:
        raise ValueError("want_std needs out[1]")
    return lin, (std_out if want_std else None)


def _flat_arguments(flat, shape, device, want_std: bool):
    """``flat`` of the linearize_*_flat fronts as the _flat entry points read it: (flat, flat std | None, flat mean), the images
    float32 and planar (C,H,W) like one frame of the outputs (``shape``: (F,C,H,W); a leading batch dimension of 1 is dropped),
    the mean (C,) float32 -- ``flatfield_mean(flat)`` -- all on ``device``.  The correction writes a std."""
    if not isinstance(flat, (tuple, list)) or len(flat) != 3:
        raise ValueError("flat must be (flat, flat_std or None, flat_mean)")
    if not want_std:
        raise ValueError("flat needs want_std: the flat-field correction writes a std")
    chw = tuple(shape[1:])
    images = []
    for name, t in (("flat[0]", flat[0]), ("flat[1]", flat[1])):
        if t is None:
            if name == "flat[0]":
                raise ValueError("flat[0], the flat field, is required")
            images.append(None)
            continue
        _require_device(t, name)
        if t.ndim == 4 and t.shape[0] == 1:
            t = t[0]
        if t.dtype != torch.float32 or tuple(t.shape) != chw or t.device != device:
            raise ValueError(f"{name} must be a float32 tensor of shape {chw} (planar, like a frame of the outputs) on {device}")
        images.append(t.contiguous())
    mean = flat[2]
    _require_device(mean, "flat[2]")
    if mean.dtype != torch.float32 or tuple(mean.shape) != chw[:1] or mean.device != device:
        raise ValueError(f"flat[2] must be the float32 tensor of {chw[0]} channel means on {device} (flatfield_mean)")
    return images[0], images[1], mean.contiguous()


def _check_stats_state(mean_state, m2_state, shape, device=None):
    """The running (mean, m2) state: contiguous float32 ``shape``; on ``device`` where the caller names one."""
    what = "(C,H,W) tensor" if device is None else f"(C,H,W) = {shape} tensor on {device}"
    for name, t in (("mean_state", mean_state), ("m2_state", m2_state)):
        _require_device(t, name)
        if (t.dtype != torch.float32 or tuple(t.shape) != shape or (device is not None and t.device != device)
                or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 {what}")


def _checked_out(out, shape, dtype, device, dtype_name=None):
    """``out`` when it is the contiguous device tensor of exactly ``shape`` / ``dtype`` a caller may pass, a fresh one
    for None."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _require_device(out, "out")
    if tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {dtype_name or dtype} tensor of shape {shape} on {device}")
    return out


def _call(entry, dev, *args):
    """The tail of every front beside the HDR merge: the library's ``entry``(*args, stream) on ``dev``, its status checked."""
    with torch.cuda.device(dev):
        rc = getattr(nv.load(), entry)(*args, _stream(dev))
    nv.check(rc, entry)


def _std_arguments(std, std_mode, normalise, refuse_unknown: bool = True):
    """(std, std_mode) of a front that takes explicit uncertainties: a given ``std`` means mode "explicit" and goes through
    ``normalise`` (``_explicit_std`` / ``_planar_std`` with the front's own wording).  ``refuse_unknown`` False is what
    linearize_frames, dark_field_blur and the two plain pair fronts have always done: they leave an unknown mode to the lookup
    in ``_STD`` (KeyError), where every other front raises ValueError here.  Callers may rely on either, so the difference is
    kept, not unified (tests/test_fronts_host.py, tests/test_ops_refusals_host.py)."""
    if std is not None:
        std_mode, std = "explicit", normalise(std)
    if refuse_unknown and std_mode not in _STD:
        raise ValueError(f"unknown std_mode {std_mode}")
    return std, std_mode


def _icrf_struct(lut: Optional[torch.Tensor], interp, channels):
    """(the ct_icrf of ``lut``, the float32 table it points to).  The table is a local of the calling front and so lives until
    that front returns, behind the call that reads it.  The rule for every pointer a front hands to ``_call``: a tensor the
    front or one of its helpers made (a contiguous or float32 copy above all) stays in a local of a frame that is still
    running when the call is made -- a helper that builds the arguments returns such tensors with them."""
    if lut is None:
        return nv.Icrf(lut_dev=None, n_points=0, interp=nv.INTERP_NONE), None
    _require_device(lut, "lut")
    if lut.ndim != 2 or lut.shape[0] != channels:
        raise ValueError(f"lut must be (C={channels}, L), got {tuple(lut.shape)}")
    if interp not in _INTERP or interp is None:
        raise ValueError(f"Unknown interpolation mode {interp}")
    lut_c = lut.detach().to(torch.float32).contiguous()
    return nv.Icrf(lut_dev=lut_c.data_ptr(), n_points=lut_c.shape[1], interp=_INTERP[interp]), lut_c


def _state_ptrs(state):
    """(mean, sumw, var) pointers of a MergeState; NULL for no state / no variance buffer."""
    if not state:
        return None, None, None
    return _ptr(state.mean), _ptr(state.sumw), _ptr(state.var)


class MergeState:
    """Device-resident WBOMean state + running variance of a streaming merge (one entry per output element)."""

    def __init__(self, shape, device, with_variance: bool):
        self.mean = torch.empty(shape, dtype=torch.float64, device=device)
        self.sumw = torch.empty(shape, dtype=torch.float32, device=device)
        self.var = torch.empty(shape, dtype=torch.float32, device=device) if with_variance else None
        self.batches = 0


def _merge_setup(out_shape, device, out_layout, state, finalize, has_std, mean_dtype, reference_order, flags, what, first=None):
    """What every hdr_merge_* front does last before its call: (flag word, mean_out, std_out) for a state / output shape
    ``out_shape`` on ``device``, after the MergeState checks.  ``first``: None = the state decides about FIRST_BATCH (a fresh
    MergeState, or none, starts the merge); True / False says so for a state filled elsewhere."""
    if state is None or state.batches == 0:
        flags |= nv.MERGE_FIRST_BATCH
    if finalize:
        flags |= nv.MERGE_FINALIZE
    if reference_order is not None:
        flags |= nv.MERGE_REFERENCE_ORDER if reference_order else nv.MERGE_CLOSED_FORM
    if mean_dtype == torch.float32:
        flags |= nv.MERGE_MEAN_OUT_F32
    elif mean_dtype != torch.float64:
        raise TypeError("mean_dtype must be float64 (reference) or float32")
    if out_layout not in ("planar", "input"):
        raise ValueError(f"unknown out_layout {out_layout!r} (planar, input)")
    if out_layout == "input":
        flags |= nv.MERGE_OUT_AS_INPUT
    if state is None and not finalize:
        raise ValueError(f"a non-final {what} needs a MergeState")
    if state is not None and has_std and state.var is None:
        raise ValueError("MergeState was created without a variance buffer")
    if state is not None and tuple(state.mean.shape) != out_shape:
        raise ValueError(f"MergeState has shape {tuple(state.mean.shape)}, this merge needs {out_shape}")
    if first is not None:
        flags = (flags | nv.MERGE_FIRST_BATCH) if first else (flags & ~nv.MERGE_FIRST_BATCH)
    mean_out = torch.empty(out_shape, dtype=mean_dtype, device=device) if finalize else None
    std_out = torch.empty(out_shape, dtype=torch.float32, device=device) if (finalize and has_std) else None
    return flags, mean_out, std_out


def _launch_merge(entry, dev, head, state, flags, batches, mean_out, std_out, *, retry_with_state=False, probe_one_launch=False,
                  retry_one_batch=True):
    """The tail of every hdr_merge_* front: the library's ``entry``(*head, state pointers, outputs, flag word, stream) on ``dev``,
    its status checked, ``state.batches`` advanced by ``batches``; -> (mean_out, std_out) of a final call, else None.

    ``retry_with_state``: a whole merge in one launch needs no state arrays at all, so a call without a MergeState goes
    without; only when the library answers CT_ERR_UNSUPPORTED (what cannot run as one launch walks the batches with the state
    in memory; nothing has been launched then) is a fresh one made and the call repeated -- unless the caller's flag word
    requires one launch.  ``probe_one_launch``: the first try without a state carries MERGE_REQUIRE_ONE_LAUNCH, for an entry
    point that answers a stateless walk with CT_ERR_INVALID_ARGUMENT.  ``retry_one_batch`` False: no second try for one batch."""
    def attempt(st, fl):
        with torch.cuda.device(dev):
            return getattr(nv.load(), entry)(*head, *_state_ptrs(st), _ptr(mean_out), _ptr(std_out), fl, _stream(dev))

    rc = attempt(state, flags | (nv.MERGE_REQUIRE_ONE_LAUNCH if probe_one_launch and state is None else 0))
    if (rc == nv.ERR_UNSUPPORTED and retry_with_state and state is None and not flags & nv.MERGE_REQUIRE_ONE_LAUNCH
            and (retry_one_batch or batches > 1)):
        state = MergeState(tuple(mean_out.shape), dev, std_out is not None)      # (no state: the call is final and has outputs)
        rc = attempt(state, flags)
    nv.check(rc, entry)
    if state is not None:
        state.batches += batches
    return None if mean_out is None else (mean_out, std_out)


def _weight(gaussian_weight):
    return nv.WEIGHT_GAUSS if gaussian_weight else nv.WEIGHT_NONE


MAX_MERGE_BATCHES = 16  # batches one ct_hdr_merge_batches call takes (the kernel's argument block holds 16 pointers)


def _all_or_none(values, what):
    """A per-batch list that holds a tensor for every batch or for none: -> the list, None for one of Nones (mixed: refused)."""
    if values is None or not any(t is None for t in values):
        return values
    if any(t is not None for t in values):
        raise ValueError(f"{what} for every batch of one call, or for none")
    return None


def _check_batch_list(stacks, lists, names, check_stack, *, all_or_none=(), refuse_empty=True, one_batch_elsewhere=False):
    """The batches of one hdr_merge_*_batches call: ``stacks`` and the ``lists`` beside it (None: not given) are non-empty and
    equally long, at most MAX_MERGE_BATCHES; the lists ``all_or_none`` names by position in ``lists``, with the message's
    subject, hold a tensor for every batch or for none; every stack passes ``check_stack``, shares dtype, image shape and device
    with the first and (``refuse_empty``) holds a frame.  -> the ``all_or_none`` lists, None for one of Nones.
    ``one_batch_elsewhere``: a single batch goes to the single-batch front, which checks the stack itself."""
    k = len(stacks)
    if k == 0 or any(v is not None and len(v) != k for v in lists):
        raise ValueError(f"{names} must be non-empty lists of equal length")
    if k > MAX_MERGE_BATCHES:
        raise ValueError(f"at most {MAX_MERGE_BATCHES} batches per call")
    settled = [_all_or_none(lists[i], what) for i, what in all_or_none]
    if k == 1 and one_batch_elsewhere:
        return settled
    s0 = stacks[0]
    for t in stacks:
        check_stack(t)
        if t.dtype != s0.dtype or t.shape[1:] != s0.shape[1:] or t.device != s0.device:
            raise ValueError("all batches of one call must share dtype, image shape and device")
        if refuse_empty and t.shape[0] < 1:
            raise ValueError("empty batch")
    return settled


def hdr_merge_batch(stack: torch.Tensor, exposures: torch.Tensor, *, lut: Optional[torch.Tensor] = None,
                    interp: Optional[str] = "linear", gaussian_weight: bool = True,
                    std: Optional[torch.Tensor] = None, std_mode: str = "none", std_value: float = 0.0,
                    max_code: Optional[float] = None, state: Optional[MergeState] = None, finalize: bool = True,
                    tile: Optional[TileGeometry] = None, mean_dtype: torch.dtype = torch.float64, layout: str = "nchw",
                    force_f64_moments: bool = False, reference_order: Optional[bool] = None, out_layout: str = "planar"):
    """One batch of the HDR merge (ct_hdr_merge_batch).  Returns (mean, std|None) when ``finalize`` else None.

    stack (B,C,H,W) uint8/uint16 codes (give ``max_code``) or float32 pixels; exposures (B) any float dtype.
    ``state`` carries the streaming state across batches (None = single-batch merge).
    ``layout`` "nhwc" / "nhwc_bgr": the stack is (B,H,W,C) as OpenCV decodes it (an explicit std stack likewise);
    outputs stay planar (C,H,W) -- unless ``out_layout="input"`` (extension, CT_MERGE_OUT_AS_INPUT): state and outputs
    then have the stack's own memory order, (H,W,C) in the input's channel order, which is what an OpenCV writer wants
    and lets the kernel store dense packets without regrouping (the MergeState must then be created with that shape).
    ``force_f64_moments`` (diagnostic, CT_MERGE_F64_MOMENTS): keep the float64-moment kernel where the pivoted
    float32 one would run (tests compare the two).
    ``reference_order``: True = evaluate the uncertainty in the reference's own float32 autograd order
    (CT_MERGE_REFERENCE_ORDER: two passes, slower, reproduces the reference's rounding); False = closed-form kernels in
    every mode (CT_MERGE_CLOSED_FORM); None = the library's default (reference order for LOOKUP / CATMULL with
    uncertainties, closed form otherwise).
    """
    _check_stack(stack)
    b = stack.shape[0]
    c, h, w = _chw(stack, layout)
    dev = stack.device
    if b < 1:
        raise ValueError("empty batch")
    if std is not None:
        std_mode = "explicit"
        _require_device(std, "std")
        if std.shape != stack.shape or std.dtype != torch.float32 or std.stride() != stack.stride():
            std = _explicit_std(std, stack, shapes=True)
            if std.stride() != stack.stride():
                stack = stack.contiguous()
    if std_mode not in _STD:
        raise ValueError(f"unknown std_mode {std_mode}")
    max_code = _default_max_code(stack, max_code)
    exposure_dev = _exposures_to_device(exposures, b, dev)
    icrf, lut_keep = _icrf_struct(lut, interp, c)      # (lut_keep: what the struct points to, alive until the call is made)
    geom = _geometry(stack, tile, layout)
    flags, mean_out, std_out = _merge_setup(_out_shape(stack, layout, out_layout), dev, out_layout, state, finalize, std_mode != "none",
                                            mean_dtype, reference_order, nv.MERGE_F64_MOMENTS if force_f64_moments else 0, "batch")
    head = (_ptr(stack), _DTYPE[stack.dtype], float(max_code or 1.0), b, ctypes.byref(geom), _ptr(std), _STD[std_mode], float(std_value),
            _ptr(exposure_dev), ctypes.byref(icrf), _weight(gaussian_weight))
    return _launch_merge("ct_hdr_merge_batch", dev, head, state, flags, 1, mean_out, std_out)


def hdr_merge_batches(stacks, exposures, *, lut: Optional[torch.Tensor] = None, interp: Optional[str] = "linear",
                      gaussian_weight: bool = True, stds=None, std_mode: str = "none", std_value: float = 0.0,
                      max_code: Optional[float] = None, state: Optional[MergeState] = None, finalize: bool = True,
                      tile: Optional[TileGeometry] = None, mean_dtype: torch.dtype = torch.float64, layout: str = "nchw",
                      reference_order: Optional[bool] = None, require_one_launch: bool = False, out_layout: str = "planar"):
    """Several CONSECUTIVE batches of one merge in one call (ct_hdr_merge_batches): the same result, bit for bit, as
    hdr_merge_batch on each of them in turn with ``state`` carried along -- but where the pivoted code-domain kernel
    applies the streaming state stays in registers between the batches (one launch, no state traffic).

    ``stacks``: list of (B_k,C,H,W) device tensors of one dtype / geometry (each sorted by exposure like custom_collate);
    ``exposures``: list of (B_k) tensors; ``stds``: list of explicit std tensors or None.  At most MAX_MERGE_BATCHES.
    ``require_one_launch`` (tests): raise instead of falling back to one launch per batch.  ``out_layout``: as in hdr_merge_batch.
    Returns (mean, std|None) when ``finalize`` else None."""
    # (an empty batch among several is left to the library, which skips it)
    _check_batch_list(stacks, (exposures, stds), "stacks / exposures / stds", _check_stack, refuse_empty=False, one_batch_elsewhere=True)
    k = len(stacks)
    if k == 1:
        return hdr_merge_batch(stacks[0], exposures[0], lut=lut, interp=interp, gaussian_weight=gaussian_weight,
                               std=None if stds is None else stds[0], std_mode=std_mode, std_value=std_value, max_code=max_code,
                               state=state, finalize=finalize, tile=tile, mean_dtype=mean_dtype, layout=layout,
                               reference_order=reference_order, out_layout=out_layout)
    dev = stacks[0].device
    c, h, w = _chw(stacks[0], layout)
    stds, std_mode = _std_arguments(stds, std_mode,
                                    lambda sds: [_explicit_std(sd.to(dev), t, shapes=True) for sd, t in zip(sds, stacks)])
    stacks = [t.contiguous() for t in stacks]
    max_code = _default_max_code(stacks[0], max_code)
    sizes = [int(t.shape[0]) for t in stacks]
    exposure_dev = _exposure_list_to_device(exposures, sizes, dev)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _geometry(stacks[0], tile, layout)
    has_std = std_mode != "none"
    out_shape = _out_shape(stacks[0], layout, out_layout)
    flags, mean_out, std_out = _merge_setup(out_shape, dev, out_layout, state, finalize, has_std, mean_dtype, reference_order,
                                            nv.MERGE_REQUIRE_ONE_LAUNCH if require_one_launch else 0, "call")
    if state is None:
        # several batches: whatever cannot run as one launch walks them with the state in memory.  This front makes the state up
        # front and never retries; the others try without one first (``_launch_merge``)
        state = MergeState(out_shape, dev, has_std)
    head = (_pointers(stacks), _pointers(stds), (ctypes.c_int32 * k)(*sizes), k, _DTYPE[stacks[0].dtype], float(max_code or 1.0),
            ctypes.byref(geom), _STD[std_mode], float(std_value), _ptr(exposure_dev), ctypes.byref(icrf), _weight(gaussian_weight))
    return _launch_merge("ct_hdr_merge_batches", dev, head, state, flags, k, mean_out, std_out)


def linearize_frames(frames: torch.Tensor, lut: torch.Tensor, interp: str = "linear", *,
                     std: Optional[torch.Tensor] = None, std_mode: str = "none", std_value: float = 0.0,
                     max_code: Optional[float] = None, want_std: bool = True, tile: Optional[TileGeometry] = None,
                     layout: str = "nchw", out=None):
    """ct_linearize_std on (F,C,H,W) frames -> (lin float32, std float32 | None); every frame is its own batch.
    ``layout`` "nhwc" / "nhwc_bgr": frames are (F,H,W,C); the outputs are planar (F,C,H,W).
    ``out`` = (lin, std | None): caller-owned contiguous float32 (F,C,H,W) device buffers to write into (the streamed
    pipeline re-uses its ring slots instead of allocating per launch)."""
    return _linearize_std(frames, lut, interp, std, std_mode, std_value, max_code, want_std, tile, layout, out, None)


def linearize_frames_flat(frames: torch.Tensor, lut: torch.Tensor, interp: str = "linear", *, flat,
                          std: Optional[torch.Tensor] = None, std_mode: str = "none", std_value: float = 0.0,
                          max_code: Optional[float] = None, want_std: bool = True, tile: Optional[TileGeometry] = None,
                          layout: str = "nchw", out=None):
    """ct_linearize_std_flat: ``linearize_frames`` followed by ``flatfield_correct(lin, std, flat, flat_std,
    input_is_variance=False, through_mean=False, flat_mean=flat_mean)``, bit for bit and in the same launch.
    ``flat`` = (flat, flat_std | None, flat_mean): ``flat`` / ``flat_std`` float32 (C,H,W) like a frame of the outputs (the
    rows of the band with ``tile``), ``flat_mean`` = ``flatfield_mean(flat)``.  Needs ``want_std``: the correction writes a
    std.  Everything else as ``linearize_frames``."""
    return _linearize_std(frames, lut, interp, std, std_mode, std_value, max_code, want_std, tile, layout, out, flat)


def _linearize_std(frames, lut, interp, std, std_mode, std_value, max_code, want_std, tile, layout, out, flat):
    """The two fronts above: ct_linearize_std, with ``flat`` ct_linearize_std_flat."""
    _check_stack(frames, "frames")
    f = frames.shape[0]
    c, h, w = _chw(frames, layout)
    dev = frames.device
    std, std_mode = _std_arguments(std, std_mode, lambda sd: _explicit_std(sd, frames, "frames"), refuse_unknown=False)
    max_code = _default_max_code(frames, max_code)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    frames = frames.contiguous()
    geom = _geometry(frames, tile, layout)
    lin, std_out = _lin_std_out(out, (f, c, h, w), dev, want_std, lin_required=False)
    args = (_ptr(frames), _DTYPE[frames.dtype], float(max_code or 1.0), f, ctypes.byref(geom), _ptr(std), _STD[std_mode],
            float(std_value), ctypes.byref(icrf), _ptr(lin), _ptr(std_out))
    if flat is None:
        _call("ct_linearize_std", dev, *args)
    else:
        flat = _flat_arguments(flat, (f, c, h, w), dev, want_std)
        _call("ct_linearize_std_flat", dev, *args, *map(_ptr, flat))
    return lin, std_out


def icrf_forward(x: torch.Tensor, lut: torch.Tensor, interp: str, tile: Optional[TileGeometry] = None):
    """ct_linearize_fwd: ICRFModelBase.forward on a float32 (N,C,H,W) device tensor."""
    _check_stack(x, "image")
    if x.dtype != torch.float32:
        raise TypeError("icrf_forward expects float32 pixel values")
    x = x.contiguous()
    icrf, lut_keep = _icrf_struct(lut, interp, x.shape[1])
    geom = _geometry(x, tile)
    out = torch.empty_like(x)
    _call("ct_linearize_fwd", x.device, _ptr(x), x.shape[0], ctypes.byref(geom), ctypes.byref(icrf), _ptr(out))
    return out


def icrf_backward(x: torch.Tensor, grad_out: torch.Tensor, lut: torch.Tensor, interp: str, need_x: bool, need_lut: bool,
                  tile: Optional[TileGeometry] = None):
    """ct_linearize_bwd: (grad wrt image | None, grad wrt LUT (C,L) | None)."""
    _check_stack(x, "image")
    x = x.contiguous()
    grad_out = grad_out.to(torch.float32).contiguous()
    icrf, lut_keep = _icrf_struct(lut, interp, x.shape[1])
    geom = _geometry(x, tile)
    gx = torch.empty_like(x) if need_x else None
    gl = torch.zeros((x.shape[1], lut.shape[1]), dtype=torch.float32, device=x.device) if need_lut else None
    _call("ct_linearize_bwd", x.device, _ptr(x), _ptr(grad_out), x.shape[0], ctypes.byref(geom), ctypes.byref(icrf), _ptr(gx),
          _ptr(gl))
    return gx, gl


# ---- exposure-pair linearity residual (training / measure_linearity) -----------------------------------------
def _pair_params(lower, upper, use_relative, use_unc_weight, std_mode, std_value, weight_scale=10.0, pair_band=0):
    return nv.PairParams(lower=float(lower), upper=float(upper), weight_scale=float(weight_scale),
                         use_relative=int(bool(use_relative)), use_uncertainty_weighting=int(bool(use_unc_weight)),
                         std_mode=_STD[std_mode], std_value=float(std_value), pair_band=int(pair_band))


def _pair_sums(entry, dev, head, pairs, channels, prm, level, center):
    """The forward half of the four pair fronts: ``entry``(*head, pair list, parameters, level, center, sums) -> the (P, C, 5)
    float64 sums; ``head``: the entry point's arguments up to the ICRF.  Without pairs nothing is launched."""
    sums = torch.zeros((pairs.n_pairs, channels, 5), dtype=torch.float64, device=dev)
    if center is not None:
        center = center.to(device=dev, dtype=torch.float64).contiguous()
        if center.shape != (pairs.n_pairs, channels):
            raise ValueError(f"center must be (P={pairs.n_pairs}, C={channels})")
    if pairs.n_pairs:
        _call(entry, dev, *head, _ptr(pairs.i), _ptr(pairs.j), _ptr(pairs.ratio), pairs.n_pairs, ctypes.byref(prm), int(level),
              _ptr(center), _ptr(sums))
    return sums


def _pair_lut_grad(entry, dev, head, pairs, channels, prm, weighted, coef, smean, n_points):
    """The backward half: ``entry``(*head, partner lists, parameters, coef, smean, grad, workspace) -> the (C, L) float64 LUT
    gradient; ``weighted``: the uncertainties weigh the pairs, which needs the forward's spatial means ``smean``."""
    if weighted:
        if smean is None:
            raise ValueError("the uncertainty-weighted backward needs the forward's spatial means")
        smean = smean.to(device=dev, dtype=torch.float64).contiguous()
    else:
        smean = None
    coef = coef.to(device=dev, dtype=torch.float64).contiguous()
    if coef.shape != (pairs.n_pairs, channels):
        raise ValueError(f"coef must be (P={pairs.n_pairs}, C={channels}), got {tuple(coef.shape)}")
    grad = torch.zeros((channels, n_points), dtype=torch.float64, device=dev)
    if pairs.n_pairs:
        ws = pairs.workspace(channels)
        _call(entry, dev, *head, _ptr(pairs.ratio), pairs.n_pairs, _ptr(pairs.part_off), _ptr(pairs.part_sample),
              _ptr(pairs.part_pair), ctypes.byref(prm), _ptr(coef), _ptr(smean), _ptr(grad), _ptr(ws), ws.numel())
    return grad


class PairList:
    """Exposure pairs on the device: (i, j, ratio) in the reference's triu order plus the per-sample partner
    lists (CSR) the backward kernel walks.  Built from get_valid_exposure_pairs' outputs (tiny, host-side)."""

    def __init__(self, i_idx: torch.Tensor, j_idx: torch.Tensor, ratio: torch.Tensor, n_images: int, device):
        i_cpu, j_cpu = i_idx.to("cpu", torch.int64), j_idx.to("cpu", torch.int64)
        self.n_pairs, self.n_images = int(i_cpu.numel()), int(n_images)
        self.i = i_cpu.to(torch.int32).to(device)
        self.j = j_cpu.to(torch.int32).to(device)
        self.ratio = ratio.to("cpu", torch.float64).to(device)
        # band of the list: every pair has 0 < j - i <= band (0 when some pair has j <= i): the hint of ct_pair_params
        distance = j_cpu - i_cpu
        self.band = int(distance.max()) if self.n_pairs and int(distance.min()) > 0 else 0
        # CSR over samples, entries of a sample in ascending pair order: (partner, p) when the sample is the pair's first
        # image, (partner, ~p) when it is the second.  Vectorised: one stable sort of the 2P (owner, pair) keys.
        p_idx = torch.arange(self.n_pairs, dtype=torch.int64)
        owner = torch.cat([i_cpu, j_cpu])
        partner = torch.cat([j_cpu, i_cpu])
        code = torch.cat([p_idx, ~p_idx])
        order = torch.argsort(owner * max(self.n_pairs, 1) + torch.cat([p_idx, p_idx]), stable=True)
        counts = torch.bincount(owner, minlength=n_images) if self.n_pairs else torch.zeros(n_images, dtype=torch.int64)
        offsets = torch.zeros(n_images + 1, dtype=torch.int64)
        offsets[1:] = torch.cumsum(counts[:n_images], dim=0)
        samples, codes = partner[order], code[order]
        self.part_off = offsets.to(torch.int32).to(device)
        self.part_sample = (samples if self.n_pairs else torch.zeros(1, dtype=torch.int64)).to(torch.int32).to(device)
        self.part_pair = (codes if self.n_pairs else torch.zeros(1, dtype=torch.int64)).to(torch.int32).to(device)
        self._workspace = {}

    def workspace(self, channels: int) -> torch.Tensor:
        """Scratch for ct_pair_residual_bwd (its per-channel partner tables), allocated once per channel count."""
        ws = self._workspace.get(channels)
        if ws is None:
            nbytes = int(nv.load().ct_pair_residual_bwd_workspace(self.n_images, self.n_pairs, channels))
            ws = torch.empty(max(nbytes, 32), dtype=torch.uint8, device=self.i.device)
            self._workspace[channels] = ws
        return ws


def pair_residual_sums(stack: torch.Tensor, pairs: PairList, *, lut: Optional[torch.Tensor], interp: Optional[str],
                       lower: float, upper: float, use_relative: bool, use_unc_weight: bool,
                       std: Optional[torch.Tensor] = None, std_mode: str = "none", std_value: float = 0.0,
                       max_code: Optional[float] = None, level: int = 1, tile: Optional[TileGeometry] = None,
                       center: Optional[torch.Tensor] = None, layout: str = "nchw"):
    """ct_pair_residual_fwd -> (P, C, 5) float64 sums [sum w m, sum v w m, sum (v-center)^2 w m, sum err m, sum m].
    ``layout`` "nhwc" / "nhwc_bgr": the stack (and an explicit std stack) is (N,H,W,C) as OpenCV decodes it."""
    _check_stack(stack)
    n = stack.shape[0]
    c, _, _ = _chw(stack, layout)
    dev = stack.device
    if n != pairs.n_images:
        raise ValueError(f"pair list was built for {pairs.n_images} images, stack has {n}")
    std, std_mode = _std_arguments(std, std_mode, lambda sd: _explicit_std(sd, stack), refuse_unknown=False)
    if std is not None:
        stack = stack.contiguous()
    max_code = _default_max_code(stack, max_code)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _geometry(stack, tile, layout)
    prm = _pair_params(lower, upper, use_relative, use_unc_weight, std_mode, std_value)
    head = (_ptr(stack), _DTYPE[stack.dtype], float(max_code or 1.0), n, ctypes.byref(geom), _ptr(std), ctypes.byref(icrf))
    return _pair_sums("ct_pair_residual_fwd", dev, head, pairs, c, prm, level, center)


def pair_residual_lut_grad(stack: torch.Tensor, pairs: PairList, coef: torch.Tensor, *, lut: torch.Tensor, interp: str,
                           lower: float, upper: float, use_relative: bool, max_code: Optional[float] = None,
                           tile: Optional[TileGeometry] = None, use_unc_weight: bool = False,
                           std: Optional[torch.Tensor] = None, std_mode: str = "none", std_value: float = 0.0,
                           smean: Optional[torch.Tensor] = None, lane_kernel: bool = True, layout: str = "nchw"):
    """ct_pair_residual_bwd -> (C, L) float64 LUT gradient of sum_pc coef_pc * D_pc * mean_pc (coef = dL/dmean / D).
    With ``use_unc_weight`` and uncertainties the weights depend on the LUT and ``smean`` (P,C) is required.
    ``lane_kernel=False`` withholds the pair list's band hint, i.e. forces the generic backward kernel (tests).
    ``layout`` as in ``pair_residual_sums``."""
    _check_stack(stack)
    n = stack.shape[0]
    c, _, _ = _chw(stack, layout)
    dev = stack.device
    # (the kernel reads explicit uncertainties at the stack's indices: same shape)
    std, std_mode = _std_arguments(std, std_mode, lambda sd: _explicit_std(sd, stack), refuse_unknown=False)
    if std is not None:
        stack = stack.contiguous()
    if not use_unc_weight:
        std, std_mode = None, "none"
    max_code = _default_max_code(stack, max_code)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _geometry(stack, tile, layout)
    prm = _pair_params(lower, upper, use_relative, use_unc_weight, std_mode, std_value,
                       pair_band=pairs.band if lane_kernel else 0)
    head = (_ptr(stack), _DTYPE[stack.dtype], float(max_code or 1.0), n, ctypes.byref(geom), _ptr(std), ctypes.byref(icrf))
    return _pair_lut_grad("ct_pair_residual_bwd", dev, head, pairs, c, prm, std_mode != "none", coef, smean, lut.shape[1])


# ---- per-band statistics (BASELINE configuration C5) -------------------------------------------------------------
def band_stats(mean: torch.Tensor, std: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ct_band_stats: (6, C) float64 = [min mean, max mean, sum mean, min std, max std, sum std] per channel of a merged
    (C, H_band, W) band in ONE pass (``std`` None: the std rows are zero).  min / max / sum combine over row bands."""
    _require_device(mean, "mean")
    if mean.dtype != torch.float64 or mean.dim() != 3:
        raise ValueError("mean must be a (C, H, W) float64 device tensor")
    mean = mean.contiguous()
    c = mean.shape[0]
    plane = mean.shape[1] * mean.shape[2]
    if std is not None:
        _require_device(std, "std")
        if std.dtype != torch.float32 or std.shape != mean.shape:
            raise ValueError("std must be float32 with the mean's shape")
        std = std.contiguous()
    ws_bytes = int(nv.load().ct_band_stats_workspace(c))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=mean.device)
    out = torch.empty((6, c), dtype=torch.float64, device=mean.device)
    _call("ct_band_stats", mean.device, _ptr(mean), _ptr(std), c, plane, _ptr(ws), ws_bytes, _ptr(out))
    return out


# ---- flat-field correction epilogues ----------------------------------------------------------------------------
def _flat_image(flat: torch.Tensor, device) -> torch.Tensor:
    """A flat field (or its uncertainty) as the kernels read it: float32, contiguous (C,H,W) on ``device``."""
    flat = flat.to(device=device, dtype=torch.float32).contiguous()
    return flat[0] if flat.ndim == 4 else flat


def _flatfield_means(value, is_f64: bool, flat: torch.Tensor, global_pixels, reduce):
    """ct_flatfield_sums on a ``_flat_image`` (and on ``value``, or None), the division and the cast: ((C,) float32 spatial
    mean of the flat field, (C,) float64 mean of value / (flat + eps) | None)."""
    c, plane, dev = flat.shape[0], flat.shape[1] * flat.shape[2], flat.device
    sums = torch.zeros((c, 2), dtype=torch.float64, device=dev)
    _call("ct_flatfield_sums", dev, _ptr(value), int(is_f64), _ptr(flat), c, plane, _ptr(sums))
    if reduce is not None:
        reduce(sums)
    n_px = float(global_pixels if global_pixels is not None else plane)
    return (sums[:, 0] / n_px).to(torch.float32).contiguous(), ((sums[:, 1] / n_px).contiguous() if value is not None else None)


def flatfield_mean(flat: torch.Tensor, *, global_pixels: Optional[int] = None, reduce=None) -> torch.Tensor:
    """The (C,) float32 spatial mean of a (C,H,W) flat field as ``flatfield_correct`` computes it (flat_field_mean with a
    mid-area of 1.0, common/general_functions.py:182-210; ct_flatfield_sums without a value): the constant of a linearization
    run, computed once and handed to ``flatfield_correct(flat_mean=...)`` or, in ``flat``, to the linearize_*_flat fronts.
    ``reduce`` / ``global_pixels`` as there."""
    _require_device(flat, "flat")
    return _flatfield_means(None, False, _flat_image(flat, flat.device), global_pixels, reduce)[0]


def flatfield_correct(value: torch.Tensor, var_or_std: Optional[torch.Tensor], flat: torch.Tensor,
                      flat_std: Optional[torch.Tensor], *, input_is_variance: bool, through_mean: bool,
                      global_pixels: Optional[int] = None, reduce=None, flat_mean: Optional[torch.Tensor] = None):
    """In-place flat-field correction of ``value`` ((C,H,W) float64 merged mean or (F,C,H,W) float32 frames) and of
    its uncertainty (ct_flatfield_sums + ct_flatfield_apply).  ``through_mean``: the gradient also flows through the
    flat field's spatial mean (compute_hdr_image) or not (linearize).  ``reduce`` all-reduces the (C,2) sums across
    ranks holding row bands; ``global_pixels`` is then the pixel count of the whole image plane.  ``flat_mean`` (without
    ``through_mean`` only): the (C,) float32 ``flatfield_mean(flat)`` computed before; ct_flatfield_sums is then skipped."""
    _require_device(value, "value")
    flat = _flat_image(flat, value.device)
    c, h, w = flat.shape
    plane = h * w
    if tuple(value.shape[-3:]) != (c, h, w):
        raise ValueError(f"flat field {tuple(flat.shape)} does not match the image {tuple(value.shape)}")
    if not value.is_contiguous():
        raise ValueError("value must be contiguous")
    frames = 1 if value.ndim == 3 else value.shape[0]
    if through_mean and frames != 1:
        # sum value / (flat + eps) is one number per channel of ONE image; several frames have no common term
        raise ValueError("through_mean=True needs a single (C,H,W) image: the term through the flat field's mean is "
                         f"per image, got {frames} frames")
    is_f64 = value.dtype == torch.float64
    if value.dtype not in (torch.float64, torch.float32):
        raise TypeError("value must be float32 or float64")
    if flat_std is not None:
        flat_std = _flat_image(flat_std, value.device)
    dev = value.device
    if flat_mean is None:
        flat_mean, through = _flatfield_means(value if through_mean else None, is_f64, flat, global_pixels, reduce)
    else:
        if through_mean:
            raise ValueError("flat_mean is a constant of the run: not with through_mean=True")
        if flat_mean.dtype != torch.float32 or tuple(flat_mean.shape) != (c,) or flat_mean.device != dev:
            raise ValueError(f"flat_mean must be the float32 tensor of {c} channel means on {dev} (flatfield_mean)")
        flat_mean, through = flat_mean.contiguous(), None
    _call("ct_flatfield_apply", dev, _ptr(value), int(is_f64), frames, _ptr(var_or_std), int(input_is_variance), _ptr(flat),
          _ptr(flat_std), _ptr(flat_mean), _ptr(through), c, plane)
    return value, var_or_std


# ---- dark-field conditional blur -----------------------------------------------------------------------------------
def _dark_arguments(stack, dark, dark_std, halo):
    """What dark_field_blur and hdr_merge_dark_batch check of the dark field, its std and the halo rows of a contiguous
    (B,C,H,W) ``stack``: (dark, dark_std, halo) as the kernels read them."""
    b, c, h, w = stack.shape
    dev = stack.device
    dark = dark.to(device=dev, dtype=torch.float32).contiguous()
    if dark.ndim != 4 or dark.shape[0] not in (1, b) or tuple(dark.shape[1:]) != (c, h, w):
        raise ValueError(f"mask_map batch dimension must be 1 or {b}, got shape {tuple(dark.shape)}")
    if dark_std is not None:
        dark_std = dark_std.to(device=dev, dtype=torch.float32).contiguous()
        if dark_std.shape != dark.shape:
            raise ValueError("dark_std shape != dark shape")
        if dark.shape[0] == 1 and b > 1:
            raise NotImplementedError(
                "one shared dark field for several frames with its uncertainty: the reference sums the dark-field gradient "
                "over the frames before squaring, which the per-frame effective sigma of this kernel cannot express; pass "
                "one (matched) dark field per frame, as get_matching_artefact_images does")
    if halo is not None:
        halo = halo.to(device=dev, dtype=stack.dtype).contiguous()
        if tuple(halo.shape) != (b, c, 2, w):
            raise ValueError(f"halo must be (B, C, 2, W) = {(b, c, 2, w)}, got {tuple(halo.shape)}")
    return dark, dark_std, halo


def dark_field_blur(stack: torch.Tensor, dark: torch.Tensor, dark_std: Optional[torch.Tensor], *,
                    std: Optional[torch.Tensor] = None, std_mode: str = "none", std_value: float = 0.0,
                    max_code: Optional[float] = None, tile: Optional[TileGeometry] = None,
                    halo: Optional[torch.Tensor] = None, threshold: float = 0.05, alpha: float = 50.0):
    """ct_dark_field_blur: (xb float32 (B,C,H,W), sigma_eff float32 | None).  ``dark`` / ``dark_std`` are (1|B,C,H,W);
    ``halo`` (B,C,2,W) holds the global rows above / below a row band (see include/clair_hip.h)."""
    _check_stack(stack)
    b, c, h, w = stack.shape
    dev = stack.device
    std, std_mode = _std_arguments(std, std_mode, lambda sd: _explicit_std(sd, stack), refuse_unknown=False)
    stack = stack.contiguous()
    max_code = _default_max_code(stack, max_code)
    dark, dark_std, halo = _dark_arguments(stack, dark, dark_std, halo)
    geom = _geometry(stack, tile)
    xb = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
    sig = torch.empty_like(xb) if dark_std is not None else None
    _call("ct_dark_field_blur", dev, _ptr(stack), _DTYPE[stack.dtype], float(max_code or 1.0), b, ctypes.byref(geom), _ptr(halo),
          _ptr(std), _STD[std_mode], float(std_value), _ptr(dark), _ptr(dark_std), dark.shape[0], float(threshold), float(alpha),
          _ptr(xb), _ptr(sig))
    return xb, sig


def hdr_merge_dark_batch(stack: torch.Tensor, exposures: torch.Tensor, dark: torch.Tensor, dark_std: Optional[torch.Tensor], *,
                         lut: Optional[torch.Tensor] = None, interp: Optional[str] = "linear", gaussian_weight: bool = True,
                         std: Optional[torch.Tensor] = None, std_mode: str = "none", std_value: float = 0.0,
                         max_code: Optional[float] = None, state: Optional[MergeState] = None, finalize: bool = True,
                         tile: Optional[TileGeometry] = None, halo: Optional[torch.Tensor] = None,
                         mean_dtype: torch.dtype = torch.float64, reference_order: Optional[bool] = None,
                         threshold: float = 0.05, alpha: float = 50.0):
    """ct_hdr_merge_dark_batch: ``xb, sig = dark_field_blur(stack, dark, dark_std, ...)`` followed by
    ``hdr_merge_batch(xb, exposures, std=sig, ...)`` bit for bit, in one launch and without the two float32 stacks in
    between.  Returns (mean, std|None), planar (C,H,W), when ``finalize`` else None.

    ``stack`` (B,C,H,W) uint8 / uint16 codes (``max_code``) or float32 pixels; ``dark``, ``dark_std``, ``std``, ``std_mode``,
    ``std_value``, ``tile``, ``halo``, ``threshold``, ``alpha``: as ``dark_field_blur`` takes them (the uncertainty of the RAW
    image; without ``dark_std`` no uncertainty is propagated, as ``hdr_merge_batch(xb, ...)`` without one).  ``exposures``,
    ``lut``, ``interp``, ``gaussian_weight``, ``state``, ``finalize``, ``mean_dtype``: as in ``hdr_merge_batch``; the
    MergeState is the same, so fused and unfused batches may alternate on one.  ``reference_order``: False = the closed-form
    kernels for LOOKUP / CATMULL with uncertainties as well (CT_MERGE_CLOSED_FORM); None leaves those two modes, and True
    every mode, to the reference-order kernel, which this entry point does not have (NativeLibraryError: use
    ``dark_field_blur`` + ``hdr_merge_batch``)."""
    _check_stack(stack)
    b, c, h, w = stack.shape
    dev = stack.device
    if b < 1:
        raise ValueError("empty batch")
    std, std_mode = _std_arguments(std, std_mode, lambda sd: _explicit_std(sd, stack))
    stack = stack.contiguous()
    max_code = _default_max_code(stack, max_code)
    dark, dark_std, halo = _dark_arguments(stack, dark, dark_std, halo)
    exposure_dev = _exposures_to_device(exposures, b, dev)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _geometry(stack, tile)
    flags, mean_out, std_out = _merge_setup((c, h, w), dev, "planar", state, finalize, dark_std is not None, mean_dtype, reference_order,
                                            0, "batch")
    head = (_ptr(stack), _DTYPE[stack.dtype], float(max_code or 1.0), b, ctypes.byref(geom), _ptr(halo), _ptr(std), _STD[std_mode],
            float(std_value), _ptr(dark), _ptr(dark_std), dark.shape[0], float(threshold), float(alpha), _ptr(exposure_dev),
            ctypes.byref(icrf), _weight(gaussian_weight))
    return _launch_merge("ct_hdr_merge_dark_batch", dev, head, state, flags, 1, mean_out, std_out)


def _dark_argument_lists(stacks, darks, dark_stds, halos):
    """``_dark_arguments`` of every batch of a list front (``dark_stds`` / ``halos`` None: none at all): lists of the dark
    fields, their stds and the halo rows as the kernels read them, None standing for what a batch lacks; halo rows are given
    for every batch or for none."""
    checked = [_dark_arguments(t, darks[i], None if dark_stds is None else dark_stds[i], None if halos is None else halos[i])
               for i, t in enumerate(stacks)]
    darks, dark_stds, halos = ([v[j] for v in checked] for j in range(3))
    _all_or_none(halos, "halo rows")
    return darks, dark_stds, halos


def hdr_merge_dark_batches(stacks, exposures, darks, dark_stds, *, stds=None, std_mode: str = "none", std_value: float = 0.0,
                           max_code: Optional[float] = None, lut: Optional[torch.Tensor] = None, interp: Optional[str] = "linear",
                           gaussian_weight: bool = True, state: Optional[MergeState] = None, finalize: bool = True,
                           first: Optional[bool] = None, tile: Optional[TileGeometry] = None, halos=None,
                           mean_dtype: torch.dtype = torch.float64, reference_order: Optional[bool] = None,
                           require_one_launch: bool = False, threshold: float = 0.05, alpha: float = 50.0):
    """Several CONSECUTIVE dark-field batches of one merge in one call (ct_hdr_merge_dark_batches): the same result, bit for
    bit, as ``hdr_merge_dark_batch`` on each of them in turn with ``state`` carried along -- but one launch walks them all with
    the streaming state in registers in between (no state traffic between the batches).

    ``stacks``: list of (B_k,C,H,W) device stacks of one dtype, image shape and device, each as ``hdr_merge_dark_batch`` takes
    it; ``exposures``: list of (B_k) tensors (concatenated on the device when they are there already); ``darks``: list of
    (1|B_k,C,H,W) dark fields; ``dark_stds``: list of their stds, or None for none at all; ``stds``: list of explicit std
    tensors of the raw images or None; ``halos``: list of (B_k,C,2,W) halo rows of a row band or None.  At most
    MAX_MERGE_BATCHES.  ``first``: None = the state decides (a fresh MergeState, or none, starts the merge); True / False
    says so for a state filled elsewhere.  ``require_one_launch`` (tests): raise instead of falling back to one launch per
    batch (more exposure times than the LDS holds beside the LUT).  Everything else as in ``hdr_merge_dark_batch``.
    Returns (mean, std|None), planar (C,H,W), when ``finalize`` else None."""
    dark_stds, = _check_batch_list(stacks, (exposures, darks, dark_stds, stds, halos), "stacks / exposures / darks / dark_stds / stds / halos",
                                   _check_stack, all_or_none=[(2, "a dark std")], one_batch_elsewhere=first is None)
    k = len(stacks)
    if k == 1 and first is None:
        return hdr_merge_dark_batch(stacks[0], exposures[0], darks[0], None if dark_stds is None else dark_stds[0], lut=lut,
                                    interp=interp, gaussian_weight=gaussian_weight, std=None if stds is None else stds[0],
                                    std_mode=std_mode, std_value=std_value, max_code=max_code, state=state, finalize=finalize,
                                    tile=tile, halo=None if halos is None else halos[0], mean_dtype=mean_dtype,
                                    reference_order=reference_order, threshold=threshold, alpha=alpha)
    s0 = stacks[0]
    _, c, h, w = s0.shape
    dev = s0.device
    stds, std_mode = _std_arguments(stds, std_mode, lambda sds: [_explicit_std(sd, t) for sd, t in zip(sds, stacks)])
    stacks = [t.contiguous() for t in stacks]
    max_code = _default_max_code(s0, max_code)
    darks, dark_stds, halos = _dark_argument_lists(stacks, darks, dark_stds, halos)
    sizes = [int(t.shape[0]) for t in stacks]
    exposure_dev = _exposure_list_to_device(exposures, sizes, dev)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _geometry(stacks[0], tile)
    flags, mean_out, std_out = _merge_setup((c, h, w), dev, "planar", state, finalize, dark_stds[0] is not None, mean_dtype, reference_order,
                                            nv.MERGE_REQUIRE_ONE_LAUNCH if require_one_launch else 0, "call", first)
    head = (_pointers(stacks), (ctypes.c_int32 * k)(*sizes), k, _DTYPE[s0.dtype], float(max_code or 1.0), ctypes.byref(geom),
            _pointers(halos), _pointers(stds), _STD[std_mode], float(std_value), _pointers(darks), _pointers(dark_stds),
            (ctypes.c_int32 * k)(*[int(t.shape[0]) for t in darks]), float(threshold), float(alpha), _ptr(exposure_dev),
            ctypes.byref(icrf), _weight(gaussian_weight))
    # (probe_one_launch would be the same here: ct_hdr_merge_dark_batches answers a walk without state arrays and one refused by
    # MERGE_REQUIRE_ONE_LAUNCH alike, with CT_ERR_UNSUPPORTED)
    return _launch_merge("ct_hdr_merge_dark_batches", dev, head, state, flags, k, mean_out, std_out, retry_with_state=True)


MAX_LINEARIZE_DARK_FRAMES =nv.LINEARIZE_DARK_MAX_FRAMES  # frames one ct_linearize_dark launch takes (longer stacks: several)


def _dark_per_frame(frames, darks, dark_stds):
    """The dark fields and their stds of ``linearize_dark_frames`` as two lists of F contiguous float32 (C,H,W) device
    tensors: each frame is a batch of one, so every entry passes ``_dark_arguments`` with B = 1."""
    f = frames.shape[0]
    if dark_stds is None:
        raise ValueError("linearize_dark_frames propagates the dark field's uncertainty: dark_stds is required")
    lists = []
    for name, v in (("darks", darks), ("dark_stds", dark_stds)):
        if isinstance(v, torch.Tensor):
            if v.ndim != 4 or v.shape[0] != f:
                raise ValueError(f"{name} must be (F, C, H, W) with F = {f} or a sequence of F tensors, got shape {tuple(v.shape)}")
            v = [v[k:k + 1] for k in range(f)]
        elif len(v) != f:
            raise ValueError(f"{len(v)} {name} for {f} frames")
        lists.append(v)
    out, seen = ([], []), {}
    for d, s in zip(*lists):
        key = (id(d), id(s))
        if key not in seen:  # a dark field shared between frames is checked (and made contiguous) once
            for name, t in (("darks", d), ("dark_stds", s)):
                if not isinstance(t, torch.Tensor):
                    raise TypeError(f"{name} must hold torch.Tensors, got {type(t)}")
            d4, s4 = (t if t.ndim == 4 else t.unsqueeze(0) for t in (d, s))
            seen[key] = _dark_arguments(frames[:1], d4, s4, None)[:2]
        out[0].append(seen[key][0])
        out[1].append(seen[key][1])
    return out


def _linearize_dark(entry, planar, head, geom, middle, darks, dark_stds, threshold, alpha, lut, interp, out, tail=()):
    """What linearize_dark_frames and linearize_dark_ingest_frames (_data) share behind their own checks: the per-frame dark
    fields, the ICRF, the (lin, std) outputs and ``entry``(*head, geometry, *middle, dark pointers, threshold, alpha, ICRF, outputs,
    *tail).  ``planar``: the frames, or a view without memory that has their planar shape (F,C,H,W) and device."""
    shape, dev = tuple(planar.shape), planar.device
    dark_list, dark_std_list = _dark_per_frame(planar, darks, dark_stds)
    icrf, lut_keep = _icrf_struct(lut, interp, shape[1])
    lin, std_out = _lin_std_out(out, shape, dev, True, lin_required=True)
    _call(entry, dev, *head, ctypes.byref(geom), *middle, _pointers(dark_list), _pointers(dark_std_list), float(threshold),
          float(alpha), ctypes.byref(icrf), _ptr(lin), _ptr(std_out), *tail)
    return lin, std_out


def linearize_dark_frames(frames: torch.Tensor, darks, dark_stds, lut: Optional[torch.Tensor], interp: Optional[str] = "linear", *,
                          std: Optional[torch.Tensor] = None, std_mode: str = "none", std_value: float = 0.0,
                          max_code: Optional[float] = None, threshold: float = 0.05, alpha: float = 50.0, out=None):
    """ct_linearize_dark on (F,C,H,W) frames -> (lin, std) float32 (F,C,H,W): for every frame k, bit for bit
    ``xb, sig = dark_field_blur(frames[k:k+1], darks[k], dark_stds[k], ...)`` followed by
    ``linearize_frames(xb, lut, interp, std=sig)``, in one launch per MAX_LINEARIZE_DARK_FRAMES frames and without the two
    float32 stacks in between.

    ``frames``: planar uint8 / uint16 codes (``max_code``) or float32 pixels; a view whose frames are contiguous but further
    apart than C*H*W is read in place unless ``std`` is given.  ``darks`` / ``dark_stds``: sequences of F device tensors
    (C,H,W) or (1,C,H,W), the dark field matched to each frame and its std (repeats allowed), or one (F,C,H,W) tensor each.
    ``std`` / ``std_mode`` / ``std_value``: the uncertainty of the RAW image as ``dark_field_blur`` takes it.  ``out`` =
    (lin, std): as in ``linearize_frames``.  LOOKUP has no gradient path to the image (RuntimeError, as ``linearize_frames``
    with uncertainties)."""
    _check_stack(frames, "frames")
    f, c, h, w = frames.shape
    if f < 1:
        raise ValueError("no frames")
    std, std_mode = _std_arguments(std, std_mode, lambda sd: _explicit_std(sd, frames, "frames"))
    if std is not None:  # (explicit uncertainties are dense: so are the frames then, the kernel strides both alike)
        frames = frames.contiguous()
    max_code = _default_max_code(frames, max_code)
    geom = _geometry(frames, None)
    if f == 1:  # (the stride of a single frame means nothing)
        geom.image_stride = c * h * w
    return _linearize_dark("ct_linearize_dark", frames, (_ptr(frames), _DTYPE[frames.dtype], float(max_code or 1.0), f), geom,
                           (_ptr(std), _STD[std_mode], float(std_value)), darks, dark_stds, threshold, alpha, lut, interp, out)


# ---- strided downscale of raw codes (StridedDownscale folded in front of the code-domain kernels) -----------------
def downscaled_shape(shape, step: int, layout: str = "nchw"):
    """Shape of ``x[..., ::step, ::step]`` taken on the spatial axes of a 4-D stack in ``layout``."""
    b, d1, d2, d3 = shape
    if layout == "nchw":
        return b, d1, -(-d2 // step), -(-d3 // step)
    return b, -(-d1 // step), -(-d2 // step), d3


def strided_downscale(stack: torch.Tensor, step: int, layout: str = "nchw", out: Optional[torch.Tensor] = None):
    """ct_strided_downscale: every ``step``-th row and column of a uint8 / uint16 / float32 device stack, compacted in
    its own dtype and layout -- (B,C,H,W) -> (B,C,ceil(H/step),ceil(W/step)) for "nchw", (B,H,W,C) ->
    (B,ceil(H/step),ceil(W/step),C) for "nhwc" / "nhwc_bgr" (the channel order is untouched) -- bit-identical to
    ``x[..., ::step, ::step]`` on the planar view.  ``out``: a contiguous caller tensor of exactly that shape and dtype
    to write into.  ``step == 1`` returns the stack itself (copied into ``out`` when given)."""
    _check_ingest_stack(stack, layout, for_ingest=False)
    if isinstance(step, bool) or not isinstance(step, int) or step < 1:
        raise ValueError(f"step must be an int >= 1, got {step!r}")
    shape = downscaled_shape(stack.shape, step, layout)
    if step == 1 and out is None:
        return stack
    out = _checked_out(out, shape, stack.dtype, stack.device)
    if step == 1:
        alias = torch.int16 if stack.dtype == torch.uint16 else stack.dtype  # torch has no uint16 copy kernel
        out.view(alias).copy_(stack.view(alias))
        return out
    stack = stack.contiguous()
    if out.numel() == 0:
        return out
    if layout == "nchw":
        planes, h, w, pixel_elems = stack.shape[0] * stack.shape[1], stack.shape[2], stack.shape[3], 1
    else:
        planes, h, w, pixel_elems = stack.shape[0], stack.shape[1], stack.shape[2], stack.shape[3]
    _call("ct_strided_downscale", stack.device, _ptr(stack), _ptr(out), stack.element_size(), planes, h, w, pixel_elems, step)
    return out


# ---- export of planar results in OpenCV order (the device half of save_image) ------------------------------------
_EXPORT_DTYPES = (torch.float32, torch.float64)


def export_shape(shape):
    """Shape ``export_cv`` gives for an input of ``shape``: (H,W) -> (H,W), (C,H,W) -> (H,W,C), (F,C,H,W) -> (F,H,W,C)."""
    if len(shape) == 2:
        return tuple(shape)
    if len(shape) == 3:
        return shape[1], shape[2], shape[0]
    if len(shape) == 4:
        return shape[0], shape[2], shape[3], shape[1]
    raise ValueError(f"x must be (H, W), (C, H, W) or (F, C, H, W), got shape {tuple(shape)}")


def export_cv(x: torch.Tensor, dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None):
    """ct_export_cv: the array the reference's ``save_image`` hands to ``cv.imwrite`` (data_io.py:228-234), made on the
    device.  ``x``: a contiguous float32 / float64 device tensor (H,W), (C,H,W) or (F,C,H,W); the result is (H,W) (a cast
    only), (H,W,C) or (F,H,W,C) in ``dtype`` (float32, float64, None = that of ``x``), with the channels reversed iff
    C == 3 (RGB -> BGR).  Casts are numpy's ``astype``; the same dtype is a bit copy.  ``out``: a contiguous caller tensor
    of exactly that shape and dtype to write into."""
    _require_device(x, "x")
    if x.dtype not in _EXPORT_DTYPES:
        raise TypeError(f"x dtype {x.dtype} unsupported (float32 or float64)")
    if dtype is None:
        dtype = x.dtype
    if dtype not in _EXPORT_DTYPES:
        raise TypeError(f"dtype {dtype} unsupported (torch.float32, torch.float64 or None)")
    shape = export_shape(tuple(x.shape))
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")
    out = _checked_out(out, shape, dtype, x.device)
    if out.numel() == 0:
        return out
    if x.ndim == 2:
        images, channels, plane = 1, 1, x.numel()
    else:
        channels, plane = x.shape[-3], x.shape[-2] * x.shape[-1]
        images = x.shape[0] if x.ndim == 4 else 1
    _call("ct_export_cv", x.device, _ptr(x), int(x.dtype == torch.float64), _ptr(out), int(dtype == torch.float64), images,
          channels, plane, int(channels == 3))
    return out


# ---- a recognised gpu_transforms chain in one pass (CastTo / Normalize / ClampAlongDims) --------------------------
def ingest_shape(shape, layout: str = "nchw"):
    """Shape of the planar (B,C,H,W) stack ``ingest_transform`` gives for a 4-D stack of ``shape`` in ``layout``."""
    b, d1, d2, d3 = shape
    return (b, d1, d2, d3) if layout == "nchw" else (b, d3, d1, d2)


def _number(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{what} must be an int or a float, got {v!r}")
    return float(v)


def _ingest_stages(stages, channels: int, data: bool = False, limit: int = nv.INGEST_MAX_STAGES):
    """The ct_ingest_stage array of ``stages``: ("affine", sub, div, mul, add) | ("clamp", [(lo, hi)] * (1 or C)) and,
    with ``data``, at most one ("affine_data", mul, add) whose sub / div the device supplies."""
    stages = list(stages)
    if len(stages) > limit:
        raise ValueError(f"at most {limit} stages, got {len(stages)}")
    kinds = ("affine", "clamp", "affine_data") if data else ("affine", "clamp")
    arr = (nv.IngestStage * max(len(stages), 1))()
    n_data = 0
    for k, st in enumerate(stages):
        if not isinstance(st, (tuple, list)) or not st or st[0] not in kinds:
            extra = " or ('affine_data', mul, add)" if data else ""
            raise ValueError(f"stage {k}: expected ('affine', sub, div, mul, add) or ('clamp', pairs){extra}, got {st!r}")
        if st[0] == "affine_data":
            n_data += 1
            if len(st) != 3 or n_data > 1:
                raise ValueError(f"stage {k}: one ('affine_data', mul, add) stage with two constants at most")
            arr[k].kind, arr[k].mul, arr[k].add = nv.INGEST_AFFINE_DATA, _number(st[1], f"stage {k}"), _number(st[2], f"stage {k}")
            continue
        if st[0] == "affine":
            if len(st) != 5:
                raise ValueError(f"stage {k}: ('affine', sub, div, mul, add) takes four constants")
            sub, div, mul, add = (_number(v, f"stage {k}") for v in st[1:])
            arr[k].kind, arr[k].sub, arr[k].div, arr[k].mul, arr[k].add = nv.INGEST_AFFINE, sub, div, mul, add
            if arr[k].div == 0.0:
                raise ValueError("Normalization range is zero (min == max); cannot normalize.")
            continue
        if len(st) != 2 or not isinstance(st[1], (tuple, list)):
            raise ValueError(f"stage {k}: ('clamp', pairs) takes a list of (lo, hi) pairs")
        pairs = list(st[1])
        if len(pairs) not in (1, channels) or (len(pairs) > 1 and channels > nv.INGEST_MAX_CHANNELS):
            raise ValueError(f"stage {k}: expected 1 or {channels} min/max pairs (at most {nv.INGEST_MAX_CHANNELS} "
                             f"channels with one pair each), got {len(pairs)}")
        if len(pairs) == 1:
            pairs = pairs * nv.INGEST_MAX_CHANNELS
        pairs += [pairs[-1]] * (nv.INGEST_MAX_CHANNELS - len(pairs))  # unused entries
        arr[k].kind = nv.INGEST_CLAMP
        for c, pair in enumerate(pairs):
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError(f"stage {k}: a clamp pair is (lo, hi), got {pair!r}")
            arr[k].lo[c], arr[k].hi[c] = _number(pair[0], f"stage {k}"), _number(pair[1], f"stage {k}")
    return arr, len(stages)


def _check_ingest_stack(stack: torch.Tensor, layout: str, for_ingest: bool = True, codes_only: Optional[str] = None):
    """A stack the ingest fronts take.  ``codes_only``: the TypeError text of a front that takes no float32 pixels."""
    _check_4d(stack, "stack", "4-dimensional")
    if layout not in _LAYOUT:
        raise ValueError(f"unknown layout {layout!r} (nchw, nhwc, nhwc_bgr)")
    if not for_ingest:  # strided_downscale: pixels of any size, and it makes the stack contiguous itself
        return
    if layout != "nchw" and stack.shape[3] != 3:
        raise ValueError(f"layout {layout!r} takes (B, H, W, 3) frames, got shape {tuple(stack.shape)}")
    if not stack.is_contiguous():
        raise ValueError("stack must be contiguous")
    if codes_only is not None and stack.dtype == torch.float32:
        raise TypeError(codes_only)


def _check_consts(consts, device):
    _require_device(consts, "consts")
    if consts.dtype != torch.float32 or tuple(consts.shape) != (4,) or consts.device != device or not consts.is_contiguous():
        raise ValueError(f"consts must be the 4-element float32 tensor of ingest_extrema on {device}")


def _check_frame_consts(consts, n_frames: int, device):
    _require_device(consts, "consts")
    if consts.dtype != torch.float32:
        raise TypeError(f"consts must be float32, got {consts.dtype}")
    if tuple(consts.shape) != (n_frames, 4) or consts.device != device or not consts.is_contiguous():
        raise ValueError(f"consts must be the contiguous ({n_frames}, 4) float32 tensor of ingest_extrema_frames on {device}, "
                         f"got shape {tuple(consts.shape)}")


def ingest_transform(stack: torch.Tensor, stages, layout: str = "nchw", out: Optional[torch.Tensor] = None,
                     consts: Optional[torch.Tensor] = None):
    """ct_ingest_transform: the chain CastTo(float32), Normalize(max, min, range), ClampAlongDims evaluated in one pass
    with the reference's float32 arithmetic (every operation rounded on its own, a correctly rounded division).
    ``stack``: a contiguous uint8 / uint16 / float32 device stack, (B,C,H,W) for "nchw" or (B,H,W,3) for "nhwc" /
    "nhwc_bgr"; the result is the planar float32 (B,C,H,W) stack (RGB planes for "nhwc_bgr").  ``stages``: up to 4 of
    ("affine", sub, div, mul, add) -- ((x - sub) / div) * mul + add, the constants rounded to float32 -- and
    ("clamp", pairs) with one (lo, hi) pair, or one per channel of the result (C <= 4).  ``out``: a contiguous float32
    caller tensor of exactly the result's shape to write into.
    ``consts``: the tensor ``ingest_extrema`` returned; then (ct_ingest_transform_data) one stage may be
    ("affine_data", mul, add) -- a data-dependent Normalize, whose sub and div the kernel reads from ``consts[0:2]`` when
    it runs.  No zero-range check happens here (see ``ingest_transform_data``)."""
    _check_ingest_stack(stack, layout)
    shape = ingest_shape(tuple(stack.shape), layout)
    arr, n_stages = _ingest_stages(stages, shape[1], data=consts is not None)
    if consts is not None:
        _check_consts(consts, stack.device)
    out = _checked_out(out, shape, torch.float32, stack.device, "float32")
    if out.numel() == 0:
        return out
    args = (_ptr(stack), _DTYPE[stack.dtype], _LAYOUT[layout], shape[0], shape[1], shape[2] * shape[3], arr, n_stages, _ptr(out))
    if consts is None:
        _call("ct_ingest_transform", stack.device, *args)
    else:
        _call("ct_ingest_transform_data", stack.device, *args, _ptr(consts))
    return out


# ---- such a chain and the linearization in one pass ----------------------------------------------------------------------
def _linearize_ingest(strided, frames, step, stages, lut, interp, std, std_mode, std_value, want_std, tile, layout, out, consts,
                      flat=None):
    """The two fronts below: ct_linearize_ingest_strided with ``strided``, else ct_linearize_ingest / ct_linearize_ingest_data;
    with ``flat`` their _flat forms (``linearize_frames_flat``; the images have the shape of a frame of the OUTPUTS)."""
    _check_ingest_stack(frames, layout)
    if strided and (isinstance(step, bool) or not isinstance(step, int) or step < 1):
        raise ValueError(f"step must be an int >= 1, got {step!r}")
    src_shape = ingest_shape(tuple(frames.shape), layout)
    f, c = src_shape[:2]
    shape = downscaled_shape(src_shape, step) if strided else src_shape
    dev = frames.device
    arr, n_stages = _ingest_stages(stages, c, data=consts is not None)
    if consts is not None:
        _check_frame_consts(consts, f, dev)
    std, std_mode = _std_arguments(std, std_mode, lambda sd: _planar_std(sd, shape, dev, "outputs"))
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _ingest_geometry(src_shape, tile, layout)
    lin, std_out = _lin_std_out(out, shape, dev, want_std, lin_required=True)
    if flat is not None:
        flat = _flat_arguments(flat, shape, dev, want_std)
    if frames.numel() == 0:
        return lin, std_out
    head = (_ptr(frames), _DTYPE[frames.dtype], f, ctypes.byref(geom))
    tail = (arr, n_stages, _ptr(std), _STD[std_mode], float(std_value), ctypes.byref(icrf), _ptr(lin), _ptr(std_out))
    if flat is not None:
        step_arg = (min(step, 0x7fffffff),) if strided else ()
        _call("ct_linearize_ingest_strided_flat" if strided else "ct_linearize_ingest_flat", dev, *head, *step_arg, *tail, _ptr(consts),
              *map(_ptr, flat))
    elif strided:
        _call("ct_linearize_ingest_strided", dev, *head, min(step, 0x7fffffff), *tail, _ptr(consts))
    elif consts is None:
        _call("ct_linearize_ingest", dev, *head, *tail)
    else:
        _call("ct_linearize_ingest_data", dev, *head, *tail, _ptr(consts))
    return lin, std_out


def linearize_ingest_frames(frames: torch.Tensor, stages, lut: Optional[torch.Tensor], interp: Optional[str] = "linear", *,
                            std: Optional[torch.Tensor] = None, std_mode: str = "none", std_value: float = 0.0,
                            want_std: bool = True, tile: Optional[TileGeometry] = None, layout: str = "nchw", out=None,
                            consts: Optional[torch.Tensor] = None):
    """ct_linearize_ingest: ``linearize_frames(ingest_transform(frames, stages, layout), lut, interp, ...)`` bit for bit,
    in one launch and without the float32 stack in between -> (lin float32, std float32 | None), planar (F,C,H,W).
    ``frames``: a contiguous uint8 / uint16 / float32 device stack, (F,C,H,W) for "nchw" or (F,H,W,3) for "nhwc" /
    "nhwc_bgr" (the order of the source: a folded CvToTorch).  ``stages``: as ``ingest_transform`` takes them, without
    ("affine_data", ...).  ``std``: explicit uncertainties, float32 and PLANAR (F,C,H,W) like the outputs whatever the
    layout of the frames (gpu_transforms never touch the uncertainty images).  ``tile``: the frames are a row band of a
    taller image, as in ``linearize_frames``.  ``out`` = (lin, std | None): caller-owned contiguous float32 (F,C,H,W)
    device buffers to write into.
    ``consts``: the (F, 4) tensor ``ingest_extrema_frames`` returned; then (ct_linearize_ingest_data) one stage may be
    ("affine_data", mul, add) -- a data-dependent Normalize with PER-FRAME bounds, whose sub and div for frame f the kernel
    reads from ``consts[f, 0:2]`` when it runs: ``linearize_frames(ingest_transform(frames[f:f+1], stages, layout,
    consts=consts[f]), ...)`` bit for bit.  No zero-range check happens here (``consts[f, 1] == 0``)."""
    return _linearize_ingest(False, frames, 1, stages, lut, interp, std, std_mode, std_value, want_std, tile, layout, out, consts)


def linearize_ingest_frames_flat(frames: torch.Tensor, stages, lut: Optional[torch.Tensor], interp: Optional[str] = "linear", *, flat,
                                 std: Optional[torch.Tensor] = None, std_mode: str = "none", std_value: float = 0.0,
                                 want_std: bool = True, tile: Optional[TileGeometry] = None, layout: str = "nchw", out=None,
                                 consts: Optional[torch.Tensor] = None):
    """ct_linearize_ingest_flat: ``linearize_ingest_frames`` (with ``consts``: its data-dependent form) and the flat-field
    correction of ``linearize_frames_flat`` in the same launch, bit for bit.  ``flat`` = (flat, flat_std | None, flat_mean) as
    there; everything else as ``linearize_ingest_frames``."""
    return _linearize_ingest(False, frames, 1, stages, lut, interp, std, std_mode, std_value, want_std, tile, layout, out, consts,
                             flat)


def linearize_ingest_frames_strided(frames: torch.Tensor, step: int, stages, lut: Optional[torch.Tensor],
                                    interp: Optional[str] = "linear", *, std: Optional[torch.Tensor] = None,
                                    std_mode: str = "none", std_value: float = 0.0, want_std: bool = True,
                                    tile: Optional[TileGeometry] = None, layout: str = "nchw", out=None,
                                    consts: Optional[torch.Tensor] = None):
    """ct_linearize_ingest_strided: ``linearize_ingest_frames(strided_downscale(frames, step, layout), stages, ...)`` bit for
    bit, in one launch and without the compacted frames in between -> (lin float32, std float32 | None), planar
    (F,C,ho,wo) with ho = ceil(H/step), wo = ceil(W/step).  ``frames``, ``stages``, ``layout``, ``consts`` as
    ``linearize_ingest_frames`` takes them; ``consts`` are those of the frames as given (``ingest_extrema_frames`` on the
    full frames: a data-dependent Normalize in FRONT of the downscale).  ``std``: explicit uncertainties, float32 and
    planar (F,C,ho,wo) -- already of the output shape, because gpu_transforms are applied to the value images only.
    ``out`` = (lin, std | None): contiguous float32 (F,C,ho,wo) device buffers.  ``tile``: with ``step == 1`` only (a row
    band behind a downscale is refused: the phase of the band is not carried)."""
    return _linearize_ingest(True, frames, step, stages, lut, interp, std, std_mode, std_value, want_std, tile, layout, out, consts)


def linearize_ingest_frames_strided_flat(frames: torch.Tensor, step: int, stages, lut: Optional[torch.Tensor],
                                         interp: Optional[str] = "linear", *, flat, std: Optional[torch.Tensor] = None,
                                         std_mode: str = "none", std_value: float = 0.0, want_std: bool = True,
                                         tile: Optional[TileGeometry] = None, layout: str = "nchw", out=None,
                                         consts: Optional[torch.Tensor] = None):
    """ct_linearize_ingest_strided_flat: ``linearize_ingest_frames_strided`` and the flat-field correction of
    ``linearize_frames_flat`` in the same launch, bit for bit.  ``flat`` = (flat, flat_std | None, flat_mean) as there, the
    images float32 (C,ho,wo) like a frame of the outputs; everything else as ``linearize_ingest_frames_strided``."""
    return _linearize_ingest(True, frames, step, stages, lut, interp, std, std_mode, std_value, want_std, tile, layout, out, consts,
                             flat)


# ---- such a chain, the dark-field blur and the linearization in one pass ------------------------------------------------------
def linearize_dark_ingest_frames(frames: torch.Tensor, stages, darks, dark_stds, lut: Optional[torch.Tensor],
                                 interp: Optional[str] = "linear", *, std: Optional[torch.Tensor] = None, std_mode: str = "none",
                                 std_value: float = 0.0, layout: str = "nchw", out=None, threshold: float = 0.05,
                                 alpha: float = 50.0):
    """ct_linearize_dark_ingest on raw frames -> (lin, std) float32, planar (F,C,H,W): for every frame k, bit for bit
    ``x = ingest_transform(frames[k:k+1], stages, layout)``, ``xb, sig = dark_field_blur(x, darks[k], dark_stds[k], ...)`` and
    ``linearize_frames(xb, lut, interp, std=sig)``, in one launch per MAX_LINEARIZE_DARK_FRAMES frames and without the three
    float32 stacks in between.

    ``frames``, ``stages``, ``layout``: as ``linearize_ingest_frames`` takes them (a contiguous uint8 / uint16 / float32 device
    stack, (F,C,H,W) for "nchw" or (F,H,W,3) for "nhwc" / "nhwc_bgr"; constant stages only).  ``darks`` / ``dark_stds``: as
    ``linearize_dark_frames`` takes them, planar (C,H,W) in the order of the result's planes.  ``std`` / ``std_mode`` /
    ``std_value``: the uncertainty of the image BEHIND the chain as ``dark_field_blur`` takes it on ``x``; ``std`` is float32
    and PLANAR (F,C,H,W) whatever the layout of the frames.  ``out`` = (lin, std): contiguous float32 (F,C,H,W) device
    buffers to write into.  LOOKUP has no gradient path to the image (RuntimeError, as ``linearize_frames`` with
    uncertainties)."""
    return _linearize_dark_ingest(frames, stages, darks, dark_stds, lut, interp, std, std_mode, std_value, layout, out, threshold,
                                  alpha, None)


def linearize_dark_ingest_frames_data(frames: torch.Tensor, stages, darks, dark_stds, lut: Optional[torch.Tensor],
                                      interp: Optional[str] = "linear", *, consts: torch.Tensor, std: Optional[torch.Tensor] = None,
                                      std_mode: str = "none", std_value: float = 0.0, layout: str = "nchw", out=None,
                                      threshold: float = 0.05, alpha: float = 50.0):
    """ct_linearize_dark_ingest_data: ``linearize_dark_ingest_frames`` whose chain may hold one ("affine_data", mul, add) stage -- a
    data-dependent Normalize with PER-FRAME bounds, whose sub and div for frame k the kernel reads from ``consts[k, 0:2]`` when
    it runs.  ``consts``: the (F, 4) tensor ``ingest_extrema_frames`` returned for these frames.  For every frame k, bit for bit
    ``x = ingest_transform(frames[k:k+1], stages, layout, consts=consts[k])``, ``xb, sig = dark_field_blur(x, darks[k],
    dark_stds[k], ...)`` and ``linearize_frames(xb, lut, interp, std=sig)``, in one launch per MAX_LINEARIZE_DARK_FRAMES frames.
    No zero-range check happens here (``consts[k, 1] == 0``).  Everything else as ``linearize_dark_ingest_frames``."""
    if consts is None:
        raise TypeError("linearize_dark_ingest_frames_data takes the (F, 4) consts of ingest_extrema_frames "
                        "(constant chains: linearize_dark_ingest_frames)")
    return _linearize_dark_ingest(frames, stages, darks, dark_stds, lut, interp, std, std_mode, std_value, layout, out, threshold,
                                  alpha, consts)


def _linearize_dark_ingest(frames, stages, darks, dark_stds, lut, interp, std, std_mode, std_value, layout, out, threshold, alpha,
                           consts):
    """The two fronts above: ct_linearize_dark_ingest, or with ``consts`` ct_linearize_dark_ingest_data."""
    _check_ingest_stack(frames, layout)
    shape = ingest_shape(tuple(frames.shape), layout)
    f, c = shape[:2]
    dev = frames.device
    if f < 1:
        raise ValueError("no frames")
    arr, n_stages = _ingest_stages(stages, c, data=consts is not None)
    if consts is not None:
        _check_frame_consts(consts, f, dev)
    std, std_mode = _std_arguments(std, std_mode, lambda sd: _planar_std(sd, shape, dev, "outputs"))
    # the dark fields are checked against the planar shape (of the stack only shape and device are read: a view without memory)
    planar = frames if layout == "nchw" else frames.new_empty((1, 1, 1, 1)).expand(shape)
    entry, tail = ("ct_linearize_dark_ingest", ()) if consts is None else ("ct_linearize_dark_ingest_data", (_ptr(consts),))
    return _linearize_dark(entry, planar, (_ptr(frames), _DTYPE[frames.dtype], f),
                           _ingest_geometry(shape, None, layout), (arr, n_stages, _ptr(std), _STD[std_mode], float(std_value)),
                           darks, dark_stds, threshold, alpha, lut, interp, out, tail)


# ---- such a chain and one batch of the HDR merge in one pass ---------------------------------------------------------------
def hdr_merge_ingest_batch(frames: torch.Tensor, stages, exposures: torch.Tensor, *, lut: Optional[torch.Tensor] = None,
                           interp: Optional[str] = "linear", gaussian_weight: bool = True, std: Optional[torch.Tensor] = None,
                           std_mode: str = "none", std_value: float = 0.0, state: Optional[MergeState] = None,
                           finalize: bool = True, tile: Optional[TileGeometry] = None, mean_dtype: torch.dtype = torch.float64,
                           layout: str = "nchw", reference_order: Optional[bool] = None, consts: Optional[torch.Tensor] = None):
    """ct_hdr_merge_ingest_batch: ``hdr_merge_batch(ingest_transform(frames, stages, layout, consts=consts), exposures, ...)``
    bit for bit, in one launch and without the float32 stack in between.  Returns (mean, std|None), planar (C,H,W), when
    ``finalize`` else None.

    ``frames``: a contiguous uint8 / uint16 device stack, (B,C,H,W) for "nchw" or (B,H,W,3) for "nhwc" / "nhwc_bgr" (the
    order of the source: a folded CvToTorch).  ``stages``: as ``ingest_transform`` takes them; with ``consts`` (the tensor
    ``ingest_extrema`` returned) one of them may be ("affine_data", mul, add).  ``std``: explicit uncertainties, float32 and
    PLANAR (B,C,H,W) like the state whatever the layout of the frames.  ``exposures``, ``lut``, ``interp``,
    ``gaussian_weight``, ``std_mode``, ``std_value``, ``state``, ``finalize``, ``tile``, ``mean_dtype``: as in
    ``hdr_merge_batch``.  ``reference_order``: False = the closed-form kernels for LOOKUP / CATMULL with uncertainties as
    well (CT_MERGE_CLOSED_FORM); None leaves those two modes, and True every mode, to the reference-order kernel, which
    this entry point does not have (NativeLibraryError: use ``ingest_transform`` + ``hdr_merge_batch``)."""
    _check_ingest_stack(frames, layout, codes_only="hdr_merge_ingest_batch takes uint8 / uint16 codes (float32 pixels: "
                                                   "ingest_transform + hdr_merge_batch)")
    shape = ingest_shape(tuple(frames.shape), layout)
    b, c, h, w = shape
    dev = frames.device
    if b < 1:
        raise ValueError("empty batch")
    arr, n_stages = _ingest_stages(stages, c, data=consts is not None)
    if consts is not None:
        _check_consts(consts, dev)
    std, std_mode = _std_arguments(std, std_mode, lambda sd: _planar_std(sd, shape, dev, "state"))
    exposure_dev = _exposures_to_device(exposures, b, dev)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _ingest_geometry(shape, tile, layout)
    # (state and outputs are planar whatever the order of the source)
    flags, mean_out, std_out = _merge_setup((c, h, w), dev, "planar", state, finalize, std_mode != "none", mean_dtype, reference_order,
                                            0, "batch")
    head = (_ptr(frames), _DTYPE[frames.dtype], b, ctypes.byref(geom), arr, n_stages, _ptr(consts), _ptr(std), _STD[std_mode],
            float(std_value), _ptr(exposure_dev), ctypes.byref(icrf), _weight(gaussian_weight))
    return _launch_merge("ct_hdr_merge_ingest_batch", dev, head, state, flags, 1, mean_out, std_out)


def hdr_merge_ingest_batches(frames_list, stages, exposures_list, *, lut: Optional[torch.Tensor] = None,
                             interp: Optional[str] = "linear", gaussian_weight: bool = True, stds=None, std_mode: str = "none",
                             std_value: float = 0.0, state: Optional[MergeState] = None, finalize: bool = True,
                             tile: Optional[TileGeometry] = None, mean_dtype: torch.dtype = torch.float64, layout: str = "nchw",
                             reference_order: Optional[bool] = None, consts=None, require_one_launch: bool = False):
    """Several CONSECUTIVE batches of one merge behind one chain in one call (ct_hdr_merge_ingest_batches): the same result,
    bit for bit, as ``hdr_merge_ingest_batch`` on each of them in turn with ``state`` carried along -- but one launch walks
    them all with the streaming state in registers in between (no state traffic between the batches).

    ``frames_list``: list of (B_k,C,H,W) / (B_k,H,W,3) uint8 / uint16 device stacks of one dtype, image shape and device,
    each as ``hdr_merge_ingest_batch`` takes it; ``exposures_list``: list of (B_k) tensors; ``stds``: list of explicit
    planar std tensors or None; ``consts``: list of the tensors ``ingest_extrema`` returned for each batch (then one stage may
    be ("affine_data", mul, add)), or None; a list may hold None for a batch without constants.  At most MAX_MERGE_BATCHES.
    ``require_one_launch`` (tests): raise instead of falling back to one launch per batch (batches with and without
    constants mixed; more exposure times than the LDS holds).  Everything else as in ``hdr_merge_ingest_batch``.
    Returns (mean, std|None), planar (C,H,W), when ``finalize`` else None."""
    def check_stack(t):
        _check_ingest_stack(t, layout, codes_only="hdr_merge_ingest_batches takes uint8 / uint16 codes (float32 pixels: "
                                                  "ingest_transform + hdr_merge_batches)")

    _check_batch_list(frames_list, (exposures_list, stds, consts), "frames / exposures / stds / consts", check_stack, one_batch_elsewhere=True)
    k = len(frames_list)
    if k == 1:
        return hdr_merge_ingest_batch(frames_list[0], stages, exposures_list[0], lut=lut, interp=interp,
                                      gaussian_weight=gaussian_weight, std=None if stds is None else stds[0], std_mode=std_mode,
                                      std_value=std_value, state=state, finalize=finalize, tile=tile, mean_dtype=mean_dtype,
                                      layout=layout, reference_order=reference_order, consts=None if consts is None else consts[0])
    f0 = frames_list[0]
    dev = f0.device
    shape0 = ingest_shape(tuple(f0.shape), layout)
    _, c, h, w = shape0
    has_consts = consts is not None and any(t is not None for t in consts)
    arr, n_stages = _ingest_stages(stages, c, data=has_consts)
    if consts is not None:
        for t in consts:
            if t is not None:
                _check_consts(t, dev)
    stds, std_mode = _std_arguments(stds, std_mode, lambda sds: [_planar_std(sd, ingest_shape(tuple(t.shape), layout), dev, "state")
                                                                 for sd, t in zip(sds, frames_list)])
    sizes = [int(t.shape[0]) for t in frames_list]
    exposure_dev = _exposure_list_to_device(exposures_list, sizes, dev)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _ingest_geometry(shape0, tile, layout)
    flags, mean_out, std_out = _merge_setup((c, h, w), dev, "planar", state, finalize, std_mode != "none", mean_dtype, reference_order,
                                            nv.MERGE_REQUIRE_ONE_LAUNCH if require_one_launch else 0, "call")
    head = (_pointers(frames_list), (ctypes.c_int32 * k)(*sizes), k, _DTYPE[f0.dtype], ctypes.byref(geom), arr, n_stages, _pointers(consts),
            _pointers(stds), _STD[std_mode], float(std_value), _ptr(exposure_dev), ctypes.byref(icrf), _weight(gaussian_weight))
    # (probe_one_launch: without it ct_hdr_merge_ingest_batches answers a walk without state arrays with CT_ERR_INVALID_ARGUMENT)
    return _launch_merge("ct_hdr_merge_ingest_batches", dev, head, state, flags, k, mean_out, std_out, retry_with_state=True,
                         probe_one_launch=True)


# ---- a StridedDownscale, such a chain and several batches of the HDR merge in one pass over the raw frames -----------------------
def hdr_merge_ingest_batches_strided(frames_list, step: int, stages, exposures_list, *, lut: Optional[torch.Tensor] = None,
                                     interp: Optional[str] = "linear", gaussian_weight: bool = True, stds=None,
                                     std_mode: str = "none", std_value: float = 0.0, state: Optional[MergeState] = None,
                                     finalize: bool = True, tile: Optional[TileGeometry] = None,
                                     mean_dtype: torch.dtype = torch.float64, layout: str = "nchw",
                                     reference_order: Optional[bool] = None, consts=None, require_one_launch: bool = False):
    """ct_hdr_merge_ingest_strided_batches: ``hdr_merge_ingest_batches([strided_downscale(f, step, layout) for f in
    frames_list], stages, exposures_list, ...)`` bit for bit, in one launch over the raw full-size frames and without the
    compacted copies in between.  Returns (mean, std|None), planar (C,ho,wo) with ho = ceil(H/step), wo = ceil(W/step), when
    ``finalize`` else None.

    ``frames_list``, ``stages``, ``exposures_list``, ``layout`` and every keyword as ``hdr_merge_ingest_batches`` takes them.
    ``consts`` are those of the frames as given (``ingest_extrema`` on the full batch: a data-dependent Normalize in FRONT of
    the downscale).  ``stds``: explicit uncertainties, float32 and planar (B_k,C,ho,wo) -- already of the downscaled shape,
    because gpu_transforms are applied to the value images only.  ``state``: a MergeState of shape (C,ho,wo).  ``step == 1``
    is ``hdr_merge_ingest_batches`` itself.  ``tile``: with ``step == 1`` only (a row band behind a downscale is refused: the
    phase of the band is not carried).  One kernel family serves one batch and sixteen."""
    if isinstance(step, bool) or not isinstance(step, int) or step < 1:
        raise ValueError(f"step must be an int >= 1, got {step!r}")
    if step == 1:
        return hdr_merge_ingest_batches(frames_list, stages, exposures_list, lut=lut, interp=interp, gaussian_weight=gaussian_weight,
                                        stds=stds, std_mode=std_mode, std_value=std_value, state=state, finalize=finalize, tile=tile,
                                        mean_dtype=mean_dtype, layout=layout, reference_order=reference_order, consts=consts,
                                        require_one_launch=require_one_launch)
    if tile is not None:
        raise ValueError("tile= cannot be combined with step > 1: which rows of a band a downscale selects depends on "
                         "row_offset % step, a phase that is not carried")

    def check_stack(t):
        _check_ingest_stack(t, layout, codes_only="hdr_merge_ingest_batches_strided takes uint8 / uint16 codes (float32 pixels: "
                                                  "strided_downscale + ingest_transform + hdr_merge_batches)")

    _check_batch_list(frames_list, (exposures_list, stds, consts), "frames / exposures / stds / consts", check_stack)
    k = len(frames_list)
    f0 = frames_list[0]
    dev = f0.device
    shape0 = ingest_shape(tuple(f0.shape), layout)
    _, c, ho, wo = downscaled_shape(shape0, step)
    has_consts = consts is not None and any(t is not None for t in consts)
    arr, n_stages = _ingest_stages(stages, c, data=has_consts)
    if consts is not None:
        for t in consts:
            if t is not None:
                _check_consts(t, dev)
    stds, std_mode = _std_arguments(stds, std_mode, lambda sds: [_planar_std(sd, (int(t.shape[0]), c, ho, wo), dev, "state")
                                                                 for sd, t in zip(sds, frames_list)])
    sizes = [int(t.shape[0]) for t in frames_list]
    exposure_dev = _exposure_list_to_device(exposures_list, sizes, dev)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _ingest_geometry(shape0, None, layout)  # of the SOURCE frames
    flags, mean_out, std_out = _merge_setup((c, ho, wo), dev, "planar", state, finalize, std_mode != "none", mean_dtype, reference_order,
                                            nv.MERGE_REQUIRE_ONE_LAUNCH if require_one_launch else 0, "call")
    head = (_pointers(frames_list), (ctypes.c_int32 * k)(*sizes), k, _DTYPE[f0.dtype], ctypes.byref(geom), min(step, 0x7fffffff), arr,
            n_stages, _pointers(consts), _pointers(stds), _STD[std_mode], float(std_value), _ptr(exposure_dev), ctypes.byref(icrf),
            _weight(gaussian_weight))
    return _launch_merge("ct_hdr_merge_ingest_strided_batches", dev, head, state, flags, k, mean_out, std_out, retry_with_state=True,
                         probe_one_launch=True)


def hdr_merge_ingest_batch_strided(frames: torch.Tensor, step: int, stages, exposures: torch.Tensor, *,
                                   std: Optional[torch.Tensor] = None, consts: Optional[torch.Tensor] = None, **kw):
    """One batch of ``hdr_merge_ingest_batches_strided``: ``hdr_merge_ingest_batch(strided_downscale(frames, step, layout),
    stages, exposures, ...)`` bit for bit.  ``std`` (planar (B,C,ho,wo)) and ``consts`` are the batch's own; every other keyword
    as ``hdr_merge_ingest_batch`` takes it."""
    return hdr_merge_ingest_batches_strided([frames], step, stages, [exposures], stds=None if std is None else [std],
                                            consts=None if consts is None else [consts], **kw)


# ---- such a chain, the dark-field blur and several batches of the HDR merge in one pass ---------------------------------------
def hdr_merge_dark_ingest_batches(frames_list, stages, exposures_list, darks, dark_stds, *, consts=None, stds=None,
                                  std_mode: str = "none", std_value: float = 0.0, lut: Optional[torch.Tensor] = None,
                                  interp: Optional[str] = "linear", gaussian_weight: bool = True,
                                  state: Optional[MergeState] = None, finalize: bool = True, first: Optional[bool] = None,
                                  tile: Optional[TileGeometry] = None, halos=None, layout: str = "nchw",
                                  mean_dtype: torch.dtype = torch.float64, reference_order: Optional[bool] = None,
                                  require_one_launch: bool = False, threshold: float = 0.05, alpha: float = 50.0):
    """1 to MAX_MERGE_BATCHES CONSECUTIVE dark-field batches of one merge behind one chain in one call, on the RAW frames
    (ct_hdr_merge_dark_ingest_batches): for every batch k, bit for bit, ``x = ingest_transform(frames_list[k], stages, layout,
    consts=consts[k])`` followed by ``hdr_merge_dark_batch(x, exposures_list[k], darks[k], dark_stds[k], ...)`` on the same
    ``state`` -- but one launch walks all batches with the streaming state in registers in between, and the float32 stack of
    a batch never exists.  One batch is a list of one (the same kernel).

    ``frames_list``: list of contiguous uint8 / uint16 / float32 device stacks of one dtype, image shape and device,
    (B_k,C,H,W) for "nchw" or (B_k,H,W,3) for "nhwc" / "nhwc_bgr" (the order of the source: a folded CvToTorch).  ``stages``:
    as ``ingest_transform`` takes them; with ``consts`` (list of the tensors ``ingest_extrema`` returned, one per batch) one
    of them may be ("affine_data", mul, add).  ``darks`` / ``dark_stds``: lists of (1|B_k,C,H,W) dark fields and their stds
    (``dark_stds`` None: no uncertainty is propagated), planar in the order of the result's planes.  ``stds`` / ``std_mode`` /
    ``std_value``: the uncertainty of the image BEHIND the chain as ``dark_field_blur`` takes it on ``x``; explicit ones are
    float32 and PLANAR (B_k,C,H,W) whatever the layout of the frames.  ``halos``: for a row band (``tile``; planar frames only)
    the list of (B_k,C,2,W) RAW rows of the frames' dtype above / below the band.  ``first``: None = the state decides; True /
    False says so for a state filled elsewhere.  ``require_one_launch`` (tests): raise (ValueError) instead of falling back to
    one launch per batch (more exposure times than the LDS holds beside the LUT).  ``reference_order``, ``exposures_list``,
    ``lut``, ``interp``, ``gaussian_weight``, ``state``, ``finalize``, ``mean_dtype``, ``threshold``, ``alpha``: as in
    ``hdr_merge_dark_batches``.  Returns (mean, std|None), planar (C,H,W), when ``finalize`` else None."""
    dark_stds, consts = _check_batch_list(frames_list, (exposures_list, darks, dark_stds, stds, halos, consts),
                                          "frames / exposures / darks / dark_stds / stds / halos / consts",
                                          lambda t: _check_ingest_stack(t, layout), all_or_none=[(2, "a dark std"), (5, "constants")])
    k = len(frames_list)
    f0 = frames_list[0]
    dev = f0.device
    shapes = [ingest_shape(tuple(t.shape), layout) for t in frames_list]
    _, c, h, w = shapes[0]
    if layout != "nchw" and tile is not None and (tile.row_offset != 0 or tile.h_global != h):
        raise ValueError("a row band (tile=) needs planar frames: no halo is built for interleaved ones")
    arr, n_stages = _ingest_stages(stages, c, data=consts is not None)
    if consts is not None:
        for t in consts:
            _check_consts(t, dev)
    stds, std_mode = _std_arguments(stds, std_mode,
                                    lambda sds: [_planar_std(sd, shape, dev, "state") for sd, shape in zip(sds, shapes)])
    # the refusals the dark ops share, against the planar shape (of the stack only shape, dtype and device are read: a view
    # without memory stands for interleaved frames)
    planar = [t if layout == "nchw" else t.new_empty((1, 1, 1, 1)).expand(shape) for t, shape in zip(frames_list, shapes)]
    darks, dark_stds, halos = _dark_argument_lists(planar, darks, dark_stds, halos)
    sizes = [int(s[0]) for s in shapes]
    exposure_dev = _exposure_list_to_device(exposures_list, sizes, dev)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _ingest_geometry(shapes[0], tile, layout)
    flags, mean_out, std_out = _merge_setup((c, h, w), dev, "planar", state, finalize, dark_stds[0] is not None, mean_dtype, reference_order,
                                            nv.MERGE_REQUIRE_ONE_LAUNCH if require_one_launch else 0, "call", first)
    head = (_pointers(frames_list), (ctypes.c_int32 * k)(*sizes), k, _DTYPE[f0.dtype], ctypes.byref(geom), arr, n_stages, _pointers(consts),
            _pointers(halos), _pointers(stds), _STD[std_mode], float(std_value), _pointers(darks), _pointers(dark_stds),
            (ctypes.c_int32 * k)(*[int(t.shape[0]) for t in darks]), float(threshold), float(alpha), _ptr(exposure_dev),
            ctypes.byref(icrf), _weight(gaussian_weight))
    # (probe_one_launch would differ here: with MERGE_REQUIRE_ONE_LAUNCH this entry point answers CT_ERR_TOO_LARGE.  retry_one_batch
    # True would only cost a state and a second call: one batch always runs as one launch, so CT_ERR_UNSUPPORTED for it is a
    # refusal of the route, which a state does not lift)
    return _launch_merge("ct_hdr_merge_dark_ingest_batches", dev, head, state, flags, k, mean_out, std_out, retry_with_state=True,
                         retry_one_batch=False)


# ---- a data-dependent Normalize (max_val / min_val None) in such a chain ------------------------------------------------
ZERO_RANGE = "Normalization range is zero (min == max); cannot normalize."  # general_functions.py:378


def _extrema_call(front, stack, prefix_stages, layout, min_val, max_val):
    """What ``ingest_extrema`` and ``ingest_extrema_frames`` (``front``: which of them, for the message) check and build
    alike: the planar shape and the arguments of the entry points up to ``fixed_max``."""
    _check_ingest_stack(stack, layout)
    if min_val is not None and max_val is not None:
        raise ValueError("min_val and max_val are both given: nothing depends on the data (use ingest_transform)")
    shape = ingest_shape(tuple(stack.shape), layout)
    arr, n_prefix = _ingest_stages(prefix_stages, shape[1], limit=nv.EXTREMA_MAX_PREFIX)
    from_data = (nv.EXTREMA_MIN if min_val is None else 0) | (nv.EXTREMA_MAX if max_val is None else 0)
    fixed_min = 0.0 if min_val is None else _number(min_val, "min_val")
    fixed_max = 0.0 if max_val is None else _number(max_val, "max_val")
    if stack.numel() == 0:
        raise RuntimeError(f"{front}: the stack is empty (the extrema of an empty tensor are undefined)")
    return shape, (_ptr(stack), _DTYPE[stack.dtype], _LAYOUT[layout], shape[0], shape[1], shape[2] * shape[3], arr, n_prefix,
                   from_data, fixed_min, fixed_max)


def ingest_extrema(stack: torch.Tensor, prefix_stages=(), layout: str = "nchw", min_val=None, max_val=None):
    """ct_ingest_extrema: the constants of a data-dependent Normalize (reference general_functions.py:373-376), as a
    4-element float32 device tensor ``consts`` = [sub, div, data min, data max].  The extrema are those of the whole
    ``stack`` (as ``ingest_transform`` takes it) after the up to 3 constant ``prefix_stages`` that stand in front of the
    Normalize; a NaN anywhere makes both NaN.  ``min_val`` / ``max_val``: None takes that bound from the data (at least
    one must be None), a number fixes it: sub = min, div = fl32(max - min) in float32, as torch forms them.  One
    streaming pass plus a fold, no synchronisation: ``div == 0``, where the reference raises, is for the caller to
    check (``ingest_transform_data``).  An empty stack raises, as torch's ``x.min()`` does."""
    _, args = _extrema_call("ingest_extrema", stack, prefix_stages, layout, min_val, max_val)
    ws_bytes = int(nv.load().ct_ingest_extrema_workspace())
    ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=stack.device)
    consts = torch.empty((4,), dtype=torch.float32, device=stack.device)
    _call("ct_ingest_extrema", stack.device, *args, _ptr(ws), ws_bytes, _ptr(consts))
    return consts


def ingest_extrema_frames_workspace(n_frames: int, device) -> torch.Tensor:
    """A float32 device tensor that serves ``ingest_extrema_frames`` as ``workspace`` for every stack of 1 to ``n_frames``
    frames (a ring slot's last group is shorter than the others): the largest ct_ingest_extrema_frames_workspace(k) over
    k <= n_frames, since that size is not monotone in k."""
    lib = nv.load()
    ws_bytes = max(int(lib.ct_ingest_extrema_frames_workspace(k)) for k in range(1, max(int(n_frames), 1) + 1))
    return torch.empty((max(ws_bytes, 16) // 4,), dtype=torch.float32, device=device)


def ingest_extrema_frames(frames: torch.Tensor, prefix_stages=(), layout: str = "nchw", min_val=None, max_val=None, *,
                          out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """ct_ingest_extrema_frames: ``ingest_extrema`` of every frame of ``frames`` on its own -- the constants of a
    data-dependent Normalize that sees one frame per batch -- as an (F, 4) float32 device tensor whose row f is bit for bit
    ``ingest_extrema(frames[f:f+1], prefix_stages, layout, min_val, max_val)``: [sub, div, data min, data max], both extrema
    NaN when that frame holds a NaN.  Two launches whatever F is, no synchronisation; ``consts[f, 1] == 0``, where the
    reference raises, is for the caller to check.  ``out``: a contiguous (F, 4) float32 device tensor to write into;
    ``workspace``: a float32 device tensor of at least the library's workspace size (``ingest_extrema_frames_workspace``);
    without them both are allocated here.  An empty stack raises, as torch's ``x.min()`` does."""
    shape, args = _extrema_call("ingest_extrema_frames", frames, prefix_stages, layout, min_val, max_val)
    dev = frames.device
    ws_bytes = int(nv.load().ct_ingest_extrema_frames_workspace(shape[0]))
    if ws_bytes == 0:
        raise ValueError(f"ingest_extrema_frames: {shape[0]} frames are more than one call takes (65535)")
    if workspace is None:
        workspace = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=dev)
    else:
        _require_device(workspace, "workspace")
        if (workspace.dtype != torch.float32 or workspace.device != dev or not workspace.is_contiguous()
                or workspace.numel() * 4 < ws_bytes):
            raise ValueError(f"workspace must be a contiguous float32 tensor of at least {ws_bytes} bytes on {dev}")
    if out is None:
        out = torch.empty((shape[0], 4), dtype=torch.float32, device=dev)
    else:
        _check_frame_consts(out, shape[0], dev)
    _call("ct_ingest_extrema_frames", dev, *args, _ptr(workspace), workspace.numel() * 4, _ptr(out))
    return out


def data_stage_prefix(stages):
    """The constant stages in front of the ("affine_data", mul, add) entry of ``stages`` (which must hold one)."""
    stages = list(stages)
    at = [k for k, st in enumerate(stages) if isinstance(st, (tuple, list)) and st and st[0] == "affine_data"]
    if len(at) != 1:
        raise ValueError(f"stages must hold exactly one ('affine_data', mul, add) stage, got {len(at)}")
    return stages[:at[0]]


def check_ingest_consts(consts: torch.Tensor):
    """Read the 16 bytes of ``ingest_extrema``'s constants back (ONE synchronisation) and raise the reference's
    ValueError when the range is zero (general_functions.py:377-378); a NaN range passes, as it does there."""
    if float(consts.cpu()[1]) == 0.0:
        raise ValueError(ZERO_RANGE)


def ingest_transform_data(stack: torch.Tensor, stages, layout: str = "nchw", min_val=None, max_val=None, check: bool = True,
                          out: Optional[torch.Tensor] = None):
    """A chain with one data-dependent Normalize: ``ingest_extrema`` over the constant stages in front of the
    ("affine_data", mul, add) entry of ``stages``, then ``ingest_transform`` with those constants -- three launches on
    the current stream.  ``check=True``: returns the planar float32 stack after reading the constants back (one
    synchronisation per batch, which the reference's own ``if denominator == 0`` costs as well) and raising its
    ValueError for a zero range.  ``check=False``: returns ``(out, consts)`` without synchronising -- the sequence can be
    captured in a graph; ``consts[1] == 0`` then means every value of ``out`` is NaN or infinite."""
    consts = ingest_extrema(stack, data_stage_prefix(stages), layout, min_val, max_val)
    out = ingest_transform(stack, stages, layout, out=out, consts=consts)
    if not check:
        return out, consts
    check_ingest_consts(consts)
    return out


# ---- streaming video statistics -----------------------------------------------------------------------------------
MAX_STATS_BATCHES = 16  # batches one ct_video_stats_batches call takes (the kernel's argument block holds 16 pointers)


def _stats_batch_list(frames_list, consts=None):
    """The batches of one ``video_stats_*_batches`` call: a non-empty list of at most MAX_STATS_BATCHES tensors."""
    if not isinstance(frames_list, (list, tuple)) or len(frames_list) == 0 or (consts is not None and len(consts) != len(frames_list)):
        raise ValueError("frames / consts must be non-empty lists of equal length")
    if len(frames_list) > MAX_STATS_BATCHES:
        raise ValueError(f"at most {MAX_STATS_BATCHES} batches per call")
    return list(frames_list)


def _same_batches(frames_list):
    f0 = frames_list[0]
    for t in frames_list:
        if t.dtype != f0.dtype or t.shape[1:] != f0.shape[1:] or t.device != f0.device:
            raise ValueError("all batches of one call must share dtype, image shape and device")


def _batch_arrays(frames_list, consts=None):
    """The HOST arrays of a ``*_batches`` entry point: frame pointers, batch sizes, and the constants' pointers or None."""
    size_arr = (ctypes.c_int32 * len(frames_list))(*[int(t.shape[0]) for t in frames_list])
    return _pointers(frames_list), size_arr, _pointers(consts)


def _video_stats(frames_list, mean_state, m2_state, frames_before, lut, interp, max_code, tile, layout, flags=None):
    """``video_stats_batch`` (``flags`` None: one batch, ct_video_stats_batch) and ``video_stats_batches``."""
    for t in frames_list:
        _check_stack(t, "frames")
    _same_batches(frames_list)
    f0 = frames_list[0]
    c, h, w = _chw(f0, layout)
    dev = f0.device
    frames_list = [t.contiguous() for t in frames_list]
    max_code = _default_max_code(f0, max_code)
    _check_stats_state(mean_state, m2_state, (c, h, w))
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _geometry(frames_list[0], tile, layout)
    tail = (ctypes.byref(geom), ctypes.byref(icrf), float(frames_before), _ptr(mean_state), _ptr(m2_state))
    if flags is None:
        _call("ct_video_stats_batch", dev, _ptr(frames_list[0]), _DTYPE[f0.dtype], float(max_code or 1.0), f0.shape[0], *tail)
    else:
        geom.image_stride = c * h * w  # contiguous batches: one stride for all (that of a 1-frame batch is arbitrary)
        ptr_arr, size_arr, _ = _batch_arrays(frames_list)
        _call("ct_video_stats_batches", dev, ptr_arr, size_arr, len(frames_list), _DTYPE[f0.dtype], float(max_code or 1.0), *tail,
              flags)


def video_stats_batch(frames: torch.Tensor, mean_state: torch.Tensor, m2_state: torch.Tensor, frames_before: int, *,
                      lut: Optional[torch.Tensor] = None, interp: Optional[str] = None,
                      max_code: Optional[float] = None, tile: Optional[TileGeometry] = None, layout: str = "nchw"):
    """ct_video_stats_batch: merge one batch of frames into the running (mean, m2) float32 state in place.
    ``layout`` "nhwc" / "nhwc_bgr": frames are (F,H,W,C) as OpenCV decodes them; the state stays planar (C,H,W)."""
    _video_stats([frames], mean_state, m2_state, frames_before, lut, interp, max_code, tile, layout)


def video_stats_batches(frames_list, mean_state: torch.Tensor, m2_state: torch.Tensor, frames_before: int, *,
                        lut: Optional[torch.Tensor] = None, interp: Optional[str] = None, max_code: Optional[float] = None,
                        tile: Optional[TileGeometry] = None, layout: str = "nchw", require_one_launch: bool = False):
    """Several CONSECUTIVE batches of one video in one call (ct_video_stats_batches): the same state, bit for bit, as
    ``video_stats_batch`` on each of them in turn with the frame count carried along -- but where every batch has at most 32
    frames one launch walks them all with (mean, m2) in registers in between (no state traffic between the batches).

    ``frames_list``: list of at most MAX_STATS_BATCHES device stacks of one dtype, image shape and device, each as
    ``video_stats_batch`` takes it (separate allocations are fine; an empty batch is skipped); ``frames_before``: the frames
    merged before the first of them.  ``require_one_launch`` (tests): raise instead of falling back to one launch per batch
    (a batch of more than 32 frames).  Everything else as in ``video_stats_batch``."""
    _video_stats(_stats_batch_list(frames_list), mean_state, m2_state, frames_before, lut, interp, max_code, tile, layout,
                 nv.STATS_REQUIRE_ONE_LAUNCH if require_one_launch else 0)


# ---- a gpu_transforms chain and the streaming video statistics in one pass ------------------------------------------------
def _video_stats_ingest(front, frames_list, stages, mean_state, m2_state, frames_before, lut, interp, tile, layout, consts, flags=None):
    """``video_stats_ingest_batch`` (``flags`` None: one batch, ct_video_stats_ingest_batch) and ``video_stats_ingest_batches``;
    ``consts``: a list like ``frames_list``, or None."""
    for t in frames_list:
        _check_ingest_stack(t, layout, codes_only=f"{front} takes uint8 / uint16 codes (float32 pixels: "
                                                  f"ingest_transform + {front.replace('_ingest', '')})")
    _same_batches(frames_list)
    f0 = frames_list[0]
    shape = ingest_shape(tuple(f0.shape), layout)
    _, c, h, w = shape
    dev = f0.device
    has_consts = consts is not None and any(t is not None for t in consts)
    arr, n_stages = _ingest_stages(stages, c, data=has_consts)
    if consts is not None:
        for t in consts:
            if t is not None:
                _check_consts(t, dev)
    _check_stats_state(mean_state, m2_state, (c, h, w), dev)
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _ingest_geometry(shape, tile, layout)
    tail = (ctypes.byref(icrf), float(frames_before), _ptr(mean_state), _ptr(m2_state))
    if flags is None:
        _call("ct_video_stats_ingest_batch", dev, _ptr(f0), _DTYPE[f0.dtype], shape[0], ctypes.byref(geom), arr, n_stages,
              _ptr(consts[0]) if consts is not None else None, *tail)
    else:
        ptr_arr, size_arr, consts_arr = _batch_arrays(frames_list, consts)
        _call("ct_video_stats_ingest_batches", dev, ptr_arr, size_arr, len(frames_list), _DTYPE[f0.dtype], ctypes.byref(geom), arr,
              n_stages, consts_arr, *tail, flags)


def video_stats_ingest_batch(frames: torch.Tensor, stages, mean_state: torch.Tensor, m2_state: torch.Tensor, frames_before: int, *,
                             lut: Optional[torch.Tensor] = None, interp: Optional[str] = None,
                             tile: Optional[TileGeometry] = None, layout: str = "nchw", consts: Optional[torch.Tensor] = None):
    """ct_video_stats_ingest_batch: ``video_stats_batch(ingest_transform(frames, stages, layout, consts=consts), ...)`` bit for
    bit, in one launch and without the float32 stack in between; the running (mean, m2) float32 state is updated in place.

    ``frames``: a contiguous uint8 / uint16 device stack, (B,C,H,W) for "nchw" or (B,H,W,3) for "nhwc" / "nhwc_bgr" (the
    order of the source: a folded CvToTorch).  ``stages``: as ``ingest_transform`` takes them; with ``consts`` (the tensor
    ``ingest_extrema`` returned) one of them may be ("affine_data", mul, add).  ``mean_state``, ``m2_state``: contiguous
    float32 (C,H,W), planar whatever the layout of the frames (``ingest_shape(frames.shape, layout)[1:]``).
    ``frames_before``, ``lut``, ``interp``, ``tile``: as in ``video_stats_batch``."""
    _video_stats_ingest("video_stats_ingest_batch", [frames], stages, mean_state, m2_state, frames_before, lut, interp, tile, layout,
                        None if consts is None else [consts])


def video_stats_ingest_batches(frames_list, stages, mean_state: torch.Tensor, m2_state: torch.Tensor, frames_before: int, *,
                               lut: Optional[torch.Tensor] = None, interp: Optional[str] = None,
                               tile: Optional[TileGeometry] = None, layout: str = "nchw", consts=None,
                               require_one_launch: bool = False):
    """Several CONSECUTIVE batches of one video behind one chain in one call (ct_video_stats_ingest_batches): the same state,
    bit for bit, as ``video_stats_ingest_batch`` on each of them in turn with the frame count carried along -- but where every
    batch has at most 32 frames one launch walks them all with (mean, m2) in registers in between.

    ``frames_list``: list of at most MAX_STATS_BATCHES uint8 / uint16 device stacks of one dtype, image shape and device, each
    as ``video_stats_ingest_batch`` takes it (separate allocations are fine; an empty batch is skipped); ``consts``: list of
    the tensors ``ingest_extrema`` returned for each batch -- every batch has its own data-dependent Normalize constants --
    or None; a list may hold None for a batch without constants.  ``require_one_launch`` (tests): raise instead of falling
    back to one launch per batch (a batch of more than 32 frames; batches with and without constants mixed).  Everything
    else as in ``video_stats_ingest_batch``."""
    _video_stats_ingest("video_stats_ingest_batches", _stats_batch_list(frames_list, consts), stages, mean_state, m2_state,
                        frames_before, lut, interp, tile, layout, consts,
                        nv.STATS_REQUIRE_ONE_LAUNCH if require_one_launch else 0)


# ---- a gpu_transforms chain and the exposure-pair residual in one pass -------------------------------------------------------
_PAIR_INGEST_CODES = ("pair_residual_ingest takes uint8 / uint16 codes (float32 pixels: ingest_transform + "
                      "pair_residual_sums / pair_residual_lut_grad)")


def _pair_ingest_setup(frames, stages, pairs, consts, layout, std, std_mode, lut, interp, tile):
    """What the two pair ingest fronts share: the checks of ``video_stats_ingest_batch`` -> (channels, std_mode, the entry
    points' arguments up to the ICRF, the tensors made here that those arguments point to).  The front keeps that last tuple
    in a local until it returns: the std as the kernel reads it may be a copy (``_planar_std``), like the ICRF's table."""
    _check_ingest_stack(frames, layout, codes_only=_PAIR_INGEST_CODES)
    shape = ingest_shape(tuple(frames.shape), layout)
    n, c = shape[0], shape[1]
    dev = frames.device
    if n != pairs.n_images:
        raise ValueError(f"pair list was built for {pairs.n_images} images, stack has {n}")
    arr, n_stages = _ingest_stages(stages, c, data=consts is not None)
    if consts is not None:
        _check_consts(consts, dev)
    std, std_mode = _std_arguments(std, std_mode, lambda sd: _planar_std(sd, shape, dev, "ingested stack"))
    icrf, lut_keep = _icrf_struct(lut, interp, c)
    geom = _ingest_geometry(shape, tile, layout)
    head = (_ptr(frames), _DTYPE[frames.dtype], arr, n_stages, _ptr(consts), n, ctypes.byref(geom), _ptr(std), ctypes.byref(icrf))
    return c, std_mode, head, (std, lut_keep)


def pair_residual_ingest_sums(frames: torch.Tensor, stages, pairs: PairList, *, lut: Optional[torch.Tensor], interp: Optional[str],
                              lower: float, upper: float, use_relative: bool, use_unc_weight: bool,
                              consts: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, std_mode: str = "none",
                              std_value: float = 0.0, level: int = 1, tile: Optional[TileGeometry] = None,
                              center: Optional[torch.Tensor] = None, layout: str = "nchw"):
    """ct_pair_residual_ingest_fwd: ``pair_residual_sums(ingest_transform(frames, stages, layout, consts=consts), pairs, ...)``
    in one launch and without the float32 stack in between -> (P, C, 5) float64 sums; every staged sample has the bits of that
    route, the sums differ by the order of the float64 additions alone.

    ``frames``: a contiguous uint8 / uint16 device stack, (N,C,H,W) for "nchw" or (N,H,W,3) for "nhwc" / "nhwc_bgr" (the
    order of the source: a folded CvToTorch).  ``stages``: as ``ingest_transform`` takes them; with ``consts`` (the tensor
    ``ingest_extrema`` returned) one of them may be ("affine_data", mul, add).  ``std``: explicit uncertainties, float32 and
    PLANAR (N,C,H,W) whatever the layout of the frames.  Everything else as in ``pair_residual_sums``."""
    c, std_mode, head, keep = _pair_ingest_setup(frames, stages, pairs, consts, layout, std, std_mode, lut, interp, tile)
    prm = _pair_params(lower, upper, use_relative, use_unc_weight, std_mode, std_value)
    return _pair_sums("ct_pair_residual_ingest_fwd", frames.device, head, pairs, c, prm, level, center)


def pair_residual_ingest_lut_grad(frames: torch.Tensor, stages, pairs: PairList, coef: torch.Tensor, *, lut: torch.Tensor,
                                  interp: str, lower: float, upper: float, use_relative: bool,
                                  consts: Optional[torch.Tensor] = None, tile: Optional[TileGeometry] = None,
                                  use_unc_weight: bool = False, std: Optional[torch.Tensor] = None, std_mode: str = "none",
                                  std_value: float = 0.0, smean: Optional[torch.Tensor] = None, lane_kernel: bool = True,
                                  layout: str = "nchw"):
    """ct_pair_residual_ingest_bwd: ``pair_residual_lut_grad(ingest_transform(frames, stages, layout, consts=consts), pairs,
    coef, ...)`` in one launch sequence and without the float32 stack -> (C, L) float64 LUT gradient.  ``frames``, ``stages``,
    ``consts`` and ``std`` as in ``pair_residual_ingest_sums``, everything else as in ``pair_residual_lut_grad``."""
    if not use_unc_weight:
        std, std_mode = None, "none"
    c, std_mode, head, keep = _pair_ingest_setup(frames, stages, pairs, consts, layout, std, std_mode, lut, interp, tile)
    prm = _pair_params(lower, upper, use_relative, use_unc_weight, std_mode, std_value,
                       pair_band=pairs.band if lane_kernel else 0)
    return _pair_lut_grad("ct_pair_residual_ingest_bwd", frames.device, head, pairs, c, prm, std_mode != "none", coef, smean,
                          lut.shape[1])
