"""The reference's transform classes (clair_torch/common/transforms.py:68-216; ``to_config`` / ``from_config`` and the
YAML registry are not part of this build).

The entry points stage a batch by ONE plan (``plan_staging``, executed by inference/_staging.py::stage_images); the first
route of this table that applies is taken:

= ============= ==================================================================== =====================================
# route         the list, behind an optional leading ``CvToTorch`` on raw frames       what runs
= ============= ==================================================================== =====================================
1 "code"        route 2's pair with ONE ``StridedDownscale`` before, between or        ct_strided_downscale compacts the raw
                behind it; 4-D batches only                                            codes, the kernels fold the pair
2 "code"        ``CastTo(float32), Normalize(max, 0)`` on uint8 / uint16 codes         nothing: the kernels' load stage
                (``isinstance``: subclasses count; any rank, any strides)              folds the pair
3 "ingest"      ``CastTo(float32)``, one to four ``Normalize(max, min, range)`` /      ct_ingest_transform: one pass, bit for
                ``ClampAlongDims`` (one pair, or one per channel) stages, at most      bit these classes on the CPU; the
                one ``StridedDownscale`` (``type(t) is``; 4-D contiguous batches)      float32 kernel variant takes the result
4 "ingest_data" route 3's grammar with exactly ONE data-dependent ``Normalize``        ct_ingest_extrema, then
                (``max_val`` and / or ``min_val`` None); batch on a CUDA device        ct_ingest_transform_data
5 "torch"       everything else: two data-dependent ``Normalize``s, other casts,       these classes' ``__call__`` (PyTorch
                clamps over a non-channel dim, more than four stages, other            ops on the device), then the float32
                classes, non-contiguous or non-4-D batches off the code pair           kernel variant
= ============= ==================================================================== =====================================

compute_hdr_image does not execute routes 3 and 4 on uint8 / uint16 frames (``stage_images(defer_ingest=True)``): the chain
is evaluated inside the merge kernel, up to 16 batches per ct_hdr_merge_ingest_batches launch and no float32 copy of a batch --
unless there is a dark-field dataset, the mode is one of the reference-order kernel's (LOOKUP / CATMULL with uncertainties
by default) or ``fused_ingest=False``; route 4 still runs ct_ingest_extrema first and checks its constants.

linearize_dataset_generator streams routes 2 and 3 (no ``StridedDownscale``, no dark field) through its copy / compute /
copy pipeline -- route 3 by ct_linearize_ingest, which evaluates the chain and the ICRF in one pass over the raw frames --
and float32 batches with an empty list (inference/linearization.py::pipeline_route) -- and route 4 (likewise without a
downscale or a dark field; ``pipeline_data_route``): every frame is a batch of its own there, so ct_ingest_extrema_frames
takes the extrema of each frame of a group in one launch pair and ct_linearize_ingest_data reads the constants per frame.
With a dark field, planar frames on route 2 without a downscale and bare float32 batches keep the pipeline
(``DarkField.fuses_with_linearize``: ct_linearize_dark blurs and linearizes the matched frames in one pass), and so does
route 3 without a downscale (``DarkField.fuses_with_linearize_ingest``: ct_linearize_dark_ingest runs the chain as well).
Route 4 without a downscale joins them only on request (``linearize_dataset_generator(fused_dark_ingest_data=True)``,
``DarkField.fuses_with_linearize_ingest_data``: ct_ingest_extrema_frames per group, then ct_linearize_dark_ingest_data with
each frame's own constants); by default it goes frame by frame.  So does everything else: with a dark field any
``StridedDownscale`` and LOOKUP, and on every run route 5.

A leading ``CvToTorch`` on (B,H,W,3) uint8 / uint16 frames is never executed on routes 1-4: the code-route kernels read the
interleaved frames as they are (layout "nhwc_bgr") and the fused ingest reads them itself.  A caller that needs a planar
stack (``planar=True``: explicit std and dark-field images are planar) gets no "nhwc_bgr": such a list goes to route 3.
"""
import ctypes
from dataclasses import dataclass, replace
from typing import Optional

import torch

from .enums import DTYPE_MAP
from .general_functions import clamp_along_dims, torch_to_cv
from .typecheck import expect


class BaseTransform:
    def __call__(self, x: torch.Tensor) -> torch.Tensor:  # pragma: no cover - interface
        raise NotImplementedError


class CvToTorch(BaseTransform):
    """OpenCV (H, W[, C]) BGR -> PyTorch (C, H, W) RGB (reference transforms.py / general_functions.py:315-335).
    Applied to a collated batch (B, H, W, C) it acts per image.  As the first entry of ``gpu_transforms`` on raw
    integer frames it is folded into the kernels' load stage (layout "nhwc_bgr") instead of being executed."""

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim == 2:
            return x.unsqueeze(0)
        if x.ndim in (3, 4) and x.shape[-1] == 3:
            # torch has no uint16 indexing / flip kernels: reverse the channels on a same-width signed view
            alias = {torch.uint16: torch.int16, torch.uint32: torch.int32}.get(x.dtype)
            y = (x.view(alias) if alias else x).flip(-1)
            y = y.view(x.dtype) if alias else y
            return y.permute(2, 0, 1) if x.ndim == 3 else y.permute(0, 3, 1, 2)
        raise ValueError(f"Unexpected image shape: {tuple(x.shape)}")


class TorchToCv(BaseTransform):
    """PyTorch (C, H, W) RGB -> OpenCV (H, W, C) BGR, (1, H, W) -> (H, W) (reference transforms.py:88-104)."""

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return torch_to_cv(x)


class ClampAlongDims(BaseTransform):
    """Clamp between one (min, max) pair, or one pair per slice along ``dim`` (reference transforms.py:137-157).  A clamp
    bound is in general not a representable code / max_code, so a list holding this transform never takes the code
    route; with one pair, or one pair per channel (``dim`` 1 / -3 of the planar view, at most 4 channels), it is a stage
    of the fused ingest (``fusable_ingest``), otherwise it runs as a torch op."""

    def __init__(self, dim, min_max_pairs):
        expect(dim, (int, tuple), "dim")
        expect(min_max_pairs, (tuple, list), "min_max_pairs")
        self.dim, self.min_max_pairs = dim, min_max_pairs

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return clamp_along_dims(x, self.dim, self.min_max_pairs)


class StridedDownscale(BaseTransform):
    """x[..., ::step_size, ::step_size] (reference transforms.py:194-216): a view of every step_size-th row and column
    of the last two axes.  In a ``gpu_transforms`` list that is otherwise the code form (see ``fusable_downscale``) the
    entry points do not call this: the raw codes are compacted on the device by ct_strided_downscale and the
    code-domain kernels run on the smaller stack, bit-identical to a stack sliced on the host."""

    def __init__(self, step_size: int):
        expect(step_size, int, "step_size")
        if step_size < 0:
            raise ValueError("step_size must be non-negative.")
        self.step_size = step_size

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return x[..., ::self.step_size, ::self.step_size]


class CastTo(BaseTransform):
    def __init__(self, data_type=None, device=None):
        if isinstance(data_type, str):
            data_type = DTYPE_MAP[data_type]
        self.data_type = data_type
        self.device = torch.device(device) if isinstance(device, str) else device

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return x.to(dtype=self.data_type if self.data_type is not None else x.dtype,
                    device=self.device if self.device is not None else x.device)


class Normalize(BaseTransform):
    """(x - min) / (max - min) * span + min_t (reference general_functions.py:359-388).  Executed as a torch op on a
    GPU tensor the division by a scalar is a multiplication by its reciprocal (torch's GPU kernels), 1 ulp away from
    the CPU result for some codes; when the kernels fold this transform (integer codes, see
    ``fusable_code_normalisation``) or the fused ingest evaluates it (``max_val`` and ``min_val`` both given, see
    ``fusable_ingest``; one of them or both None -- the batch's own extrema, taken over everything the transform
    receives -- see ``fusable_ingest_data``) the CPU reference's correctly rounded division is reproduced instead."""

    def __init__(self, max_val: Optional[float] = None, min_val: Optional[float] = None, target_range=(0.0, 1.0)):
        self.max_val, self.min_val, self.target_range = max_val, min_val, tuple(target_range)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        # clair_torch/common/general_functions.py:359-388
        max_val = x.max() if self.max_val is None else self.max_val
        min_val = x.min() if self.min_val is None else self.min_val
        den = max_val - min_val
        if den == 0:
            raise ValueError("Normalization range is zero (min == max); cannot normalize.")
        lo, hi = self.target_range
        return (x - min_val) / den * (hi - lo) + lo


def fusable_layout(images: torch.Tensor, transforms):
    """("nhwc_bgr", remaining transforms) when the list starts with CvToTorch on a (B,H,W,3) integer batch -- the
    channel reversal and the HWC->CHW transpose are then done by the kernel's addressing -- else ("nchw", transforms)."""
    ts = [t for t in transforms if t is not None]
    if ts and isinstance(ts[0], CvToTorch) and images.ndim == 4 and images.shape[3] == 3 and \
            images.dtype in (torch.uint8, torch.uint16):
        return "nhwc_bgr", ts[1:]
    return "nchw", ts


_CODES = (torch.uint8, torch.uint16)


def _code_pair(ts):
    """max_code when ``ts`` is exactly CastTo(float32), Normalize(max, 0, (0, 1)) with an integer max in [1, 65535]."""
    if len(ts) != 2 or not isinstance(ts[0], CastTo) or ts[0].data_type != torch.float32 or ts[0].device is not None:
        return None
    n = ts[1]
    if isinstance(n, Normalize) and n.max_val is not None and (n.min_val in (0, 0.0)) and tuple(n.target_range) == (0.0, 1.0):
        mc = float(n.max_val)
        if 1.0 <= mc <= 65535.0 and mc == int(mc):
            return mc
    return None


def fusable_code_normalisation(images: torch.Tensor, transforms):
    """If ``transforms`` applied to integer codes is exactly CastTo(float32) + Normalize(max, 0, (0,1)),
    return max_code so the kernels can ingest the raw codes; otherwise None."""
    return _code_pair([t for t in transforms if t is not None]) if images.dtype in _CODES else None


def fusable_downscale(transforms, images: Optional[torch.Tensor] = None):
    """(step, transforms without it) when the list holds exactly one StridedDownscale with step_size >= 1 that the
    device can apply to the raw codes: anywhere after an optional leading CvToTorch -- before it, on (B,H,W,3) frames,
    the slicing would stride W and C -- and before, between or after the CastTo(float32) / Normalize(max, 0) pair, with
    nothing else in the list (selecting pixels commutes with that pair, not with arbitrary transforms).  With
    ``images`` the stack must also be what that remaining list folds for: uint8 / uint16 codes, (B,H,W,3) when the list
    starts with CvToTorch.  Otherwise (None, the list as given)."""
    ts = [t for t in transforms if t is not None]
    found = [k for k, t in enumerate(ts) if isinstance(t, StridedDownscale)]
    if len(found) != 1 or ts[found[0]].step_size < 1:
        return None, ts
    rest = ts[:found[0]] + ts[found[0] + 1:]
    leading_cv = bool(rest) and isinstance(rest[0], CvToTorch)
    if _code_pair(rest[1:] if leading_cv else rest) is None or (leading_cv and found[0] == 0):
        return None, ts
    if images is not None and (images.dtype not in _CODES or (leading_cv and fusable_layout(images, rest)[0] == "nchw")):
        return None, ts
    return ts[found[0]].step_size, rest


@dataclass(frozen=True)
class IngestPlan:
    """What ``fusable_ingest`` recognised: the stack's memory ``layout`` ("nchw", or "nhwc_bgr" for raw frames behind a
    leading CvToTorch), the StridedDownscale ``step`` to apply to the raw stack first (1 = none) and the arithmetic
    ``stages`` in list order, as ``ops.ingest_transform`` takes them: ("affine", sub, div, mul, add) for a Normalize,
    ("clamp", [(lo, hi), ...]) with one pair or one per channel for a ClampAlongDims."""
    layout: str
    step: int
    stages: tuple


INGEST_MAX_STAGES, INGEST_MAX_CHANNELS = 4, 4


def _is_number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _clamp_stage(t: ClampAlongDims, channels: int):
    pairs = t.min_max_pairs
    if isinstance(pairs, tuple):  # one pair for every element, whatever dim says (clamp_along_dims)
        if len(pairs) != 2 or not all(_is_number(v) for v in pairs):
            return None
        return "clamp", [(pairs[0], pairs[1])]
    dim = t.dim[0] if isinstance(t.dim, tuple) and len(t.dim) == 1 else t.dim
    if isinstance(dim, bool) or not isinstance(dim, int) or dim not in (1, -3):
        return None
    if len(pairs) != channels or channels > INGEST_MAX_CHANNELS:  # a wrong count raises on the torch route, as ever
        return None
    if not all(isinstance(p, (tuple, list)) and len(p) == 2 and all(_is_number(v) for v in p) for p in pairs):
        return None
    return "clamp", [(p[0], p[1]) for p in pairs]


@dataclass(frozen=True)
class StagingPlan:
    """Everything ``stage_images`` needs to stage one batch.  ``route``: "code" | "ingest" | "ingest_data" | "torch" (the
    table at the top of this module); ``layout``: of the staged result, "nhwc_bgr" only on the code route;
    ``source_layout``: how the fused ingest reads the batch ("nhwc_bgr": raw frames behind a leading CvToTorch);
    ``step``: the StridedDownscale to apply to the raw stack (1 = none); ``max_code``: of the code route; ``stages``,
    ``step_first``, ``prefix``, ``min_val`` / ``max_val``: as in ``IngestPlan`` / ``DataIngestPlan``; ``no_transforms``: the
    list is empty (route "torch" with nothing to run); ``step_in_kernel``: the consumer asked ``plan_staging`` for a plan
    whose ``step > 1`` its own kernel applies to the raw stack (ct_linearize_ingest_strided) instead of the staging's
    ct_strided_downscale -- never set on a plan nobody asked that of."""
    route: str
    layout: str = "nchw"
    step: int = 1
    step_first: bool = False
    max_code: Optional[float] = None
    stages: tuple = ()
    prefix: tuple = ()
    min_val: Optional[float] = None
    max_val: Optional[float] = None
    source_layout: str = "nchw"
    no_transforms: bool = False
    step_in_kernel: bool = False


def _recognise_ingest(images: torch.Tensor, transforms) -> Optional[StagingPlan]:
    """The "ingest" / "ingest_data" plan of the grammar that ``fusable_ingest`` and ``fusable_ingest_data`` share, or None."""
    if images.ndim != 4 or images.dtype not in (torch.uint8, torch.uint16, torch.float32) or not images.is_contiguous():
        return None
    layout, ts = fusable_layout(images, transforms)
    channels = images.shape[1] if layout == "nchw" else 3
    is_float, step, stages, data, data_at, step_first = images.dtype == torch.float32, None, [], None, None, False
    for t in ts:
        if type(t) is StridedDownscale:
            if step is not None or t.step_size < 1:
                return None
            step, step_first = t.step_size, data is None
        elif type(t) is CastTo:
            if t.data_type != torch.float32 or t.device is not None:
                return None
            is_float = True
        elif type(t) is Normalize:
            if not is_float:
                return None
            lo, hi = t.target_range if len(t.target_range) == 2 else (None, None)
            if not _is_number(lo) or not _is_number(hi):
                return None
            if t.max_val is None or t.min_val is None:
                given = t.min_val if t.max_val is None else t.max_val
                if data is not None or not (given is None or _is_number(given)):
                    return None
                data, data_at = t, len(stages)
                stages.append(("affine_data", hi - lo, lo))
                continue
            if not _is_number(t.max_val) or not _is_number(t.min_val):
                return None
            den = t.max_val - t.min_val
            if den == 0 or ctypes.c_float(den).value == 0.0:  # (a range that only float32 rounds to zero divides by it)
                return None
            stages.append(("affine", t.min_val, den, hi - lo, lo))
        elif type(t) is ClampAlongDims:
            stage = _clamp_stage(t, channels) if is_float else None
            if stage is None:
                return None
            stages.append(stage)
        else:
            return None
    if not is_float or not 1 <= len(stages) <= INGEST_MAX_STAGES:
        return None
    if data is None:
        return StagingPlan("ingest", source_layout=layout, step=step or 1, stages=tuple(stages))
    return StagingPlan("ingest_data", source_layout=layout, step=step or 1, step_first=step is not None and step_first,
                       stages=tuple(stages), prefix=tuple(stages[:data_at]), min_val=data.min_val, max_val=data.max_val)


def fusable_ingest(images: torch.Tensor, transforms) -> Optional[IngestPlan]:
    """An ``IngestPlan`` when ct_ingest_transform can evaluate ``transforms`` on the 4-D batch ``images`` in one pass,
    else None (the list then runs as torch ops).  Recognised: an optional leading CvToTorch on (B,H,W,3) uint8 / uint16
    frames (``fusable_layout``); at most one StridedDownscale(step >= 1) anywhere after it (selecting pixels commutes
    with per-pixel stages, so the raw stack is compacted first); CastTo(float32, device=None), required before the first
    arithmetic stage of an integer batch and the identity afterwards; and one to four arithmetic stages, each a
    Normalize with ``max_val`` and ``min_val`` given (a zero range is left to the torch route, which raises) or a
    ClampAlongDims with a single (min, max) tuple or a list of C <= 4 pairs along the channel axis (``dim`` 1 or -3).
    The constants are formed as ``Normalize.__call__`` forms them (``max - min`` and ``hi - lo`` in Python's own
    arithmetic); the kernel rounds them to float32 as torch does a Python scalar."""
    p = _recognise_ingest(images, transforms)
    return IngestPlan(p.source_layout, p.step, p.stages) if p is not None and p.route == "ingest" else None


@dataclass(frozen=True)
class DataIngestPlan:
    """What ``fusable_ingest_data`` recognised: ``layout`` and ``step`` as in ``IngestPlan``; ``step_first``: the
    StridedDownscale stands in front of the data-dependent Normalize, whose extrema are then those of the selected
    pixels (behind it they are those of the full-resolution batch: the two do not commute); ``stages`` in list order with
    one ("affine_data", mul, add) entry for that Normalize; ``prefix``: the constant stages in front of it, which
    ct_ingest_extrema evaluates; ``min_val`` / ``max_val``: the bound that was given, None for one taken from the data."""
    layout: str
    step: int
    step_first: bool
    stages: tuple
    prefix: tuple
    min_val: Optional[float]
    max_val: Optional[float]


def fusable_ingest_data(images: torch.Tensor, transforms) -> Optional[DataIngestPlan]:
    """A ``DataIngestPlan`` when ``transforms`` is a list of ``fusable_ingest``'s grammar that holds exactly ONE
    data-dependent Normalize -- ``max_val`` and / or ``min_val`` None (the reference's default,
    clair_torch/common/transforms.py:108-133), the other bound, if given, a plain number -- among its one to four
    arithmetic stages; else None.  Lists without such a Normalize belong to ``fusable_ingest``; two of them, subclasses
    and everything ``fusable_ingest`` declines stay on the torch route.  A zero range cannot be seen here: the staging
    checks the constants the device formed and raises as the reference does."""
    p = _recognise_ingest(images, transforms)
    if p is None or p.route != "ingest_data":
        return None
    return DataIngestPlan(p.source_layout, p.step, p.step_first, p.stages, p.prefix, p.min_val, p.max_val)


def plan_staging(images: torch.Tensor, transforms, planar: bool = False, on_device: bool = False,
                 step_in_kernel: bool = False) -> StagingPlan:
    """The route ``transforms`` take on ``images``, read off the batch's shape, dtype, contiguity and device type alone
    (no device call).  ``planar``: the caller cannot take an interleaved stack; the layout is then always "nchw".
    ``on_device``: ``images`` is a host probe of batches that are staged on a CUDA device: plan as for a batch there.
    ``step_in_kernel``: the caller has a kernel that applies a plan's ``step > 1`` to the raw stack itself
    (linearize_dataset_generator: ct_linearize_ingest_strided); such a plan of route "code", "ingest" or "ingest_data" then
    says so, and nothing else about it changes."""
    plan = _plan_staging(images, transforms, planar, on_device)
    if step_in_kernel and plan.step > 1 and plan.route in ("code", "ingest", "ingest_data"):
        return replace(plan, step_in_kernel=True)
    return plan


def _plan_staging(images: torch.Tensor, transforms, planar: bool, on_device: bool) -> StagingPlan:
    ts = [t for t in transforms if t is not None]
    # 1, 2: the code pair, behind one StridedDownscale (4-D batches) or alone; raw frames stay interleaved unless ``planar``
    step, rest = fusable_downscale(ts)
    if step is None or images.ndim != 4:
        step, rest = 1, ts
    layout, pair = ("nchw", rest) if planar else fusable_layout(images, rest)
    max_code = fusable_code_normalisation(images, pair)
    if max_code is not None:
        return StagingPlan("code", layout, step, max_code=max_code, source_layout=layout)
    # 3, 4: the fused ingest; with a data-dependent Normalize only on a CUDA device (on a CPU "device" the classes run)
    fused = _recognise_ingest(images, ts)
    if fused is not None and (fused.route == "ingest" or images.is_cuda or on_device):
        return fused
    return StagingPlan("torch", no_transforms=not ts)  # 5
