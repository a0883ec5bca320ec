"""Shared staging of a collated batch onto the device for the inference / training entry points."""
from dataclasses import dataclass
from typing import Iterable, Optional

import torch

from .. import ops
from ..common.transforms import StridedDownscale, plan_staging


def resolve_device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"device={device!r}: clair_torch_amd computes on MI355X only (use 'cuda' / 'cuda:k'); "
                           "it has no CPU path -- the reference's CPU behaviour is reproduced by oracle/ for tests.")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def normalise_transform_list(gpu_transforms) -> list:
    if gpu_transforms is None:
        return []
    if isinstance(gpu_transforms, Iterable):
        return [t for t in gpu_transforms if t is not None]
    return [gpu_transforms]


@dataclass
class DeferredIngest:
    """A batch on routes "ingest" / "ingest_data" whose chain has NOT been executed (``stage_images(defer_ingest=True)``): the
    raw device ``frames`` (behind the StridedDownscale compaction where the plan has one), the ``stages`` as
    ``ops.ingest_transform`` takes them, the ``layout`` of the frames, and for "ingest_data" the ``consts`` of
    ``ops.ingest_extrema`` (already checked for a zero range), else None.  ``ops.hdr_merge_ingest_batch`` takes all four.
    ``step`` (``stage_images(step_in_kernel=True)``): above 1 the StridedDownscale has NOT been applied either -- ``frames`` are
    the raw full-size ones and the consumer's kernel selects every ``step``-th row and column (``ops.hdr_merge_ingest_batches_strided``),
    or ``materialise`` compacts them first."""
    frames: torch.Tensor
    stages: tuple
    layout: str
    consts: Optional[torch.Tensor] = None
    step: int = 1

    def materialise(self) -> torch.Tensor:
        """The float32 planar pixels the staging would have returned without ``defer_ingest``: the downscale where it is still
        owed, then ct_ingest_transform(_data)."""
        frames = ops.strided_downscale(self.frames, self.step, layout=self.layout) if self.step > 1 else self.frames
        return ops.ingest_transform(frames, self.stages, layout=self.layout, consts=self.consts)


def stage_images(val_batch: torch.Tensor, device: torch.device, transforms: list, planar: bool = False,
                 defer_ingest: bool = False, step_in_kernel: bool = False):
    """Move the value batch to the device and run / fuse the device transforms: (images, max_code, layout).

    ``plan_staging`` picks the route (the table in common/transforms.py); what each of them does here and returns:

    ============= ================================================================= ====================================
    route         device work                                                       returns
    ============= ================================================================= ====================================
    "code"        ct_strided_downscale of the raw codes when the list holds one     integer codes, their max_code,
                                                                                    "nchw" | "nhwc_bgr" (raw frames)
    "ingest"      the downscale, then ct_ingest_transform: one pass, the            float32 planar pixels, None, "nchw"
                  reference's CPU arithmetic
    "ingest_data" ct_ingest_extrema -- of the compacted stack when the downscale    float32 planar pixels, None, "nchw"
                  stands in front of the data-dependent Normalize, else of the full
                  one --, the downscale where it stands, ct_ingest_transform_data,
                  then ONE 16-byte readback for the reference's zero-range error
    "torch"       the classes' ``__call__`` as torch ops                            float32 planar pixels, None, "nchw"
    ============= ================================================================= ====================================

    ``planar``: the caller holds explicit std or dark-field images, which are planar: the layout is then always "nchw".
    ``defer_ingest`` (opt-in): routes "ingest" and "ingest_data" do everything but ct_ingest_transform(_data) and return a
    ``DeferredIngest`` in place of the float32 pixels, for a kernel that evaluates the chain itself; the other routes
    return what they always do.
    ``step_in_kernel`` (opt-in, read with ``defer_ingest`` only): the caller's kernel applies a StridedDownscale itself.  Route
    "ingest" then skips the compaction and returns the raw full-size frames with ``DeferredIngest.step`` = the plan's step;
    route "ingest_data" does the same when the Normalize stands IN FRONT of the downscale (the extrema are those of the full
    stack, as ever); with the downscale in front (``step_first``) it compacts as before and the step is 1.  Route "code" with
    a downscale, and everything without ``defer_ingest``, is staged as without the flag."""
    images = val_batch.to(device=device, non_blocking=True)  # the ONE host-to-device copy of the batch (a plain DMA when pinned)
    # (a caller that passes nothing new plans exactly as before: the call itself is the old one)
    plan = plan_staging(images, transforms, planar, step_in_kernel=True) if step_in_kernel and defer_ingest else \
        plan_staging(images, transforms, planar)
    keep_step = plan.step_in_kernel and plan.route in ("ingest", "ingest_data") and not plan.step_first
    if plan.route == "code":
        if plan.step > 1:
            images = ops.strided_downscale(images, plan.step, layout=plan.layout)
        return images, plan.max_code, plan.layout
    if plan.route == "ingest":
        if keep_step:
            return DeferredIngest(images, plan.stages, plan.source_layout, step=plan.step), None, "nchw"
        images = ops.strided_downscale(images, plan.step, layout=plan.source_layout)
        if defer_ingest:
            return DeferredIngest(images, plan.stages, plan.source_layout), None, "nchw"
        return ops.ingest_transform(images, plan.stages, layout=plan.source_layout), None, "nchw"
    if plan.route == "ingest_data":
        if plan.step_first:
            images = ops.strided_downscale(images, plan.step, layout=plan.source_layout)
        consts = ops.ingest_extrema(images, plan.prefix, plan.source_layout, plan.min_val, plan.max_val)
        if keep_step:
            ops.check_ingest_consts(consts)
            return DeferredIngest(images, plan.stages, plan.source_layout, consts, step=plan.step), None, "nchw"
        if not plan.step_first:
            images = ops.strided_downscale(images, plan.step, layout=plan.source_layout)
        if defer_ingest:
            ops.check_ingest_consts(consts)
            return DeferredIngest(images, plan.stages, plan.source_layout, consts), None, "nchw"
        out = ops.ingest_transform(images, plan.stages, layout=plan.source_layout, consts=consts)
        ops.check_ingest_consts(consts)
        return out, None, "nchw"
    for t in transforms:
        images = t(images)
    if images.dtype in (torch.uint8, torch.uint16):
        raise TypeError("integer images reached the kernel without a Normalize transform; pass "
                        "gpu_transforms=[CastTo('float32'), Normalize(max_val=<max code>, min_val=0)]")
    return images.to(torch.float32).contiguous(), None, "nchw"


def has_downscale(transforms) -> bool:
    return any(isinstance(t, StridedDownscale) for t in transforms)


def refuse_tile_with_downscale(tile, transforms):
    """Row bands (``tile=``) hold rows [row_offset, row_offset + h) of the global image; which of them a
    StridedDownscale selects depends on row_offset % step, a phase the staging does not carry."""
    if tile is not None and has_downscale(transforms):
        raise ValueError("tile= cannot be combined with a StridedDownscale in gpu_transforms: downscale the row bands "
                         "before sharding, or run untiled")


def std_arguments(std_batch: Optional[torch.Tensor], dataset, device):
    """(explicit std tensor | None, std_mode, std_value): explicit tensors as the reference, or the dataset's
    ``std_hint`` for uncertainties derived in-kernel (see datasets/stack_dataset.py)."""
    if std_batch is not None:
        return std_batch.to(device=device, dtype=torch.float32, non_blocking=True), "explicit", 0.0
    hint = getattr(dataset, "std_hint", None)
    if hint is not None:
        return None, hint[0], float(hint[1])
    return None, "none", 0.0
