"""Shared staging of a collated batch onto the device for the inference / training entry points."""
from typing import Iterable, Optional

import torch

from .. import ops
from ..common.transforms import (StridedDownscale, fusable_code_normalisation, fusable_downscale, fusable_ingest,
                                 fusable_ingest_data, fusable_layout)


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


def stage_images(val_batch: torch.Tensor, device: torch.device, transforms: list, want_layout: bool = False):
    """Move the value batch to the device and run / fuse the device transforms.

    Returns (images, max_code): integer codes with their max_code when the transform list is the
    CastTo(float32)+Normalize(max, 0) pair the kernels ingest directly, else float32 pixels and None.
    With ``want_layout`` a third value is returned: "nhwc_bgr" when the list additionally starts with CvToTorch
    on raw (B,H,W,3) frames (the kernel then reads the interleaved BGR frames as they are), else "nchw".
    One StridedDownscale in such a list (``fusable_downscale``) keeps the code route: the raw codes are compacted on
    the device in their own dtype and layout, and the smaller integer stack is returned.
    Any other list that ``fusable_ingest`` recognises (a black level, a target range, clamps, ...) is evaluated by
    ct_ingest_transform in one pass with the reference's CPU arithmetic.  A list of that grammar with one data-dependent
    Normalize (``max_val`` / ``min_val`` None, ``fusable_ingest_data``) first has the batch's extrema reduced on the
    device (ct_ingest_extrema) -- of the compacted stack when the StridedDownscale stands in front of that Normalize, of
    the full-resolution one when it stands behind -- and costs one 16-byte readback per batch for the reference's
    zero-range error.  The rest runs as torch ops.  All of these give float32 planar pixels."""
    images = val_batch.to(device=device, non_blocking=True)  # the ONE host-to-device copy of the batch (a plain DMA when pinned)
    step, rest = fusable_downscale(transforms)
    if step is not None and images.ndim == 4:
        layout, tail = fusable_layout(images, rest) if want_layout else ("nchw", rest)
        max_code = fusable_code_normalisation(images, tail)
        if max_code is not None:
            images = ops.strided_downscale(images, step, layout=layout)
            return (images, max_code, layout) if want_layout else (images, max_code)
    if want_layout:
        layout, rest = fusable_layout(images, transforms)
        if layout != "nchw":
            max_code = fusable_code_normalisation(images, rest)
            if max_code is not None:
                return images, max_code, layout
        out = stage_images(images, device, transforms)  # already on the device: .to() is then the identity
        return out[0], out[1], "nchw"
    max_code = fusable_code_normalisation(images, transforms)
    if max_code is not None:
        return images, max_code
    plan = fusable_ingest(images, transforms)
    if plan is not None:
        images = ops.strided_downscale(images, plan.step, layout=plan.layout)
        return ops.ingest_transform(images, plan.stages, layout=plan.layout), None
    plan = fusable_ingest_data(images, transforms) if images.is_cuda else None  # on a CPU "device" the classes run
    if plan is not None:
        if plan.step_first:
            images = ops.strided_downscale(images, plan.step, layout=plan.layout)
        consts = ops.ingest_extrema(images, plan.prefix, plan.layout, plan.min_val, plan.max_val)
        if not plan.step_first:
            images = ops.strided_downscale(images, plan.step, layout=plan.layout)
        out = ops.ingest_transform(images, plan.stages, layout=plan.layout, consts=consts)
        ops.check_ingest_consts(consts)
        return out, None
    for t in transforms:
        images = t(images)
    if images.dtype in (torch.uint8, torch.uint16):
        raise TypeError("integer images reached the kernel without a Normalize transform; pass "
                        "gpu_transforms=[CastTo('float32'), Normalize(max_val=<max code>, min_val=0)]")
    return images.to(torch.float32).contiguous(), None


def restage_planar(val_batch: torch.Tensor, images: torch.Tensor, device: torch.device, transforms: list):
    """(images, max_code, "nchw") for a batch that ``stage_images`` handed over interleaved but that has to be planar
    after all (explicit std / dark-field images are planar): the transforms run on the generic route.  ``images`` is
    what ``stage_images`` returned -- the batch itself, already on the device, unless it was compacted by a
    StridedDownscale, which must not be applied a second time: then staging starts over from ``val_batch``."""
    source = val_batch if has_downscale(transforms) else images
    return stage_images(source, device, transforms) + ("nchw",)


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
