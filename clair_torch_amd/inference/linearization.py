"""linearize_dataset_generator with the reference's signature (clair_torch/inference/linearization.py:17-132).

The reference handles one frame per iteration: host-to-device copy (:62-63), forward + autograd.grad + square + sqrt
(:95-106), optional flat field (:118-130), and a blocking device-to-host copy of both results (:132).  The arithmetic
per frame is 8 us of HBM time; moving 12 MB in and 50 MB out over PCIe is ~1 ms, so end to end this path is a copy
pipeline (BASELINE config C4).  Here the per-frame yield order and the yielded values are the reference's -- value and
LINEAR / LOOKUP std bit for bit -- but the frames move through a three-stage pipeline:

    DataLoader (one frame per item, as the reference requires)
      -> host-to-device copies of a GROUP of frames on a copy stream (plain DMA when the dataset hands out pinned memory)
      -> ONE multi-frame ct_linearize_std launch -- or, for a transform list the fused ingest evaluates, ONE
         ct_linearize_ingest launch on the raw frames -- (+ ct_flatfield_*) on the compute stream, into re-used ring slots
      -> device-to-host copies of (lin, std) into pinned host tensors on a second copy stream
      -> each frame is yielded once its group's copy event has completed; the next groups are already in flight.

Which inputs take the pipeline is ``pipeline_route``'s answer: the code pair ``[CastTo(float32), Normalize(max, 0)]`` on raw
codes (folded into ct_linearize_std's load), float32 pixels with no transform list, and every list of ``plan_staging``'s
route "ingest" -- a black level, a target range, ``ClampAlongDims``, raw BGR frames behind ``CvToTorch`` with explicit
(planar) uncertainty images.  For the latter the ring slot keeps the RAW frames in their own dtype and memory order and
ct_linearize_ingest evaluates chain and ICRF in one pass, bit for bit what ct_ingest_transform followed by
ct_linearize_std gives on the frame-by-frame route.

A ``StridedDownscale`` in such a list -- or beside the code pair, which then runs as the one-stage chain x / max_code --
keeps the pipeline: the slot still holds the raw full-size frames, ct_linearize_ingest_strided reads every step-th row and
column of them, and outputs, exports, pinned host tensors and the group size follow the downscaled shape.  Explicit
uncertainty images must arrive at that shape (the reference applies gpu_transforms to the value images only); another
shape is a ValueError before anything is queued.

A list with a data-dependent ``Normalize`` (``max_val`` and / or ``min_val`` None -- ``Normalize()`` is the reference's
default; every frame is its own batch here, so the bounds are per frame) is ``pipeline_data_route``'s: ONE
ct_ingest_extrema_frames launch pair leaves four constants per frame of the group in the slot, ct_linearize_ingest_data
reads them per frame, and the constants ride the device-to-host stage so that the reference's zero-range ValueError is
raised -- without a synchronisation of its own -- exactly where the frame-by-frame route raises it: after the frames in
front of the offending one have been yielded.  A StridedDownscale BEHIND that Normalize keeps this route (the extrema are
those of the full frames, which ct_ingest_extrema_frames reads; the strided kernel takes the constants); one in FRONT of it
needs the extrema of the selected pixels and stays frame by frame.  Lists that run as torch ops go frame by frame.

A dark-field dataset is ``DarkField.fuses_with_linearize``'s to decide (inference/dark_field.py), not ``pipeline_route``'s:
with ``fused_dark=True`` planar raw codes behind the code pair and bare float32 pixels (LINEAR / CATMULL) take the pipeline.
Every frame is matched on the host when it is copied into the slot, the matched dark fields are uploaded once on the copy
stream (a device cache of 4 pairs) and each group is cut into maximal runs of matched frames -- ONE ct_linearize_dark launch
on that range of the slot's raw frames: conditional blur and ICRF in one pass, bit for bit what ct_dark_field_blur followed
by ct_linearize_std gives frame by frame -- and unmatched ones (ct_linearize_std).  An exception of the match (no dark std,
no image uncertainties) is raised where the frame-by-frame route raises it: after the frames in front have been yielded.
What that decision declines goes to ``DarkField.fuses_with_linearize_ingest`` when ``fused_dark_ingest=True``: every list of
route "ingest" without a StridedDownscale -- a black level, a target range, ``ClampAlongDims``, raw (H,W,3) BGR frames behind
``CvToTorch`` -- on uint8 / uint16 / float32 frames (LINEAR / CATMULL) takes the same pipeline with the RAW frames in the slot
(explicit uncertainty images planar): matched runs go to ct_linearize_dark_ingest -- chain, blur and ICRF in one pass, bit for
bit what ct_ingest_transform, ct_dark_field_blur and ct_linearize_std give frame by frame; 18 B per uint16 sample (22 with
explicit uncertainties) against 42 (46), from the shapes; measured in profiles/linearize_dark_ingest.md -- and unmatched ones
to ct_linearize_ingest.  What both declined goes to ``DarkField.fuses_with_linearize_ingest_data`` when
``fused_dark_ingest_data=True`` (opt-in; the default is False): route "ingest_data" -- ONE data-dependent Normalize,
``Normalize()`` above all -- without a StridedDownscale takes the pipeline too: ONE ct_ingest_extrema_frames launch pair per
group leaves every frame's constants in the slot BEFORE the dark runs, matched runs go to ct_linearize_dark_ingest_data with
their slice of the constants (chain, blur and ICRF in one pass: bit for bit what ct_ingest_extrema, ct_ingest_transform_data,
ct_dark_field_blur and ct_linearize_std give frame by frame; 18 + 2 B per uint16 sample from the shapes;
profiles/linearize_dark_ingest_data.md) and unmatched ones to ct_linearize_ingest_data; the constants ride the device-to-host
stage and the zero-range ValueError is raised where the frame-by-frame route raises it, as without a dark field.  A frame whose
match raises is staged BEFORE it is matched on the frame-by-frame route, so a zero range of that frame wins: its constants
alone are taken once the queue has drained.  Everything else with a dark field (a data-dependent Normalize with the keyword
off, a StridedDownscale, LOOKUP, torch lists), and ``fused_dark=False``, goes frame by frame as ever.

``output_layout="cv"`` (extension): every yielded pair is in the order the reference's ``save_image`` writes -- (H,W,C),
a 3-channel frame reversed to BGR -- made by two ct_export_cv launches per group before the device-to-host copy, which
then carries the final bytes.

Ownership: the yielded tensors are CPU tensors (pinned, from PyTorch's caching host allocator) that belong to the caller,
like the reference's ``.cpu()`` results; the pipeline never writes to them again.
"""
from collections import deque
from typing import Optional

import torch
from torch.utils.data import DataLoader

from .. import ops
from ..common.typecheck import expect
from ..models.base import ICRFModelBase
from ._staging import normalise_transform_list, resolve_device, stage_images, std_arguments
from ..common.transforms import plan_staging

_GROUP_BYTES = 256 << 20  # device-to-host bytes per group (two float32 planes per frame): ~5 frames of 1080p RGB
_SLOTS = 3                # ring slots = groups in flight (copy-in | compute | copy-out)
# linearize_dataset_generator(fused_dark=...).  The rule, set before measuring (profiles/linearize_dark.md): True only if, end
# to end on 64 uint16 1080p frames from pinned memory, every fused run was faster than every frame-by-frame run.  Measured:
# 1037 [715 .. 1041] frames/s fused against 456 [388 .. 461] frame by frame, 2.27x at the medians, the slowest fused run (89 ms)
# ahead of the fastest frame-by-frame run (139 ms): True.
FUSED_DARK_DEFAULT = True
# linearize_dataset_generator(fused_dark_ingest=...).  The rule, set before measuring (profiles/linearize_dark_ingest.md): True
# only if, end to end on 64 uint16 1080p frames from pinned memory, every fused run was faster than every frame-by-frame run in
# BOTH comparisons -- raw (H,W,3) BGR frames behind [CvToTorch, CastTo, Normalize(65535, 0)] and a planar black-level list.
# Measured: BGR 1042 [790 .. 1043] frames/s fused against 462 [246 .. 462] frame by frame, 2.26x at the medians, the slowest fused
# run (81 ms) ahead of the fastest frame-by-frame run (139 ms); planar black level 1042 [1022 .. 1044] against 460 [313 .. 461],
# 2.27x, 63 ms ahead of 139 ms: True.
FUSED_DARK_INGEST_DEFAULT = True
# linearize_dataset_generator(fused_dark_ingest_data=...).  The rule for a later flip, set before measuring
# (profiles/linearize_dark_ingest_data.md), is the standing one: True only if, end to end on 64 uint16 1080p frames from pinned
# memory, every fused run was faster than every frame-by-frame run in BOTH comparisons -- raw (H,W,3) BGR frames behind
# [CvToTorch, CastTo, Normalize()] and planar frames behind [CastTo, Normalize()].  Measured: BGR 1035 [734 .. 1039] frames/s fused
# against 444 [288 .. 455] frame by frame, 2.33x at the medians, the slowest fused run (87 ms) ahead of the fastest frame-by-frame
# run (141 ms); planar 1033 [1032 .. 1038] against 386 [368 .. 454], 2.68x, 62 ms ahead of 141 ms: the rule is met.  The default
# stays False all the same: the route is opt-in, tests/test_gpu_linearize_dark_ingest.py documents the frame-by-frame route as
# today's behaviour for these lists, and changing a default is a decision of its own.
FUSED_DARK_INGEST_DATA_DEFAULT = False
# linearize_dataset_generator(fused_flat=...).  The rule, set before measuring (profiles/linearize_flat.md): True only if every
# fused run was faster than every run of the pair of launches, in every comparison made there.  Measured: per group of 16
# 1080p frames the fused launch takes 0.41 to 0.51 of the time of linearize + flatfield_correct in all five comparisons, every
# fused run faster (uint16 MULTIPLIER LINEAR 0.235 ms against 0.560 ms); end to end on 64 uint16 1080p frames from pinned
# memory, which the copy-out bounds, 1029 [1004 .. 1041] frames/s against 1019 [997 .. 1035]: the ranges overlap: False.
FUSED_FLAT_DEFAULT = False


def linearize_dataset_generator(dataloader: DataLoader, device, icrf_model: ICRFModelBase, flatfield_dataset=None,
                                gpu_transforms=None, dark_field_dataset=None, output_layout: str = "planar",
                                fused_dark: bool = FUSED_DARK_DEFAULT, fused_dark_ingest: bool = FUSED_DARK_INGEST_DEFAULT,
                                fused_flat: bool = FUSED_FLAT_DEFAULT,
                                fused_dark_ingest_data: bool = FUSED_DARK_INGEST_DATA_DEFAULT):
    """``fused_dark`` (extension; only read with a ``dark_field_dataset``): True lets inputs that
    ``DarkField.fuses_with_linearize`` accepts take the streamed pipeline with ct_linearize_dark; False is the frame-by-frame
    route through ct_dark_field_blur and ct_linearize_std.  The yielded values are the same bit for bit.  The default and the
    measurement behind it: FUSED_DARK_DEFAULT above (True: 2.27x the frames/s of the frame-by-frame route on 64 uint16 1080p
    frames, every fused run faster than every frame-by-frame run; profiles/linearize_dark.md).

    ``fused_dark_ingest`` (extension; only read with a ``dark_field_dataset`` and ``fused_dark=True``): True lets inputs that
    ``fuses_with_linearize`` declined and ``DarkField.fuses_with_linearize_ingest`` accepts -- every ``plan_staging`` route
    "ingest" without a StridedDownscale: a black level, a target range, ``ClampAlongDims``, raw (H,W,3) BGR frames behind a
    leading ``CvToTorch`` -- take the streamed pipeline with ct_linearize_dark_ingest on the slot's raw frames (chain, blur and
    ICRF in one pass: 18 B per uint16 sample with derived uncertainties, 22 with explicit ones, where ct_ingest_transform,
    ct_dark_field_blur and ct_linearize_std move 42 / 46; byte counts from the shapes); False is the frame-by-frame route
    through those three.  The yielded values are the same bit for bit.  The default and the measurement behind it:
    FUSED_DARK_INGEST_DEFAULT above (True: 2.26x the frames/s of the frame-by-frame route on 64 uint16 1080p raw BGR frames
    and 2.27x on planar frames behind a black level, every fused run faster than every frame-by-frame run; the kernel alone
    takes 0.55 to 0.63 of the time of the three launches; profiles/linearize_dark_ingest.md).

    ``fused_flat`` (extension; only read with a ``flatfield_dataset``, on the streamed pipeline): True computes the flat field's
    mean once per run (``ops.flatfield_mean``) and lets every launch without dark-field pairs -- ct_linearize_std,
    ct_linearize_ingest / _data, ct_linearize_ingest_strided -- apply the correction to each (lin, std) before it is stored
    (their _flat entry points: 10 + 8/F bytes per uint16 sample with derived uncertainties and F frames per launch, where the
    launch followed by ct_flatfield_sums and ct_flatfield_apply moves 26 + 8/F; byte counts from the shapes); runs of
    dark-matched frames keep their launch and ct_flatfield_apply, with that mean.  False is the pair of launches per group, as
    ever; so are the frame-by-frame route and a flat field whose shape is not the outputs'.  The yielded values are the same bit
    for bit.  The default and the measurement behind it: FUSED_FLAT_DEFAULT above (False: the fused launch takes 0.41 to 0.51 of
    the pair's time per group, but end to end the copy-out bounds the run and the two ranges of frames/s overlap;
    profiles/linearize_flat.md).

    ``fused_dark_ingest_data`` (extension, opt-in; only read with a ``dark_field_dataset``, ``fused_dark=True`` and
    ``fused_dark_ingest=True``): True lets inputs that both decisions above declined and
    ``DarkField.fuses_with_linearize_ingest_data`` accepts -- ``plan_staging`` route "ingest_data": the fused-ingest grammar with
    ONE data-dependent ``Normalize`` (``Normalize()``, the reference's default transform, above all; per-frame bounds, since every
    frame is its own batch here) on 4-D uint8 / uint16 / float32 frames, planar or raw (H,W,3) BGR behind a leading ``CvToTorch``,
    LINEAR / CATMULL -- take the streamed pipeline: ct_ingest_extrema_frames once per group, ct_linearize_dark_ingest_data on the
    runs of matched frames and ct_linearize_ingest_data on the others (18 + 2 B per uint16 sample with derived uncertainties
    where the four launches of the frame-by-frame route move 2 + 42; byte counts from the shapes).  Not fused: a
    ``StridedDownscale`` on either side of that Normalize, LOOKUP, two data-dependent stages.  The yielded values, and the
    place, type and message of every error (a zero range, a failing match, both in one frame: the zero range), are those of the
    frame-by-frame route.  False, the default, is that route.  The rule for a later flip and the measurement behind it:
    FUSED_DARK_INGEST_DATA_DEFAULT above (2.33x the frames/s of the frame-by-frame route on 64 uint16 1080p raw BGR frames and
    2.68x on planar ones, every fused run faster than every frame-by-frame run; per group of 16 frames the extrema call and the
    fused launch take 0.48 to 0.55 of the time of the four launches; profiles/linearize_dark_ingest_data.md)."""
    for name, flag in (("fused_flat", fused_flat), ("fused_dark_ingest_data", fused_dark_ingest_data)):
        if not isinstance(flag, bool):
            raise TypeError(f"{name} must be a bool, got {type(flag).__qualname__}")
    if output_layout not in ("planar", "cv"):
        raise ValueError(f"unknown output_layout {output_layout!r} (planar, cv)")
    expect(dataloader, DataLoader, "dataloader")
    expect(device, (str, torch.device), "device")
    expect(icrf_model, ICRFModelBase, "icrf_model")
    if not dataloader.batch_size == 1:
        raise ValueError("For linearization only batch_size of 1 is allowed.")
    dev = resolve_device(device)
    transforms = normalise_transform_list(gpu_transforms)
    lut, interp = icrf_model.icrf.detach().to(dev), icrf_model.interp_name
    flat = flat_std = None
    if flatfield_dataset is not None:  # linearization.py:48-57
        _, flat, flat_std, _ = flatfield_dataset.get_matching_artefact_images([dataloader.dataset.files[0]])
        flat = flat.to(dev)
        flat_std = flat_std.to(dev) if flat_std is not None else None
    dark = None
    if dark_field_dataset is not None:  # linearization.py:73-92: looked up per frame in the reference; one image here
        from .dark_field import DarkField
        dark = DarkField.from_dataset(dark_field_dataset, dataloader.dataset, dev)

    items = iter(dataloader)
    first = next(items, None)
    if first is None:
        return
    plan = _pipeline_plan(first[1], first[2] is not None, transforms, dev, interp, dark, fused_dark, fused_dark_ingest,
                          fused_dark_ingest_data)
    if plan is None:
        yield from _frame_by_frame(first, items, dataloader, dev, transforms, lut, interp, flat, flat_std, dark,
                                   output_layout == "cv")
    else:  # (a dark field only ever comes with the plan its own decisions accepted)
        yield from _pipelined(first, items, dataloader, dev, lut, interp, flat, flat_std, plan, output_layout == "cv", dark,
                              fused_flat)


def _pipeline_plan(probe, with_std, transforms, dev, interp, dark, fused_dark, fused_dark_ingest, fused_dark_ingest_data=False):
    """The plan the streamed pipeline runs with for a run whose first value batch is ``probe`` (``with_std``: it comes with an
    explicit uncertainty image), or None for the frame-by-frame route.  Every decision is asked here, each on the plan made
    for it."""
    # explicit uncertainty images are planar; a StridedDownscale is ct_linearize_ingest_strided's to apply (step_in_kernel)
    plan = plan_staging(probe, transforms, planar=with_std, step_in_kernel=True)
    route = pipeline_route(probe, plan, dark is not None)
    if dark is not None and fused_dark:
        # the dark field's own decision, on the first frame planned as _frame_by_frame plans it (dark images are planar) ... and,
        # for what that declined, the chain's: route "ingest" keeps the raw frames in the slot (ct_linearize_dark_ingest)
        dark_plan = plan_staging(probe, transforms, planar=True)
        if dark.fuses_with_linearize(probe, dark_plan, interp) or (
                fused_dark_ingest and dark.fuses_with_linearize_ingest(probe, dark_plan, interp)):
            return dark_plan
        if fused_dark_ingest and fused_dark_ingest_data:
            # ... and for what both declined, the data-dependent chain's: planned as for the batch on the device (route
            # "ingest_data" exists only there); the slot keeps the raw frames and their constants (ct_linearize_dark_ingest_data)
            data_plan = plan_staging(probe, transforms, planar=True, on_device=dev.type == "cuda")
            if dark.fuses_with_linearize_ingest_data(probe, data_plan, interp):
                return data_plan
    if route == "pipelined":
        return plan
    # the second, separate decision: a data-dependent Normalize with per-frame constants.  The probe is a host tensor;
    # the list is planned as stage_images plans it for the batch on the device (route "ingest_data" exists only there)
    staged = plan_staging(probe, transforms, planar=with_std, on_device=dev.type == "cuda", step_in_kernel=True)
    return staged if pipeline_data_route(probe, staged, dark is not None) == "pipelined" else None


def pipeline_route(probe: torch.Tensor, plan, has_dark: bool) -> str:
    """"pipelined" | "frame_by_frame" for a run whose first value batch is ``probe`` (shape and dtype only: a CPU tensor
    will do) and whose transform list ``plan_staging`` planned as ``plan``.  The pipeline ingests what one kernel
    ingests from a ring slot: raw integer codes whose normalisation (and OpenCV layout) fold into ct_linearize_std's
    load, float32 pixels with no device transform at all, or -- route "ingest" -- raw frames whose whole chain
    ct_linearize_ingest evaluates; with a StridedDownscale in the list (``plan.step > 1``) and a plan made for a consumer
    that applies the step in its kernel (``plan.step_in_kernel``, which the generator asks ``plan_staging`` for; a plan
    without it leaves the step to the staging and goes frame by frame, as ever) ct_linearize_ingest_strided
    reads every step-th row and column of the raw frames, the code pair then as the one-stage chain x / max_code (measured
    in profiles/linearize_ingest_strided.md).  Anything else goes frame by frame through the generic staging: lists that run
    as torch ops, a dark field as far as THIS function is concerned (``has_dark``: the generator asks
    ``DarkField.fuses_with_linearize`` first when ``fused_dark`` is on, and comes here only for what that declined) -- and, as far as THIS
    function is concerned, a data-dependent Normalize: its extrema are per frame here, per stack in ct_ingest_extrema, so
    it has a decision of its own, ``pipeline_data_route``, which the generator asks when this one said "frame_by_frame"."""
    if has_dark or probe.ndim != 4:
        return "frame_by_frame"
    if plan.route in ("code", "ingest") and (plan.step == 1 or plan.step_in_kernel):
        return "pipelined"
    if plan.route == "torch" and plan.no_transforms and probe.dtype == torch.float32:
        return "pipelined"
    return "frame_by_frame"


def pipeline_data_route(probe: torch.Tensor, plan, has_dark: bool) -> str:
    """"pipelined" | "frame_by_frame" for what ``pipeline_route`` declined: route "ingest_data" -- the fused-ingest grammar
    with ONE data-dependent Normalize -- on uint8 / uint16 / float32 frames without a dark field takes the pipeline with
    per-frame constants (ct_ingest_extrema_frames + ct_linearize_ingest_data per group).  A StridedDownscale BEHIND the
    Normalize keeps it when the plan says ``step_in_kernel`` (see ``pipeline_route``): the extrema are those of the full
    frames and ct_linearize_ingest_strided takes the constants.  One in
    FRONT of it (``plan.step_first``) needs the extrema of the selected pixels, which no kernel here reduces from the raw
    frames, and stays frame by frame.  A dark field always does here: of the decisions that send a dark-field run to the
    pipeline only ``DarkField.fuses_with_linearize_ingest_data`` takes a data-dependent Normalize, and the generator asks it
    itself (``fused_dark_ingest_data``), in front of this function.  Measured against the frame-by-frame route in profiles/linearize_ingest_data.md;
    everything else stays frame by frame."""
    if has_dark or probe.ndim != 4 or plan.route != "ingest_data":
        return "frame_by_frame"
    if plan.step != 1 and (plan.step_first or not plan.step_in_kernel):
        return "frame_by_frame"
    if probe.dtype not in (torch.uint8, torch.uint16, torch.float32):
        return "frame_by_frame"
    return "pipelined"


def _frame_by_frame(first, items, dataloader, dev, transforms, lut, interp, flat, flat_std, dark, cv):
    item = first
    while item is not None:
        index_batch, val_batch, std_batch, meta_batch = item
        planar = std_batch is not None or dark is not None  # explicit std / dark images are planar
        images, max_code, layout = stage_images(val_batch, dev, transforms, planar)
        std, std_mode, std_value = std_arguments(std_batch, dataloader.dataset, dev)
        if dark is not None:
            lin, lin_std = dark.linearize(index_batch, images, max_code, std, std_mode, std_value, lut, interp)
        else:
            lin, lin_std = ops.linearize_frames(images, lut, interp, std=std, std_mode=std_mode, std_value=std_value,
                                                max_code=max_code, want_std=True, layout=layout)
        if flat is not None:  # linearization.py:118-130: mean is a constant, the image term is not rescaled
            ops.flatfield_correct(lin, lin_std, flat, flat_std, input_is_variance=False, through_mean=False)
        if cv:
            lin, lin_std = ops.export_cv(lin.contiguous()), ops.export_cv(lin_std.contiguous())
        yield lin.squeeze().cpu(), lin_std.squeeze().cpu(), meta_batch
        item = next(items, None)


class _Slot:
    """One ring slot: device buffers for a group of frames and the events that order its three stages."""

    def __init__(self, group, frame_shape, dtype, std_shape, chw, dev, cv, data=False):
        self.frames = torch.empty((group,) + tuple(frame_shape), dtype=dtype, device=dev)
        # explicit uncertainty images: frame-shaped beside ct_linearize_std, planar (C,H,W) beside ct_linearize_ingest
        self.std = torch.empty((group,) + tuple(std_shape), dtype=torch.float32, device=dev) if std_shape is not None else None
        self.lin_out = torch.empty((group,) + tuple(chw), dtype=torch.float32, device=dev)
        self.std_out = torch.empty_like(self.lin_out)
        # output_layout="cv": the (group, H, W, C) exports the device-to-host copy reads instead
        self.lin_cv = torch.empty((group, chw[1], chw[2], chw[0]), dtype=torch.float32, device=dev) if cv else None
        self.std_cv = torch.empty_like(self.lin_cv) if cv else None
        # a data-dependent Normalize: the (group, 4) constants of ct_ingest_extrema_frames, its workspace, and the pinned
        # host copy that drain_one reads for the zero-range check (the slot is not re-used before its group is drained)
        self.consts = torch.empty((group, 4), dtype=torch.float32, device=dev) if data else None
        self.workspace = ops.ingest_extrema_frames_workspace(group, dev) if data else None
        self.consts_host = torch.empty((group, 4), dtype=torch.float32, pin_memory=True) if data else None
        self.copied_in, self.computed, self.copied_out = (torch.cuda.Event() for _ in range(3))
        self.busy = False


def _pipelined(first, items, dataloader, dev, lut, interp, flat, flat_std, plan, cv, dark=None, fused_flat=False):
    # Memory note for consumers: the yielded CPU tensors of one group (up to _GROUP_BYTES = 256 MB of output, 5 frames of
    # 1080p RGB) are views of two pinned host tensors, so keeping ONE frame alive keeps its group's pinned pages, and
    # list(generator) page-locks the whole output.  The reference hands out independent pageable .cpu() copies; copying
    # here would cost a 50 MB host memcpy per frame (a fifth of the pipeline's throughput), so a consumer that collects
    # frames should .clone() what it keeps.
    probe = first[1]
    frame_shape = tuple(probe.shape[1:])
    # an ingest plan: the slot keeps the RAW frames, (H,W,3) behind a folded CvToTorch, and the kernel runs the chain
    data = plan.route == "ingest_data"  # per-frame constants of a data-dependent Normalize (pipeline_data_route)
    # a StridedDownscale: the slot still keeps the raw full-size frames, ct_linearize_ingest_strided reads every step-th row
    # and column of them, and everything behind the kernel -- outputs, exports, pinned host tensors, the group size -- has
    # the downscaled shape.  The code pair then runs as the one-stage chain x / max_code (the same correctly rounded division)
    step = plan.step
    fused = plan.route == "ingest" or data or step > 1
    stages = (("affine", 0, plan.max_code, 1, 0),) if plan.route == "code" else plan.stages
    layout, max_code = (plan.source_layout if fused else plan.layout), plan.max_code
    chw = frame_shape if layout == "nchw" else (frame_shape[2], frame_shape[0], frame_shape[1])
    chw = (chw[0], -(-chw[1] // step), -(-chw[2] // step))
    out_bytes = 2 * 4 * chw[0] * chw[1] * chw[2]
    group = max(1, min(16, _GROUP_BYTES // out_bytes))
    std_probe, std_mode, std_value = std_arguments(first[2], dataloader.dataset, torch.device("cpu"))
    with_std = std_probe is not None
    std_shape = (chw if fused else frame_shape) if with_std else None
    if with_std and step > 1 and tuple(std_probe.shape[1:]) != chw:
        # gpu_transforms are applied to the value images only: explicit uncertainties arrive at the downscaled size
        raise ValueError(f"uncertainty images must have the downscaled shape {chw}, got {tuple(std_probe.shape[1:])}")
    slots = [_Slot(group, frame_shape, probe.dtype, std_shape, chw, dev, cv, data) for _ in range(_SLOTS)]
    # fused_flat: (flat, flat std | None, flat mean) as the _flat entry points read them, the mean computed once for the run.  A
    # flat field of another shape than the outputs is left to flatfield_correct, which refuses it
    flat_fused = None
    if flat is not None and fused_flat:
        images = [None if t is None else ops._flat_image(t, dev) for t in (flat, flat_std)]
        if tuple(images[0].shape) == tuple(chw) and (images[1] is None or images[1].shape == images[0].shape):
            flat_fused = (images[0], images[1], ops.flatfield_mean(images[0]))
    compute = torch.cuda.current_stream(dev)
    h2d, d2h = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    in_flight = deque()  # (slot, n frames, pinned lin, pinned std, metas, device dark fields the group's launches read)
    pending = None       # what dark.match raised for a frame: raised once the frames in front of it have been yielded
    pending_frame = None  # ... and, with per-frame constants, that frame: its zero range is raised in place of ``pending``

    def drain_one():
        slot, k, lin_host, std_host, metas, _ = in_flight.popleft()
        slot.copied_out.synchronize()
        slot.busy = False
        ranges = slot.consts_host[:k, 1].tolist() if data else None
        for i in range(k):
            if data and ranges[i] == 0.0:  # general_functions.py:377-378, at the frame it belongs to; a NaN range passes
                raise ValueError(ops.ZERO_RANGE)
            yield lin_host[i].squeeze(), std_host[i].squeeze(), metas[i]

    item, g = first, 0
    while item is not None:
        slot = slots[g % _SLOTS]
        if slot.busy:  # its previous group is the oldest in flight: hand those frames over first
            yield from drain_one()
        g += 1
        k, metas, pairs = 0, [], []
        with torch.cuda.stream(h2d):
            # the slot's input buffers were last read by the kernel of its previous group
            h2d.wait_event(slot.computed)
            while item is not None and k < group:
                index_batch, val_batch, std_batch, meta_batch = item
                if tuple(val_batch.shape[1:]) != frame_shape or val_batch.dtype != probe.dtype:
                    raise ValueError("all frames of one linearization run must share shape and dtype")
                if dark is not None:
                    try:
                        matched = dark.match(index_batch, std_batch, std_mode)
                    except Exception as exc:  # stop queueing here; the frames in front are still handed over first
                        pending, pending_frame, item = exc, val_batch if data else None, None
                        break
                    # (uploaded on this copy stream when the cache does not hold the pair)
                    pairs.append(None if matched is None else dark.device_pair(*matched))
                slot.frames[k].copy_(val_batch[0], non_blocking=True)
                if with_std != (std_batch is not None):
                    # the pipeline's buffers and kernel variant follow the FIRST frame; a stream that mixes frames with
                    # and without an uncertainty image is refused rather than silently ignoring some of them
                    raise ValueError("uncertainty images present for some frames only")
                if with_std:
                    if step > 1 and tuple(std_batch.shape[1:]) != chw:
                        raise ValueError(f"uncertainty images must have the downscaled shape {chw}, got {tuple(std_batch.shape[1:])}")
                    slot.std[k].copy_(std_batch[0], non_blocking=True)
                metas.append(meta_batch)
                k += 1
                item = next(items, None)
            slot.copied_in.record(h2d)
        if k == 0:  # (the match of the group's first frame raised)
            break
        compute.wait_event(slot.copied_in)
        compute.wait_event(slot.copied_out)  # the slot's output buffers were last read by its previous copy-out
        consts = None
        if data:  # two launches for the group's k sets of constants, into the slot's own buffers (in front of the dark runs)
            consts = ops.ingest_extrema_frames(slot.frames[:k], plan.prefix, layout, plan.min_val, plan.max_val,
                                               out=slot.consts[:k], workspace=slot.workspace)
        if dark is not None:
            lin, lin_std = _linearize_dark_runs(slot, k, pairs, with_std, lut, interp, std_mode, std_value, max_code,
                                                (stages, layout) if fused else None, flat_fused, consts=consts)
        else:
            lin, lin_std = _linearize_run(slot, 0, k, with_std, lut, interp, std_mode, std_value, max_code,
                                          stages if fused else None, layout, step, consts, flat=flat_fused)
        if flat is not None and flat_fused is None:  # linearization.py:118-130
            ops.flatfield_correct(lin, lin_std, flat, flat_std, input_is_variance=False, through_mean=False)
        if cv:
            lin = ops.export_cv(lin, out=slot.lin_cv[:k])
            lin_std = ops.export_cv(lin_std, out=slot.std_cv[:k])
        slot.computed.record(compute)
        with torch.cuda.stream(d2h):
            d2h.wait_event(slot.computed)
            if data:  # 16 bytes per frame, in front of copied_out
                slot.consts_host[:k].copy_(slot.consts[:k], non_blocking=True)
            lin_host = torch.empty(lin.shape, dtype=torch.float32, pin_memory=True)
            std_host = torch.empty(lin.shape, dtype=torch.float32, pin_memory=True)
            lin_host.copy_(lin, non_blocking=True)
            std_host.copy_(lin_std, non_blocking=True)
            slot.copied_out.record(d2h)
        slot.busy = True
        in_flight.append((slot, k, lin_host, std_host, metas, pairs))
    while in_flight:
        yield from drain_one()
    if pending is not None:
        if pending_frame is not None:
            # the frame-by-frame route stages a frame before it matches it: a zero range of the frame whose match raised wins.
            # Its constants alone, now that every frame in front has been handed over (one 16-byte readback)
            frame = pending_frame.to(device=dev, non_blocking=True).contiguous()
            ops.check_ingest_consts(ops.ingest_extrema(frame, plan.prefix, layout, plan.min_val, plan.max_val))
        raise pending


def _linearize_run(slot, a, b, with_std, lut, interp, std_mode, std_value, max_code, stages=None, layout="nchw", step=1,
                   consts=None, pairs=None, flat=None):
    """Frames [a:b] of ``slot`` into the same range of its output buffers, in ONE launch of the kernel they belong to.
    ``stages``: the chain of a plan whose slot holds the RAW frames in ``layout`` (explicit uncertainties planar), None for
    frames ct_linearize_std reads as they are; ``step``: a StridedDownscale the kernel applies; ``consts``: the per-frame
    constants of a data-dependent Normalize, rows [a:b] of the group's; ``pairs``: the device (dark, dark std) matched to each frame of the run, None for a
    run without dark fields; ``flat``: the (flat, flat std | None, flat mean) of ``fused_flat``, applied by the launch itself on a
    run without dark fields (ct_linearize_std_flat, ct_linearize_ingest_flat, ct_linearize_ingest_strided_flat) and by
    ct_flatfield_apply with that mean behind the launch of a run with them.

        pairs   stages  step    front
        None    None    1       linearize_frames                 (ct_linearize_std)
        None    given   1       linearize_ingest_frames          (ct_linearize_ingest / _data with ``consts``)
        None    given   > 1     linearize_ingest_frames_strided  (ct_linearize_ingest_strided)
        given   None    1       linearize_dark_frames            (ct_linearize_dark)
        given   given   1       linearize_dark_ingest_frames     (ct_linearize_dark_ingest)
        given   given   1       linearize_dark_ingest_frames_data   with ``consts`` (ct_linearize_dark_ingest_data)"""
    frames = slot.frames[a:b]
    args = dict(std=slot.std[a:b] if with_std else None, std_mode=std_mode, std_value=std_value,
                out=(slot.lin_out[a:b], slot.std_out[a:b]))
    if pairs is not None:
        darks, dark_stds = [p[0] for p in pairs], [p[1] for p in pairs]
        if stages is None:
            lin, lin_std = ops.linearize_dark_frames(frames, darks, dark_stds, lut, interp, max_code=max_code, **args)
        elif consts is None:
            lin, lin_std = ops.linearize_dark_ingest_frames(frames, stages, darks, dark_stds, lut, interp, layout=layout, **args)
        else:
            lin, lin_std = ops.linearize_dark_ingest_frames_data(frames, stages, darks, dark_stds, lut, interp, consts=consts,
                                                                 layout=layout, **args)
        if flat is not None:
            ops.flatfield_correct(lin, lin_std, flat[0], flat[1], input_is_variance=False, through_mean=False, flat_mean=flat[2])
        return lin, lin_std
    args.update(want_std=True, layout=layout)
    if flat is not None:  # the same three fronts with the correction in their launch
        if stages is None:
            return ops.linearize_frames_flat(frames, lut, interp, flat=flat, max_code=max_code, **args)
        if step > 1:
            return ops.linearize_ingest_frames_strided_flat(frames, step, stages, lut, interp, flat=flat, consts=consts, **args)
        return ops.linearize_ingest_frames_flat(frames, stages, lut, interp, flat=flat, consts=consts, **args)
    if stages is None:
        return ops.linearize_frames(frames, lut, interp, max_code=max_code, **args)
    if step > 1:
        return ops.linearize_ingest_frames_strided(frames, step, stages, lut, interp, consts=consts, **args)
    return ops.linearize_ingest_frames(frames, stages, lut, interp, consts=consts, **args)


def _linearize_dark_runs(slot, k, pairs, with_std, lut, interp, std_mode, std_value, max_code, chain=None, flat=None, consts=None):
    """The first ``k`` frames of ``slot`` into its output buffers, cut into maximal runs of frames with a matched dark
    field (``pairs[i]``: its device (dark, dark std)) and without one (None: MissingValMode.SKIP_BATCH leaves the frame
    uncorrected), one ``_linearize_run`` each.  ``chain`` = (stages, layout) of a route "ingest" / "ingest_data" plan: the slot
    holds the raw frames in that layout; ``consts``: the (k, 4) per-frame constants of an "ingest_data" plan, made for the whole
    group before the runs -- every run gets its rows."""
    stages, layout = chain if chain is not None else (None, "nchw")
    a = 0
    while a < k:
        b = a + 1
        while b < k and (pairs[b] is None) == (pairs[a] is None):
            b += 1
        _linearize_run(slot, a, b, with_std, lut, interp, std_mode, std_value, max_code, stages, layout,
                       consts=None if consts is None else consts[a:b], pairs=None if pairs[a] is None else pairs[a:b], flat=flat)
        a = b
    return slot.lin_out[:k], slot.std_out[:k]
