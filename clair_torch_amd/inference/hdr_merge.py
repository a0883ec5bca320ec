"""compute_hdr_image with the reference's signature (clair_torch/inference/hdr_merge.py:19-155).

Per batch the reference linearizes, divides by the exposure time, weights, updates a WBOMean, and back-propagates
through all of it to get the variance; here each batch is ONE fused kernel launch (ct_hdr_merge_batch) that updates
device-resident state, and the closed form of that variance is evaluated in registers.  Streaming semantics are the
reference's, including the batch-partition dependence of the variance (state detached per batch, hdr_merge.py:128).
"""
from typing import Callable, NamedTuple, Optional

import torch
from torch.utils.data import DataLoader

from .. import ops
from ..common.typecheck import expect
from ..models.base import ICRFModelBase
from ._staging import DeferredIngest, normalise_transform_list, refuse_tile_with_downscale, resolve_device, stage_images, std_arguments

# The most the queued dark-field batches of one launch may hold on the device: frames, explicit stds, dark fields, dark stds and
# halo rows.  Under 3 % of the device's memory, and about four batches of 4 frames of 3 x 4096 x 4096 uint16 with a dark field and
# a dark std per frame (2 GB each: the dark fields are 8 B per element and frame).
DARK_QUEUE_BYTES = 8 << 30

# compute_hdr_image(fused_dark_ingest=...).  The rule, set before measuring (profiles/merge_dark_ingest.md): True only if every
# timed run of the fused launch is faster than every timed run of ops.ingest_transform + ops.hdr_merge_dark_batch(es) at every
# measured shape -- the rule ``fused_dark`` was decided by.
FUSED_DARK_INGEST_DEFAULT = False

# compute_hdr_image(fused_downscale=...).  The same rule, set before measuring (profiles/merge_ingest_strided.md): True only if
# every timed run of the fused launch (ops.hdr_merge_ingest_batches_strided) is faster than every timed run of
# ops.strided_downscale + ops.hdr_merge_ingest_batches at every measured shape -- and only if no existing test notices the route.
FUSED_DOWNSCALE_DEFAULT = False


class _QueueKind(NamedTuple):
    """What the queued batches of compute_hdr_image have in common, and what tells one launch of them from the next."""
    key: tuple                  # batches of one key go into one launch
    cap: int                    # ... at most so many of them
    held: int                   # ... of at most DARK_QUEUE_BYTES together: the bytes THIS batch holds on the device (0: not counted)
    state_shape: tuple          # the MergeState their launch needs when it is not the whole merge
    with_variance: bool
    launch: Callable            # (first queued batch, **merge keywords) -> (mean, std) of a final launch | None


def _dark_batch_bytes(images, std, matched, halo):
    """What a queued dark-field batch holds on the device (dark field and dark std as the float32 the kernel reads)."""
    held = sum(t.numel() * t.element_size() for t in (images, std, halo) if t is not None)
    return held + sum(4 * t.numel() for t in matched if t is not None)


def compute_hdr_image(dataloader: DataLoader, device, icrf_model: Optional[ICRFModelBase] = None,
                      weight_fn: Optional[Callable] = None, flat_field_dataset=None, gpu_transforms=None,
                      dark_field_dataset=None, tile: Optional[ops.TileGeometry] = None, group=None,
                      output_layout: str = "planar", reference_order: Optional[bool] = None, fused_ingest: bool = True,
                      fused_dark: bool = True, dark_batches_per_launch: int = 1,
                      fused_dark_ingest: bool = FUSED_DARK_INGEST_DEFAULT, fused_downscale: bool = FUSED_DOWNSCALE_DEFAULT):
    """Merge the exposure stack served by ``dataloader`` into an HDR image and its standard uncertainty.

    Returns ``(mean float64 (C,H,W), std float32 (C,H,W) | None)`` on ``device`` (squeezed like the reference).
    ``weight_fn``: None = unit weights, anything else = Gaussian weights, scale 30 (hdr_merge.py:95).
    ``flat_field_dataset``: any object with the reference's ``get_matching_artefact_images`` (e.g.
    ``clair_torch_amd.datasets.ArtefactStack``); its image must cover the rows this process holds.
    ``dark_field_dataset``: likewise; the matched dark fields drive a conditional 3x3 blur of every batch and add their
    own variance term (inference/dark_field.py; parity unpinned -- the blur is torchvision's, restated).
    ``tile`` / ``group`` (extensions): the rows this process holds of a taller global image (multi-GPU row bands) and
    the process group over which the flat field's spatial sums are all-reduced and the blur's halo rows exchanged.
    ``output_layout`` (extension): "planar" = the reference's (C,H,W); "input" = when the frames are ingested interleaved
    (``gpu_transforms`` starting with CvToTorch on raw (H,W,3) frames), leave mean and uncertainty in that (H,W,C) order and
    channel sequence -- what ``cv2.imwrite`` takes; the kernel then stores dense packets (CT_MERGE_OUT_AS_INPUT).  Not
    combinable with flat-field / dark-field correction, whose kernels work on planar data.  "cv" = the arrays the
    reference's ``save_image`` writes, made on the device by ``ops.export_cv`` from the "planar" result after every
    correction: mean float64 and std float32 as (H,W,C) with a 3-channel image reversed to BGR, (H,W) for one channel;
    works with every ingest form, with flat-field / dark-field correction and with ``tile`` (a band exports its own rows).
    ``reference_order`` (extension): how the uncertainty is evaluated.  None = the library's default -- LOOKUP and CATMULL
    with uncertainties follow the reference's own float32 autograd order (within 1e-5 of what the reference computes, 4-5x
    the time), LINEAR / no model the closed form; False = the closed-form kernels in every mode (better conditioned than the
    reference, up to 4e-5 away from it on single pixels in those two modes); True = reference order in every mode.
    ``fused_ingest`` (extension): a ``gpu_transforms`` list on route "ingest" / "ingest_data" (common/transforms.py: a black
    level, a clamp, a target range, a data-dependent Normalize on raw codes) is evaluated inside the merge kernel
    (ct_hdr_merge_ingest_batches: up to 16 batches per launch, no float32 copy of a batch) when there is no dark-field dataset and
    the mode is a closed-form one; False = ct_ingest_transform, then the float32 merge.  The results are the same bit for bit.
    ``fused_dark`` (extension): a batch that a dark field matched is blurred and merged in ONE pass over its staged images
    (ct_hdr_merge_dark_batch: no float32 copy of the batch and of its uncertainty) when those are planar codes or float32
    pixels and the mode is a closed-form one (the rule of ``fused_ingest``: not ``reference_order=True``, and LOOKUP / CATMULL
    only with ``reference_order=False``); such a batch is launched on its own, after the batches queued before it.  False =
    ct_dark_field_blur, then the float32 merge.  The results are the same bit for bit.  On by default: the fused launch
    was faster than the pair at every measured shape, beyond the run-to-run spread (0.89-0.94 of its time for batches of 4,
    0.41-0.45 for batches of 32; profiles/merge_dark.md).
    ``dark_batches_per_launch`` (extension, 1 .. 16): how many consecutive batches of that kind one launch takes.  1 = one launch
    per matched batch, as above.  Above 1 such a batch is queued like the others -- staged images, its uncertainties, the
    matched dark fields and, for a row band, the halo rows exchanged right then, so that every rank sends and receives in
    loader order -- and the queue goes through ct_hdr_merge_dark_batches (one launch, the streaming state in registers between
    the batches, bit for bit the launches it replaces) when the next batch is of another kind (unmatched, not fused, another
    shape, dtype or uncertainty mode), when it holds ``dark_batches_per_launch`` batches, when the next batch would take it
    above DARK_QUEUE_BYTES (8 GiB; a larger single batch runs alone), and at the end.  Measured on 32 exposures of 3x4096x4096:
    0.67-0.74 of the time of one launch per batch for batches of 4 and 0.82-0.92 for batches of 8, every run faster than every
    per-batch run (profiles/merge_dark_batches.md).  The default stays 1, one launch per matched batch as before this keyword
    existed; pass 16 to queue.
    ``fused_dark_ingest`` (extension; only read with a ``dark_field_dataset`` and ``fused_dark=True``): a ``gpu_transforms`` list
    on route "ingest" / "ingest_data" (a black level, a target range, ``ClampAlongDims``, raw (H,W,3) BGR frames behind
    ``CvToTorch``, a data-dependent ``Normalize()``) in front of a dark-field dataset.  True = the chain is not executed when
    the batch is staged; a batch that a dark field matched goes through ct_hdr_merge_dark_ingest_batches -- chain, blur and merge
    in one pass over the RAW frames, no float32 copy of the batch; 10 B per uint16 sample with derived uncertainties against 18,
    from the shapes -- when ``DarkField.fuses_with_merge_ingest`` accepts it (uint8 / uint16 / float32 frames, a closed-form
    mode, interleaved frames only without a row band).  Such batches are queued under a key of their own (dtype, shape, layout,
    chain, uncertainty mode, with or without constants) and flushed like the queue above: on a change of kind, at
    ``dark_batches_per_launch`` batches (1: one batch per launch), at DARK_QUEUE_BYTES and at the end; for a row band the halo
    rows are exchanged on the RAW frames when the batch is queued.  Unmatched batches take the ``fused_ingest`` queue
    (ct_hdr_merge_ingest_batches; float32 frames and the reference-order modes get the float32 stack, as there), declined ones
    are materialised with ct_ingest_transform and go on as without this keyword.  The results are the same bit for bit.
    False = ct_ingest_transform when the batch is staged, as before this keyword existed.  Measured: see
    profiles/merge_dark_ingest.md for the numbers and for the default, which follows the rule stated there.
    ``fused_downscale`` (extension; only read without a ``dark_field_dataset`` and with ``fused_ingest=True``): a ``gpu_transforms``
    list on route "ingest" / "ingest_data" that holds a ``StridedDownscale``.  True = the staging does not compact the batch
    (ct_strided_downscale: a copy written once to be read once); the queued batches stay the raw full-size frames and one launch
    of ct_hdr_merge_ingest_strided_batches selects every step-th row and column while it merges them.  The results are the same
    bit for bit.  These keep today's route whatever the keyword says: route "code" with a downscale (the pivoted code-domain
    kernel is other arithmetic, so bit-identity with it cannot be promised), a data-dependent Normalize BEHIND the downscale (its
    extrema are those of the selected pixels: the staging compacts first), dark-field batches, row bands (``tile`` with a
    downscale is refused as ever), float32 frames and the reference-order modes (compacted, then the float32 stack), and the
    video-statistics and pair kernels.  Measured: see profiles/merge_ingest_strided.md for the numbers and for the default,
    which follows the rule stated there.
    """
    if type(dark_batches_per_launch) is not int or not 1 <= dark_batches_per_launch <= ops.MAX_MERGE_BATCHES:
        raise ValueError(f"dark_batches_per_launch must be an int in 1 .. {ops.MAX_MERGE_BATCHES}, got {dark_batches_per_launch!r}")
    if output_layout not in ("planar", "input", "cv"):
        raise ValueError(f"unknown output_layout {output_layout!r} (planar, input, cv)")
    if output_layout == "input" and (flat_field_dataset is not None or dark_field_dataset is not None):
        raise ValueError('output_layout="input" cannot be combined with flat-field / dark-field correction')
    expect(dataloader, DataLoader, "dataloader")
    expect(device, (str, torch.device), "device")
    expect(icrf_model, ICRFModelBase, "icrf_model", allow_none=True)
    if weight_fn is not None and not callable(weight_fn):
        expect(weight_fn, type(None), "weight_fn")
    dev = resolve_device(device)
    dark = None
    if dark_field_dataset is not None:  # hdr_merge.py:76-92 (PARITY UNPINNED: the blur is torchvision's, restated)
        from .dark_field import DarkField, exchange_halo
        dark = DarkField.from_dataset(dark_field_dataset, dataloader.dataset, dev)
    transforms = normalise_transform_list(gpu_transforms)
    refuse_tile_with_downscale(tile, transforms)
    lut = interp = None
    if icrf_model is not None:
        lut, interp = icrf_model.icrf.detach().to(dev), icrf_model.interp_name

    state = result = None
    batches = iter(dataloader)
    pending = next(batches, None)
    if pending is None:
        raise ValueError("dataloader yielded no batches")
    # Consecutive batches are queued (staged on the device, not yet merged) and handed over together: one
    # ct_hdr_merge_batches call keeps the streaming state in registers across up to 16 batches instead of writing and
    # re-reading 32 B per element after every one of them (the reference's default is batch_size: 4).  The result is the
    # same bit for bit as merging batch by batch (per-batch detach of the state, hdr_merge.py:128, included).
    # What is queued is of one kind (``_QueueKind``): the key its batches share, how many of them and how many bytes one launch
    # takes, the MergeState they need and the function that launches them.
    queue, queue_kind, queue_bytes = [], None, 0

    def merge_args(state_shape, with_variance, final):
        """The keywords every merge op takes; a launch that is not the whole merge gets the MergeState, made here once."""
        nonlocal state
        if state is None and (not final or flat_field_dataset is not None):
            state = ops.MergeState(state_shape, dev, with_variance=with_variance)
        return dict(lut=lut, interp=interp, gaussian_weight=weight_fn is not None, state=state,
                    finalize=final and flat_field_dataset is None, reference_order=reference_order)

    def column(name):
        """What the queued batches hold under ``name``, one entry per batch; None where they hold none."""
        return None if queue[0][name] is None else [q[name] for q in queue]

    def flush(final):
        nonlocal result, queue_bytes
        if queue:
            result = queue_kind.launch(queue[0], **merge_args(queue_kind.state_shape, queue_kind.with_variance, final))
            del queue[:]
            queue_bytes = 0

    def enqueue(kind, **batch):
        """Flush what is queued if this batch is of another kind or would take the queue over its cap, queue it, and flush at
        the end of the loader."""
        nonlocal queue_kind, queue_bytes
        if queue and (kind.key != queue_kind.key or len(queue) == kind.cap or queue_bytes + kind.held > DARK_QUEUE_BYTES):
            flush(False)
        queue_kind = kind
        queue_bytes += kind.held
        queue.append(batch)
        if last:
            flush(True)

    def launch_dark_ingest(k0, **args):
        # chain, blur and merge of every queued dark-field batch in one launch over the raw frames (ct_hdr_merge_dark_ingest_batches)
        return dark.merge_ingest_batches(column("matched"), column("images"), column("exposure"), column("std"), k0["std_mode"],
                                         k0["std_value"], tile, column("halo"), **args)

    def launch_dark(k0, **args):
        # blur and merge of every queued dark-field batch in one launch (ct_hdr_merge_dark_batches)
        return dark.merge_batches(column("matched"), column("images"), column("exposure"), k0["max_code"], column("std"), k0["std_mode"],
                                  k0["std_value"], tile, column("halo"), **args)

    def launch_ingest(k0, **args):
        # the chain and the merge of every queued batch in one launch (ct_hdr_merge_ingest_batches): the raw frames are read once
        # and the streaming state stays in registers between the batches, as on the code route
        d = k0["images"]
        consts = None if d.consts is None else [q["images"].consts for q in queue]
        kw = dict(stds=column("std"), std_mode=k0["std_mode"], std_value=k0["std_value"], tile=tile, layout=d.layout, consts=consts, **args)
        frames = [q["images"].frames for q in queue]
        if d.step > 1:  # ... and so is the StridedDownscale: the load selects every step-th row and column of the raw frames
            return ops.hdr_merge_ingest_batches_strided(frames, d.step, d.stages, column("exposure"), **kw)
        return ops.hdr_merge_ingest_batches(frames, d.stages, column("exposure"), **kw)

    def launch_plain(k0, **args):
        return ops.hdr_merge_batches(column("images"), column("exposure"), stds=column("std"), std_mode=k0["std_mode"],
                                     std_value=k0["std_value"], max_code=k0["max_code"], tile=tile, layout=k0["layout"],
                                     out_layout=k0["out_layout"], **args)

    while pending is not None:
        index_batch, val_batch, std_batch, meta_batch = pending
        pending = next(batches, None)
        last = pending is None
        planar = std_batch is not None or dark is not None  # explicit std / dark images are planar
        defer = fused_ingest if dark is None else (fused_dark and fused_dark_ingest)
        images, max_code, layout = stage_images(val_batch, dev, transforms, planar, defer_ingest=defer,
                                                step_in_kernel=dark is None and fused_downscale)
        std, std_mode, std_value = std_arguments(std_batch, dataloader.dataset, dev)
        exposure = meta_batch["exposure_time"]
        fused = isinstance(images, DeferredIngest)
        matched, asked = None, False
        if fused and dark is not None:
            matched, asked = dark.match(index_batch, std, std_mode), True
            if matched is not None and dark.fuses_with_merge_ingest(images, interp, reference_order, tile):
                # queued under a key of its own; the halo rows are exchanged now, on the RAW frames, in loader order on every rank
                halo = exchange_halo(images.frames, tile, group) if images.layout == "nchw" else None
                key = ("dark_ingest", images.frames.dtype, tuple(images.frames.shape[1:]), images.layout, images.stages, std_mode,
                       std_value, std is None, images.consts is None)
                enqueue(_QueueKind(key, dark_batches_per_launch, _dark_batch_bytes(images.frames, std, matched, halo),
                                   ops.ingest_shape(tuple(images.frames.shape), images.layout)[1:], True, launch_dark_ingest),
                        images=images, exposure=exposure, std=std, std_mode=std_mode, std_value=std_value, matched=matched, halo=halo)
                continue
            if matched is not None:  # declined: the float32 stack, then as without the keyword
                images = images.materialise()
                fused = False
        if fused and (images.frames.dtype == torch.float32 or reference_order is True or
                      (interp in ("lookup", "catmull") and std_mode != "none" and reference_order is None)):
            # float32 frames have no copy to save, and the reference-order kernel is not fused: they get the float32 stack
            images = images.materialise()
            fused = False
        if dark is not None:
            if not asked:
                matched = dark.match(index_batch, std, std_mode)
            fuses = matched is not None and fused_dark and dark.fuses_with_merge(images, layout, interp, reference_order)
            if fuses and dark_batches_per_launch > 1:
                # queued under a key of its own; the halo rows are exchanged now, in loader order on every rank
                halo = exchange_halo(images, tile, group)
                key = ("dark", images.dtype, tuple(images.shape[1:]), max_code, std_mode, std_value, std is None)
                enqueue(_QueueKind(key, dark_batches_per_launch, _dark_batch_bytes(images, std, matched, halo), tuple(images.shape[1:]), True,
                                   launch_dark),
                        images=images, exposure=exposure, std=std, std_mode=std_mode, std_value=std_value, max_code=max_code,
                        matched=matched, halo=halo)
                continue
            if fuses:
                # blur and merge in one pass over the staged images (ct_hdr_merge_dark_batch), on the state the queued
                # batches leave: they are merged first
                flush(False)
                result = dark.merge(matched, images, exposure, max_code, std, std_mode, std_value, tile, group,
                                    **merge_args(tuple(images.shape[1:]), True, last))
                continue
            if matched is not None:  # the blurred batch replaces the images; its uncertainty carries both variance terms
                xb, sig = dark.apply(index_batch, images, max_code, std, std_mode, std_value, tile, group, matched=matched)
                images, max_code, std, std_mode, std_value = xb, None, sig, "explicit", 0.0
        if fused:  # one dtype, shape, layout and chain per call; every batch with constants of its own, or none
            key = ("ingest", images.frames.dtype, tuple(images.frames.shape[1:]), images.layout, images.stages, std_mode, std_value,
                   std is None, images.consts is None, images.step)
            chw = ops.downscaled_shape(ops.ingest_shape(tuple(images.frames.shape), images.layout), images.step)[1:]
            enqueue(_QueueKind(key, ops.MAX_MERGE_BATCHES, 0, chw, std_mode != "none", launch_ingest),
                    images=images, exposure=exposure, std=std, std_mode=std_mode, std_value=std_value)
        else:
            key = (images.dtype, tuple(images.shape[1:]), max_code, layout, std_mode, std_value, std is None)
            out_layout = "input" if (output_layout == "input" and layout != "nchw") else "planar"
            chw = tuple(images.shape[1:]) if (layout == "nchw" or out_layout == "input") else \
                (images.shape[3], images.shape[1], images.shape[2])
            enqueue(_QueueKind(key, ops.MAX_MERGE_BATCHES, 0, chw, std_mode != "none", launch_plain),
                    images=images, exposure=exposure, std=std, std_mode=std_mode, std_value=std_value, max_code=max_code, layout=layout,
                    out_layout=out_layout)
    if flat_field_dataset is not None:
        mean, std = _flat_field_epilogue(state, flat_field_dataset, dataloader.dataset, dev, tile, group)
    else:
        mean, std = result
        mean, std = mean.squeeze(), (std.squeeze() if std is not None else None)
    if output_layout == "cv":
        mean, std = _export_cv(mean), (_export_cv(std) if std is not None else None)
    return mean, std


def _export_cv(planar):
    """The squeezed planar result in OpenCV order; squeezed to fewer than two axes (a 1-pixel-high image) it has no
    channel axis left to move and stays as it is."""
    return ops.export_cv(planar.contiguous()) if planar.ndim in (2, 3) else planar


def _flat_field_epilogue(state, flat_field_dataset, main_dataset, dev, tile, group):
    """hdr_merge.py:131-153 on the device-resident merged state."""
    import torch.distributed as dist
    _, flat, flat_std, _ = flat_field_dataset.get_matching_artefact_images([main_dataset.files[0]])
    if flat_std is None:
        # the reference dereferences the std unconditionally (hdr_merge.py:134)
        raise AttributeError("'NoneType' object has no attribute 'to'")
    if state.var is None:
        # hdr_merge.py:151: running_variance is None without image uncertainties
        raise TypeError("unsupported operand type(s) for +: 'NoneType' and 'Tensor'")
    flat, flat_std = flat.to(dev), flat_std.to(dev)
    c, h, w = state.mean.shape
    reduce = global_px = None
    if tile is not None:
        global_px = tile.h_global * w
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            reduce = lambda t: dist.all_reduce(t, group=group)  # noqa: E731
    mean, std = ops.flatfield_correct(state.mean, state.var, flat, flat_std, input_is_variance=True, through_mean=True,
                                      global_pixels=global_px, reduce=reduce)
    return mean.squeeze(), std.squeeze()
