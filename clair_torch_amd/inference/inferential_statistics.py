"""compute_video_mean_and_std with the reference's signature (clair_torch/inference/inferential_statistics.py:19-49).

Every batch of frames is one launch of ct_video_stats_batch (optional ICRF linearization fused with the unweighted
WBOMeanVar update) or, behind a general gpu_transforms chain on raw codes, of ct_video_stats_ingest_batch (the chain as
well); the running mean and m2 stay on the device.  ``batches_per_launch`` above 1 hands up to 16 consecutive batches to
one launch (ct_video_stats_batches / ct_video_stats_ingest_batches), the state in registers in between.
"""
import math
from typing import Optional

import torch
from torch.utils.data import DataLoader

from .. import ops
from .._native import STATS_MAX_BATCHES
from ..common.typecheck import expect
from ..models.base import ICRFModelBase
from ._staging import DeferredIngest, normalise_transform_list, resolve_device, stage_images


def compute_video_mean_and_std(dataloader: DataLoader, device, icrf_model: Optional[ICRFModelBase] = None,
                               gpu_transforms=None, fused_ingest: bool = True, batches_per_launch: int = 1):
    """Mean and standard deviation of the mean over all frames served by ``dataloader``; returns float32
    ``(mean, std)`` squeezed like the reference.  ``gpu_transforms`` (extension): raw integer frames with
    [CastTo('float32'), Normalize(max, 0)] are normalised inside the kernel.
    ``fused_ingest`` (extension): a ``gpu_transforms`` list on route "ingest" / "ingest_data" (common/transforms.py: a black
    level, a clamp, a target range, a data-dependent Normalize on raw uint8 / uint16 codes) is evaluated inside the
    statistics kernel (ct_video_stats_ingest_batch: one launch per batch, no float32 copy of the batch); False =
    ct_ingest_transform, then the float32 ct_video_stats_batch.  The results are the same bit for bit.  Measured on
    32 x 1080p batches (profiles/video_ingest_timing.json) the fused launch takes 0.50 of the pair's time on planar frames
    and 0.95 (uint16) / 0.90 (uint8) on raw (H,W,3) frames behind CvToTorch.  A data-dependent Normalize takes the extrema
    of each batch, as the reference's loop over ``gpu_transforms`` does.
    ``batches_per_launch`` (extension, 1 .. 16): with a value above 1, consecutive staged batches are queued on the device
    and handed over together (``ops.video_stats_batches`` / ``ops.video_stats_ingest_batches``): one launch walks up to that
    many batches with the running (mean, m2) in registers in between instead of reading and writing 16 B of state per
    element after every batch -- at the reference's ``batch_size: 4`` the larger part of what a launch per batch moves.  The
    results are the same bit for bit.  The queue holds up to ``batches_per_launch`` staged batches in device memory at a time
    (the raw frames; the float32 stacks where a chain is not fused); it is flushed when full, when dtype, frame shape, layout,
    chain, ``max_code`` or the presence of constants change, and at the end.  The zero-range error of a data-dependent
    Normalize is still raised per batch, when the batch is staged.  Measured on 64 batches of 4 x 1080p frames
    (profiles/video_batches.md), 16 batches per launch take 0.53 (uint8) / 0.72 (uint16) of the time of one launch per batch on
    planar codes, 0.36 / 0.44 on raw (H,W,3) codes, 0.68 / 0.90 behind a fused chain on planar frames and 0.63 behind one on raw
    uint16 frames -- but 1.07 behind a fused chain on raw uint8 (H,W,3) frames, which is why the default stays 1: one launch
    per batch, as before."""
    expect(dataloader, DataLoader, "dataloader")
    expect(device, (str, torch.device), "device")
    expect(icrf_model, ICRFModelBase, "icrf_model", allow_none=True)
    if isinstance(batches_per_launch, bool) or not isinstance(batches_per_launch, int) or not 1 <= batches_per_launch <= STATS_MAX_BATCHES:
        raise ValueError(f"batches_per_launch must be an int in 1 .. {STATS_MAX_BATCHES}, got {batches_per_launch!r}")
    dev = resolve_device(device)
    transforms = normalise_transform_list(gpu_transforms)
    lut = interp = None
    if icrf_model is not None:
        lut, interp = icrf_model.icrf.detach().to(dev), icrf_model.interp_name
    mean = m2 = None
    n_frames = 0
    queue, queue_key = [], None  # batches_per_launch > 1: staged batches that wait for their launch

    def flush():
        nonlocal n_frames, queue
        if not queue:
            return
        k0 = queue[0]
        if isinstance(k0, DeferredIngest):  # the chain and the statistics of every queued batch in one launch
            consts = None if k0.consts is None else [q.consts for q in queue]
            ops.video_stats_ingest_batches([q.frames for q in queue], k0.stages, mean, m2, n_frames, lut=lut, interp=interp,
                                           layout=k0.layout, consts=consts)
            n_frames += sum(q.frames.shape[0] for q in queue)
        else:
            ops.video_stats_batches([q[0] for q in queue], mean, m2, n_frames, lut=lut, interp=interp, max_code=k0[1], layout=k0[2])
            n_frames += sum(q[0].shape[0] for q in queue)
        queue = []

    def enqueue(key, staged):
        nonlocal queue_key
        if queue and key != queue_key:
            flush()
        queue_key = key
        queue.append(staged)
        if len(queue) == batches_per_launch:
            flush()

    for _, val_batch, _std_batch, _meta in dataloader:
        frames, max_code, layout = stage_images(val_batch, dev, transforms, defer_ingest=fused_ingest)
        if isinstance(frames, DeferredIngest):
            d = frames
            if d.frames.dtype == torch.float32:  # float32 frames have no copy to save: they get the float32 stack
                frames = ops.ingest_transform(d.frames, d.stages, layout=d.layout, consts=d.consts)
            else:  # the chain and the statistics in one launch
                if mean is None:
                    mean = torch.empty(ops.ingest_shape(tuple(d.frames.shape), d.layout)[1:], dtype=torch.float32, device=dev)
                    m2 = torch.empty_like(mean)
                if batches_per_launch > 1:
                    key = ("ingest", d.frames.dtype, tuple(d.frames.shape[1:]), d.layout, d.stages, d.consts is None)
                    enqueue(key, d)
                    continue
                ops.video_stats_ingest_batch(d.frames, d.stages, mean, m2, n_frames, lut=lut, interp=interp, layout=d.layout,
                                             consts=d.consts)
                n_frames += d.frames.shape[0]
                continue
        if mean is None:
            f = frames.shape  # interleaved frames as decoded (CvToTorch folded into the kernel): the state is planar
            chw = tuple(f[1:]) if layout == "nchw" else (f[3], f[1], f[2])
            mean = torch.empty(chw, dtype=torch.float32, device=dev)
            m2 = torch.empty_like(mean)
        if batches_per_launch > 1:
            key = (frames.dtype, tuple(frames.shape[1:]), layout, max_code)
            enqueue(key, (frames, max_code, layout))
            continue
        ops.video_stats_batch(frames, mean, m2, n_frames, lut=lut, interp=interp, max_code=max_code, layout=layout)
        n_frames += frames.shape[0]
    flush()
    if mean is None:
        raise ValueError("dataloader yielded no batches")
    variance = m2 * (1 / (n_frames - 1)) if n_frames > 1 else m2 * float("inf")  # SAMPLE_FREQUENCY scale
    return mean.squeeze(), torch.sqrt(variance.squeeze()) / math.sqrt(n_frames)
