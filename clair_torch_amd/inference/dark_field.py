"""Dark-field correction of a batch before merging / linearizing (PARITY UNPINNED, see
csrc/ct_darkfield.hip).

The reference applies conditional_gaussian_blur with the batch's matched dark fields right after the device transforms
(clair_torch/inference/hdr_merge.py:76-92, linearization.py:73-92) and later adds the dark field's variance term by a
second autograd.grad (hdr_merge.py:117-126, linearization.py:108-116).  Here one kernel (ct_dark_field_blur) produces the
blurred batch and a per-sample uncertainty that carries both variance terms; the merge / linearize kernels then run
unchanged on (float32 pixels, explicit uncertainty).  In compute_hdr_image a matched batch in a closed-form mode can
instead take ct_hdr_merge_dark_batch, which forms both per sample in registers and merges them in the same pass
(``DarkField.fuses_with_merge`` / ``merge``; bit-identical to the pair), and several consecutive such batches can share one
launch (``merge_batches``, ct_hdr_merge_dark_batches; bit-identical to the launches it replaces).  linearize_dataset_generator does the same for its
frames: where ``DarkField.fuses_with_linearize`` says so, the streamed pipeline hands each run of matched frames of a group to
ct_linearize_dark (blur and ICRF in one pass, bit-identical to the pair) with the matched dark fields uploaded once and kept in
a small device cache (``device_pair``).

Row bands: the 3x3 blur needs the rows just above and below a band.  ``exchange_halo`` gets them from the neighbouring
ranks (one send / receive pair per side over torch.distributed; 2 rows of B x C x W elements, latency-bound on xGMI).
"""
from collections import OrderedDict
from typing import Optional

import torch
import torch.distributed as dist

from .. import ops


def exchange_halo(images: torch.Tensor, tile: Optional[ops.TileGeometry], group=None) -> Optional[torch.Tensor]:
    """(B, C, 2, W) rows [above, below] of this rank's band, from the ranks holding them; None for an untiled image.
    Bands are assumed stacked in rank order (rank r holds the rows right below rank r - 1), as bench.py / C5 lay them out."""
    if tile is None:
        return None
    b, c, h, w = images.shape
    halo = torch.zeros((b, c, 2, w), dtype=images.dtype, device=images.device)
    has_up, has_down = tile.row_offset > 0, tile.row_offset + h < tile.h_global
    if not (has_up or has_down):
        return halo
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("a row band that does not span the image needs its neighbours' rows: initialise "
                           "torch.distributed (one rank per band) or pass the whole image")
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    peers = dist.get_process_group_ranks(group) if group is not None else list(range(world))
    first_row, last_row = images[:, :, 0].contiguous(), images[:, :, h - 1].contiguous()
    up_buf = torch.empty_like(first_row) if has_up else None
    down_buf = torch.empty_like(last_row) if has_down else None
    ops_list = []
    if has_up:
        ops_list += [dist.P2POp(dist.isend, first_row, peers[rank - 1], group), dist.P2POp(dist.irecv, up_buf, peers[rank - 1], group)]
    if has_down:
        ops_list += [dist.P2POp(dist.isend, last_row, peers[rank + 1], group), dist.P2POp(dist.irecv, down_buf, peers[rank + 1], group)]
    for req in dist.batch_isend_irecv(ops_list):
        req.wait()
    if has_up:
        halo[:, :, 0] = up_buf
    if has_down:
        halo[:, :, 1] = down_buf
    return halo


class DarkField:
    """The dark-field dataset of one compute_hdr_image / linearize_dataset_generator call."""

    CACHE_PAIRS = 4  # matched (dark, dark std) pairs kept on the device by ``device_pair``

    def __init__(self, dataset, main_dataset, device):
        self.dataset, self.main_dataset, self.device = dataset, main_dataset, device
        self._cache = OrderedDict()  # cache_key -> (host dark, host std, device dark, device std), least recently used first

    @classmethod
    def from_dataset(cls, dataset, main_dataset, device):
        return cls(dataset, main_dataset, device)

    def match(self, index_batch, std, std_mode):
        """-> (dark, dark std) of the dark fields matched to this batch, or None when none matches
        (MissingValMode.SKIP_BATCH: the reference then leaves the batch uncorrected, hdr_merge.py:84).

        Error behaviour follows the reference: the dark std is dereferenced unconditionally (AttributeError without it),
        and with a dark std but no image uncertainties autograd finds no path to the dark field (RuntimeError)."""
        frames = [self.main_dataset.files[int(i)] for i in index_batch]
        _, dark, dark_std, _ = self.dataset.get_matching_artefact_images(frames)
        if dark is None:
            return None
        if dark_std is None:
            raise AttributeError("'NoneType' object has no attribute 'to'")  # hdr_merge.py:87 / linearization.py:86
        if std is None and std_mode == "none":
            # hdr_merge.py:97-99,118: the ICRF runs under set_grad_enabled(stds is not None), so nothing connects the
            # running average to dark_field_val
            raise RuntimeError("element 0 of tensors does not require grad and does not have a grad_fn")
        return dark, dark_std

    @staticmethod
    def fuses_with_merge(images, layout, interp, reference_order) -> bool:
        """The route decision of a matched batch in compute_hdr_image: True = ct_hdr_merge_dark_batch (blur and merge in one
        pass over the staged images), False = ct_dark_field_blur into float32 stacks, then the float32 merge.  Fused are
        planar codes or float32 pixels in a closed-form mode -- the rule of the fused ingest: the reference-order kernel
        (``reference_order=True``, and LOOKUP / CATMULL by default: a matched batch always carries uncertainties) is not
        fused."""
        if not isinstance(images, torch.Tensor) or layout != "nchw" or images.ndim != 4:
            return False
        if images.dtype not in (torch.uint8, torch.uint16, torch.float32):
            return False
        return not (reference_order is True or (interp in ("lookup", "catmull") and reference_order is None))

    @staticmethod
    def fuses_with_merge_ingest(deferred, interp, reference_order, tile=None) -> bool:
        """The route decision of a matched batch whose chain has not been executed (a ``DeferredIngest`` of routes "ingest" /
        "ingest_data", ``compute_hdr_image(fused_dark_ingest=True)``): True = ct_hdr_merge_dark_ingest_batches (chain, blur and
        merge in one pass over the raw frames), False = ``ops.ingest_transform`` into the float32 stack, then what
        ``fuses_with_merge`` decides for that.  Fused are 4-D uint8 / uint16 / float32 frames, planar or -- without a row band
        (``tile`` None or the whole image) -- interleaved (H,W,3), in a closed-form mode (``fuses_with_merge``'s rule: not
        ``reference_order=True``, and LOOKUP / CATMULL only with ``reference_order=False``)."""
        frames = getattr(deferred, "frames", None)
        if not isinstance(frames, torch.Tensor) or frames.ndim != 4 or deferred.layout not in ("nchw", "nhwc", "nhwc_bgr"):
            return False
        if frames.dtype not in (torch.uint8, torch.uint16, torch.float32):
            return False
        if deferred.layout != "nchw":
            if frames.shape[3] != 3:
                return False
            if tile is not None and (tile.row_offset != 0 or tile.h_global != frames.shape[1]):
                return False
        return not (reference_order is True or (interp in ("lookup", "catmull") and reference_order is None))

    @staticmethod
    def fuses_with_linearize(images_or_probe, plan, interp) -> bool:
        """The route decision of linearize_dataset_generator with a dark-field dataset: True = the streamed pipeline with
        ct_linearize_dark on the matched frames (blur and ICRF in one pass over the slot's raw frames), False = frame by
        frame through ct_dark_field_blur and ct_linearize_std.  ``images_or_probe``: the first value batch (shape and dtype
        only: a CPU tensor will do); ``plan``: its ``plan_staging`` plan with ``planar=True``.  Fused are planar 4-D frames
        on route "code" without a StridedDownscale (raw uint8 / uint16 codes and their max_code) and float32 pixels with no
        transform list.  LOOKUP (no gradient path: the frame-by-frame route raises at the first matched frame), routes
        "ingest", "ingest_data" and "torch" with transforms, and any StridedDownscale stay frame by frame."""
        t = images_or_probe
        if not isinstance(t, torch.Tensor) or t.ndim != 4 or interp not in ("linear", "catmull"):
            return False
        if plan.route == "code":
            return plan.step == 1 and plan.layout == "nchw" and t.dtype in (torch.uint8, torch.uint16)
        return plan.route == "torch" and plan.no_transforms and t.dtype == torch.float32

    @staticmethod
    def fuses_with_linearize_ingest(probe, plan, interp) -> bool:
        """The second route decision of linearize_dataset_generator with a dark-field dataset, asked for what
        ``fuses_with_linearize`` declined (``fused_dark_ingest``): True = the streamed pipeline with ct_linearize_dark_ingest on
        the matched frames (chain, blur and ICRF in one pass over the slot's raw frames).  ``probe`` and ``plan`` as above.
        Fused are 4-D uint8 / uint16 / float32 frames on route "ingest" -- a black level, a target range, ``ClampAlongDims``,
        raw (H,W,3) BGR frames behind a leading ``CvToTorch`` -- without a StridedDownscale, LINEAR / CATMULL.  A
        data-dependent Normalize (route "ingest_data"), a StridedDownscale, LOOKUP and lists that run as torch ops stay frame
        by frame."""
        t = probe
        if not isinstance(t, torch.Tensor) or t.ndim != 4 or interp not in ("linear", "catmull"):
            return False
        if plan.route != "ingest" or plan.step != 1:
            return False
        return t.dtype in (torch.uint8, torch.uint16, torch.float32) and plan.source_layout in ("nchw", "nhwc_bgr")

    @staticmethod
    def fuses_with_linearize_ingest_data(probe, plan, interp) -> bool:
        """The third route decision of linearize_dataset_generator with a dark-field dataset, asked for what the two above
        declined (``fused_dark_ingest_data``): True = the streamed pipeline with ct_ingest_extrema_frames once per group and
        ct_linearize_dark_ingest_data on the matched frames (the chain with the frame's own constants, blur and ICRF in one pass
        over the slot's raw frames).  ``probe``: as above; ``plan``: its ``plan_staging`` plan with ``planar=True`` and
        ``on_device=True`` (route "ingest_data" exists only there).  Fused are 4-D uint8 / uint16 / float32 frames on route
        "ingest_data" -- the fused-ingest grammar with ONE data-dependent Normalize, ``Normalize()`` above all; planar frames or
        raw (H,W,3) BGR frames behind a leading ``CvToTorch`` -- without a StridedDownscale on either side of that Normalize
        (the blur would run on the compacted image: another window walk), LINEAR / CATMULL.  Constant chains (the two
        decisions above), LOOKUP and lists that run as torch ops are declined."""
        t = probe
        if not isinstance(t, torch.Tensor) or t.ndim != 4 or interp not in ("linear", "catmull"):
            return False
        if plan.route != "ingest_data" or plan.step != 1:
            return False
        return t.dtype in (torch.uint8, torch.uint16, torch.float32) and plan.source_layout in ("nchw", "nhwc_bgr")

    @staticmethod
    def cache_key(dark, dark_std):
        """What identifies the contents of a matched host pair: address, in-place version counter, shape and dtype of both
        (an in-place edit bumps ``_version``; the cache holds the host tensors, so an address is not re-used while its
        entry lives)."""
        return tuple((t.data_ptr(), t._version, tuple(t.shape), t.dtype) for t in (dark, dark_std))

    def device_pair(self, dark, dark_std):
        """-> (dark, dark std) of ``match`` as contiguous float32 device tensors, uploaded on the CURRENT stream (the
        pipeline's copy stream) the first time a pair is seen and kept for the next frames: get_matching_artefact_images
        usually hands the same host tensors back for many frames, and 8 B per element per frame would triple the copy-in.
        At most CACHE_PAIRS pairs are kept, the least recently used one goes first; the caller keeps what it got alive for
        as long as queued work reads it (the pipeline: in the group's in_flight record)."""
        key = self.cache_key(dark, dark_std)
        entry = self._cache.get(key)
        if entry is None:
            dev_pair = tuple(t.to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous() for t in (dark, dark_std))
            entry = (dark, dark_std) + dev_pair
            self._cache[key] = entry
            while len(self._cache) > self.CACHE_PAIRS:
                self._cache.popitem(last=False)
        else:
            self._cache.move_to_end(key)
        return entry[2], entry[3]

    def apply(self, index_batch, images, max_code, std, std_mode, std_value, tile=None, group=None, matched=None):
        """-> (blurred float32 batch, explicit per-sample uncertainty | None), or (None, None) when no dark field matches
        this batch.  ``matched``: what ``match`` returned for it, where the caller has asked already."""
        if matched is None:
            matched = self.match(index_batch, std, std_mode)
        if matched is None:
            return None, None
        dark, dark_std = matched
        halo = exchange_halo(images, tile, group)
        return ops.dark_field_blur(images, dark, dark_std, std=std, std_mode=std_mode, std_value=std_value,
                                   max_code=max_code, tile=tile, halo=halo)

    def merge(self, matched, images, exposures, max_code, std, std_mode, std_value, tile=None, group=None, **merge_args):
        """The matched batch through ct_hdr_merge_dark_batch: what ``apply`` and ``ops.hdr_merge_batch`` on its two stacks
        give, bit for bit.  ``merge_args``: lut, interp, gaussian_weight, state, finalize, reference_order."""
        dark, dark_std = matched
        halo = exchange_halo(images, tile, group)
        return ops.hdr_merge_dark_batch(images, exposures, dark, dark_std, std=std, std_mode=std_mode, std_value=std_value,
                                        max_code=max_code, tile=tile, halo=halo, **merge_args)

    @staticmethod
    def merge_batches(matched, images, exposures, max_code, stds, std_mode, std_value, tile=None, halos=None, **merge_args):
        """Several consecutive matched batches through ct_hdr_merge_dark_batches: what ``merge`` on each of them in turn gives,
        bit for bit, in one launch.  Lists, one entry per batch: ``matched`` (what ``match`` returned), ``images``,
        ``exposures``, ``stds`` (or None) and ``halos`` -- the rows ``exchange_halo`` got for each batch when it was queued,
        so that every rank issues its sends and receives in loader order (None for an untiled image).  ``merge_args``: lut,
        interp, gaussian_weight, state, finalize, reference_order."""
        return ops.hdr_merge_dark_batches(images, exposures, [m[0] for m in matched], [m[1] for m in matched], stds=stds,
                                          std_mode=std_mode, std_value=std_value, max_code=max_code, tile=tile, halos=halos,
                                          **merge_args)

    @staticmethod
    def merge_ingest_batches(matched, deferred, exposures, stds, std_mode, std_value, tile=None, halos=None, **merge_args):
        """Several consecutive matched batches whose chain has not been executed through ct_hdr_merge_dark_ingest_batches: what
        ``ops.ingest_transform`` and ``merge`` on each of them in turn give, bit for bit, in one launch over the raw frames.
        Lists, one entry per batch: ``matched``, ``deferred`` (``DeferredIngest`` of one chain and layout), ``exposures``,
        ``stds`` (or None) and ``halos`` -- the RAW rows ``exchange_halo`` got for each batch's frames when it was queued (None
        for an untiled image).  ``merge_args``: lut, interp, gaussian_weight, state, finalize, reference_order."""
        d0 = deferred[0]
        consts = None if d0.consts is None else [d.consts for d in deferred]
        return ops.hdr_merge_dark_ingest_batches([d.frames for d in deferred], d0.stages, exposures, [m[0] for m in matched],
                                                 [m[1] for m in matched], consts=consts, stds=stds, std_mode=std_mode,
                                                 std_value=std_value, tile=tile, halos=halos, layout=d0.layout, **merge_args)

    def linearize(self, index_batch, images, max_code, std, std_mode, std_value, lut, interp):
        xb, sig = self.apply(index_batch, images, max_code, std, std_mode, std_value)
        if xb is None:
            return ops.linearize_frames(images, lut, interp, std=std, std_mode=std_mode, std_value=std_value,
                                        max_code=max_code, want_std=True)
        return ops.linearize_frames(xb, lut, interp, std=sig, want_std=True)
