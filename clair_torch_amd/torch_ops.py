"""The C-ABI entry points as ``torch.library`` custom ops (namespace ``clair_hip``), SURVEY 8(b).

``clair_torch_amd.ops`` (ctypes) stays the implementation; this module registers the same kernels with PyTorch's
dispatcher so that they are visible as ``torch.ops.clair_hip.*``, carry schemas and fake (meta) implementations -- i.e.
they trace under FakeTensorMode / torch.compile and export -- and, for the ICRF sampler, an autograd formula that calls
the backward kernel.  Tensor-only signatures (optional tensors, ints, floats, strings): the streaming state, geometry
and pair lists are passed as their component tensors / scalars.

    torch.ops.clair_hip.icrf_forward(image, lut, interp, h_global, row_offset) -> Tensor      (differentiable)
    torch.ops.clair_hip.icrf_backward(image, grad_out, lut, interp, need_image, need_lut, h_global, row_offset)
    torch.ops.clair_hip.hdr_merge(stack, exposures, lut?, interp, gaussian, std?, std_mode, std_value, max_code,
                                  h_global, row_offset, layout) -> (mean float64, std float32)
    torch.ops.clair_hip.linearize_std(frames, lut, interp, std?, std_mode, std_value, max_code, layout) -> (lin, std)
    torch.ops.clair_hip.pair_residual_sums(stack, i_idx, j_idx, ratio, lut?, interp, lower, upper, relative,
                                           unc_weight, std_mode, std_value, max_code, level) -> (P, C, 5) float64
    torch.ops.clair_hip.pair_residual_lut_grad(stack, i_idx, j_idx, ratio, coef, lut, interp, lower, upper, relative,
                                               max_code) -> (C, L) float64
    torch.ops.clair_hip.pair_residual_ingest_sums(frames, stages, i_idx, j_idx, ratio, lut?, interp, lower, upper, relative,
                                  unc_weight, std?, std_mode, std_value, level, layout, consts?) -> (P, C, 5) float64
    torch.ops.clair_hip.pair_residual_ingest_lut_grad(frames, stages, i_idx, j_idx, ratio, coef, lut, interp, lower, upper,
                                  relative, layout, consts?) -> (C, L) float64   (a chain -- stages flattened as for
                                  ingest_transform -- and the two pair ops above in one pass over raw uint8 / uint16 frames)

    torch.ops.clair_hip.strided_downscale(stack, step, layout) -> Tensor   (x[..., ::step, ::step], same dtype / layout)
    torch.ops.clair_hip.export_cv(x, to_f64) -> Tensor   (planar result -> the (H,W,C) BGR array save_image writes)
    torch.ops.clair_hip.ingest_transform(stack, stages, layout) -> Tensor   (CastTo / Normalize / ClampAlongDims chain in
                                  one pass; stages = 13 floats each: kind, sub, div, mul, add, lo[0..3], hi[0..3])
    torch.ops.clair_hip.linearize_ingest(frames, stages, lut, interp, std?, std_mode, std_value, layout, h_global,
                                  row_offset) -> (lin, std)   (such a chain and linearize_std in one pass; stages flattened
                                  likewise; an explicit std is planar (F,C,H,W) like the outputs)
    torch.ops.clair_hip.ingest_extrema(stack, prefix, layout, min_val?, max_val?) -> Tensor   (4 floats: sub, div, data
                                  min, data max of a data-dependent Normalize behind the constant ``prefix`` stages)
    torch.ops.clair_hip.ingest_extrema_frames(frames, prefix, layout, min_val?, max_val?) -> Tensor   ((F, 4): row f is
                                  ingest_extrema of frame f alone, in two launches for the whole stack)
    torch.ops.clair_hip.linearize_ingest_data(frames, stages, consts, lut, interp, std?, std_mode, std_value, layout,
                                  h_global, row_offset) -> (lin, std)   (linearize_ingest whose chain may hold one stage of
                                  kind 2, the data-dependent Normalize with per-frame sub / div = consts[f, 0:2])
    torch.ops.clair_hip.flatfield_mean(flat) -> Tensor   ((C,) float32 spatial mean of a (C,H,W) flat field)
    torch.ops.clair_hip.linearize_std_flat(frames, lut, interp, std?, std_mode, std_value, max_code, flat, flat_std?,
                                  flat_mean, layout) -> (lin, std)
    torch.ops.clair_hip.linearize_ingest_flat(frames, stages, lut, interp, std?, std_mode, std_value, flat, flat_std?,
                                  flat_mean, layout, h_global, row_offset, consts?) -> (lin, std)
    torch.ops.clair_hip.linearize_ingest_strided_flat(frames, step, stages, lut, interp, std?, std_mode, std_value, flat,
                                  flat_std?, flat_mean, layout, consts?) -> (lin, std)   (linearize_std, linearize_ingest /
                                  _data and linearize_ingest_strided with the linearization's flat-field correction -- the
                                  mean a constant, ``flatfield_mean(flat)`` -- on every (lin, std) before it is stored; flat
                                  and flat_std are (C,H,W) float32 like a frame of the outputs)
    torch.ops.clair_hip.hdr_merge_ingest_batch(frames, stages, exposures, lut?, interp, gaussian, std?, std_mode, std_value,
                                  layout, h_global, row_offset, closed_form, consts?) -> (mean float64, std float32)   (such
                                  a chain and hdr_merge in one pass over the raw frames; with ``consts`` a stage of kind 2 is
                                  the data-dependent Normalize: kind, 0, 0, mul, add)
    torch.ops.clair_hip.hdr_merge_dark_ingest_batches(frames[], stages, exposures[], darks[], dark_stds[], consts[], stds[],
                                  lut?, interp, gaussian, std_mode, std_value, layout, closed_form) -> (mean float64,
                                  std float32)   (such a chain, the dark-field blur and 1 to 16 consecutive batches of one
                                  whole merge in one pass over the raw frames; lists hold one tensor per batch, the last
                                  three may be empty)
    torch.ops.clair_hip.hdr_merge_ingest_batches_strided(frames[], step, stages, exposures[], consts[], stds[], lut?, interp,
                                  gaussian, std_mode, std_value, layout, closed_form) -> (mean float64, std float32)
                                  (strided_downscale of every batch, such a chain and 1 to 16 consecutive batches of one
                                  whole merge in one pass over the raw full-size frames; results and explicit stds have the
                                  downscaled shape; the last two lists may be empty)
    torch.ops.clair_hip.hdr_merge_ingest_batch_strided(frames, step, stages, exposures, lut?, interp, gaussian, std?, std_mode,
                                  std_value, layout, closed_form, consts?) -> (mean float64, std float32)   (its single-batch form)

CPU tensors are refused by the kernels' front-end exactly as through ``ops`` (there is no CPU path).
"""
from typing import Optional, Sequence, Tuple

import torch

from . import ops

_LIB = "clair_hip"


def _tile(h_global: int, row_offset: int):
    return None if h_global <= 0 else ops.TileGeometry(h_global=h_global, row_offset=row_offset)


def _chw(t: torch.Tensor, layout: str):
    return (t.shape[1], t.shape[2], t.shape[3]) if layout == "nchw" else (t.shape[3], t.shape[1], t.shape[2])


@torch.library.custom_op(f"{_LIB}::icrf_forward", mutates_args=())
def icrf_forward(image: torch.Tensor, lut: torch.Tensor, interp: str, h_global: int = 0, row_offset: int = 0) -> torch.Tensor:
    return ops.icrf_forward(image, lut, interp, _tile(h_global, row_offset))


@icrf_forward.register_fake
def _(image, lut, interp, h_global=0, row_offset=0):
    return torch.empty_like(image, dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::icrf_backward", mutates_args=())
def icrf_backward(image: torch.Tensor, grad_out: torch.Tensor, lut: torch.Tensor, interp: str, need_image: bool,
                  need_lut: bool, h_global: int = 0, row_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    gx, gl = ops.icrf_backward(image, grad_out, lut, interp, need_image, need_lut, _tile(h_global, row_offset))
    return (gx if gx is not None else image.new_zeros(0), gl if gl is not None else lut.new_zeros(0))


@icrf_backward.register_fake
def _(image, grad_out, lut, interp, need_image, need_lut, h_global=0, row_offset=0):
    return (torch.empty_like(image) if need_image else image.new_empty(0),
            torch.empty_like(lut, dtype=torch.float32) if need_lut else lut.new_empty(0))


def _icrf_setup(ctx, inputs, output):
    image, lut, interp, h_global, row_offset = inputs
    ctx.save_for_backward(image, lut)
    ctx.meta = (interp, h_global, row_offset)


def _icrf_backward(ctx, grad_out):
    image, lut = ctx.saved_tensors
    interp, h_global, row_offset = ctx.meta
    need_image = ctx.needs_input_grad[0] and interp != "lookup"
    need_lut = ctx.needs_input_grad[1]
    gx, gl = icrf_backward(image, grad_out.contiguous(), lut, interp, need_image, need_lut, h_global, row_offset)
    return (gx if need_image else None), (gl if need_lut else None), None, None, None


icrf_forward.register_autograd(_icrf_backward, setup_context=_icrf_setup)


@torch.library.custom_op(f"{_LIB}::hdr_merge", mutates_args=())
def hdr_merge(stack: torch.Tensor, exposures: torch.Tensor, lut: Optional[torch.Tensor], interp: str, gaussian: bool,
              std: Optional[torch.Tensor], std_mode: str, std_value: float, max_code: float, h_global: int = 0,
              row_offset: int = 0, layout: str = "nchw") -> Tuple[torch.Tensor, torch.Tensor]:
    mean, sd = ops.hdr_merge_batch(stack, exposures, lut=lut, interp=interp if lut is not None else None,
                                   gaussian_weight=gaussian, std=std, std_mode=std_mode, std_value=std_value,
                                   max_code=max_code if max_code > 0 else None, tile=_tile(h_global, row_offset),
                                   layout=layout)
    return mean, (sd if sd is not None else mean.new_zeros(0, dtype=torch.float32))


@hdr_merge.register_fake
def _(stack, exposures, lut, interp, gaussian, std, std_mode, std_value, max_code, h_global=0, row_offset=0, layout="nchw"):
    chw = _chw(stack, layout)
    has_std = std is not None or std_mode != "none"
    return (stack.new_empty(chw, dtype=torch.float64),
            stack.new_empty(chw if has_std else (0,), dtype=torch.float32))


@torch.library.custom_op(f"{_LIB}::linearize_std", mutates_args=())
def linearize_std(frames: torch.Tensor, lut: torch.Tensor, interp: str, std: Optional[torch.Tensor], std_mode: str,
                  std_value: float, max_code: float, layout: str = "nchw") -> Tuple[torch.Tensor, torch.Tensor]:
    return ops.linearize_frames(frames, lut, interp, std=std, std_mode=std_mode, std_value=std_value,
                                max_code=max_code if max_code > 0 else None, want_std=True, layout=layout)


@linearize_std.register_fake
def _(frames, lut, interp, std, std_mode, std_value, max_code, layout="nchw"):
    shape = (frames.shape[0],) + tuple(_chw(frames, layout))
    return frames.new_empty(shape, dtype=torch.float32), frames.new_empty(shape, dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::pair_residual_sums", mutates_args=())
def pair_residual_sums(stack: torch.Tensor, i_idx: torch.Tensor, j_idx: torch.Tensor, ratio: torch.Tensor,
                       lut: Optional[torch.Tensor], interp: str, lower: float, upper: float, relative: bool,
                       unc_weight: bool, std_mode: str, std_value: float, max_code: float, level: int = 1) -> torch.Tensor:
    pairs = ops.PairList(i_idx, j_idx, ratio, stack.shape[0], stack.device)
    return ops.pair_residual_sums(stack, pairs, lut=lut, interp=interp if lut is not None else None, lower=lower,
                                  upper=upper, use_relative=relative, use_unc_weight=unc_weight, std_mode=std_mode,
                                  std_value=std_value, max_code=max_code if max_code > 0 else None, level=level)


@pair_residual_sums.register_fake
def _(stack, i_idx, j_idx, ratio, lut, interp, lower, upper, relative, unc_weight, std_mode, std_value, max_code, level=1):
    return stack.new_empty((i_idx.shape[0], stack.shape[1], 5), dtype=torch.float64)


@torch.library.custom_op(f"{_LIB}::pair_residual_lut_grad", mutates_args=())
def pair_residual_lut_grad(stack: torch.Tensor, i_idx: torch.Tensor, j_idx: torch.Tensor, ratio: torch.Tensor,
                           coef: torch.Tensor, lut: torch.Tensor, interp: str, lower: float, upper: float, relative: bool,
                           max_code: float) -> torch.Tensor:
    pairs = ops.PairList(i_idx, j_idx, ratio, stack.shape[0], stack.device)
    return ops.pair_residual_lut_grad(stack, pairs, coef, lut=lut, interp=interp, lower=lower, upper=upper,
                                      use_relative=relative, max_code=max_code if max_code > 0 else None)


@pair_residual_lut_grad.register_fake
def _(stack, i_idx, j_idx, ratio, coef, lut, interp, lower, upper, relative, max_code):
    return lut.new_empty(lut.shape, dtype=torch.float64)


@torch.library.custom_op(f"{_LIB}::pair_residual_ingest_sums", mutates_args=())
def pair_residual_ingest_sums(frames: torch.Tensor, stages: Sequence[float], i_idx: torch.Tensor, j_idx: torch.Tensor,
                              ratio: torch.Tensor, lut: Optional[torch.Tensor], interp: str, lower: float, upper: float,
                              relative: bool, unc_weight: bool, std: Optional[torch.Tensor], std_mode: str, std_value: float,
                              level: int = 1, layout: str = "nchw", consts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ct_pair_residual_ingest_fwd: ingest_transform followed by pair_residual_sums in one pass over the raw frames
    (stages flattened as for ``ingest_transform``; an explicit std is planar (N,C,H,W))."""
    pairs = ops.PairList(i_idx, j_idx, ratio, frames.shape[0], frames.device)
    return ops.pair_residual_ingest_sums(frames, _listed_ingest_stages(frames, stages, layout), pairs, lut=lut,
                                         interp=interp if lut is not None else None, lower=lower, upper=upper,
                                         use_relative=relative, use_unc_weight=unc_weight, consts=consts, std=std,
                                         std_mode=std_mode, std_value=std_value, level=level, layout=layout)


@pair_residual_ingest_sums.register_fake
def _(frames, stages, i_idx, j_idx, ratio, lut, interp, lower, upper, relative, unc_weight, std, std_mode, std_value, level=1,
      layout="nchw", consts=None):
    return frames.new_empty((i_idx.shape[0], ops.ingest_shape(tuple(frames.shape), layout)[1], 5), dtype=torch.float64)


@torch.library.custom_op(f"{_LIB}::pair_residual_ingest_lut_grad", mutates_args=())
def pair_residual_ingest_lut_grad(frames: torch.Tensor, stages: Sequence[float], i_idx: torch.Tensor, j_idx: torch.Tensor,
                                  ratio: torch.Tensor, coef: torch.Tensor, lut: torch.Tensor, interp: str, lower: float,
                                  upper: float, relative: bool, layout: str = "nchw",
                                  consts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ct_pair_residual_ingest_bwd: ingest_transform followed by pair_residual_lut_grad in one pass over the raw frames."""
    pairs = ops.PairList(i_idx, j_idx, ratio, frames.shape[0], frames.device)
    return ops.pair_residual_ingest_lut_grad(frames, _listed_ingest_stages(frames, stages, layout), pairs, coef, lut=lut,
                                             interp=interp, lower=lower, upper=upper, use_relative=relative, consts=consts,
                                             layout=layout)


@pair_residual_ingest_lut_grad.register_fake
def _(frames, stages, i_idx, j_idx, ratio, coef, lut, interp, lower, upper, relative, layout="nchw", consts=None):
    return lut.new_empty(lut.shape, dtype=torch.float64)


@torch.library.custom_op(f"{_LIB}::band_stats", mutates_args=())
def band_stats(mean: torch.Tensor, std: Optional[torch.Tensor]) -> torch.Tensor:
    """ct_band_stats: (6, C) float64 per-channel min / max / sum of a merged band's mean and std (configuration C5)."""
    return ops.band_stats(mean, std)


@band_stats.register_fake
def _(mean, std):
    return mean.new_empty((6, mean.shape[0]), dtype=torch.float64)



@torch.library.custom_op(f"{_LIB}::strided_downscale", mutates_args=())
def strided_downscale(stack: torch.Tensor, step: int, layout: str = "nchw") -> torch.Tensor:
    """ct_strided_downscale: every step-th row and column of a code / pixel stack, compacted in its dtype and layout."""
    out = ops.strided_downscale(stack, step, layout)
    return out.clone() if out is stack else out  # step 1: an op's result may not alias its input


@strided_downscale.register_fake
def _(stack, step, layout="nchw"):
    return stack.new_empty(ops.downscaled_shape(stack.shape, step, layout))


@torch.library.custom_op(f"{_LIB}::export_cv", mutates_args=())
def export_cv(x: torch.Tensor, to_f64: bool) -> torch.Tensor:
    """ct_export_cv: a planar (H,W) / (C,H,W) / (F,C,H,W) result in OpenCV order, float64 or float32."""
    return ops.export_cv(x, torch.float64 if to_f64 else torch.float32)


@export_cv.register_fake
def _(x, to_f64):
    return x.new_empty(ops.export_shape(tuple(x.shape)), dtype=torch.float64 if to_f64 else torch.float32)


_STAGE_FLOATS = 13  # kind (0 affine, 1 clamp, 2 affine_data: mul and add only), sub, div, mul, add, lo[0..3], hi[0..3]: ct_ingest_stage, flattened


def flatten_ingest_stages(stages, channels: int):
    """``ops.ingest_transform``'s stage list as the flat float list the custom op takes."""
    flat = []
    for st in stages:
        if st[0] == "affine":
            flat += [0.0] + [float(v) for v in st[1:5]] + [0.0] * 8
        elif st[0] == "affine_data":
            flat += [2.0, 0.0, 0.0, float(st[1]), float(st[2])] + [0.0] * 8
        else:
            pairs = list(st[1]) * (4 if len(st[1]) == 1 else 1)
            pairs += [pairs[-1]] * (4 - len(pairs))
            flat += [1.0] + [0.0] * 4 + [float(p[0]) for p in pairs[:4]] + [float(p[1]) for p in pairs[:4]]
    return flat


def _listed_ingest_stages(stack, stages, layout):
    if len(stages) % _STAGE_FLOATS != 0:
        raise ValueError(f"stages holds {_STAGE_FLOATS} floats per stage, got {len(stages)}")
    channels = ops.ingest_shape(tuple(stack.shape), layout)[1]
    listed = []
    for k in range(0, len(stages), _STAGE_FLOATS):
        kind, sub, div, mul, add = stages[k:k + 5]
        lo, hi = stages[k + 5:k + 9], stages[k + 9:k + 13]
        if kind == 0:
            listed.append(("affine", sub, div, mul, add))
        elif kind == 2:
            listed.append(("affine_data", mul, add))
        else:
            n = channels if channels <= 4 else 1
            listed.append(("clamp", [(lo[c], hi[c]) for c in range(n)]))
    return listed


@torch.library.custom_op(f"{_LIB}::ingest_transform", mutates_args=())
def ingest_transform(stack: torch.Tensor, stages: Sequence[float], layout: str = "nchw") -> torch.Tensor:
    """ct_ingest_transform: a CastTo(float32) / Normalize / ClampAlongDims chain in one pass, planar float32 result."""
    return ops.ingest_transform(stack, _listed_ingest_stages(stack, stages, layout), layout)


@ingest_transform.register_fake
def _(stack, stages, layout="nchw"):
    return stack.new_empty(ops.ingest_shape(tuple(stack.shape), layout), dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::linearize_ingest", mutates_args=())
def linearize_ingest(frames: torch.Tensor, stages: Sequence[float], lut: torch.Tensor, interp: str, std: Optional[torch.Tensor],
                     std_mode: str, std_value: float, layout: str = "nchw", h_global: int = 0,
                     row_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """ct_linearize_ingest: ingest_transform followed by linearize_std, bit for bit, in one pass over the raw frames."""
    return ops.linearize_ingest_frames(frames, _listed_ingest_stages(frames, stages, layout), lut, interp, std=std,
                                       std_mode=std_mode, std_value=std_value, want_std=True, tile=_tile(h_global, row_offset),
                                       layout=layout)


@linearize_ingest.register_fake
def _(frames, stages, lut, interp, std, std_mode, std_value, layout="nchw", h_global=0, row_offset=0):
    shape = ops.ingest_shape(tuple(frames.shape), layout)
    return frames.new_empty(shape, dtype=torch.float32), frames.new_empty(shape, dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::linearize_ingest_strided", mutates_args=())
def linearize_ingest_strided(frames: torch.Tensor, step: int, stages: Sequence[float], lut: torch.Tensor, interp: str,
                             std: Optional[torch.Tensor], std_mode: str, std_value: float, layout: str = "nchw",
                             consts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ct_linearize_ingest_strided: strided_downscale followed by linearize_ingest (with ``consts``: linearize_ingest_data),
    bit for bit, in one pass over the raw frames; an explicit std is planar and of the downscaled shape."""
    return ops.linearize_ingest_frames_strided(frames, step, _listed_ingest_stages(frames, stages, layout), lut, interp, std=std,
                                               std_mode=std_mode, std_value=std_value, want_std=True, layout=layout, consts=consts)


@linearize_ingest_strided.register_fake
def _(frames, step, stages, lut, interp, std, std_mode, std_value, layout="nchw", consts=None):
    shape = ops.downscaled_shape(ops.ingest_shape(tuple(frames.shape), layout), step)
    return frames.new_empty(shape, dtype=torch.float32), frames.new_empty(shape, dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::ingest_extrema", mutates_args=())
def ingest_extrema(stack: torch.Tensor, prefix: Sequence[float], layout: str = "nchw", min_val: Optional[float] = None,
                   max_val: Optional[float] = None) -> torch.Tensor:
    """ct_ingest_extrema: [sub, div, data min, data max] of a data-dependent Normalize behind the constant ``prefix``
    stages (flattened as for ``ingest_transform``); a bound that is None comes from the data."""
    return ops.ingest_extrema(stack, _listed_ingest_stages(stack, prefix, layout), layout, min_val, max_val)


@ingest_extrema.register_fake
def _(stack, prefix, layout="nchw", min_val=None, max_val=None):
    return stack.new_empty((4,), dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::ingest_extrema_frames", mutates_args=())
def ingest_extrema_frames(frames: torch.Tensor, prefix: Sequence[float], layout: str = "nchw", min_val: Optional[float] = None,
                          max_val: Optional[float] = None) -> torch.Tensor:
    """ct_ingest_extrema_frames: (F, 4), row f = [sub, div, data min, data max] of frame f alone behind the constant
    ``prefix`` stages (flattened as for ``ingest_transform``); a bound that is None comes from the data."""
    return ops.ingest_extrema_frames(frames, _listed_ingest_stages(frames, prefix, layout), layout, min_val, max_val)


@ingest_extrema_frames.register_fake
def _(frames, prefix, layout="nchw", min_val=None, max_val=None):
    return frames.new_empty((frames.shape[0], 4), dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::linearize_ingest_data", mutates_args=())
def linearize_ingest_data(frames: torch.Tensor, stages: Sequence[float], consts: torch.Tensor, lut: torch.Tensor, interp: str,
                          std: Optional[torch.Tensor], std_mode: str, std_value: float, layout: str = "nchw", h_global: int = 0,
                          row_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """ct_linearize_ingest_data: ``linearize_ingest`` with the per-frame constants of ``ingest_extrema_frames`` for one
    data-dependent Normalize in the chain (a stage of kind 2: kind, 0, 0, mul, add)."""
    return ops.linearize_ingest_frames(frames, _listed_ingest_stages(frames, stages, layout), lut, interp, std=std,
                                       std_mode=std_mode, std_value=std_value, want_std=True, tile=_tile(h_global, row_offset),
                                       layout=layout, consts=consts)


@linearize_ingest_data.register_fake
def _(frames, stages, consts, lut, interp, std, std_mode, std_value, layout="nchw", h_global=0, row_offset=0):
    shape = ops.ingest_shape(tuple(frames.shape), layout)
    return frames.new_empty(shape, dtype=torch.float32), frames.new_empty(shape, dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::flatfield_mean", mutates_args=())
def flatfield_mean(flat: torch.Tensor) -> torch.Tensor:
    """ct_flatfield_sums without a value, the division and the cast: the (C,) float32 mean the _flat ops below take."""
    return ops.flatfield_mean(flat)


@flatfield_mean.register_fake
def _(flat):
    return flat.new_empty((flat.shape[-3],), dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::linearize_std_flat", mutates_args=())
def linearize_std_flat(frames: torch.Tensor, lut: torch.Tensor, interp: str, std: Optional[torch.Tensor], std_mode: str,
                       std_value: float, max_code: float, flat: torch.Tensor, flat_std: Optional[torch.Tensor],
                       flat_mean: torch.Tensor, layout: str = "nchw") -> Tuple[torch.Tensor, torch.Tensor]:
    """ct_linearize_std_flat: linearize_std followed by the flat-field correction of its outputs, bit for bit, in one launch."""
    return ops.linearize_frames_flat(frames, lut, interp, std=std, std_mode=std_mode, std_value=std_value,
                                     max_code=max_code if max_code > 0 else None, want_std=True, layout=layout,
                                     flat=(flat, flat_std, flat_mean))


@linearize_std_flat.register_fake
def _(frames, lut, interp, std, std_mode, std_value, max_code, flat, flat_std, flat_mean, layout="nchw"):
    shape = (frames.shape[0],) + tuple(_chw(frames, layout))
    return frames.new_empty(shape, dtype=torch.float32), frames.new_empty(shape, dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::linearize_ingest_flat", mutates_args=())
def linearize_ingest_flat(frames: torch.Tensor, stages: Sequence[float], lut: torch.Tensor, interp: str, std: Optional[torch.Tensor],
                          std_mode: str, std_value: float, flat: torch.Tensor, flat_std: Optional[torch.Tensor],
                          flat_mean: torch.Tensor, layout: str = "nchw", h_global: int = 0, row_offset: int = 0,
                          consts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ct_linearize_ingest_flat: linearize_ingest (with ``consts``: linearize_ingest_data) followed by the flat-field correction
    of its outputs, bit for bit, in one launch."""
    return ops.linearize_ingest_frames_flat(frames, _listed_ingest_stages(frames, stages, layout), lut, interp, std=std,
                                            std_mode=std_mode, std_value=std_value, want_std=True, tile=_tile(h_global, row_offset),
                                            layout=layout, consts=consts, flat=(flat, flat_std, flat_mean))


@linearize_ingest_flat.register_fake
def _(frames, stages, lut, interp, std, std_mode, std_value, flat, flat_std, flat_mean, layout="nchw", h_global=0, row_offset=0,
      consts=None):
    shape = ops.ingest_shape(tuple(frames.shape), layout)
    return frames.new_empty(shape, dtype=torch.float32), frames.new_empty(shape, dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::linearize_ingest_strided_flat", mutates_args=())
def linearize_ingest_strided_flat(frames: torch.Tensor, step: int, stages: Sequence[float], lut: torch.Tensor, interp: str,
                                  std: Optional[torch.Tensor], std_mode: str, std_value: float, flat: torch.Tensor,
                                  flat_std: Optional[torch.Tensor], flat_mean: torch.Tensor, layout: str = "nchw",
                                  consts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ct_linearize_ingest_strided_flat: linearize_ingest_strided followed by the flat-field correction of its outputs, bit for
    bit, in one launch; flat and flat_std have the downscaled shape."""
    return ops.linearize_ingest_frames_strided_flat(frames, step, _listed_ingest_stages(frames, stages, layout), lut, interp,
                                                    std=std, std_mode=std_mode, std_value=std_value, want_std=True, layout=layout,
                                                    consts=consts, flat=(flat, flat_std, flat_mean))


@linearize_ingest_strided_flat.register_fake
def _(frames, step, stages, lut, interp, std, std_mode, std_value, flat, flat_std, flat_mean, layout="nchw", consts=None):
    shape = ops.downscaled_shape(ops.ingest_shape(tuple(frames.shape), layout), step)
    return frames.new_empty(shape, dtype=torch.float32), frames.new_empty(shape, dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::hdr_merge_ingest_batch", mutates_args=())
def hdr_merge_ingest_batch(frames: torch.Tensor, stages: Sequence[float], exposures: torch.Tensor, lut: Optional[torch.Tensor],
                           interp: str, gaussian: bool, std: Optional[torch.Tensor], std_mode: str, std_value: float,
                           layout: str = "nchw", h_global: int = 0, row_offset: int = 0, closed_form: bool = False,
                           consts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ct_hdr_merge_ingest_batch: ingest_transform followed by hdr_merge, bit for bit, in one pass over the raw frames
    (a single-batch merge; an explicit std is planar (B,C,H,W))."""
    mean, sd = ops.hdr_merge_ingest_batch(frames, _listed_ingest_stages(frames, stages, layout), exposures, lut=lut,
                                          interp=interp if lut is not None else None, gaussian_weight=gaussian, std=std,
                                          std_mode=std_mode, std_value=std_value, tile=_tile(h_global, row_offset), layout=layout,
                                          reference_order=False if closed_form else None, consts=consts)
    return mean, (sd if sd is not None else mean.new_zeros(0, dtype=torch.float32))


@hdr_merge_ingest_batch.register_fake
def _(frames, stages, exposures, lut, interp, gaussian, std, std_mode, std_value, layout="nchw", h_global=0, row_offset=0,
      closed_form=False, consts=None):
    chw = ops.ingest_shape(tuple(frames.shape), layout)[1:]
    has_std = std is not None or std_mode != "none"
    return frames.new_empty(chw, dtype=torch.float64), frames.new_empty(chw if has_std else (0,), dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::hdr_merge_dark_ingest_batches", mutates_args=())
def hdr_merge_dark_ingest_batches(frames: Sequence[torch.Tensor], stages: Sequence[float], exposures: Sequence[torch.Tensor],
                                  darks: Sequence[torch.Tensor], dark_stds: Sequence[torch.Tensor], consts: Sequence[torch.Tensor],
                                  stds: Sequence[torch.Tensor], lut: Optional[torch.Tensor], interp: str, gaussian: bool,
                                  std_mode: str, std_value: float, layout: str = "nchw",
                                  closed_form: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """ct_hdr_merge_dark_ingest_batches: per batch ingest_transform followed by the fused dark-field blur + merge, bit for bit,
    in one pass over the raw frames (a whole merge: first and final).  One tensor per batch in every list; ``dark_stds``,
    ``consts`` and ``stds`` may be empty (none); explicit stds are planar (B_k,C,H,W)."""
    mean, sd = ops.hdr_merge_dark_ingest_batches(list(frames), _listed_ingest_stages(frames[0], stages, layout), list(exposures),
                                                 list(darks), list(dark_stds) or None, consts=list(consts) or None,
                                                 stds=list(stds) or None, std_mode=std_mode, std_value=std_value, lut=lut,
                                                 interp=interp if lut is not None else None, gaussian_weight=gaussian,
                                                 layout=layout, reference_order=False if closed_form else None)
    return mean, (sd if sd is not None else mean.new_zeros(0, dtype=torch.float32))


@hdr_merge_dark_ingest_batches.register_fake
def _(frames, stages, exposures, darks, dark_stds, consts, stds, lut, interp, gaussian, std_mode, std_value, layout="nchw",
      closed_form=False):
    chw = ops.ingest_shape(tuple(frames[0].shape), layout)[1:]
    return frames[0].new_empty(chw, dtype=torch.float64), frames[0].new_empty(chw if len(dark_stds) else (0,), dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::hdr_merge_ingest_batches_strided", mutates_args=())
def hdr_merge_ingest_batches_strided(frames: Sequence[torch.Tensor], step: int, stages: Sequence[float],
                                     exposures: Sequence[torch.Tensor], consts: Sequence[torch.Tensor], stds: Sequence[torch.Tensor],
                                     lut: Optional[torch.Tensor], interp: str, gaussian: bool, std_mode: str, std_value: float,
                                     layout: str = "nchw", closed_form: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """ct_hdr_merge_ingest_strided_batches: per batch strided_downscale followed by the fused chain + merge, bit for bit, in one
    pass over the raw full-size frames (a whole merge: first and final).  One tensor per batch in every list; ``consts`` and
    ``stds`` may be empty (none); explicit stds are planar and of the downscaled shape (B_k,C,ho,wo)."""
    mean, sd = ops.hdr_merge_ingest_batches_strided(list(frames), step, _listed_ingest_stages(frames[0], stages, layout),
                                                    list(exposures), lut=lut, interp=interp if lut is not None else None,
                                                    gaussian_weight=gaussian, stds=list(stds) or None, std_mode=std_mode,
                                                    std_value=std_value, layout=layout, reference_order=False if closed_form else None,
                                                    consts=list(consts) or None)
    return mean, (sd if sd is not None else mean.new_zeros(0, dtype=torch.float32))


@hdr_merge_ingest_batches_strided.register_fake
def _(frames, step, stages, exposures, consts, stds, lut, interp, gaussian, std_mode, std_value, layout="nchw", closed_form=False):
    chw = ops.downscaled_shape(ops.ingest_shape(tuple(frames[0].shape), layout), step)[1:]
    has_std = len(stds) > 0 or std_mode != "none"
    return frames[0].new_empty(chw, dtype=torch.float64), frames[0].new_empty(chw if has_std else (0,), dtype=torch.float32)


@torch.library.custom_op(f"{_LIB}::hdr_merge_ingest_batch_strided", mutates_args=())
def hdr_merge_ingest_batch_strided(frames: torch.Tensor, step: int, stages: Sequence[float], exposures: torch.Tensor,
                                   lut: Optional[torch.Tensor], interp: str, gaussian: bool, std: Optional[torch.Tensor],
                                   std_mode: str, std_value: float, layout: str = "nchw", closed_form: bool = False,
                                   consts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The single-batch form of hdr_merge_ingest_batches_strided (strided_downscale followed by hdr_merge_ingest_batch, bit for
    bit, in one pass); an explicit std is planar (B,C,ho,wo)."""
    mean, sd = ops.hdr_merge_ingest_batch_strided(frames, step, _listed_ingest_stages(frames, stages, layout), exposures, lut=lut,
                                                  interp=interp if lut is not None else None, gaussian_weight=gaussian, std=std,
                                                  std_mode=std_mode, std_value=std_value, layout=layout,
                                                  reference_order=False if closed_form else None, consts=consts)
    return mean, (sd if sd is not None else mean.new_zeros(0, dtype=torch.float32))


@hdr_merge_ingest_batch_strided.register_fake
def _(frames, step, stages, exposures, lut, interp, gaussian, std, std_mode, std_value, layout="nchw", closed_form=False, consts=None):
    chw = ops.downscaled_shape(ops.ingest_shape(tuple(frames.shape), layout), step)[1:]
    has_std = std is not None or std_mode != "none"
    return frames.new_empty(chw, dtype=torch.float64), frames.new_empty(chw if has_std else (0,), dtype=torch.float32)
