"""ctypes binding of the C ABI in include/clair_hip.h.

There is no CPU fallback: if the HIP library is missing or a call fails, this module raises.  The
library is built in-tree by ``clair_torch_amd.build`` (hipcc, gfx950) and loaded from
``clair_torch_amd/lib/libclair_hip.so``.
"""
import ctypes
import os

from . import build as _build

# include/clair_hip.h constants
DTYPE_U8, DTYPE_U16, DTYPE_F32 = 0, 1, 2
INTERP_LOOKUP, INTERP_LINEAR, INTERP_CATMULL, INTERP_NONE = 0, 1, 2, 3
STD_NONE, STD_CONSTANT, STD_MULTIPLIER, STD_EXPLICIT = 0, 1, 2, 3
WEIGHT_NONE, WEIGHT_GAUSS = 0, 1
LAYOUT_NCHW, LAYOUT_NHWC, LAYOUT_NHWC_BGR = 0, 1, 2
MERGE_FIRST_BATCH, MERGE_FINALIZE, MERGE_MEAN_OUT_F32, MERGE_F64_MOMENTS = 1, 2, 4, 8
MERGE_REFERENCE_ORDER, MERGE_CLOSED_FORM, MERGE_STD_HINT, MERGE_REQUIRE_ONE_LAUNCH, MERGE_OUT_AS_INPUT = 16, 32, 64, 128, 256
STATS_REQUIRE_ONE_LAUNCH, STATS_MAX_BATCHES = 1, 16
LINEARIZE_DARK_MAX_FRAMES = 16
INGEST_AFFINE, INGEST_CLAMP, INGEST_MAX_STAGES, INGEST_MAX_CHANNELS = 0, 1, 4, 4
INGEST_AFFINE_DATA, EXTREMA_MIN, EXTREMA_MAX, EXTREMA_MAX_PREFIX = 2, 1, 2, 3
ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, ERR_LAUNCH, ERR_NO_GRADIENT_PATH, ERR_TOO_LARGE = -1, -2, -3, -4, -5

ABI_VERSION = 3
EXPORTS = ("ct_abi_version", "ct_error_string", "ct_hdr_merge_batch", "ct_hdr_merge_batches", "ct_linearize_std", "ct_linearize_fwd",
           "ct_linearize_bwd", "ct_pair_residual_fwd", "ct_pair_residual_bwd", "ct_pair_residual_bwd_workspace", "ct_flatfield_sums",
           "ct_flatfield_apply", "ct_video_stats_batch", "ct_dark_field_blur", "ct_hdr_merge_kernel_name",
           "ct_merge_set_retry_counter", "ct_norm_constants", "ct_index_constants", "ct_pivot_index_constants",
           "ct_pivot_floor_constants", "ct_pivot_interval_constants", "ct_band_stats", "ct_band_stats_workspace",
           "ct_strided_downscale", "ct_export_cv", "ct_ingest_transform", "ct_ingest_extrema_workspace", "ct_ingest_extrema",
           "ct_ingest_transform_data", "ct_linearize_ingest", "ct_hdr_merge_ingest_batch", "ct_video_stats_ingest_batch",
           "ct_hdr_merge_ingest_batches", "ct_ingest_extrema_frames_workspace", "ct_ingest_extrema_frames",
           "ct_linearize_ingest_data", "ct_pair_residual_ingest_fwd", "ct_pair_residual_ingest_bwd", "ct_linearize_ingest_strided",
           "ct_video_stats_batches", "ct_video_stats_ingest_batches", "ct_hdr_merge_dark_batch", "ct_linearize_dark",
           "ct_hdr_merge_dark_batches", "ct_linearize_dark_ingest", "ct_hdr_merge_dark_ingest_batches",
           "ct_linearize_std_flat", "ct_linearize_ingest_flat", "ct_linearize_ingest_strided_flat",
           "ct_linearize_dark_ingest_data", "ct_hdr_merge_ingest_strided_batches")


class Geometry(ctypes.Structure):
    _fields_ = [("channels", ctypes.c_int32), ("h_tile", ctypes.c_int64), ("width", ctypes.c_int64),
                ("h_global", ctypes.c_int64), ("row_offset", ctypes.c_int64), ("image_stride", ctypes.c_int64),
                ("layout", ctypes.c_int32)]


class Icrf(ctypes.Structure):
    _fields_ = [("lut_dev", ctypes.c_void_p), ("n_points", ctypes.c_int32), ("interp", ctypes.c_int32)]


class PairParams(ctypes.Structure):
    _fields_ = [("lower", ctypes.c_float), ("upper", ctypes.c_float), ("weight_scale", ctypes.c_float),
                ("use_relative", ctypes.c_int32), ("use_uncertainty_weighting", ctypes.c_int32),
                ("std_mode", ctypes.c_int32), ("std_value", ctypes.c_float), ("pair_band", ctypes.c_int32)]


class IngestStage(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("sub", ctypes.c_float), ("div", ctypes.c_float), ("mul", ctypes.c_float),
                ("add", ctypes.c_float), ("lo", ctypes.c_float * 4), ("hi", ctypes.c_float * 4)]


class NativeLibraryError(RuntimeError):
    pass


_lib = None


def library_path():
    return _build.LIB_PATH


def load():
    """Load (once) the HIP shared library; raises NativeLibraryError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise NativeLibraryError(
            f"{path} is missing: build it with `python -m clair_torch_amd.build` (hipcc, gfx950). "
            "clair_torch_amd has no CPU fallback for its kernels.")
    # torch first: its wheel carries a HIP runtime of its own under a file name that is not the soname this library asks
    # for.  Loaded after torch, the library binds to that runtime; loaded before it, the system's runtime comes in as a
    # second one beside torch's, and the first launch on one of torch's streams fails (CT_ERR_LAUNCH).
    import torch  # noqa: F401
    lib = ctypes.CDLL(path)
    vp, i32, i64, f32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_uint32
    gp, ip = ctypes.POINTER(Geometry), ctypes.POINTER(Icrf)
    lib.ct_abi_version.restype = i32
    lib.ct_error_string.restype = ctypes.c_char_p
    lib.ct_error_string.argtypes = [i32]
    lib.ct_hdr_merge_batch.restype = i32
    lib.ct_hdr_merge_batch.argtypes = [vp, i32, f32, i32, gp, vp, i32, f32, vp, ip, i32, vp, vp, vp, vp, vp, u32, vp]
    lib.ct_hdr_merge_batches.restype = i32
    lib.ct_hdr_merge_batches.argtypes = [vp, vp, vp, i32, i32, f32, gp, i32, f32, vp, ip, i32, vp, vp, vp, vp, vp, u32, vp]
    lib.ct_pivot_interval_constants.restype = i32
    lib.ct_pivot_interval_constants.argtypes = [f32, i32, i32, i32, ctypes.POINTER(f32)]
    lib.ct_linearize_std.restype = i32
    lib.ct_linearize_std.argtypes = [vp, i32, f32, i64, gp, vp, i32, f32, ip, vp, vp, vp]
    lib.ct_linearize_fwd.restype = i32
    lib.ct_linearize_fwd.argtypes = [vp, i64, gp, ip, vp, vp]
    lib.ct_linearize_bwd.restype = i32
    lib.ct_linearize_bwd.argtypes = [vp, vp, i64, gp, ip, vp, vp, vp]
    pp = ctypes.POINTER(PairParams)
    lib.ct_pair_residual_fwd.restype = i32
    lib.ct_pair_residual_fwd.argtypes = [vp, i32, f32, i32, gp, vp, ip, vp, vp, vp, i32, pp, i32, vp, vp, vp]
    lib.ct_pair_residual_bwd.restype = i32
    lib.ct_pair_residual_bwd.argtypes = [vp, i32, f32, i32, gp, vp, ip, vp, i32, vp, vp, vp, pp, vp, vp, vp, vp, i64, vp]
    lib.ct_pair_residual_bwd_workspace.restype = i64
    lib.ct_pair_residual_bwd_workspace.argtypes = [i32, i32, i32]
    lib.ct_hdr_merge_kernel_name.restype = ctypes.c_char_p
    lib.ct_hdr_merge_kernel_name.argtypes = [i32, f32, i32, i32, u32]
    lib.ct_merge_set_retry_counter.restype = None
    lib.ct_merge_set_retry_counter.argtypes = [vp]
    lib.ct_flatfield_sums.restype = i32
    lib.ct_flatfield_sums.argtypes = [vp, i32, vp, i32, i64, vp, vp]
    lib.ct_flatfield_apply.restype = i32
    lib.ct_flatfield_apply.argtypes = [vp, i32, i64, vp, i32, vp, vp, vp, vp, i32, i64, vp]
    lib.ct_dark_field_blur.restype = i32
    lib.ct_dark_field_blur.argtypes = [vp, i32, f32, i32, gp, vp, vp, i32, f32, vp, vp, i32, f32, f32, vp, vp, vp]
    lib.ct_hdr_merge_dark_batch.restype = i32
    lib.ct_hdr_merge_dark_batch.argtypes = [vp, i32, f32, i32, gp, vp, vp, i32, f32, vp, vp, i32, f32, f32, vp, ip, i32, vp, vp, vp,
                                            vp, vp, u32, vp]
    lib.ct_hdr_merge_dark_batches.restype = i32
    lib.ct_hdr_merge_dark_batches.argtypes = [vp, vp, i32, i32, f32, gp, vp, vp, i32, f32, vp, vp, vp, f32, f32, vp, ip, i32, vp, vp, vp,
                                              vp, vp, u32, vp]
    lib.ct_hdr_merge_dark_ingest_batches.restype = i32
    lib.ct_hdr_merge_dark_ingest_batches.argtypes = [vp, vp, i32, i32, gp, ctypes.POINTER(IngestStage), i32, vp, vp, vp, i32, f32, vp, vp, vp,
                                                     f32, f32, vp, ip, i32, vp, vp, vp, vp, vp, u32, vp]
    lib.ct_linearize_dark.restype = i32
    lib.ct_linearize_dark.argtypes = [vp, i32, f32, i64, gp, vp, i32, f32, vp, vp, f32, f32, ip, vp, vp, vp]
    lib.ct_linearize_dark_ingest.restype = i32
    lib.ct_linearize_dark_ingest.argtypes = [vp, i32, i64, gp, ctypes.POINTER(IngestStage), i32, vp, i32, f32, vp, vp, f32, f32, ip, vp,
                                             vp, vp]
    # ... _data: the parent's arguments, then the (n_frames, 4) per-frame constants in front of the stream
    lib.ct_linearize_dark_ingest_data.restype = i32
    lib.ct_linearize_dark_ingest_data.argtypes = [vp, i32, i64, gp, ctypes.POINTER(IngestStage), i32, vp, i32, f32, vp, vp, f32, f32, ip,
                                                  vp, vp, vp, vp]
    lib.ct_band_stats_workspace.restype = i64
    lib.ct_band_stats_workspace.argtypes = [i32]
    lib.ct_band_stats.restype = i32
    lib.ct_band_stats.argtypes = [vp, vp, i32, i64, vp, i64, vp, vp]
    lib.ct_strided_downscale.restype = i32
    lib.ct_strided_downscale.argtypes = [vp, vp, i32, i64, i64, i64, i32, i32, vp]
    lib.ct_export_cv.restype = i32
    lib.ct_export_cv.argtypes = [vp, i32, vp, i32, i64, i32, i64, i32, vp]
    lib.ct_ingest_transform.restype = i32
    lib.ct_ingest_transform.argtypes = [vp, i32, i32, i64, i32, i64, ctypes.POINTER(IngestStage), i32, vp, vp]
    lib.ct_ingest_extrema_workspace.restype = i64
    lib.ct_ingest_extrema_workspace.argtypes = []
    lib.ct_ingest_extrema.restype = i32
    lib.ct_ingest_extrema.argtypes = [vp, i32, i32, i64, i32, i64, ctypes.POINTER(IngestStage), i32, i32, f32, f32, vp, i64, vp, vp]
    lib.ct_ingest_transform_data.restype = i32
    lib.ct_ingest_transform_data.argtypes = [vp, i32, i32, i64, i32, i64, ctypes.POINTER(IngestStage), i32, vp, vp, vp]
    lib.ct_linearize_ingest.restype = i32
    lib.ct_linearize_ingest.argtypes = [vp, i32, i64, gp, ctypes.POINTER(IngestStage), i32, vp, i32, f32, ip, vp, vp, vp]
    lib.ct_ingest_extrema_frames_workspace.restype = i64
    lib.ct_ingest_extrema_frames_workspace.argtypes = [i64]
    lib.ct_ingest_extrema_frames.restype = i32
    lib.ct_ingest_extrema_frames.argtypes = [vp, i32, i32, i64, i32, i64, ctypes.POINTER(IngestStage), i32, i32, f32, f32, vp, i64, vp,
                                             vp]
    lib.ct_linearize_ingest_data.restype = i32
    lib.ct_linearize_ingest_data.argtypes = [vp, i32, i64, gp, ctypes.POINTER(IngestStage), i32, vp, i32, f32, ip, vp, vp, vp, vp]
    lib.ct_linearize_ingest_strided.restype = i32
    lib.ct_linearize_ingest_strided.argtypes = [vp, i32, i64, gp, i32, ctypes.POINTER(IngestStage), i32, vp, i32, f32, ip, vp, vp, vp, vp]
    # ... _flat: the parent's arguments, then flat, flat std (or NULL) and the C channel means in front of the stream
    lib.ct_linearize_std_flat.restype = i32
    lib.ct_linearize_std_flat.argtypes = [vp, i32, f32, i64, gp, vp, i32, f32, ip, vp, vp, vp, vp, vp, vp]
    lib.ct_linearize_ingest_flat.restype = i32
    lib.ct_linearize_ingest_flat.argtypes = [vp, i32, i64, gp, ctypes.POINTER(IngestStage), i32, vp, i32, f32, ip, vp, vp, vp, vp, vp, vp, vp]
    lib.ct_linearize_ingest_strided_flat.restype = i32
    lib.ct_linearize_ingest_strided_flat.argtypes = [vp, i32, i64, gp, i32, ctypes.POINTER(IngestStage), i32, vp, i32, f32, ip, vp, vp, vp, vp,
                                                     vp, vp, vp]
    lib.ct_hdr_merge_ingest_batch.restype = i32
    lib.ct_hdr_merge_ingest_batch.argtypes = [vp, i32, i32, gp, ctypes.POINTER(IngestStage), i32, vp, vp, i32, f32, vp, ip, i32, vp, vp,
                                              vp, vp, vp, u32, vp]
    lib.ct_hdr_merge_ingest_batches.restype = i32
    lib.ct_hdr_merge_ingest_batches.argtypes = [vp, vp, i32, i32, gp, ctypes.POINTER(IngestStage), i32, vp, vp, i32, f32, vp, ip, i32, vp,
                                                vp, vp, vp, vp, u32, vp]
    # ... _strided: the parent's arguments with the step behind the geometry
    lib.ct_hdr_merge_ingest_strided_batches.restype = i32
    lib.ct_hdr_merge_ingest_strided_batches.argtypes = [vp, vp, i32, i32, gp, i32, ctypes.POINTER(IngestStage), i32, vp, vp, i32, f32, vp,
                                                        ip, i32, vp, vp, vp, vp, vp, u32, vp]
    lib.ct_video_stats_ingest_batch.restype = i32
    lib.ct_video_stats_ingest_batch.argtypes = [vp, i32, i32, gp, ctypes.POINTER(IngestStage), i32, vp, ip, f32, vp, vp, vp]
    stages = ctypes.POINTER(IngestStage)
    lib.ct_pair_residual_ingest_fwd.restype = i32
    lib.ct_pair_residual_ingest_fwd.argtypes = [vp, i32, stages, i32, vp, i32, gp, vp, ip, vp, vp, vp, i32, pp, i32, vp, vp, vp]
    lib.ct_pair_residual_ingest_bwd.restype = i32
    lib.ct_pair_residual_ingest_bwd.argtypes = [vp, i32, stages, i32, vp, i32, gp, vp, ip, vp, i32, vp, vp, vp, pp, vp, vp, vp, vp,
                                                i64, vp]
    lib.ct_video_stats_batch.restype = i32
    lib.ct_video_stats_batch.argtypes = [vp, i32, f32, i32, gp, ip, f32, vp, vp, vp]
    lib.ct_video_stats_batches.restype = i32
    lib.ct_video_stats_batches.argtypes = [vp, vp, i32, i32, f32, gp, ip, f32, vp, vp, u32, vp]
    lib.ct_video_stats_ingest_batches.restype = i32
    lib.ct_video_stats_ingest_batches.argtypes = [vp, vp, i32, i32, gp, stages, i32, vp, ip, f32, vp, vp, u32, vp]
    if lib.ct_abi_version() != ABI_VERSION:
        raise NativeLibraryError(f"{path}: ABI version {lib.ct_abi_version()} != {ABI_VERSION}; rebuild the library")
    _lib = lib
    return lib


def check(rc, what):
    """Translate a C status code into the exception type the reference raises at that point."""
    if rc == 0:
        return
    msg = load().ct_error_string(rc).decode()
    if rc == ERR_NO_GRADIENT_PATH:
        # torch.autograd.grad's error text in the reference (hdr_merge.py:108, linearization.py:100)
        raise RuntimeError("element 0 of tensors does not require grad and does not have a grad_fn")
    if rc in (ERR_INVALID_ARGUMENT, ERR_TOO_LARGE):
        raise ValueError(f"{what}: {msg}")
    raise NativeLibraryError(f"{what}: {msg} (code {rc})")
