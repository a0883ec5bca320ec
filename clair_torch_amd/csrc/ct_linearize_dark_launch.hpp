// ct_linearize_dark_launch.hpp -- what the fused dark-field blur + linearization kernels share (linearize_dark_kernel of
// ct_linearize_dark.hip on codes or pixels, linearize_dark_ingest_planar_kernel / _packed3_kernel of
// ct_linearize_dark_ingest.hip on raw frames behind a chain): the slot scheme of their walk and the host path in front of
// a launch.  One copy of each.
//
// The walk.  A workgroup row (blockIdx.y) is one frame of this launch and one of its planes, or all 3 planes of an
// interleaved frame, so the frame -- its dark-field pointers travel in the argument block: at most
// CT_LINEARIZE_DARK_MAX_FRAMES frames per launch -- and the planes are wave-uniform.  A thread owns kLdGroup consecutive
// columns (pixels) of ONE image row; what is left of a row whose width is no multiple of kLdGroup goes through the same
// window one element after the other.  A workgroup walks kLdSlots groups per thread, a workgroup apart, so one staging of the
// LUT (stage_lut) serves kLdSlots * 1024 samples per plane.  Outputs are one packet where the group is 16-byte aligned in
// memory (li_store), else elements.  No atomics, no LDS tile, no row bands: no halo is built here.
//
// The text of the walk stays in the three kernels: every function it was moved into -- the whole walk, the slot arithmetic
// alone, the sample-and-store step alone -- changed their instructions (profiles/linearize_dark_walk_isa.md).
#pragma once
#include <algorithm>
#include "ct_dark_window.hpp"
#include "ct_linearize_ingest.hpp"

namespace ct {

constexpr int kLdGroup = kLiGroup;  // columns / pixels per thread
constexpr int kLdSlots = 4;         // groups per thread

// groups of kLdGroup columns in a row, the last one possibly short
static inline __host__ __device__ uint32_t ld_groups_per_row(uint32_t width) { return (width + kLdGroup - 1) / kLdGroup; }

// ---- host ----------------------------------------------------------------------------------------------------------------
// Predicates and steps of ct_linearize_dark and ct::linearize_dark_ingest; each entry point places its own tests between
// them, in its own order (ct_args.hpp: predicates are shared, the order is per entry point).

// what both refuse first: a missing pointer, the frame count, a frame without its dark field or without its std
static inline bool ld_pointers_present(const void *frames_dev, const ct_geometry *geom, const float *const *dark_devs,
                                       const float *const *dark_std_devs, const float *lin_out_dev, const float *std_out_dev,
                                       int64_t n_frames)
{
    if (!frames_dev || !geom || !dark_devs || !dark_std_devs || !lin_out_dev || !std_out_dev || n_frames <= 0 || n_frames > 0x7fffffff)
        return false;
    for (int64_t k = 0; k < n_frames; ++k)
        if (!dark_devs[k] || !dark_std_devs[k]) return false;
    return true;
}

// ... then what ct_dark_field_blur refuses for each frame as a batch of one, in its order (ct_darkfield.hip), on the geometry
// `g` of the planar image that is blurred; a row band would need the rows above and below it, and the streamed generator has
// no tile=, so no halo is built here
static inline int ld_check_geometry(const ct_geometry *g, int32_t std_mode, const float *std_dev)
{
    if (int rc = check_dark_frames(g, 1, 1, true, std_mode, std_dev)) return rc;
    if (g->row_offset != 0 || g->h_tile != g->h_global) return CT_ERR_UNSUPPORTED;
    return check_dark_band(g, nullptr);  // (the whole image: what is left of it is the stride)
}

// frames per launch: what the argument block holds, and a grid's y extent (65535) in workgroup rows; 0: none fits
static inline int64_t ld_frames_per_launch(int64_t rows_per_frame)
{
    return std::min<int64_t>(CT_LINEARIZE_DARK_MAX_FRAMES, (int64_t)kLiMaxRows / rows_per_frame);
}

static inline bool ld_darks_aligned(const float *const *dark_devs, const float *const *dark_std_devs, int64_t n_frames)
{
    for (int64_t k = 0; k < n_frames; ++k)
        if (!aligned(dark_devs[k], sizeof(float)) || !aligned(dark_std_devs[k], sizeof(float))) return false;
    return true;
}

// the members every argument block of the family has
template <typename Args>
static void ld_fill_args(Args &a, const ct_icrf *icrf, const ct_geometry *geom, int n_points, NormConst norm, int32_t std_mode,
                         float std_value, float threshold, float alpha)
{
    a.lut = icrf->lut_dev;
    a.image_stride = geom->image_stride;
    a.plane = (uint32_t)(geom->h_tile * geom->width);
    a.width = (uint32_t)geom->width;
    a.h_tile = (uint32_t)geom->h_tile;
    a.channels = (uint32_t)geom->channels;
    a.n_points = (uint32_t)n_points;
    fill_blur_args(a, norm, std_mode, std_value, threshold, alpha);
}

// one launch of `kernel` over `rows` workgroup rows
template <typename Args>
static int ld_launch(void (*kernel)(const Args), const Args &a, int interp, uint32_t rows, hipStream_t s)
{
    const size_t lds = lut_lds_bytes(interp, (int)a.channels, (int)a.n_points);
    const uint64_t slots = (uint64_t)ld_groups_per_row(a.width) * a.h_tile;
    const uint64_t per_block = (uint64_t)kBlock * kLdSlots;
    const dim3 grid((uint32_t)((slots + per_block - 1) / per_block), rows);
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, s, a);
    return hipGetLastError() == hipSuccess ? CT_OK : CT_ERR_LAUNCH;
}

// The frames in launches of at most per_launch.  For each the block's pointers move to its first frame -- the frames by
// image_stride elements, the explicit sigma (std_dev, or NULL in any other mode) by std_stride floats, the dense outputs by
// channels * plane --, the dark fields of its frames are copied in, and launch(T{}, a, first, n) launches them for the
// frames' element type T; the first error ends the walk.
template <typename Args, typename Launch>
static int ld_launch_frames(Args a, const void *frames_dev, int32_t dtype, const float *std_dev, int64_t std_stride, float *lin_out_dev,
                            float *std_out_dev, const float *const *dark_devs, const float *const *dark_std_devs, int64_t n_frames,
                            int64_t per_launch, Launch &&launch)
{
    const int64_t out_stride = (int64_t)a.channels * a.plane;
    for (int64_t first = 0; first < n_frames; first += per_launch) {
        const int nf = (int)std::min<int64_t>(per_launch, n_frames - first);
        a.frames = static_cast<const char *>(frames_dev) + first * a.image_stride * (int64_t)dtype_bytes(dtype);
        a.std_in = std_dev ? std_dev + first * std_stride : nullptr;
        a.lin_out = lin_out_dev + first * out_stride;
        a.std_out = std_out_dev + first * out_stride;
        for (int k = 0; k < nf; ++k) {
            a.dark[k] = dark_devs[first + k];
            a.dark_std[k] = dark_std_devs[first + k];
        }
        int rc;
        switch (dtype) {
            case CT_DTYPE_U8: rc = launch(uint8_t{}, a, first, nf); break;
            case CT_DTYPE_U16: rc = launch(uint16_t{}, a, first, nf); break;
            default: rc = launch(float{}, a, first, nf); break;
        }
        if (rc != CT_OK) return rc;
    }
    return CT_OK;
}

}  // namespace ct
