// ct_args.hpp -- host only: the argument checks of the entry points and the fillers of the kernels' argument blocks, one
// copy of each.  They are predicates, not one validator: every entry point calls them in an order of its own, because the
// order decides which status a call with two faults gets (pinned by tests/test_malformed_calls_host.py and the merge / pair
// tables of tests/test_abi_and_host.py).  No __device__ code: including this header changes no kernel.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "ct_device.hpp"

namespace ct {

// ---- geometry (ct_geometry, non-NULL) ---------------------------------------------------------------------------------
// rows [row_offset, row_offset + h_tile) lie inside the global image
static inline bool band_fits(const ct_geometry *g)
{
    return g->h_global >= g->h_tile && g->row_offset >= 0 && g->row_offset + g->h_tile <= g->h_global;
}

// allow_empty: a plane without rows or columns is a call with nothing to do, not a fault (the ingest statistics and merges)
static inline bool shape_positive(const ct_geometry *g, bool allow_empty = false)
{
    return g->channels > 0 && (allow_empty ? g->h_tile >= 0 && g->width >= 0 : g->h_tile > 0 && g->width > 0);
}

static inline bool layout_ok(const ct_geometry *g) { return g->layout >= CT_LAYOUT_NCHW && g->layout <= CT_LAYOUT_NHWC_BGR; }

// the kernels index the GLOBAL image with 32 bits
static inline bool global_below_2_31(const ct_geometry *g) { return g->h_global * g->width * g->channels < (int64_t)1 << 31; }

static inline int64_t local_elements(const ct_geometry *g) { return g->h_tile * g->width * g->channels; }

static inline bool stride_holds_image(const ct_geometry *g) { return g->image_stride >= local_elements(g); }

// A stack as ct_linearize_std / _bwd and the pair entry points take it: shape and row band, then the 2^31 limit, then the
// stride and the layout.
static inline int check_stack_geometry(const ct_geometry *g)
{
    if (!shape_positive(g) || !band_fits(g)) return CT_ERR_INVALID_ARGUMENT;
    if (!global_below_2_31(g)) return CT_ERR_TOO_LARGE;
    return stride_holds_image(g) && layout_ok(g) ? CT_OK : CT_ERR_INVALID_ARGUMENT;
}

// The prefix the three ingest entry points share: shape and row band, then the layout, then the 2^31 limit.
static inline int check_ingest_geometry(const ct_geometry *g, bool allow_empty)
{
    if (!shape_positive(g, allow_empty) || !band_fits(g) || !layout_ok(g)) return CT_ERR_INVALID_ARGUMENT;
    return global_below_2_31(g) ? CT_OK : CT_ERR_TOO_LARGE;
}

// NULL is aligned: a pointer that is not there is not used.  Where NULL is a fault the caller tests the pointer itself.
static inline bool aligned(const void *p, size_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// the bytes of an element of a stack of a (validated) CT_DTYPE_*, which is also the alignment of its pointer
static inline size_t dtype_bytes(int32_t dtype) { return dtype == CT_DTYPE_U8 ? 1 : (dtype == CT_DTYPE_U16 ? 2 : 4); }

// ---- model and uncertainty mode ---------------------------------------------------------------------------------------
// allow_none: CT_INTERP_NONE (no LUT) is a model
static inline bool icrf_ok(const ct_icrf *icrf, bool allow_none = true)
{
    if (icrf->interp < CT_INTERP_LOOKUP || icrf->interp > (allow_none ? CT_INTERP_NONE : CT_INTERP_CATMULL)) return false;
    return icrf->interp == CT_INTERP_NONE || (icrf->lut_dev && icrf->n_points >= 2);
}

// n_points as the kernels take it (CT_INTERP_NONE never reads a LUT; 2 keeps L - 1 positive)
static inline int icrf_points(const ct_icrf *icrf) { return icrf->interp == CT_INTERP_NONE ? 2 : icrf->n_points; }

constexpr size_t kLdsBudget = 160 * 1024;  // LDS of a compute unit (CDNA4), the most a workgroup can ask for

static inline size_t lut_lds_bytes(int interp, int channels, int n_points)
{
    return interp == CT_INTERP_NONE ? 0 : (size_t)channels * (size_t)n_points * lut_entry_bytes(interp);
}

// Workgroups that can be resident on the whole device at once, for kernels that walk their work in a grid-stride
// loop: a grid that is a multiple of this runs as full rounds of equal work.  (1026 long-running workgroups on 256
// one-slot units run 4 full rounds plus 2 stragglers that cost a whole fifth round.)
static inline int resident_workgroups(size_t lds_bytes, int block_threads)
{
    const size_t by_lds = lds_bytes ? kLdsBudget / lds_bytes : 64;
    const size_t by_waves = (size_t)2048 / (size_t)block_threads;  // 32 wavefronts per unit
    size_t slots = by_lds < by_waves ? by_lds : by_waves;
    if (slots < 1) slots = 1;
    return compute_units() * (int)slots;
}

static inline bool std_mode_in_range(int32_t std_mode) { return std_mode >= CT_STD_NONE && std_mode <= CT_STD_EXPLICIT; }

// ... and EXPLICIT comes with its pointer (the merges test that per batch, next to their stack pointers)
static inline bool std_mode_ok(int32_t std_mode, const void *std_dev)
{
    return std_mode_in_range(std_mode) && (std_mode != CT_STD_EXPLICIT || std_dev);
}

// The fl(u / max_code) constants of a stack of `dtype`; float32 pixels take none.
static inline int norm_for_dtype(int32_t dtype, float max_code, NormConst *norm)
{
    *norm = NormConst{1.0f, 0.0f};
    if (dtype == CT_DTYPE_F32) return CT_OK;
    if (dtype != CT_DTYPE_U8 && dtype != CT_DTYPE_U16) return CT_ERR_UNSUPPORTED;
    return ct_norm_constants(max_code, &norm->hi, &norm->lo) == CT_OK ? CT_OK : CT_ERR_UNSUPPORTED;
}

// ---- dark field: what ct_dark_field_blur refuses, for it and for the two entry points that fuse it ------------------------
// Two runs of its order; what an entry point tests in between, before and after stays with it.  First the frames: shape (the
// 3 x 3 blur reflects at the borders: two columns and two global rows at least), layout, the dark fields (one per frame or one
// for all), the std mode.  ct_linearize_dark's frames are batches of one with a dark field each.
static inline int check_dark_frames(const ct_geometry *g, int32_t batch, int32_t dark_batch, bool propagates, int32_t std_mode,
                                    const void *std_dev)
{
    if (!shape_positive(g) || g->width < 2 || g->h_global < 2 || !band_fits(g)) return CT_ERR_INVALID_ARGUMENT;
    if (g->layout != CT_LAYOUT_NCHW) return CT_ERR_UNSUPPORTED;
    if (dark_batch != 1 && dark_batch != batch) return CT_ERR_INVALID_ARGUMENT;
    // One SHARED dark field for several frames with its uncertainty propagated: the reference's autograd on a (1, C, H, W)
    // mask_map sums the gradient over the frames BEFORE squaring, (sum_n g_n)^2 sigma_D^2, which a per-frame effective
    // sigma cannot express (it would give sum_n (g_n sigma_D)^2).  Not built; refuse rather than return the other quantity.
    if (dark_batch == 1 && batch > 1 && propagates) return CT_ERR_UNSUPPORTED;
    return std_mode_ok(std_mode, std_dev) ? CT_OK : CT_ERR_INVALID_ARGUMENT;
}

// ... then the row band: one that does not touch the global top / bottom needs its neighbours' rows in `halo`; so does a
// one-row band's reflection.  Last the stride.
static inline int check_dark_band(const ct_geometry *g, const void *halo_dev)
{
    const bool top = g->row_offset == 0, bottom = g->row_offset + g->h_tile == g->h_global;
    if ((!top || !bottom) && !halo_dev) return CT_ERR_INVALID_ARGUMENT;
    if ((top || bottom) && g->h_tile < 2 && !(top && bottom)) return CT_ERR_UNSUPPORTED;
    return stride_holds_image(g) ? CT_OK : CT_ERR_INVALID_ARGUMENT;
}

// ---- argument blocks --------------------------------------------------------------------------------------------------
// What DarkArgs, MergeDarkArgs and LinDarkArgs have in common (each keeps its own layout): the blur's parameters.
template <typename Args>
static inline void fill_blur_args(Args &a, NormConst norm, int32_t std_mode, float std_value, float threshold, float alpha)
{
    a.norm = norm;
    a.std_mode = std_mode;
    a.std_value = std_value;
    a.threshold = threshold;
    a.alpha = alpha;
    // torchvision _get_gaussian_kernel1d(3, 1.0): pdf = exp(-0.5 x^2), x = -1, 0, 1; normalised in float32
    const float side = expf(-0.5f), sum = (side + 1.0f) + side;
    a.k0 = 1.0f / sum;
    a.k1 = side / sum;
}

static inline TileMap make_tile(const ct_geometry *g)
{
    TileMap t;
    t.plane_local = (uint32_t)(g->h_tile * g->width);
    t.chan_skip = (uint32_t)((g->h_global - g->h_tile) * g->width);
    t.base = (uint32_t)(g->row_offset * g->width);
    t.layout = (uint32_t)g->layout;  // of the input stack (and of an explicit std stack); states and outputs are planar
    t.channels = (uint32_t)g->channels;
    return t;
}

// What LinIngestArgs, StatsIngestArgs and MergeIngestArgs have in common (each keeps its own layout and field types).
template <typename Args>
static inline void fill_ingest_args(Args &a, const ct_geometry *g, int n_points, bool by_channel, const ct_ingest_stage *stages,
                                    int32_t n_stages)
{
    a.image_stride = g->image_stride;
    a.plane = (decltype(a.plane))(g->h_tile * g->width);
    a.plane_global = (uint32_t)(g->h_global * g->width);
    a.base = (uint32_t)(g->row_offset * g->width);
    a.channels = (decltype(a.channels))g->channels;
    a.n_points = (decltype(a.n_points))n_points;
    a.reversed = g->layout == CT_LAYOUT_NHWC_BGR ? 1u : 0u;
    a.by_channel = by_channel ? 1u : 0u;
    a.n_stages = (uint32_t)n_stages;
    for (int32_t k = 0; k < n_stages; ++k) a.stage[k] = stages[k];
}

}  // namespace ct
