// ct_merge.hpp -- argument block and packet type shared by the merge kernels (ct_merge.hip, ct_merge_exact.hip) and, host side,
// what every merge entry point shares: the mode dispatch (with_merge_modes) and the FIRST_BATCH / FINALIZE split of a batch
// list that is walked one launch per batch (merge_batch_flags).
#pragma once
#include "ct_args.hpp"

namespace ct {

#define GLOBAL_AS __attribute__((address_space(1)))  // global memory (keeps laundered addresses off the flat path)

struct MergeArgs {
    const void *stack;
    const float *std_stack;
    const double *exposure;
    const float *lut;
    double *mean_state;
    float *sumw_state;
    float *var_state;
    void *mean_out;
    float *std_out;
    int64_t image_stride;  // elements
    uint32_t q_begin;      // first local element handled by this launch
    uint32_t q_count;      // number of local elements handled by this launch (multiple of V)
    TileMap tile;
    int32_t batch, channels, n_points;
    NormConst norm;       // code -> pixel (un-folded path)
    NormConst index;      // code -> LUT coordinate s = u * (L-1) / max_code (folded path)
    float inv_max_code;   // 1 / max_code (1 for float input)
    float std_value;
    float weight_scale;   // Gaussian scale (30)
    uint32_t flags;
    // index of memory element m of one image in the state / output arrays: planar (C, H, W) unless CT_MERGE_OUT_AS_INPUT
    __device__ __forceinline__ uint32_t out_index(uint32_t m) const
    {
        return (flags & CT_MERGE_OUT_AS_INPUT) ? m : tile.planar_index(m);
    }
};

// ---- host ----------------------------------------------------------------------------------------------------------------
// f(INTERP, WEIGHT, STD) with the three run-time modes of a merge as compile-time constants; CT_ERR_INVALID_ARGUMENT for a
// value that is none.  STDS: the uncertainty modes the kernel family is built for, all four where none are given (the
// dark-field families see sigma_eff or nothing: <CT_STD_NONE, CT_STD_EXPLICIT>).
template <int... STDS, typename F>
static int with_merge_modes(int interp, int weight_mode, int std_mode, F &&f)
{
    return with_enum<CT_INTERP_LOOKUP, CT_INTERP_LINEAR, CT_INTERP_CATMULL, CT_INTERP_NONE>(interp, [&](auto I) {
        return with_enum<CT_WEIGHT_NONE, CT_WEIGHT_GAUSS>(weight_mode, [&](auto W) {
            if constexpr (sizeof...(STDS) == 0)
                return with_enum<CT_STD_NONE, CT_STD_CONSTANT, CT_STD_MULTIPLIER, CT_STD_EXPLICIT>(std_mode, [&](auto S) { return f(I, W, S); });
            else
                return with_enum<STDS...>(std_mode, [&](auto S) { return f(I, W, S); });
        });
    });
}

// The flags of one batch of a list that is walked one launch per batch: FIRST_BATCH is the first one's and FINALIZE the last
// one's, where the call has them; CT_MERGE_REQUIRE_ONE_LAUNCH is the list's matter.
static inline uint32_t merge_batch_flags(uint32_t flags, bool is_first, bool is_last)
{
    const uint32_t own = (is_first ? CT_MERGE_FIRST_BATCH : 0u) | (is_last ? CT_MERGE_FINALIZE : 0u);
    return (flags & ~(CT_MERGE_FIRST_BATCH | CT_MERGE_FINALIZE | CT_MERGE_REQUIRE_ONE_LAUNCH)) | (flags & own);
}

constexpr float kPivotCondLimit = 8.0f;  // sum |terms| / result above which a wavefront repeats the batch about the mean

template <typename T, int V>
struct alignas(sizeof(T) * V) Packet {
    T v[V];
};


// Several consecutive batches in one launch (ct_hdr_merge_batches): batch b has batch_size[b] exposures at batch_ptr[b]
// (explicit uncertainties at std_ptr[b]); the exposure times of all batches follow each other in MergeArgs::exposure and
// MergeArgs::batch is their total.  n_batches == 0: the one batch MergeArgs itself describes.
constexpr int kMaxMergeBatches = 16;
struct MergeBatches {
    int32_t n_batches;
    int32_t batch_size[kMaxMergeBatches];
    const void *batch_ptr[kMaxMergeBatches];
    const float *std_ptr[kMaxMergeBatches];
};

// ct_merge_exact.hip: the merge with the reference's float32 autograd order (two passes over each batch); `q_count` elements
// from `q_begin`, dispatched on dtype / interpolation / weight / std mode.  With `batches` the launch walks them with the
// streaming state in registers in between (bit-identical to one launch per batch).  Returns a CT_* status.
int merge_reference_order(const MergeArgs &a, int dtype, uint32_t q_total, int interp, int weight_mode, int std_mode,
                          hipStream_t stream, const MergeBatches *batches = nullptr);

}  // namespace ct
