// ct_merge_dark.hip -- the dark-field conditional blur and one batch of the HDR merge in ONE pass over the raw frames (gfx950).
// State and outputs are bit for bit those of ct_dark_field_blur (ct_darkfield.hip) into dense float32 stacks xb and sigma_eff
// followed by ct_hdr_merge_batch on them (float32 pixels, explicit uncertainties, CT_MERGE_CLOSED_FORM): the blur is
// dark_blur_kernel's expressions in its operation order on values that never leave the registers, and the merge is the
// arithmetic of merge_kernel<float, V, INTERP, WEIGHT, STD, false> restated per element in ct_merge_ingest.hpp (pivot from
// exposure B / 2 or from the mean state, conditioning test, one repeat about the mean).
//
// Roofline: HBM.  Per sample sizeof(T) bytes of the frame (its neighbours in the 3 x 3 window are L1 / L2 hits: the rows
// above and below belong to the wavefronts next door), 4 of the dark field and 4 of its std (+ 4 with explicit image
// uncertainties); 12 written per output element.  10 B per sample of a uint16 batch with derived uncertainties where the two
// launches move 26 (10 read and 8 written by the blur, 8 read again by the merge), and no float32 copy of the batch exists.
//
// Ownership: a workgroup row (blockIdx.y) is one channel plane; a thread owns 4 consecutive columns of ONE image row, so
// the three rows of its window are three pointers and its 4 x 3 window is 3 x (1 + 4 + 1) loads per exposure: the column
// left of the group (or the reflected one), the group, the column right of it.  What is left of a row whose width is no
// multiple of 4 goes through the same code one element after the other.  State and outputs move as packets where the
// group is aligned in memory (mi_store), else element by element.  No atomics, no LDS tile, the frames are read only.
// Row bands: the rows above / below the band come from `halo` exactly as dark_blur_kernel takes them.
#include <algorithm>
#include "ct_merge_dark_kernel.hpp"

namespace ct {

template <typename T, int INTERP, int WEIGHT, int STD>
__global__ __launch_bounds__(kBlock) void merge_dark_kernel(const MergeDarkArgs a)
{
    extern __shared__ __align__(16) char lds[];
    constexpr bool kGauss = WEIGHT == CT_WEIGHT_GAUSS;
    const int C = a.channels, L = a.n_points, B = a.batch;
    const int lut_bytes = INTERP == CT_INTERP_NONE ? 0 : C * L * lut_entry_bytes(INTERP);
    float *inv_t = reinterpret_cast<float *>(lds + lut_bytes);  // 1 / t_n
    float *cq = inv_t + B;                                      // derivative scale per exposure
    const float top = INTERP == CT_INTERP_NONE ? 1.0f : (float)(L - 1);
    const float kk = sqrtf(a.weight_scale * 1.4426950408889634f);
    const float K = -2.0f * a.weight_scale;
    stage_lut<INTERP, true>(lds, a.lut, C, L);
    for (int n = threadIdx.x; n < B; n += blockDim.x) {
        const float it = (float)(1.0 / a.exposure[n]);
        inv_t[n] = it;
        cq[n] = kGauss ? kk * top * it / K : top * it;
    }
    __syncthreads();

    const uint32_t W = (uint32_t)a.width;
    const uint32_t gpr = md_groups_per_row(W);
    const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (slot >= (uint64_t)gpr * (uint32_t)a.h_tile) return;
    const uint32_t h = (uint32_t)(slot / gpr);
    const uint32_t w0 = ((uint32_t)slot - h * gpr) * kMdGroup;
    const uint32_t c0 = blockIdx.y;
    if (W - w0 >= (uint32_t)kMdGroup) {
        md_run<T, kMdGroup, INTERP, WEIGHT, STD, false>(a, nullptr, lds, inv_t, cq, c0, h, w0);
        return;
    }
    // the end of a row whose width is no multiple of the group (at most kMdGroup - 1 elements): one lane, one element after
    // the other, each with its own walk over the batch
#pragma unroll 1
    for (uint32_t w = w0; w < W; ++w) md_run<T, 1, INTERP, WEIGHT, STD, false>(a, nullptr, lds, inv_t, cq, c0, h, w);
}

template <typename T, int INTERP, int WEIGHT, int STD>
static int md_launch(const MergeDarkArgs &a, hipStream_t s)
{
    if constexpr (INTERP == CT_INTERP_LOOKUP && WEIGHT == CT_WEIGHT_NONE && STD != CT_STD_NONE) {
        return CT_ERR_NO_GRADIENT_PATH;  // (refused by the entry point before it gets here)
    } else {
        const size_t lds = mi_lds_bytes(INTERP, a.channels, a.n_points, a.batch);
        hipLaunchKernelGGL((merge_dark_kernel<T, INTERP, WEIGHT, STD>), md_grid(a), dim3(kBlock), lds, s, a);
        return hipGetLastError() == hipSuccess ? CT_OK : CT_ERR_LAUNCH;
    }
}

template <typename T>
static int md_dispatch(const MergeDarkArgs &a, int interp, int weight_mode, bool has_std, hipStream_t s)
{
    return with_enum<CT_INTERP_LOOKUP, CT_INTERP_LINEAR, CT_INTERP_CATMULL, CT_INTERP_NONE>(interp, [&](auto I) {
        return with_enum<CT_WEIGHT_NONE, CT_WEIGHT_GAUSS>(weight_mode, [&](auto W) {
            return has_std ? md_launch<T, I, W, CT_STD_EXPLICIT>(a, s) : md_launch<T, I, W, CT_STD_NONE>(a, s);
        });
    });
}

// (MergeDarkCall, md_validate and md_fill_args -- what the entry points below and ct_hdr_merge_dark_ingest_batches check and fill
//  alike -- are host code of ct_merge_dark_kernel.hpp)

}  // namespace ct

extern "C" int ct_hdr_merge_dark_batch(const void *stack_dev, int32_t dtype, float max_code, int32_t batch, const ct_geometry *geom,
                                       const void *halo_dev, const float *std_dev, int32_t std_mode, float std_value,
                                       const float *dark_dev, const float *dark_std_dev, int32_t dark_batch, float threshold,
                                       float alpha, const double *exposure_dev, const ct_icrf *icrf, int32_t weight_mode,
                                       double *mean_state_dev, float *sumw_state_dev, float *var_state_dev, void *mean_out_dev,
                                       float *std_out_dev, uint32_t flags, void *stream)
{
    using namespace ct;
    const MergeDarkCall c{dtype, max_code, geom, std_mode, std_value, threshold, alpha, icrf, weight_mode, mean_state_dev,
                          sumw_state_dev, var_state_dev, mean_out_dev, std_out_dev, flags};
    NormConst norm;
    if (const int rc = md_validate(c, stack_dev, batch, halo_dev, std_dev, dark_dev, dark_std_dev, dark_batch, exposure_dev, norm); rc != CT_OK)
        return rc;
    const bool has_std = dark_std_dev != nullptr;
    MergeDarkArgs a = md_fill_args(c, has_std, norm, exposure_dev, batch);
    a.stack = stack_dev;
    a.halo = halo_dev;
    a.std_stack = std_mode == CT_STD_EXPLICIT ? std_dev : nullptr;
    a.dark = dark_dev;
    a.dark_std = dark_std_dev;
    a.dark_stride = dark_batch == 1 ? 0 : (int64_t)a.plane * geom->channels;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case CT_DTYPE_U8: return md_dispatch<uint8_t>(a, icrf->interp, weight_mode, has_std, s);
        case CT_DTYPE_U16: return md_dispatch<uint16_t>(a, icrf->interp, weight_mode, has_std, s);
        default: return md_dispatch<float>(a, icrf->interp, weight_mode, has_std, s);
    }
}

// Several consecutive dark-field batches of one merge: ONE launch of the MULTI kernels (ct_merge_dark_multi.hip) where the
// exposures of all batches fit the LDS together; otherwise one launch per batch with the state in memory, exactly what the
// caller would have done.
extern "C" int ct_hdr_merge_dark_batches(const void *const *stack_devs, const int32_t *batch_sizes, int32_t n_batches, int32_t dtype,
                                         float max_code, const ct_geometry *geom, const void *const *halo_devs,
                                         const float *const *std_devs, int32_t std_mode, float std_value,
                                         const float *const *dark_devs, const float *const *dark_std_devs, const int32_t *dark_batches,
                                         float threshold, float alpha, const double *exposure_dev, const ct_icrf *icrf,
                                         int32_t weight_mode, double *mean_state_dev, float *sumw_state_dev, float *var_state_dev,
                                         void *mean_out_dev, float *std_out_dev, uint32_t flags, void *stream)
{
    using namespace ct;
    if (n_batches < 1 || n_batches > kMaxDarkBatches || !stack_devs || !batch_sizes || !dark_devs || !dark_batches) return CT_ERR_INVALID_ARGUMENT;
    const uint32_t single_flags = flags & ~CT_MERGE_REQUIRE_ONE_LAUNCH;
    const int n = n_batches;
    auto halo_of = [&](int b) { return halo_devs ? halo_devs[b] : nullptr; };
    auto std_of = [&](int b) { return std_devs ? std_devs[b] : nullptr; };
    auto dark_std_of = [&](int b) { return dark_std_devs ? dark_std_devs[b] : nullptr; };
    if (n == 1)
        return ct_hdr_merge_dark_batch(stack_devs[0], dtype, max_code, batch_sizes[0], geom, halo_of(0), std_of(0), std_mode, std_value,
                                       dark_devs[0], dark_std_of(0), dark_batches[0], threshold, alpha, exposure_dev, icrf, weight_mode,
                                       mean_state_dev, sumw_state_dev, var_state_dev, mean_out_dev, std_out_dev, single_flags, stream);
    // a dark std for every batch or for none (the kernels propagate an uncertainty or do not), and likewise the halo rows
    for (int b = 1; b < n; ++b)
        if ((dark_std_of(b) != nullptr) != (dark_std_of(0) != nullptr) || (halo_of(b) != nullptr) != (halo_of(0) != nullptr))
            return CT_ERR_INVALID_ARGUMENT;
    // every batch as the single-batch entry point would judge it (FIRST_BATCH / FINALIZE: of the whole call, so that a state
    // is needed unless the call is a whole merge); nothing has touched the device when one of them is refused
    const MergeDarkCall c{dtype, max_code, geom, std_mode, std_value, threshold, alpha, icrf, weight_mode, mean_state_dev,
                          sumw_state_dev, var_state_dev, mean_out_dev, std_out_dev, single_flags};
    NormConst norm;
    int64_t offset[kMaxDarkBatches] = {}, total = 0;
    for (int b = 0; b < n; ++b) {
        offset[b] = total;
        if (const int rc = md_validate(c, stack_devs[b], batch_sizes[b], halo_of(b), std_of(b), dark_devs[b], dark_std_of(b), dark_batches[b],
                                       exposure_dev ? exposure_dev + total : nullptr, norm);
            rc != CT_OK)
            return rc;
        total += batch_sizes[b];
    }
    const bool has_std = dark_std_of(0) != nullptr;
    const bool has_state = mean_state_dev && sumw_state_dev && (!has_std || var_state_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mi_lds_bytes(icrf->interp, geom->channels, icrf_points(icrf), total) <= kLdsBudget) {
        const MergeDarkArgs a = md_fill_args(c, has_std, norm, exposure_dev, (int32_t)total);
        MergeDarkBatches mb = {};
        for (int b = 0; b < n; ++b) {
            mb.stack[b] = stack_devs[b];
            mb.halo[b] = halo_of(b);
            mb.std_stack[b] = std_mode == CT_STD_EXPLICIT ? std_of(b) : nullptr;
            mb.dark[b] = dark_devs[b];
            mb.dark_std[b] = dark_std_of(b);
            mb.dark_stride[b] = dark_batches[b] == 1 ? 0 : (int64_t)a.plane * geom->channels;
            mb.batch[b] = batch_sizes[b];
            mb.offset[b] = (int32_t)offset[b];
        }
        mb.n_batches = n;
        return merge_dark_multi(a, mb, dtype, icrf->interp, weight_mode, has_std, s);
    }
    // the scales of all exposures do not fit the LDS beside the LUT, those of each batch do: one launch per batch
    if ((flags & CT_MERGE_REQUIRE_ONE_LAUNCH) || !has_state) return CT_ERR_UNSUPPORTED;
    const bool first = flags & CT_MERGE_FIRST_BATCH, finalize = flags & CT_MERGE_FINALIZE;
    for (int b = 0; b < n; ++b) {
        const uint32_t f = (single_flags & ~(CT_MERGE_FIRST_BATCH | CT_MERGE_FINALIZE)) | ((first && b == 0) ? CT_MERGE_FIRST_BATCH : 0u) |
                           ((finalize && b == n - 1) ? CT_MERGE_FINALIZE : 0u);
        const int rc = ct_hdr_merge_dark_batch(stack_devs[b], dtype, max_code, batch_sizes[b], geom, halo_of(b), std_of(b), std_mode,
                                               std_value, dark_devs[b], dark_std_of(b), dark_batches[b], threshold, alpha,
                                               exposure_dev + offset[b], icrf, weight_mode, mean_state_dev, sumw_state_dev, var_state_dev,
                                               mean_out_dev, std_out_dev, f, stream);
        if (rc != CT_OK) return rc;
    }
    return CT_OK;
}
