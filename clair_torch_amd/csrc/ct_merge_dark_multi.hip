// ct_merge_dark_multi.hip -- the several-batches-per-launch (MULTI) instantiations of the fused dark-field blur + merge kernel,
// behind ct::merge_dark_multi (ct_hdr_merge_dark_batches).  The body is ct::md_run of ct_merge_dark_kernel.hpp
// with MULTI set: one thread owns the same 4 columns of one image row for every batch and keeps (mean
// float64, sum of weights, variance) in registers between them, so the 32 B of state per element and batch that one launch per
// batch moves shrink to one read (not even that on a first batch) and one write per call.  A translation unit of its own, as
// ct_merge_ingest_multi.hip is for the chain kernel: the instantiations compile next to ct_merge_dark.hip's instead of after them.
#include "ct_merge_dark_kernel.hpp"

namespace ct {

// merge_dark_kernel's workgroup (ct_merge_dark.hip) with the scales of all batches staged once, concatenated behind the LUT
template <typename T, int INTERP, int WEIGHT, int STD>
__global__ __launch_bounds__(kBlock) void merge_dark_multi_kernel(const MergeDarkArgs a, const MergeDarkBatches mb)
{
    extern __shared__ __align__(16) char lds[];
    constexpr bool kGauss = WEIGHT == CT_WEIGHT_GAUSS;
    const int C = a.channels, L = a.n_points, B = a.batch;  // B: the exposures of all batches
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
    const uint32_t gpr = groups_per_row<kMdGroup>(W);
    const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (slot >= (uint64_t)gpr * (uint32_t)a.h_tile) return;
    const uint32_t h = (uint32_t)(slot / gpr);
    const uint32_t w0 = ((uint32_t)slot - h * gpr) * kMdGroup;
    const uint32_t c0 = blockIdx.y;
    if (W - w0 >= (uint32_t)kMdGroup) {
        md_run<T, kMdGroup, INTERP, WEIGHT, STD, true>(a, &mb, lds, inv_t, cq, c0, h, w0);
        return;
    }
    // the end of a row whose width is no multiple of the group (at most kMdGroup - 1 elements): one lane, one element after
    // the other, each with its own walk over the batches
#pragma unroll 1
    for (uint32_t w = w0; w < W; ++w) md_run<T, 1, INTERP, WEIGHT, STD, true>(a, &mb, lds, inv_t, cq, c0, h, w);
}

int merge_dark_multi(const MergeDarkArgs &a, const MergeDarkBatches &mb, int dtype, int interp, int weight_mode, bool has_std,
                     hipStream_t s)
{
    return with_pixel_dtype(dtype, [&](auto t) {
        return with_dark_merge_modes(interp, weight_mode, has_std, [&](auto I, auto W, auto S) {
            return merge_fused_launch(merge_dark_multi_kernel<decltype(t), I, W, S>, md_grid<kMdGroup>(a, (uint32_t)a.channels), I, a.channels,
                                      a.n_points, a.batch, s, a, mb);
        });
    });
}

}  // namespace ct
