// ct_merge_ingest_multi.hip -- the several-batches-per-launch (MULTI) instantiations of the fused chain + merge kernel, behind
// ct::merge_ingest_multi (ct_hdr_merge_ingest_batches).  The body is ct::mi_run of ct_merge_ingest_kernel.hpp
// with MULTI set (the workgroup around it is merge_ingest_kernel's, written out below): one thread owns the same elements for every batch and keeps (mean float64, sum of
// weights, variance) in registers between them, so the 32 B of state per element and batch that one launch per batch moves
// shrink to one read (not even that on a first batch) and one write per call.  A translation unit of its own, as
// ct_merge_multi.hip is for the pivot kernel: the instantiations compile next to ct_merge_ingest.hip's instead of after them.
#include "ct_merge_ingest_kernel.hpp"

namespace ct {

// merge_ingest_kernel's workgroup (ct_merge_ingest.hip) with the scales of all batches staged once, concatenated; the constants
// of a data-dependent Normalize are each batch's own and read inside mi_run
template <typename T, bool PACKED, int INTERP, int WEIGHT, int STD>
__global__ __launch_bounds__(kBlock) void merge_ingest_multi_kernel(const MergeIngestArgs a, const MergeIngestBatches mb)
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

    const uint32_t c0 = PACKED ? 0u : blockIdx.y;
    constexpr uint32_t kG = PACKED ? kMiPackedGroup : kMiGroup;
    const uint32_t head = PACKED ? 0u : (0u - c0 * a.plane) & (kG - 1);  // elements in front of the plane's first index-aligned packet
    const uint32_t slot = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    uint32_t p0 = 0, n = head < a.plane ? head : a.plane;
    if (slot > 0) {
        const uint64_t at = (uint64_t)head + (uint64_t)(slot - 1) * kG;
        if (at >= a.plane) return;
        p0 = (uint32_t)at;
        n = a.plane - p0 < kG ? a.plane - p0 : kG;
    }
    if (n == kG) {
        mi_run<T, PACKED, (int)kG, INTERP, WEIGHT, STD, true>(a, &mb, lds, inv_t, cq, c0, p0, 0.0f, 1.0f);
        return;
    }
    // a plane's head and tail (at most kG - 1 elements each): one lane, one element (pixel) after the other, each with its
    // own walk over the batches -- a few serial batches of latency in two lanes per plane, nothing next to a plane's packets
#pragma unroll 1
    for (uint32_t k = 0; k < n; ++k) mi_run<T, PACKED, 1, INTERP, WEIGHT, STD, true>(a, &mb, lds, inv_t, cq, c0, p0 + k, 0.0f, 1.0f);
}

template <typename T, bool PACKED>
static int mi_dispatch_multi(const MergeIngestArgs &a, const MergeIngestBatches &mb, int interp, int weight_mode, int std_mode,
                             hipStream_t s)
{
    return with_fused_merge_modes(interp, weight_mode, std_mode, [&](auto I, auto W, auto S) {
        return merge_fused_launch(merge_ingest_multi_kernel<T, PACKED, I, W, S>, mi_grid<PACKED>(a), I, a.channels, a.n_points, a.batch, s, a, mb);
    });
}

int merge_ingest_multi(const MergeIngestArgs &a, const MergeIngestBatches &mb, int dtype, bool packed, int interp, int weight_mode,
                       int std_mode, hipStream_t s)
{
    return with_code_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return packed ? mi_dispatch_multi<T, true>(a, mb, interp, weight_mode, std_mode, s)
                      : mi_dispatch_multi<T, false>(a, mb, interp, weight_mode, std_mode, s);
    });
}

}  // namespace ct
