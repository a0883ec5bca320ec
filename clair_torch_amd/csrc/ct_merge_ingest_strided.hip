// ct_merge_ingest_strided.hip -- StridedDownscale(step), a recognised gpu_transforms chain and 1 to 16 consecutive batches of
// the HDR merge in ONE pass over the RAW full-size frames (gfx950), behind ct::merge_ingest_strided
// (ct_hdr_merge_ingest_strided_batches, ct_merge_ingest.hip).  State and outputs are bit for bit those of ct_strided_downscale
// (ct_downscale.hip) on every batch followed by ct_hdr_merge_ingest_batches on the compacted frames: selecting pixels commutes
// with the per-sample chain, and the body is ct::mi_run of ct_merge_ingest_kernel.hpp itself with STRIDED set -- ingest_stages,
// mi_sample, mi_accumulate, mi_epilogue, the ring of kMiPF samples in flight, the pivot, the conditioning test with its one
// repeat and the state in registers between the batches are that code, not a restatement.
//
// Roofline: HBM.  Only every step-th source row is touched; within such a row whole 128-byte lines arrive whenever
// step * pixel_bytes is below the line size, so the floor per output sample and exposure is the selected rows at full width
// (step * sizeof(T) bytes; + 4 with explicit uncertainties), and 12 B of outputs per element.  The compacted copy of the two
// launches -- written once, read once -- is gone.
//
// Everything is in OUTPUT coordinates: ho = ceil(H / step), wo = ceil(W / step), plane = ho * wo.  Ownership is that of
// ct_merge_ingest.hip on the output plane: PLANAR, a workgroup row (blockIdx.y) is one channel plane and a thread owns 4
// consecutive output elements; PACKED3 (interleaved (B,H,W,3), RGB or BGR), a thread owns 2 pixels; slot 0 and the tail go
// element by element.  Output element p is row i = p / wo, column j = p % wo: one division for the first element, then
// (i, j) is carried, across an output-row boundary where the group straddles one (ct_linearize_ingest_strided.hip).  Its
// source is row i * step, column j * step of the same plane (frame): per exposure one load per selected element
// (interleaved: one pixel of 3), never a neighbour.  The LINEAR / CATMULL LUT row is the flat NCHW index OF THE DOWNSCALED
// frame modulo C, (c * ho * wo + p) % C; source coordinates do not enter it.  Explicit uncertainties are planar and already
// (B, C, ho, wo).  The constants of a data-dependent Normalize are per batch and the caller's, computed on the full stack.
//
// One family: the several-batches body (MULTI) serves 1 .. 16 batches, so a single batch, a list in one launch and a list
// walked batch by batch with the state in memory are the same instantiations.  LDS is mi_lds_bytes.  No atomics, the frames
// are read only, every store lies in the thread's own elements of the (C, ho * wo) state and outputs.
#include "ct_merge_ingest_kernel.hpp"

namespace ct {

// merge_ingest_multi_kernel's workgroup (ct_merge_ingest_multi.hip) on the output plane
template <typename T, bool PACKED, int INTERP, int WEIGHT, int STD>
__global__ __launch_bounds__(kBlock) void merge_ingest_strided_kernel(const MergeIngestArgs a, const MergeIngestBatches mb,
                                                                      const MergeIngestStride sd)
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
        mi_run<T, PACKED, (int)kG, INTERP, WEIGHT, STD, true, true>(a, &mb, lds, inv_t, cq, c0, p0, 0.0f, 1.0f, &sd);
        return;
    }
    // a plane's head and tail (at most kG - 1 elements each): one lane, one element (pixel) after the other
#pragma unroll 1
    for (uint32_t k = 0; k < n; ++k) mi_run<T, PACKED, 1, INTERP, WEIGHT, STD, true, true>(a, &mb, lds, inv_t, cq, c0, p0 + k, 0.0f, 1.0f, &sd);
}

template <typename T, bool PACKED>
static int mi_dispatch_strided(const MergeIngestArgs &a, const MergeIngestBatches &mb, const MergeIngestStride &sd, int interp,
                               int weight_mode, int std_mode, hipStream_t s)
{
    return with_fused_merge_modes(interp, weight_mode, std_mode, [&](auto I, auto W, auto S) {
        return merge_fused_launch(merge_ingest_strided_kernel<T, PACKED, I, W, S>, mi_grid<PACKED>(a), I, a.channels, a.n_points, a.batch, s, a,
                                  mb, sd);
    });
}

int merge_ingest_strided(const MergeIngestArgs &a, const MergeIngestBatches &mb, const MergeIngestStride &sd, int dtype, bool packed,
                         int interp, int weight_mode, int std_mode, hipStream_t s)
{
    return with_code_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return packed ? mi_dispatch_strided<T, true>(a, mb, sd, interp, weight_mode, std_mode, s)
                      : mi_dispatch_strided<T, false>(a, mb, sd, interp, weight_mode, std_mode, s);
    });
}

}  // namespace ct
