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
    const uint32_t gpr = groups_per_row<kMdGroup>(W);
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

// the launch of one batch, dispatched on dtype / interpolation / weight / dark std (has_std: CT_STD_EXPLICIT, else none)
static int merge_dark_single(const MergeDarkArgs &a, int dtype, int interp, int weight_mode, bool has_std, hipStream_t s)
{
    return with_pixel_dtype(dtype, [&](auto t) {
        return with_dark_merge_modes(interp, weight_mode, has_std, [&](auto I, auto W, auto S) {
            return merge_fused_launch(merge_dark_kernel<decltype(t), I, W, S>, md_grid<kMdGroup>(a, (uint32_t)a.channels), I, a.channels, a.n_points,
                                      a.batch, s, a);
        });
    });
}

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
    return merge_dark_single(a, dtype, icrf->interp, weight_mode, has_std, static_cast<hipStream_t>(stream));
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
    if (!batch_list_ok(n_batches, batch_sizes, stack_devs, dark_devs, dark_batches)) return CT_ERR_INVALID_ARGUMENT;
    const uint32_t single_flags = flags & ~CT_MERGE_REQUIRE_ONE_LAUNCH;
    const int n = n_batches;
    auto single = [&](int b, uint32_t f, int64_t offset) {
        return ct_hdr_merge_dark_batch(stack_devs[b], dtype, max_code, batch_sizes[b], geom, batch_item(halo_devs, b), batch_item(std_devs, b),
                                       std_mode, std_value, dark_devs[b], batch_item(dark_std_devs, b), dark_batches[b], threshold, alpha,
                                       exposure_dev + offset, icrf, weight_mode, mean_state_dev, sumw_state_dev, var_state_dev, mean_out_dev,
                                       std_out_dev, f, stream);
    };
    if (n == 1) return single(0, single_flags, 0);
    // a dark std for every batch or for none (the kernels propagate an uncertainty or do not), and likewise the halo rows
    if (!all_or_none(dark_std_devs, n) || !all_or_none(halo_devs, n)) return CT_ERR_INVALID_ARGUMENT;
    const MergeDarkCall c{dtype, max_code, geom, std_mode, std_value, threshold, alpha, icrf, weight_mode, mean_state_dev,
                          sumw_state_dev, var_state_dev, mean_out_dev, std_out_dev, single_flags};
    const bool has_std = batch_item(dark_std_devs, 0) != nullptr;
    // an empty batch is refused like any other fault of a batch; what cannot be walked batch by batch is not built
    constexpr MergeBatchPolicy kPolicy{/*skip_empty*/ false, /*no_state*/ CT_ERR_UNSUPPORTED, /*require_one_launch*/ CT_ERR_UNSUPPORTED};
    NormConst norm;
    return merge_batches(
        batch_sizes, n, flags, c.has_state(has_std), kPolicy,
        // FIRST_BATCH / FINALIZE: of the whole call, so that a state is needed unless the call is a whole merge
        [&](int b, int64_t offset) {
            return md_validate(c, stack_devs[b], batch_sizes[b], batch_item(halo_devs, b), batch_item(std_devs, b), dark_devs[b],
                               batch_item(dark_std_devs, b), dark_batches[b], exposure_dev ? exposure_dev + offset : nullptr, norm);
        },
        [&](const MergeBatchList &list) {
            // one launch: the scales of all exposures fit the LDS beside the LUT (those of each batch do: md_validate)
            if (!merge_scales_fit(icrf, geom->channels, list.total)) return kMergePerBatch;
            const MergeDarkArgs a = md_fill_args(c, has_std, norm, exposure_dev, (int32_t)list.total);
            MergeDarkBatches mb = {};
            for (int b = 0; b < n; ++b) {
                mb.stack[b] = stack_devs[b];
                mb.halo[b] = batch_item(halo_devs, b);
                mb.std_stack[b] = std_mode == CT_STD_EXPLICIT ? batch_item(std_devs, b) : nullptr;
                mb.dark[b] = dark_devs[b];
                mb.dark_std[b] = batch_item(dark_std_devs, b);
                mb.dark_stride[b] = dark_batches[b] == 1 ? 0 : (int64_t)a.plane * geom->channels;
                mb.batch[b] = batch_sizes[b];
                mb.offset[b] = (int32_t)list.offset[b];
            }
            mb.n_batches = n;
            return merge_dark_multi(a, mb, dtype, icrf->interp, weight_mode, has_std, static_cast<hipStream_t>(stream));
        },
        single);
}
