// ct_merge_dark_ingest.hip -- a recognised gpu_transforms chain, the dark-field conditional blur and 1 to 16 consecutive batches
// of the HDR merge in ONE pass over the RAW frames (gfx950).  For every batch the state and the outputs are bit for bit those
// of ct_ingest_transform (with constants: ct_ingest_transform_data, ct_ingest.hip) into a dense planar float32 stack followed
// by ct_hdr_merge_dark_batch (ct_merge_dark.hip) on that stack with CT_DTYPE_F32, the same dark fields, uncertainties, halo,
// geometry and flags, batch after batch on the same state: the same device functions run here on values that never leave
// the registers.  The 9 taps of a sample's window are cast to float and go through ct::ingest_stages<true>
// (ct_ingest_stages.hpp) with the tap's PLANE channel, the blur is dark_blur_staged (ct_dark_window.hpp: dark_blur_kernel's
// expressions in its order, on floats), the merge is mi_sample / mi_accumulate / mi_epilogue (ct_merge_ingest.hpp) in the walk
// of md_run (ct_merge_dark_kernel.hpp).  float32 throughout, every operation rounded on its own (-ffp-contract=off).
// tests/test_gpu_merge_dark_ingest.py holds the kernels to the two launches bit for bit.
//
// Roofline by bytes: HBM (measured: not reached, see the resources below).  Per sample sizeof(T) bytes of the frame (window neighbours are L1 / L2 hits), 4 of the dark field and 4 of
// its std (+ 4 with explicit image uncertainties); 12 written per output element and call.  10 B per uint16 sample with
// derived uncertainties and a dark field per frame where the two launches move 2 + 4, then 4 + 8 = 18; with one shared dark
// field per batch about 2 B against about 10 B; the float32 stack of a batch never exists.  (Byte counts from the shapes; what
// was timed and what was not: profiles/merge_dark_ingest.md.)
//
// Ownership.  One kernel family; one batch is a list of one (there is no single-batch kernel).  A thread keeps (mean float64,
// sum of weights, variance) of its elements in registers between the batches; the state is read at most once and written at
// most once.  A data-dependent stage (CT_INGEST_AFFINE_DATA) is a wave-uniform run-time branch, its two constants read per
// batch; the stage loop and the std mode of the image behind the chain are wave-uniform too.
// PLANAR (CT_LAYOUT_NCHW, any C): the walk of md_run.  A workgroup row (blockIdx.y) is one channel plane, so the clamp pair is
//   wave-uniform; a thread owns 4 consecutive columns of ONE image row, 3 x (1 + 4 + 1) window loads per exposure, 2 exposures
//   in flight ahead of the one being reduced; the end of a row whose width is no multiple of 4 goes one element after the
//   other.  Row bands: the rows above / below the band come from `halo`, RAW rows of the frames' dtype, and go through the
//   chain like any other tap (the chain is pointwise, so this is the halo of the staged stack).
// PACKED3 (CT_LAYOUT_NHWC / NHWC_BGR, raw (B, H, W, 3) frames): one workgroup row.  A thread owns kMiPackedGroup = 2
//   consecutive PIXELS of one image row with all 3 channels: on each of the three rows the 6 contiguous elements of its pixels
//   and the 3 of the pixel left and of the pixel right of them (or the reflected ones) -- neighbours of a sample lie 3 elements
//   apart in a row.  Memory channel cm feeds plane 2 - cm with BGR (a wave-uniform index, not a variant).  One exposure in
//   flight ahead of the one being reduced (kMdiPackedPF).  No row bands (no interleaved halo is built: CT_ERR_UNSUPPORTED).
// The dark field, its std, explicit image uncertainties, the state and the outputs are planar (C, H, W) in plane (RGB) order
// whatever the layout of the frames.  State and outputs move as packets where the group is aligned in memory (mi_store), else
// element by element.  No atomics, no LDS tile, no StridedDownscale (the caller compacts first); frames, dark fields and
// uncertainties are read only.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): scratch is 0 bytes for all 90 kernels.
// VGPRs, unit weights without a dark std .. Gaussian weights with one:
//   planar   uint8 127 .. 227, uint16 134 .. 234, float32 146 .. 246 (2 to 4 wavefronts per SIMD)
//   packed3  uint8 167 .. 256, uint16 149 .. 253, float32 170 .. 254 (+ up to 18 AGPRs; 1 to 3 wavefronts per SIMD)
// Measured on 32 x 3 x 4096 x 4096, LINEAR, Gaussian weights (profiles/merge_dark_ingest.md), fused time / time of the pair:
// float32 frames 0.79 to 0.98, every run faster; uint8 / uint16 planar 1.04 to 1.25 and uint16 BGR 1.13 to 1.40, every run
// SLOWER: the chain runs on the 18 taps of a thread's window where the pair runs it once per sample (4.5 divisions per sample
// against 1), and at these register counts the latency is not hidden.  The byte counts above did not decide it.  So
// compute_hdr_image(fused_dark_ingest=...) is off by default; what it saves today is the float32 stack of a batch.  First
// things to look at: the chain on a row shared through the LDS, or one division per tap replaced where the divisor allows.
#include "ct_merge_dark_ingest_kernel.hpp"

namespace ct {

static int merge_dark_ingest_launch(const MergeDarkIngestArgs &a, const MergeDarkIngestBatches &mb, int dtype, bool packed, int interp,
                                    int weight_mode, bool has_std, hipStream_t s)
{
    if (packed) return merge_dark_ingest_packed(a, mb, dtype, interp, weight_mode, has_std, s);
    return mdi_dispatch<false>(a, mb, dtype, interp, weight_mode, has_std, s);
}

}  // namespace ct

// 1 to 16 consecutive dark-field batches of one merge behind one chain: ONE launch where the exposures of all batches fit the
// LDS beside the LUT; otherwise one launch per batch (a list of one each) with the state in memory.
extern "C" int ct_hdr_merge_dark_ingest_batches(const void *const *frames_devs, const int32_t *batch_sizes, int32_t n_batches,
                                                int32_t dtype, const ct_geometry *geom, const ct_ingest_stage *stages, int32_t n_stages,
                                                const float *const *consts_devs, const void *const *halo_devs,
                                                const float *const *std_devs, int32_t std_mode, float std_value,
                                                const float *const *dark_devs, const float *const *dark_std_devs,
                                                const int32_t *dark_batches, float threshold, float alpha, const double *exposure_dev,
                                                const ct_icrf *icrf, int32_t weight_mode, double *mean_state_dev, float *sumw_state_dev,
                                                float *var_state_dev, void *mean_out_dev, float *std_out_dev, uint32_t flags, void *stream)
{
    using namespace ct;
    // ---- the batch list itself ----
    if (!batch_list_ok(n_batches, batch_sizes, frames_devs, dark_devs, dark_batches, geom)) return CT_ERR_INVALID_ARGUMENT;
    const int n = n_batches;
    // a dark std for every batch or for none (the kernels propagate an uncertainty or do not); likewise the halo rows and the
    // constants of a data-dependent stage
    if (!all_or_none(dark_std_devs, n) || !all_or_none(halo_devs, n) || !all_or_none(consts_devs, n)) return CT_ERR_INVALID_ARGUMENT;
    // ---- the stage list and the layout of the raw frames: a data-dependent stage needs constants, and there is one at most ----
    bool by_channel = false;
    if (int rc = ingest_validate(dtype, geom->layout, 1, geom->channels, geom->h_tile * geom->width, stages, n_stages, CT_INGEST_MAX_STAGES,
                                 batch_item(consts_devs, 0) ? 1 : 0, by_channel))
        return rc;
    const bool packed = geom->layout != CT_LAYOUT_NCHW;
    if (packed && (geom->row_offset != 0 || geom->h_tile != geom->h_global)) return CT_ERR_UNSUPPORTED;  // no interleaved halo is built
    // ---- every batch as ct_hdr_merge_dark_batch judges the planar float32 stack the chain yields (the layout of the raw frames
    //      is the stage list's matter; pointers are aligned to the raw element); FIRST_BATCH / FINALIZE: of the whole call ----
    ct_geometry planar = *geom;
    planar.layout = CT_LAYOUT_NCHW;
    const MergeDarkCall c{dtype, 1.0f, &planar, std_mode, std_value, threshold, alpha, icrf, weight_mode, mean_state_dev,
                          sumw_state_dev, var_state_dev, mean_out_dev, std_out_dev, flags & ~CT_MERGE_REQUIRE_ONE_LAUNCH};
    const bool has_std = batch_item(dark_std_devs, 0) != nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    NormConst norm;

    MergeDarkIngestArgs a{};
    a.reversed = geom->layout == CT_LAYOUT_NHWC_BGR ? 1u : 0u;
    a.by_channel = by_channel ? 1u : 0u;
    a.n_stages = (uint32_t)n_stages;
    for (int32_t k = 0; k < n_stages; ++k) a.stage[k] = stages[k];
    auto fill_batch = [&](MergeDarkIngestBatches &mb, int slot, int b, int32_t at) {
        mb.frames[slot] = frames_devs[b];
        mb.halo[slot] = batch_item(halo_devs, b);
        mb.std_stack[slot] = std_mode == CT_STD_EXPLICIT ? batch_item(std_devs, b) : nullptr;
        mb.dark[slot] = dark_devs[b];
        mb.dark_std[slot] = batch_item(dark_std_devs, b);
        mb.consts[slot] = batch_item(consts_devs, b);
        mb.dark_stride[slot] = dark_batches[b] == 1 ? 0 : geom->h_tile * geom->width * geom->channels;
        mb.batch[slot] = batch_sizes[b];
        mb.offset[slot] = at;
    };
    // an empty batch is refused like any other fault of a batch; a list that is not one launch is "too large" under the flag
    constexpr MergeBatchPolicy kPolicy{/*skip_empty*/ false, /*no_state*/ CT_ERR_UNSUPPORTED, /*require_one_launch*/ CT_ERR_TOO_LARGE};
    return merge_batches(
        batch_sizes, n, flags, c.has_state(has_std), kPolicy,
        [&](int b, int64_t offset) {
            if (const int rc = md_validate(c, frames_devs[b], batch_sizes[b], batch_item(halo_devs, b), batch_item(std_devs, b), dark_devs[b],
                                           batch_item(dark_std_devs, b), dark_batches[b], exposure_dev ? exposure_dev + offset : nullptr, norm);
                rc != CT_OK)
                return rc;
            return aligned(batch_item(consts_devs, b), sizeof(float)) ? (int)CT_OK : (int)CT_ERR_INVALID_ARGUMENT;
        },
        [&](const MergeBatchList &list) {
            // one launch: the scales of all exposures fit the LDS beside the LUT (those of each batch do: md_validate)
            if (!merge_scales_fit(icrf, geom->channels, list.total)) return kMergePerBatch;
            a.d = md_fill_args(c, has_std, norm, exposure_dev, (int32_t)list.total);
            MergeDarkIngestBatches mb = {};
            for (int b = 0; b < n; ++b) fill_batch(mb, b, b, (int32_t)list.offset[b]);
            mb.n_batches = n;
            return merge_dark_ingest_launch(a, mb, dtype, packed, icrf->interp, weight_mode, has_std, s);
        },
        [&](int b, uint32_t f, int64_t offset) {  // a list of one
            MergeDarkCall cb = c;
            cb.flags = f;
            a.d = md_fill_args(cb, has_std, norm, exposure_dev + offset, batch_sizes[b]);
            MergeDarkIngestBatches mb = {};
            fill_batch(mb, 0, b, 0);
            mb.n_batches = 1;
            return merge_dark_ingest_launch(a, mb, dtype, packed, icrf->interp, weight_mode, has_std, s);
        });
}
