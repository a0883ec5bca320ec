// ct_merge_ingest.hip -- a recognised gpu_transforms chain and one batch of the HDR merge in ONE pass (gfx950): raw codes in,
// streaming state and (mean, std) out.  State and outputs are bit for bit those of ct_ingest_transform (or _data,
// ct_ingest.hip) into a dense planar float32 stack followed by ct_hdr_merge_batch on that stack -- the same device functions
// run here on a value that never leaves the registers: ct::ingest_stages (ct_ingest_stages.hpp) and the arithmetic of
// merge_kernel<float, V, INTERP, WEIGHT, STD, false> restated per element in ct_merge_ingest.hpp (float clamp and gradient
// mask, the pivot from exposure B / 2 or from the mean state, the conditioning test and the one repeat about the mean).
//
// Roofline: HBM.  B * sizeof(T) bytes read (+ 4 B with explicit uncertainties) and 12 written per output element, every
// byte once: 76 B per element of a 32-exposure uint16 stack where the two launches move 332.
//
// Ownership is that of the ingest kernels; LUT, 1 / t_n and the derivative scales live in LDS as in merge_kernel:
// PLANAR (any C): a workgroup row (blockIdx.y) is one channel plane, so the channel -- the clamp pair, the LOOKUP row -- is
//   wave-uniform.  A thread owns 4 consecutive output elements whose state and output accesses are 16-byte aligned packets
//   and fetches their codes with one 4- or 8-byte load per exposure.  The LINEAR / CATMULL row is the reference's flat NCHW
//   index modulo C (base.py:173-176): one modulo for the first element, an add and a conditional subtract for the others.
// PACKED3 (interleaved (B,H,W,3), RGB or BGR): a thread owns 2 pixels: per exposure it reads their 6 codes with one dense
//   load, regroups in registers and keeps one 8-byte (float32) / 16-byte (float64) packet per plane for sums, state and
//   outputs.  BGR is a wave-uniform plane index (2 - memory channel), not a variant.  (Four pixels per thread, the ingest
//   kernels' ownership, was built first: 12 elements with five sums and a pivot each took 222 VGPRs, two wavefronts per
//   SIMD, and ran slower than the two launches it replaces -- profiles/merge_ingest.md.)
// Packets are aligned in the index space of the planar (C, plane) arrays (slot 0 holds what precedes a plane's first one);
// an array whose packet is not aligned in memory -- planes 1 and 2 of an interleaved image with an odd H*W, a base pointer
// inside a larger buffer -- is accessed element by element.  What precedes the first packet of a plane
// and what follows the last whole one goes through the same code with ONE element (pixel) per step.  PF samples are in
// flight ahead of the one being reduced, as in merge_kernel's ring.  No atomics, no LDS regroup, the frames are read only.
#include "ct_merge_ingest_kernel.hpp"

namespace ct {

template <typename T, bool PACKED, int INTERP, int WEIGHT, int STD>
__global__ __launch_bounds__(kBlock) void merge_ingest_kernel(const MergeIngestArgs a)
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
    // the constants of a data-dependent Normalize: one wave-uniform load, before anything is stored
    const float dsub = a.consts ? a.consts[0] : 0.0f, ddiv = a.consts ? a.consts[1] : 1.0f;
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
        mi_run<T, PACKED, (int)kG, INTERP, WEIGHT, STD, false>(a, nullptr, lds, inv_t, cq, c0, p0, dsub, ddiv);
        return;
    }
    // a plane's head and tail (at most kG - 1 elements each): one lane, one element (pixel) after the other, each with its
    // own walk over the batch -- a few serial batches of latency in two lanes per plane, nothing next to a plane's packets
#pragma unroll 1
    for (uint32_t k = 0; k < n; ++k) mi_run<T, PACKED, 1, INTERP, WEIGHT, STD, false>(a, nullptr, lds, inv_t, cq, c0, p0 + k, dsub, ddiv);
}

template <typename T, bool PACKED>
static int mi_dispatch(const MergeIngestArgs &a, int interp, int weight_mode, int std_mode, hipStream_t s)
{
    return with_fused_merge_modes(interp, weight_mode, std_mode, [&](auto I, auto W, auto S) {
        return merge_fused_launch(merge_ingest_kernel<T, PACKED, I, W, S>, mi_grid<PACKED>(a), I, a.channels, a.n_points, a.batch, s, a);
    });
}

// What ct_hdr_merge_ingest_batch and ct_hdr_merge_ingest_batches have in common besides the frames: one geometry, one stage
// list, one dtype, one set of modes, the state and the outputs.
struct MergeIngestCall {
    int32_t dtype;
    const ct_geometry *geom;
    const ct_ingest_stage *stages;
    int32_t n_stages;
    int32_t std_mode;
    float std_value;
    const double *exposure;
    const ct_icrf *icrf;
    int32_t weight_mode;
    double *mean_state;
    float *sumw_state, *var_state;
    void *mean_out;
    float *std_out;
    uint32_t flags;
    bool has_state() const { return mean_state && sumw_state && (std_mode == CT_STD_NONE || var_state); }
    int64_t plane() const { return geom->h_tile * geom->width; }
    int n_points() const { return icrf_points(icrf); }
};

// Everything that needs no pointer into device memory, in the order the status codes are documented: geometry, a stack of
// `batch` frames of codes, the stage list and the model (check_code_ingest), the modes (as validate_merge of ct_merge.hip),
// the flags these entry points do not take.  FIRST_BATCH / FINALIZE in c.flags are those of the whole call.
static int mi_validate(const MergeIngestCall &c, int32_t batch, const float *consts_dev, bool &by_channel)
{
    const ct_geometry *geom = c.geom;
    const ct_icrf *icrf = c.icrf;
    const int32_t std_mode = c.std_mode, weight_mode = c.weight_mode;
    const uint32_t flags = c.flags;
    if (const int rc = check_code_ingest(c.dtype, batch, geom, c.stages, c.n_stages, consts_dev, icrf, by_channel); rc != CT_OK) return rc;
    const int interp = icrf->interp;
    if (!std_mode_in_range(std_mode) || (weight_mode != CT_WEIGHT_NONE && weight_mode != CT_WEIGHT_GAUSS)) return CT_ERR_INVALID_ARGUMENT;
    // hdr_merge.py:107-113: autograd.grad raises when nothing connects the mean to the image
    if (std_mode != CT_STD_NONE && interp == CT_INTERP_LOOKUP && weight_mode == CT_WEIGHT_NONE) return CT_ERR_NO_GRADIENT_PATH;
    if (flags & (CT_MERGE_F64_MOMENTS | CT_MERGE_REFERENCE_ORDER | CT_MERGE_OUT_AS_INPUT)) return CT_ERR_UNSUPPORTED;
    // what ct_hdr_merge_batch sends to the reference-order kernel (float64-VALU bound: its bytes are not what it waits for)
    if ((interp == CT_INTERP_CATMULL || interp == CT_INTERP_LOOKUP) && std_mode != CT_STD_NONE && !(flags & CT_MERGE_CLOSED_FORM))
        return CT_ERR_UNSUPPORTED;
    if (!c.has_state() && !((flags & CT_MERGE_FIRST_BATCH) && (flags & CT_MERGE_FINALIZE))) return CT_ERR_INVALID_ARGUMENT;
    if ((flags & CT_MERGE_FINALIZE) && (!c.mean_out || (std_mode != CT_STD_NONE && !c.std_out))) return CT_ERR_INVALID_ARGUMENT;
    if (!stride_holds_image(geom)) return CT_ERR_INVALID_ARGUMENT;
    return merge_scales_fit(icrf, geom->channels, batch) ? CT_OK : CT_ERR_TOO_LARGE;
}

// the pointers of a call that has something to do: present and aligned to their element
static bool mi_pointers_ok(const MergeIngestCall &c, const void *frames_dev, const float *std_dev)
{
    if (!frames_dev || !c.exposure || (c.std_mode == CT_STD_EXPLICIT && !std_dev)) return false;
    return aligned(frames_dev, c.dtype == CT_DTYPE_U16 ? 2 : 1) && aligned(c.exposure, sizeof(double)) && aligned(std_dev, sizeof(float)) &&
           aligned(c.mean_state, sizeof(double)) && aligned(c.sumw_state, sizeof(float)) && aligned(c.var_state, sizeof(float)) &&
           aligned(c.mean_out, (c.flags & CT_MERGE_MEAN_OUT_F32) ? sizeof(float) : sizeof(double)) && aligned(c.std_out, sizeof(float));
}

// the kernels' argument block for `batch` exposures (MULTI: of all batches) whose times are at `exposure`
static MergeIngestArgs mi_fill_args(const MergeIngestCall &c, const void *frames_dev, const float *std_dev, const float *consts_dev,
                                    const double *exposure, int32_t batch, uint32_t flags, bool by_channel)
{
    const ct_geometry *geom = c.geom;
    const bool has_state = c.has_state();
    MergeIngestArgs a = {};
    a.frames = frames_dev;
    a.std_stack = c.std_mode == CT_STD_EXPLICIT ? std_dev : nullptr;
    a.consts = consts_dev;
    a.exposure = exposure;
    a.lut = c.icrf->lut_dev;
    a.mean_state = has_state ? c.mean_state : nullptr;
    a.sumw_state = has_state ? c.sumw_state : nullptr;
    a.var_state = has_state ? c.var_state : nullptr;
    a.mean_out = c.mean_out;
    a.std_out = c.std_out;
    fill_ingest_args(a, geom, c.n_points(), by_channel, c.stages, c.n_stages);
    a.batch = batch;
    a.std_value = c.std_value;
    a.weight_scale = 30.0f;  // gaussian_value_weights default scale, hdr_merge.py:95
    a.flags = flags;
    return a;
}

}  // namespace ct

extern "C" int ct_hdr_merge_ingest_batch(const void *frames_dev, int32_t dtype, int32_t batch, const ct_geometry *geom,
                                         const ct_ingest_stage *stages, int32_t n_stages, const float *consts_dev,
                                         const float *std_dev, int32_t std_mode, float std_value, const double *exposure_dev,
                                         const ct_icrf *icrf, int32_t weight_mode, double *mean_state_dev, float *sumw_state_dev,
                                         float *var_state_dev, void *mean_out_dev, float *std_out_dev, uint32_t flags, void *stream)
{
    using namespace ct;
    const MergeIngestCall c{dtype, geom, stages, n_stages, std_mode, std_value, exposure_dev, icrf, weight_mode, mean_state_dev,
                            sumw_state_dev, var_state_dev, mean_out_dev, std_out_dev, flags};
    bool by_channel = false;
    if (const int rc = mi_validate(c, batch, consts_dev, by_channel); rc != CT_OK) return rc;
    if (batch == 0 || c.plane() == 0) return CT_OK;
    if (!mi_pointers_ok(c, frames_dev, std_dev)) return CT_ERR_INVALID_ARGUMENT;
    const MergeIngestArgs a = mi_fill_args(c, frames_dev, std_dev, consts_dev, exposure_dev, batch, flags, by_channel);
    const bool packed = geom->layout != CT_LAYOUT_NCHW;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_code_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return packed ? mi_dispatch<T, true>(a, icrf->interp, weight_mode, std_mode, s) : mi_dispatch<T, false>(a, icrf->interp, weight_mode, std_mode, s);
    });
}

// Several consecutive batches of one merge behind one chain: ONE launch of the MULTI kernels (ct_merge_ingest_multi.hip) where
// the batches agree on having constants and their exposures fit the LDS together; otherwise one launch per batch with the
// state in memory, exactly what the caller would have done.
extern "C" int ct_hdr_merge_ingest_batches(const void *const *frames_devs, const int32_t *batch_sizes, int32_t n_batches, int32_t dtype,
                                           const ct_geometry *geom, const ct_ingest_stage *stages, int32_t n_stages,
                                           const float *const *consts_devs, const float *const *std_devs, int32_t std_mode,
                                           float std_value, const double *exposure_dev, const ct_icrf *icrf, int32_t weight_mode,
                                           double *mean_state_dev, float *sumw_state_dev, float *var_state_dev, void *mean_out_dev,
                                           float *std_out_dev, uint32_t flags, void *stream)
{
    using namespace ct;
    if (!batch_list_ok(n_batches, batch_sizes, frames_devs)) return CT_ERR_INVALID_ARGUMENT;
    const uint32_t single_flags = flags & ~CT_MERGE_REQUIRE_ONE_LAUNCH;
    auto single = [&](int b, const float *std_dev, uint32_t f, int64_t offset) {
        return ct_hdr_merge_ingest_batch(frames_devs[b], dtype, batch_sizes[b], geom, stages, n_stages, batch_item(consts_devs, b), std_dev,
                                         std_mode, std_value, exposure_dev + offset, icrf, weight_mode, mean_state_dev, sumw_state_dev,
                                         var_state_dev, mean_out_dev, std_out_dev, f, stream);
    };
    if (n_batches == 1) return single(0, batch_item(std_devs, 0), single_flags, 0);
    const MergeIngestCall c{dtype, geom, stages, n_stages, std_mode, std_value, exposure_dev, icrf, weight_mode, mean_state_dev,
                            sumw_state_dev, var_state_dev, mean_out_dev, std_out_dev, single_flags};
    // the list reads explicit uncertainties only where the mode asks for them
    auto std_of = [&](int b) { return std_mode == CT_STD_EXPLICIT ? batch_item(std_devs, b) : nullptr; };
    // an empty batch is skipped (FIRST_BATCH is the first and FINALIZE the last of those with frames); a missing state is the
    // caller's fault here, as in ct_hdr_merge_batches
    constexpr MergeBatchPolicy kPolicy{/*skip_empty*/ true, /*no_state*/ CT_ERR_INVALID_ARGUMENT, /*require_one_launch*/ CT_ERR_UNSUPPORTED};
    bool by_channel = false;
    return merge_batches(
        batch_sizes, n_batches, flags, c.has_state(), kPolicy,
        // FIRST_BATCH / FINALIZE: of the whole call, so that a state is needed unless the call is a whole merge
        [&](int b, int64_t) { return mi_validate(c, batch_sizes[b], batch_item(consts_devs, b), by_channel); },
        [&](const MergeBatchList &list) {
            if (list.n == 0 || c.plane() == 0) return (int)CT_OK;
            MergeIngestBatches mb = {};
            int n_consts = 0;
            for (int k = 0; k < list.n; ++k) {
                const int b = list.index[k];
                mb.frames[k] = frames_devs[b];
                mb.std_stack[k] = std_of(b);
                mb.consts[k] = batch_item(consts_devs, b);
                mb.batch[k] = batch_sizes[b];
                n_consts += mb.consts[k] ? 1 : 0;
                if (!mi_pointers_ok(c, mb.frames[k], mb.std_stack[k])) return (int)CT_ERR_INVALID_ARGUMENT;
            }
            mb.n_batches = list.n;
            // one launch: two batches or more, constants for all of them or for none (the MULTI kernels read them per batch,
            // but a chain has a data-dependent stage or has none), and the scales of all exposures beside the LUT
            if (list.n < 2 || (n_consts != 0 && n_consts != list.n) || !merge_scales_fit(icrf, geom->channels, list.total)) return kMergePerBatch;
            const MergeIngestArgs a = mi_fill_args(c, nullptr, nullptr, nullptr, exposure_dev, (int32_t)list.total, single_flags, by_channel);
            return merge_ingest_multi(a, mb, dtype, geom->layout != CT_LAYOUT_NCHW, icrf->interp, weight_mode, std_mode, static_cast<hipStream_t>(stream));
        },
        [&](int b, uint32_t f, int64_t offset) { return single(b, std_of(b), f, offset); });
}

// ... behind a StridedDownscale(step) that the load applies (ct_merge_ingest_strided.hip): `geom` is the SOURCE frames', the state,
// the outputs and explicit uncertainties are (C, ho, wo).  One kernel family serves one batch and sixteen, so the list in one
// launch and the list walked batch by batch differ in the MergeIngestBatches block alone.
extern "C" int ct_hdr_merge_ingest_strided_batches(const void *const *frames_devs, const int32_t *batch_sizes, int32_t n_batches,
                                                   int32_t dtype, const ct_geometry *geom, int32_t step, const ct_ingest_stage *stages,
                                                   int32_t n_stages, const float *const *consts_devs, const float *const *std_devs,
                                                   int32_t std_mode, float std_value, const double *exposure_dev, const ct_icrf *icrf,
                                                   int32_t weight_mode, double *mean_state_dev, float *sumw_state_dev,
                                                   float *var_state_dev, void *mean_out_dev, float *std_out_dev, uint32_t flags,
                                                   void *stream)
{
    using namespace ct;
    if (step < 1) return CT_ERR_INVALID_ARGUMENT;
    if (step == 1)
        return ct_hdr_merge_ingest_batches(frames_devs, batch_sizes, n_batches, dtype, geom, stages, n_stages, consts_devs, std_devs, std_mode,
                                           std_value, exposure_dev, icrf, weight_mode, mean_state_dev, sumw_state_dev, var_state_dev,
                                           mean_out_dev, std_out_dev, flags, stream);
    if (!batch_list_ok(n_batches, batch_sizes, frames_devs)) return CT_ERR_INVALID_ARGUMENT;
    const uint32_t single_flags = flags & ~CT_MERGE_REQUIRE_ONE_LAUNCH;
    const MergeIngestCall c{dtype, geom, stages, n_stages, std_mode, std_value, exposure_dev, icrf, weight_mode, mean_state_dev,
                            sumw_state_dev, var_state_dev, mean_out_dev, std_out_dev, single_flags};
    auto std_of = [&](int b) { return std_mode == CT_STD_EXPLICIT ? batch_item(std_devs, b) : nullptr; };
    bool by_channel = false;
    // `batches` exposures (of the batches in mb, times at `exposure`) in one launch, on the output plane
    auto launch = [&](const MergeIngestBatches &mb, const double *exposure, int32_t batches, uint32_t f) {
        const bool packed = geom->layout != CT_LAYOUT_NCHW;
        const int64_t ho = (geom->h_tile + step - 1) / step, wo = (geom->width + step - 1) / step;
        MergeIngestArgs a = mi_fill_args(c, nullptr, nullptr, nullptr, exposure, batches, f, by_channel);  // plane, base: of step 1
        a.plane = (uint32_t)(ho * wo);  // untiled (validated): the downscaled frame is the whole image
        a.plane_global = a.plane;
        const uint32_t pe = packed ? 3u : 1u;
        const MergeIngestStride sd{(uint32_t)wo, (uint32_t)(step * geom->width * pe), (uint32_t)step * pe, (uint32_t)(geom->h_tile * geom->width)};
        return merge_ingest_strided(a, mb, sd, dtype, packed, icrf->interp, weight_mode, std_mode, static_cast<hipStream_t>(stream));
    };
    constexpr MergeBatchPolicy kPolicy{/*skip_empty*/ true, /*no_state*/ CT_ERR_INVALID_ARGUMENT, /*require_one_launch*/ CT_ERR_UNSUPPORTED};
    return merge_batches(
        batch_sizes, n_batches, flags, c.has_state(), kPolicy,
        // every batch as ct_hdr_merge_ingest_batch judges it on the source geometry (a stride that holds a SOURCE frame holds
        // the selected elements), then: no row band behind a downscale -- its phase, row_offset % step, is not carried
        [&](int b, int64_t) {
            if (const int rc = mi_validate(c, batch_sizes[b], batch_item(consts_devs, b), by_channel); rc != CT_OK) return rc;
            return geom->row_offset != 0 || geom->h_tile != geom->h_global ? (int)CT_ERR_INVALID_ARGUMENT : (int)CT_OK;
        },
        [&](const MergeBatchList &list) {
            if (list.n == 0 || c.plane() == 0) return (int)CT_OK;
            MergeIngestBatches mb = {};
            int n_consts = 0;
            for (int k = 0; k < list.n; ++k) {
                const int b = list.index[k];
                mb.frames[k] = frames_devs[b];
                mb.std_stack[k] = std_of(b);
                mb.consts[k] = batch_item(consts_devs, b);
                mb.batch[k] = batch_sizes[b];
                n_consts += mb.consts[k] ? 1 : 0;
                if (!mi_pointers_ok(c, mb.frames[k], mb.std_stack[k])) return (int)CT_ERR_INVALID_ARGUMENT;
            }
            mb.n_batches = list.n;
            // one launch: constants for all batches or for none, and the scales of all exposures beside the LUT
            if ((n_consts != 0 && n_consts != list.n) || !merge_scales_fit(icrf, geom->channels, list.total)) return kMergePerBatch;
            return launch(mb, exposure_dev, (int32_t)list.total, single_flags);
        },
        [&](int b, uint32_t f, int64_t offset) {
            MergeIngestBatches mb = {};
            mb.frames[0] = frames_devs[b];
            mb.std_stack[0] = std_of(b);
            mb.consts[0] = batch_item(consts_devs, b);
            mb.batch[0] = batch_sizes[b];
            mb.n_batches = 1;
            return launch(mb, exposure_dev + offset, batch_sizes[b], f);
        });
}
