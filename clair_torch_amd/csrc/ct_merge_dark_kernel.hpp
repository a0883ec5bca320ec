// ct_merge_dark_kernel.hpp -- what the kernels of ct_merge_dark.hip (one dark-field batch per launch) and ct_merge_dark_multi.hip
// (several per launch, the streaming state in registers in between) share: the argument blocks and md_run, the walk of one
// thread over the batch(es) of the columns it owns.  The head of ct_merge_dark.hip describes ownership, the window and the
// packets.  MULTI is a template flag of that one body, as in ct_merge_ingest_kernel.hpp: everything it adds is behind
// `if constexpr`, and the order of the text is kept so that the single-batch kernels compile to the instructions they had
// without it.  Host side: MergeDarkCall, md_validate and md_fill_args, what the dark-field merge entry points and
// ct_hdr_merge_dark_ingest_batches check and fill alike.
#pragma once
#include "ct_dark_window.hpp"
#include "ct_merge_ingest_kernel.hpp"

namespace ct {

struct MergeDarkArgs {
    const void *stack;       // (B, C, H_tile, W) T
    const void *halo;        // (B, C, 2, W) T or NULL
    const float *std_stack;  // explicit sigma of the raw image, laid out like the stack, or NULL
    const float *dark;       // (Bd, C, H_tile, W), Bd = 1 or B
    const float *dark_std;   // same shape, or NULL (then no uncertainty is propagated)
    const double *exposure;
    const float *lut;
    double *mean_state;
    float *sumw_state;
    float *var_state;
    void *mean_out;
    float *std_out;
    int64_t image_stride, dark_stride;  // elements between frames (dark_stride = 0 for one shared dark field)
    uint32_t plane;         // H_tile * W
    uint32_t plane_global;  // H_global * W
    uint32_t base;          // row_offset * W
    int32_t width, h_tile;
    uint32_t at_top, at_bottom;  // the band touches the global top / bottom: reflect there instead of reading the halo
    int32_t batch, channels, n_points;
    NormConst norm;
    int32_t std_mode;       // of the RAW image: how sigma enters sigma_eff
    float std_value, threshold, alpha;
    float k0, k1;           // the two distinct taps of the normalised 1-D kernel: k0 (centre), k1 (sides)
    float weight_scale;     // Gaussian scale (30)
    uint32_t flags;
};

// MULTI (ct_hdr_merge_dark_batches): batch b has batch[b] >= 1 exposures at stack[b] with the halo rows, explicit sigma, dark
// field and dark std of its own (dark_stride[b]: 0 for one shared dark field, C * H_tile * W for one per frame); its exposure
// times start at offset[b] of MergeDarkArgs::exposure, where those of all batches follow each other, and MergeDarkArgs::batch
// is their total.  MergeDarkArgs::stack, halo, std_stack, dark, dark_std and dark_stride are not read.
constexpr int kMaxDarkBatches = kMaxFusedBatches;
struct MergeDarkBatches {
    const void *stack[kMaxDarkBatches];
    const void *halo[kMaxDarkBatches];
    const float *std_stack[kMaxDarkBatches];
    const float *dark[kMaxDarkBatches];
    const float *dark_std[kMaxDarkBatches];
    int64_t dark_stride[kMaxDarkBatches];
    int32_t batch[kMaxDarkBatches];
    int32_t offset[kMaxDarkBatches];
    int32_t n_batches;  // 2 .. kMaxDarkBatches
};

// ct_merge_dark_multi.hip: the several-batches launch, dispatched on dtype / interpolation / weight / dark std.
// Returns a CT_* status (CT_ERR_TOO_LARGE: the LUT and the scales of all exposures exceed the LDS).
int merge_dark_multi(const MergeDarkArgs &a, const MergeDarkBatches &mb, int dtype, int interp, int weight_mode, bool has_std,
                     hipStream_t stream);

constexpr int kMdGroup = 4;  // columns per thread
constexpr int kMdPF = 2;     // samples in flight ahead of the one being reduced, as mi_run

// what dark_rows (ct_dark_window.hpp) reads of an argument block, with the halo rows of one batch of a MULTI launch
struct MdBand {
    const void *halo;
    int64_t image_stride;
    int32_t width, h_tile, channels;
    uint32_t at_top, at_bottom;
};

// Columns w0 .. w0 + G - 1 of local row h of plane c0: the whole batch, state and outputs.  STD: CT_STD_EXPLICIT (a dark std:
// sigma_eff is propagated) or CT_STD_NONE (none); the std mode of the raw image is a wave-uniform run-time branch.
// MULTI: batch 0 .. mb->n_batches - 1 in turn, each exactly as a launch of its own would run it -- pivot, sample loop,
// epilogue, conditioning test and one repeat -- with (mean, sum of weights, variance) in registers in between: the state
// arrays are read once, before batch 0 (unless it starts the merge), and written once, after the last batch; FIRST_BATCH is
// batch 0's and FINALIZE the last one's.  inv_t and cq hold the scales of all batches, concatenated.
template <typename T, int G, int INTERP, int WEIGHT, int STD, bool MULTI>
__device__ __forceinline__ void md_run(const MergeDarkArgs &a, const MergeDarkBatches *mb, const char *lds, const float *inv_t,
                                       const float *cq, uint32_t c0, uint32_t h, uint32_t w0)
{
    static_assert(STD == CT_STD_NONE || STD == CT_STD_EXPLICIT, "the merge sees sigma_eff or nothing");
    constexpr bool kHasStd = STD != CT_STD_NONE;
    constexpr bool kGauss = WEIGHT == CT_WEIGHT_GAUSS;
    constexpr int kEntry = lut_entry_bytes(INTERP);
    const int C = a.channels, L = a.n_points;
    int B = a.batch;
    const uint32_t W = (uint32_t)a.width;
    const float top = INTERP == CT_INTERP_NONE ? 1.0f : (float)(L - 1);
    const float kk = sqrtf(a.weight_scale * 1.4426950408889634f);
    const float K = -2.0f * a.weight_scale;
    const float dk_mul = kk, dk_add = -0.5f * kk;
    bool first = a.flags & CT_MERGE_FIRST_BATCH;
    const bool finalize = a.flags & CT_MERGE_FINALIZE;
    const bool keep_state = a.mean_state != nullptr;
    [[maybe_unused]] const bool explicit_sigma = a.std_mode == CT_STD_EXPLICIT;

    const uint32_t p0 = h * W + w0;         // first element inside the plane
    const uint32_t q = c0 * a.plane + p0;   // ... and inside the planar (C, plane) arrays
    int row_off[G];                         // byte offset of each element's LUT row inside the LDS table
    {
        const uint32_t qg = c0 * a.plane_global + a.base + p0;  // global flat NCHW index (< 2^31)
        int r = (int)(qg % (uint32_t)C);
#pragma unroll
        for (int e = 0; e < G; ++e) {
            row_off[e] = (INTERP == CT_INTERP_LOOKUP ? (int)c0 : r) * L * kEntry;
            ++r;
            r = r >= C ? r - C : r;
        }
    }

    // the window of this group (ct_dark_window.hpp): its rows, frame n as loaded, and xb and sigma_eff of that
    DarkRows<T> rw = dark_rows<T, G, true>(a, static_cast<const T *>(a.stack) + (int64_t)c0 * a.plane, c0, h, w0);
    const float *dark = nullptr, *dark_std = nullptr, *sigma = nullptr;  // MULTI: the batch's
    int64_t dark_stride = 0;
    auto load_raw = [&](int64_t n) {
        DarkRaw<T, G> r{};
        if constexpr (MULTI)
            dark_load<T, G, kHasStd>(r, rw, n, a.image_stride, dark, dark_std, dark_stride, explicit_sigma, sigma, q);
        else
            dark_load<T, G, kHasStd>(r, rw, n, a.image_stride, a.dark, a.dark_std, a.dark_stride, explicit_sigma, a.std_stack, q);
        return r;
    };
    auto blur = [&](const DarkRaw<T, G> &r, float (&xb)[G], float (&sig)[G]) { dark_blur<T, G, kHasStd>(a, r, explicit_sigma, xb, sig); };

    // MULTI: batch b's frames, halo rows, uncertainties, dark field and size take the place of the launch's
    int b = 0;
    const float *inv_t_all = inv_t, *cq_all = cq;
    auto select_batch = [&]() {
        B = mb->batch[b];
        const MdBand band{mb->halo[b], a.image_stride, a.width, a.h_tile, a.channels, a.at_top, a.at_bottom};
        rw = dark_rows<T, G, true>(band, static_cast<const T *>(mb->stack[b]) + (int64_t)c0 * a.plane, c0, h, w0);
        dark = mb->dark[b];
        dark_std = mb->dark_std[b];
        sigma = mb->std_stack[b];
        dark_stride = mb->dark_stride[b];
        inv_t = inv_t_all + mb->offset[b];
        cq = cq_all + mb->offset[b];
    };
    // ... and the state between the batches is in registers: what a launch per batch would have stored and read again
    constexpr int NS = MULTI ? G : 1;
    double st_mean[NS] = {};
    float st_w[NS] = {}, st_var[NS] = {};
    if constexpr (MULTI) select_batch();

    // ---- pivot: the middle exposure's sample on a first batch, else the running mean ----
    float p[G];
    if (first) {
        const int probe = B / 2;
        const DarkRaw<T, G> raw = load_raw(probe);
        const float itp = inv_t[probe];
        float xb[G], sig[G];
        blur(raw, xb, sig);
#pragma unroll
        for (int e = 0; e < G; ++e) {
            float lin, dfds;
            mi_sample<INTERP>(xb[e], lds + row_off[e], top, lin, dfds);
            p[e] = lin * itp;
        }
    } else {
        double m[G];
        mi_load(a.mean_state + q, m);
#pragma unroll
        for (int e = 0; e < G; ++e) p[e] = (float)m[e];
        if constexpr (MULTI) {  // the one read of the state
            float w[G], v[G] = {};
            mi_load(a.sumw_state + q, w);
            if constexpr (kHasStd) mi_load(a.var_state + q, v);
#pragma unroll
            for (int e = 0; e < G; ++e) {
                st_mean[e] = m[e];
                st_w[e] = w[e];
                st_var[e] = v[e];
            }
        }
    }

    // scale of the folded second moments back to true units (explicit uncertainties carry their own)
    double fs = 1.0;
    if constexpr (kGauss) fs = (double)K / (double)kk;
    const double sv2 = fs * fs;

    MiResult res[G];
    do {  // MULTI: once per batch
        for (int pass_no = 0;; ++pass_no) {
            MiSums sum[G];
#pragma unroll
            for (int k = 0; k < G; ++k) sum[k] = MiSums{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

            // software pipeline, as mi_run's: kMdPF exposures in flight per thread ahead of the one being reduced
            DarkRaw<T, G> ring[kMdPF];
#pragma unroll
            for (int k = 0; k < kMdPF; ++k) ring[k] = load_raw(k < B ? k : B - 1);
#pragma unroll kMdPF
            for (int n = 0; n < B; ++n) {
                const int nn = n + kMdPF < B ? n + kMdPF : B - 1;  // the tail re-loads the last exposure (cache hit, unused)
                // (the exposure index is laundered through an empty asm, as in merge_kernel: otherwise the compiler re-loads the
                //  sample at its point of use and the prefetch is gone)
                int64_t opaque_zero = 0;
                asm volatile("" : "+s"(opaque_zero));
                const DarkRaw<T, G> incoming = load_raw((int64_t)nn + opaque_zero);
                const DarkRaw<T, G> raw = ring[0];
#pragma unroll
                for (int k = 0; k + 1 < kMdPF; ++k) ring[k] = ring[k + 1];
                ring[kMdPF - 1] = incoming;
                const float it = inv_t[n];
                const float cqn = cq[n];
                float xb[G], sig[G], lin[G], dfds[G];
                blur(raw, xb, sig);
#pragma unroll
                for (int e = 0; e < G; ++e) mi_sample<INTERP>(xb[e], lds + row_off[e], top, lin[e], dfds[e]);  // the G gathers issue together
#pragma unroll
                for (int e = 0; e < G; ++e)
                    mi_accumulate<INTERP, WEIGHT, STD>(xb[e], lin[e], dfds[e], sig[e], it, cqn, p[e], dk_mul, dk_add, sum[e]);
            }

            bool any_bad = false;
            float WA[G] = {}, varA[G] = {};
            double meanA[G] = {};
            if constexpr (MULTI) {
#pragma unroll
                for (int e = 0; e < G; ++e) {
                    WA[e] = st_w[e];
                    meanA[e] = st_mean[e];
                    varA[e] = st_var[e];
                }
            } else if (!first) {
                mi_load(a.sumw_state + q, WA);
                mi_load(a.mean_state + q, meanA);
                if constexpr (kHasStd) mi_load(a.var_state + q, varA);
            }
#pragma unroll
            for (int e = 0; e < G; ++e) {
                res[e] = mi_epilogue<WEIGHT, STD>(sum[e], p[e], B, first, WA[e], meanA[e], varA[e], sv2);
                any_bad |= res[e].bad;
            }
            // an ill-conditioned pivot anywhere in the wavefront: repeat the batch once with those elements' pivot at the now
            // known mean; the others recompute bit-identically, so an element's result does not depend on its neighbours
            if (pass_no == 0 && __any(any_bad)) {
#pragma unroll
                for (int k = 0; k < G; ++k) p[k] = res[k].bad ? res[k].mb : p[k];
                continue;
            }
            break;
        }

        if constexpr (MULTI) {
            if (++b == mb->n_batches) break;
            // what the next batch finds as its state; its pivot is the running mean
#pragma unroll
            for (int k = 0; k < G; ++k) {
                st_mean[k] = res[k].mean;
                st_w[k] = res[k].Wt;
                st_var[k] = res[k].var;
                p[k] = (float)res[k].mean;
            }
            first = false;
            select_batch();
        }
    } while (MULTI);

    double mean[G];
    float var[G], wt[G], sd[G];
#pragma unroll
    for (int e = 0; e < G; ++e) {
        mean[e] = res[e].mean;
        var[e] = res[e].var;
        wt[e] = res[e].Wt;
        sd[e] = __builtin_amdgcn_sqrtf(var[e]);
    }
    if (keep_state) {
        mi_store<false>(a.mean_state + q, mean);
        mi_store<false>(a.sumw_state + q, wt);
        if constexpr (kHasStd) mi_store<false>(a.var_state + q, var);
    }
    if (finalize) {
        if (a.flags & CT_MERGE_MEAN_OUT_F32) {
            float m32[G];
#pragma unroll
            for (int e = 0; e < G; ++e) m32[e] = (float)mean[e];
            mi_store<true>(static_cast<float *>(a.mean_out) + q, m32);
        } else {
            mi_store<true>(static_cast<double *>(a.mean_out) + q, mean);
        }
        if constexpr (kHasStd) mi_store<true>(a.std_out + q, sd);
    }
}

// groups of G columns (or pixels) in a row, the last one possibly short
template <int G>
static inline __host__ __device__ uint32_t groups_per_row(uint32_t width)
{
    return (width + G - 1) / G;
}

// grid of a launch: one slot per group of G columns of every row, one workgroup row per plane
template <int G>
static inline dim3 md_grid(const MergeDarkArgs &a, uint32_t planes)
{
    const uint64_t slots = (uint64_t)groups_per_row<G>((uint32_t)a.width) * (uint64_t)a.h_tile;
    return dim3((uint32_t)((slots + kBlock - 1) / kBlock), planes);
}

// The modes of a dark-field family: interpolation and weight as ever; has_std (a dark std comes with the call, sigma_eff is
// propagated) is CT_STD_EXPLICIT, without one no uncertainty exists at all
template <typename F>
static int with_dark_merge_modes(int interp, int weight_mode, bool has_std, F &&f)
{
    return with_fused_merge_modes<CT_STD_NONE, CT_STD_EXPLICIT>(interp, weight_mode, has_std ? CT_STD_EXPLICIT : CT_STD_NONE, f);
}

// ---- host: the checks and the argument block the dark-field merge entry points share -------------------------------------
// What ct_hdr_merge_dark_batch and ct_hdr_merge_dark_batches have in common besides the frames and dark fields of a batch: one
// dtype, one geometry, one set of modes, the state and the outputs.
struct MergeDarkCall {
    int32_t dtype;
    float max_code;
    const ct_geometry *geom;
    int32_t std_mode;
    float std_value, threshold, alpha;
    const ct_icrf *icrf;
    int32_t weight_mode;
    double *mean_state;
    float *sumw_state, *var_state;
    void *mean_out;
    float *std_out;
    uint32_t flags;
    // has_std: a dark std comes with the call, so the variance is part of the state
    bool has_state(bool has_std) const { return mean_state && sumw_state && (!has_std || var_state); }
};

// One batch as ct_hdr_merge_dark_batch judges it, every check in its order; nothing is read.  FIRST_BATCH / FINALIZE in
// c.flags are those of the whole call.  norm: the constants of the dtype.
static inline int md_validate(const MergeDarkCall &c, const void *stack_dev, int32_t batch, const void *halo_dev, const float *std_dev,
                       const float *dark_dev, const float *dark_std_dev, int32_t dark_batch, const double *exposure_dev, NormConst &norm)
{
    const ct_geometry *geom = c.geom;
    const ct_icrf *icrf = c.icrf;
    const int32_t std_mode = c.std_mode, weight_mode = c.weight_mode;
    const uint32_t flags = c.flags;
    // ---- what ct_dark_field_blur refuses, in its order (ct_darkfield.hip); a dark std is always propagated here ----
    if (!stack_dev || !geom || !dark_dev || batch <= 0) return CT_ERR_INVALID_ARGUMENT;
    if (int rc = check_dark_frames(geom, batch, dark_batch, dark_std_dev != nullptr, std_mode, std_dev)) return rc;
    if (int rc = check_dark_band(geom, halo_dev)) return rc;
    if (norm_for_dtype(c.dtype, c.max_code, &norm) != CT_OK) return CT_ERR_UNSUPPORTED;
    // ---- what ct_hdr_merge_batch refuses for (xb, sigma_eff): float32 pixels, explicit uncertainties with a dark std and
    //      none without, in the order of validate_merge (ct_merge.hip) ----
    const bool has_std = dark_std_dev != nullptr;
    if (!icrf || !exposure_dev) return CT_ERR_INVALID_ARGUMENT;
    if (!icrf_ok(icrf)) return CT_ERR_INVALID_ARGUMENT;
    if (weight_mode != CT_WEIGHT_NONE && weight_mode != CT_WEIGHT_GAUSS) return CT_ERR_INVALID_ARGUMENT;
    const int interp = icrf->interp;
    // hdr_merge.py:107-113: autograd.grad raises when nothing connects the mean to the image
    if (has_std && interp == CT_INTERP_LOOKUP && weight_mode == CT_WEIGHT_NONE) return CT_ERR_NO_GRADIENT_PATH;
    if (!c.has_state(has_std) && !((flags & CT_MERGE_FIRST_BATCH) && (flags & CT_MERGE_FINALIZE))) return CT_ERR_INVALID_ARGUMENT;
    if ((flags & CT_MERGE_FINALIZE) && (!c.mean_out || (has_std && !c.std_out))) return CT_ERR_INVALID_ARGUMENT;
    if (!global_below_2_31(geom)) return CT_ERR_TOO_LARGE;
    // ---- what this entry point does not have: the routes of ct_hdr_merge_batch besides the closed-form float32 kernel ----
    if (flags & (CT_MERGE_F64_MOMENTS | CT_MERGE_REFERENCE_ORDER | CT_MERGE_OUT_AS_INPUT)) return CT_ERR_UNSUPPORTED;
    if ((interp == CT_INTERP_CATMULL || interp == CT_INTERP_LOOKUP) && has_std && !(flags & CT_MERGE_CLOSED_FORM)) return CT_ERR_UNSUPPORTED;
    if (!merge_scales_fit(icrf, geom->channels, batch)) return CT_ERR_TOO_LARGE;
    const size_t elem = dtype_bytes(c.dtype);
    if (!aligned(stack_dev, elem) || !aligned(halo_dev, elem) || !aligned(std_dev, sizeof(float)) || !aligned(dark_dev, sizeof(float)) ||
        !aligned(dark_std_dev, sizeof(float)) || !aligned(exposure_dev, sizeof(double)) || !aligned(c.mean_state, sizeof(double)) ||
        !aligned(c.sumw_state, sizeof(float)) || !aligned(c.var_state, sizeof(float)) ||
        !aligned(c.mean_out, (flags & CT_MERGE_MEAN_OUT_F32) ? sizeof(float) : sizeof(double)) || !aligned(c.std_out, sizeof(float)))
        return CT_ERR_INVALID_ARGUMENT;
    return CT_OK;
}

// the kernels' argument block of a validated call without what belongs to a batch (MULTI: `batch` exposures in all batches)
static inline MergeDarkArgs md_fill_args(const MergeDarkCall &c, bool has_std, NormConst norm, const double *exposure_dev, int32_t batch)
{
    const ct_geometry *geom = c.geom;
    const bool has_state = c.has_state(has_std);
    const int64_t plane = geom->h_tile * geom->width;
    MergeDarkArgs a{};
    a.exposure = exposure_dev;
    a.lut = c.icrf->lut_dev;
    a.mean_state = has_state ? c.mean_state : nullptr;
    a.sumw_state = has_state ? c.sumw_state : nullptr;
    a.var_state = has_state ? c.var_state : nullptr;
    a.mean_out = c.mean_out;
    a.std_out = c.std_out;
    a.image_stride = geom->image_stride;
    a.plane = (uint32_t)plane;
    a.plane_global = (uint32_t)(geom->h_global * geom->width);
    a.base = (uint32_t)(geom->row_offset * geom->width);
    a.width = (int32_t)geom->width;
    a.h_tile = (int32_t)geom->h_tile;
    a.at_top = geom->row_offset == 0 ? 1u : 0u;
    a.at_bottom = geom->row_offset + geom->h_tile == geom->h_global ? 1u : 0u;
    a.batch = batch;
    a.channels = geom->channels;
    a.n_points = icrf_points(c.icrf);
    fill_blur_args(a, norm, c.std_mode, c.std_value, c.threshold, c.alpha);
    a.weight_scale = 30.0f;  // gaussian_value_weights default scale, hdr_merge.py:95
    a.flags = c.flags;
    return a;
}

}  // namespace ct
