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

constexpr int kMdGroup = 4;  // columns per thread
constexpr int kMdPF = 2;     // samples in flight ahead of the one being reduced, as mi_run

// Columns w0 .. w0 + G - 1 of local row h of plane c0: the whole batch, state and outputs.  STD: CT_STD_EXPLICIT (a dark std:
// sigma_eff is propagated) or CT_STD_NONE (none); the std mode of the raw image is a wave-uniform run-time branch.
template <typename T, int G, int INTERP, int WEIGHT, int STD>
__device__ __forceinline__ void md_run(const MergeDarkArgs &a, const char *lds, const float *inv_t, const float *cq, uint32_t c0,
                                       uint32_t h, uint32_t w0)
{
    static_assert(STD == CT_STD_NONE || STD == CT_STD_EXPLICIT, "the merge sees sigma_eff or nothing");
    constexpr bool kHasStd = STD != CT_STD_NONE;
    constexpr bool kGauss = WEIGHT == CT_WEIGHT_GAUSS;
    constexpr int kEntry = lut_entry_bytes(INTERP);
    const int C = a.channels, L = a.n_points, B = a.batch;
    const uint32_t W = (uint32_t)a.width;
    const float top = INTERP == CT_INTERP_NONE ? 1.0f : (float)(L - 1);
    const float kk = sqrtf(a.weight_scale * 1.4426950408889634f);
    const float K = -2.0f * a.weight_scale;
    const float dk_mul = kk, dk_add = -0.5f * kk;
    const bool first = a.flags & CT_MERGE_FIRST_BATCH;
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
    const DarkRows<T> rw = dark_rows<T, G, true>(a, static_cast<const T *>(a.stack) + (int64_t)c0 * a.plane, c0, h, w0);
    auto load_raw = [&](int64_t n) {
        DarkRaw<T, G> r{};
        dark_load<T, G, kHasStd>(r, rw, n, a.image_stride, a.dark, a.dark_std, a.dark_stride, explicit_sigma, a.std_stack, q);
        return r;
    };
    auto blur = [&](const DarkRaw<T, G> &r, float (&xb)[G], float (&sig)[G]) { dark_blur<T, G, kHasStd>(a, r, explicit_sigma, xb, sig); };

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
    }

    // scale of the folded second moments back to true units (explicit uncertainties carry their own)
    double fs = 1.0;
    if constexpr (kGauss) fs = (double)K / (double)kk;
    const double sv2 = fs * fs;

    MiResult res[G];
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
        if (!first) {
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

// groups of kMdGroup columns in a row, the last one possibly short
static inline __host__ __device__ uint32_t md_groups_per_row(uint32_t width) { return (width + kMdGroup - 1) / kMdGroup; }

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
        md_run<T, kMdGroup, INTERP, WEIGHT, STD>(a, lds, inv_t, cq, c0, h, w0);
        return;
    }
    // the end of a row whose width is no multiple of the group (at most kMdGroup - 1 elements): one lane, one element after
    // the other, each with its own walk over the batch
#pragma unroll 1
    for (uint32_t w = w0; w < W; ++w) md_run<T, 1, INTERP, WEIGHT, STD>(a, lds, inv_t, cq, c0, h, w);
}

template <typename T, int INTERP, int WEIGHT, int STD>
static int md_launch(const MergeDarkArgs &a, hipStream_t s)
{
    if constexpr (INTERP == CT_INTERP_LOOKUP && WEIGHT == CT_WEIGHT_NONE && STD != CT_STD_NONE) {
        return CT_ERR_NO_GRADIENT_PATH;  // (refused by the entry point before it gets here)
    } else {
        const size_t lds = mi_lds_bytes(INTERP, a.channels, a.n_points, a.batch);
        const uint64_t slots = (uint64_t)md_groups_per_row((uint32_t)a.width) * (uint64_t)a.h_tile;
        const dim3 grid((uint32_t)((slots + kBlock - 1) / kBlock), (uint32_t)a.channels);
        hipLaunchKernelGGL((merge_dark_kernel<T, INTERP, WEIGHT, STD>), grid, dim3(kBlock), lds, s, a);
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

}  // namespace ct

extern "C" int ct_hdr_merge_dark_batch(const void *stack_dev, int32_t dtype, float max_code, int32_t batch, const ct_geometry *geom,
                                       const void *halo_dev, const float *std_dev, int32_t std_mode, float std_value,
                                       const float *dark_dev, const float *dark_std_dev, int32_t dark_batch, float threshold,
                                       float alpha, const double *exposure_dev, const ct_icrf *icrf, int32_t weight_mode,
                                       double *mean_state_dev, float *sumw_state_dev, float *var_state_dev, void *mean_out_dev,
                                       float *std_out_dev, uint32_t flags, void *stream)
{
    using namespace ct;
    // ---- what ct_dark_field_blur refuses, in its order (ct_darkfield.hip); a dark std is always propagated here ----
    if (!stack_dev || !geom || !dark_dev || batch <= 0) return CT_ERR_INVALID_ARGUMENT;
    if (int rc = check_dark_frames(geom, batch, dark_batch, dark_std_dev != nullptr, std_mode, std_dev)) return rc;
    if (int rc = check_dark_band(geom, halo_dev)) return rc;
    NormConst norm;
    if (norm_for_dtype(dtype, max_code, &norm) != CT_OK) return CT_ERR_UNSUPPORTED;
    // ---- what ct_hdr_merge_batch refuses for (xb, sigma_eff): float32 pixels, explicit uncertainties with a dark std and
    //      none without, in the order of validate_merge (ct_merge.hip) ----
    const bool has_std = dark_std_dev != nullptr;
    if (!icrf || !exposure_dev) return CT_ERR_INVALID_ARGUMENT;
    if (!icrf_ok(icrf)) return CT_ERR_INVALID_ARGUMENT;
    if (weight_mode != CT_WEIGHT_NONE && weight_mode != CT_WEIGHT_GAUSS) return CT_ERR_INVALID_ARGUMENT;
    const int interp = icrf->interp;
    // hdr_merge.py:107-113: autograd.grad raises when nothing connects the mean to the image
    if (has_std && interp == CT_INTERP_LOOKUP && weight_mode == CT_WEIGHT_NONE) return CT_ERR_NO_GRADIENT_PATH;
    const bool has_state = mean_state_dev && sumw_state_dev && (!has_std || var_state_dev);
    if (!has_state && !((flags & CT_MERGE_FIRST_BATCH) && (flags & CT_MERGE_FINALIZE))) return CT_ERR_INVALID_ARGUMENT;
    if ((flags & CT_MERGE_FINALIZE) && (!mean_out_dev || (has_std && !std_out_dev))) return CT_ERR_INVALID_ARGUMENT;
    if (!global_below_2_31(geom)) return CT_ERR_TOO_LARGE;
    // ---- what this entry point does not have: the routes of ct_hdr_merge_batch besides the closed-form float32 kernel ----
    if (flags & (CT_MERGE_F64_MOMENTS | CT_MERGE_REFERENCE_ORDER | CT_MERGE_OUT_AS_INPUT)) return CT_ERR_UNSUPPORTED;
    if ((interp == CT_INTERP_CATMULL || interp == CT_INTERP_LOOKUP) && has_std && !(flags & CT_MERGE_CLOSED_FORM)) return CT_ERR_UNSUPPORTED;
    const int n_points = icrf_points(icrf);
    if (mi_lds_bytes(interp, geom->channels, n_points, batch) > kLdsBudget) return CT_ERR_TOO_LARGE;
    const size_t elem = dtype_bytes(dtype);
    if (!aligned(stack_dev, elem) || !aligned(halo_dev, elem) || !aligned(std_dev, sizeof(float)) || !aligned(dark_dev, sizeof(float)) ||
        !aligned(dark_std_dev, sizeof(float)) || !aligned(exposure_dev, sizeof(double)) || !aligned(mean_state_dev, sizeof(double)) ||
        !aligned(sumw_state_dev, sizeof(float)) || !aligned(var_state_dev, sizeof(float)) ||
        !aligned(mean_out_dev, (flags & CT_MERGE_MEAN_OUT_F32) ? sizeof(float) : sizeof(double)) || !aligned(std_out_dev, sizeof(float)))
        return CT_ERR_INVALID_ARGUMENT;

    const int64_t plane = geom->h_tile * geom->width;
    MergeDarkArgs a{};
    a.stack = stack_dev;
    a.halo = halo_dev;
    a.std_stack = std_mode == CT_STD_EXPLICIT ? std_dev : nullptr;
    a.dark = dark_dev;
    a.dark_std = dark_std_dev;
    a.exposure = exposure_dev;
    a.lut = icrf->lut_dev;
    a.mean_state = has_state ? mean_state_dev : nullptr;
    a.sumw_state = has_state ? sumw_state_dev : nullptr;
    a.var_state = has_state ? var_state_dev : nullptr;
    a.mean_out = mean_out_dev;
    a.std_out = std_out_dev;
    a.image_stride = geom->image_stride;
    a.dark_stride = dark_batch == 1 ? 0 : plane * geom->channels;
    a.plane = (uint32_t)plane;
    a.plane_global = (uint32_t)(geom->h_global * geom->width);
    a.base = (uint32_t)(geom->row_offset * geom->width);
    a.width = (int32_t)geom->width;
    a.h_tile = (int32_t)geom->h_tile;
    a.at_top = geom->row_offset == 0 ? 1u : 0u;
    a.at_bottom = geom->row_offset + geom->h_tile == geom->h_global ? 1u : 0u;
    a.batch = batch;
    a.channels = geom->channels;
    a.n_points = n_points;
    fill_blur_args(a, norm, std_mode, std_value, threshold, alpha);
    a.weight_scale = 30.0f;  // gaussian_value_weights default scale, hdr_merge.py:95
    a.flags = flags;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case CT_DTYPE_U8: return md_dispatch<uint8_t>(a, interp, weight_mode, has_std, s);
        case CT_DTYPE_U16: return md_dispatch<uint16_t>(a, interp, weight_mode, has_std, s);
        default: return md_dispatch<float>(a, interp, weight_mode, has_std, s);
    }
}
