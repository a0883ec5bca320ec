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
#include "ct_ingest_stages.hpp"
#include "ct_merge_ingest.hpp"

namespace ct {

struct MergeIngestArgs {
    const void *frames;
    const float *std_stack;  // EXPLICIT: planar (B, C, plane) float32, dense
    const float *consts;     // sub, div of a CT_INGEST_AFFINE_DATA stage (ct_ingest_extrema), or NULL
    const double *exposure;
    const float *lut;
    double *mean_state;
    float *sumw_state;
    float *var_state;
    void *mean_out;
    float *std_out;
    int64_t image_stride;   // source elements between consecutive frames
    uint32_t plane;         // H_tile * W
    uint32_t plane_global;  // H_global * W: global flat index of (c, local p) = c * plane_global + base + p
    uint32_t base;          // row_offset * W
    int32_t batch, channels, n_points;
    uint32_t reversed;      // PACKED3: memory channel cm feeds plane 2 - cm (BGR)
    uint32_t by_channel;    // some clamp holds different pairs for different channels (then C <= CT_INGEST_MAX_CHANNELS)
    float std_value;
    float weight_scale;     // Gaussian scale (30)
    uint32_t flags;
    uint32_t n_stages;
    ct_ingest_stage stage[CT_INGEST_MAX_STAGES];
};

constexpr int kMiGroup = 4;        // PLANAR: output elements per thread, one 16-byte packet
constexpr int kMiPackedGroup = 2;  // PACKED3: pixels per thread (see the head of this file)
constexpr int kMiPF = 2;     // samples in flight ahead of the one being reduced

template <typename T, int N>
struct MiRaw {
    T v[N];
};

// alignment at which G values of X move as whole packets: their size, 16 bytes at the most
template <typename X, int G>
constexpr uintptr_t mi_packet_align() { return sizeof(X) * G < 16 ? sizeof(X) * G : 16; }

// G values at p[0..G): one or two packet accesses where the packet is aligned in memory, else element by element
template <typename X, int G>
__device__ __forceinline__ void mi_load(const X *p, X (&v)[G])
{
    if constexpr (G > 1) {
        constexpr uintptr_t kAlign = mi_packet_align<X, G>();
        if ((reinterpret_cast<uintptr_t>(p) & (kAlign - 1)) == 0) {
            __builtin_memcpy(v, __builtin_assume_aligned(p, kAlign), sizeof(v));
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < G; ++e) v[e] = p[e];
}

template <bool STREAM, typename X, int G>
__device__ __forceinline__ void mi_store(X *p, const X (&v)[G])
{
    if constexpr (G > 1) {
        if ((reinterpret_cast<uintptr_t>(p) & (mi_packet_align<X, G>() - 1)) == 0) {
            Packet<X, G> o;
#pragma unroll
            for (int e = 0; e < G; ++e) o.v[e] = v[e];
            if constexpr (STREAM)
                store_stream(reinterpret_cast<Packet<X, G> *>(p), o);  // outputs: written once, never re-read here
            else
                *reinterpret_cast<Packet<X, G> *>(p) = o;
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < G; ++e) p[e] = v[e];
}

// G consecutive elements of every plane the thread owns, from local pixel p0: the whole batch, state and outputs
template <typename T, bool PACKED, int G, int INTERP, int WEIGHT, int STD>
__device__ __forceinline__ void mi_run(const MergeIngestArgs &a, const char *lds, const float *inv_t, const float *cq, uint32_t c0,
                                       uint32_t p0, float dsub, float ddiv)
{
    constexpr int NP = PACKED ? 3 : 1;  // planes per thread
    constexpr int NE = NP * G;
    constexpr bool kHasStd = STD != CT_STD_NONE;
    constexpr bool kGauss = WEIGHT == CT_WEIGHT_GAUSS;
    constexpr int kEntry = lut_entry_bytes(INTERP);
    const int C = a.channels, L = a.n_points, B = a.batch;
    const float top = INTERP == CT_INTERP_NONE ? 1.0f : (float)(L - 1);
    const float kk = sqrtf(a.weight_scale * 1.4426950408889634f);
    const float K = -2.0f * a.weight_scale;
    const float dk_mul = kk, dk_add = -0.5f * kk;
    const bool first = a.flags & CT_MERGE_FIRST_BATCH;
    const bool finalize = a.flags & CT_MERGE_FINALIZE;
    const bool keep_state = a.mean_state != nullptr;

    uint32_t cj[NP];   // plane of the state / outputs (wave-uniform)
    uint32_t q[NP];    // index of the first element in the planar (C, plane) arrays
    int row_off[NE];   // byte offset of each element's LUT row inside the LDS table
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        cj[j] = PACKED ? (a.reversed ? (uint32_t)(NP - 1 - j) : (uint32_t)j) : c0;
        q[j] = cj[j] * a.plane + p0;
        const uint32_t qg = cj[j] * a.plane_global + a.base + p0;  // global flat NCHW index (< 2^31)
        int r = PACKED ? (int)(qg % 3u) : (int)(qg % (uint32_t)C);
#pragma unroll
        for (int e = 0; e < G; ++e) {
            row_off[j * G + e] = (INTERP == CT_INTERP_LOOKUP ? (int)cj[j] : r) * L * kEntry;
            ++r;
            r = r >= C ? r - C : r;
        }
    }
    const T *src = static_cast<const T *>(a.frames) + (PACKED ? (int64_t)p0 * NP : (int64_t)c0 * a.plane + p0);
    const int64_t std_stride = (int64_t)C * a.plane;  // the explicit uncertainties are planar and dense

    auto load_raw = [&](int64_t frame_offset) {
        MiRaw<T, NE> r;
        __builtin_memcpy(&r, src + frame_offset, sizeof(r));  // any alignment: planes are only element-aligned in general
        return r;
    };
    // the G pixels of plane j behind the chain
    auto pixels = [&](const MiRaw<T, NE> &raw, int j, float (&x)[G]) {
#pragma unroll
        for (int e = 0; e < G; ++e) x[e] = (float)raw.v[e * NP + j];
        ingest_stages<true>(x, a, a.by_channel ? cj[j] : 0u, dsub, ddiv);
    };

    // ---- pivot: the middle exposure's sample on a first batch, else the running mean ----
    float p[NE];
    if (first) {
        const int probe = B / 2;
        const MiRaw<T, NE> raw = load_raw((int64_t)probe * a.image_stride);
        const float itp = inv_t[probe];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            float x[G];
            pixels(raw, j, x);
#pragma unroll
            for (int e = 0; e < G; ++e) {
                float lin, dfds;
                mi_sample<INTERP>(x[e], lds + row_off[j * G + e], top, lin, dfds);
                p[j * G + e] = lin * itp;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            double m[G];
            mi_load(a.mean_state + q[j], m);
#pragma unroll
            for (int e = 0; e < G; ++e) p[j * G + e] = (float)m[e];
        }
    }

    // scale of the folded second moments back to true units
    double fs = 1.0;
    if constexpr (kGauss) fs = (double)K / (double)kk;
    if constexpr (STD == CT_STD_CONSTANT || STD == CT_STD_MULTIPLIER) fs *= (double)a.std_value;
    const double sv2 = fs * fs;

    MiResult res[NE];
    for (int pass_no = 0;; ++pass_no) {
        MiSums sum[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) sum[k] = MiSums{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

        // software pipeline, as merge_kernel's: kMiPF loads in flight per thread ahead of the sample being reduced
        MiRaw<T, NE> ring[kMiPF];
        float sring[STD == CT_STD_EXPLICIT ? kMiPF : 1][NE];
        auto load_std = [&](int64_t nn, float (&sg)[NE]) {
#pragma unroll
            for (int j = 0; j < NP; ++j) __builtin_memcpy(&sg[j * G], a.std_stack + nn * std_stride + q[j], G * sizeof(float));
        };
#pragma unroll
        for (int k = 0; k < kMiPF; ++k) {
            const int nn = k < B ? k : B - 1;
            ring[k] = load_raw((int64_t)nn * a.image_stride);
            if constexpr (STD == CT_STD_EXPLICIT) load_std(nn, sring[k]);
        }
#pragma unroll kMiPF
        for (int n = 0; n < B; ++n) {
            const int nn = n + kMiPF < B ? n + kMiPF : B - 1;  // the tail re-loads the last exposure (cache hit, unused)
            // (the exposure index is laundered through an empty asm, as in merge_kernel: otherwise the compiler re-loads the
            //  sample at its point of use and the prefetch is gone)
            int64_t opaque_zero = 0;
            asm volatile("" : "+s"(opaque_zero));
            const int64_t nl = (int64_t)nn + opaque_zero;
            const MiRaw<T, NE> incoming = load_raw(nl * a.image_stride);
            float sincoming[NE];
            if constexpr (STD == CT_STD_EXPLICIT) load_std(nl, sincoming);
            const MiRaw<T, NE> raw = ring[0];
            float sg[NE];
#pragma unroll
            for (int k = 0; k < NE; ++k) sg[k] = STD == CT_STD_EXPLICIT ? sring[0][k] : 1.0f;
#pragma unroll
            for (int k = 0; k + 1 < kMiPF; ++k) {
                ring[k] = ring[k + 1];
                if constexpr (STD == CT_STD_EXPLICIT) {
#pragma unroll
                    for (int i = 0; i < NE; ++i) sring[k][i] = sring[k + 1][i];
                }
            }
            ring[kMiPF - 1] = incoming;
            if constexpr (STD == CT_STD_EXPLICIT) {
#pragma unroll
                for (int i = 0; i < NE; ++i) sring[kMiPF - 1][i] = sincoming[i];
            }
            const float it = inv_t[n];
            const float cqn = cq[n];
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                float x[G], lin[G], dfds[G];
                pixels(raw, j, x);
#pragma unroll
                for (int e = 0; e < G; ++e) mi_sample<INTERP>(x[e], lds + row_off[j * G + e], top, lin[e], dfds[e]);  // the G gathers issue together
#pragma unroll
                for (int e = 0; e < G; ++e)
                    mi_accumulate<INTERP, WEIGHT, STD>(x[e], lin[e], dfds[e], sg[j * G + e], it, cqn, p[j * G + e], dk_mul, dk_add,
                                                       sum[j * G + e]);
            }
        }

        bool any_bad = false;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            float WA[G] = {}, varA[G] = {};
            double meanA[G] = {};
            if (!first) {
                mi_load(a.sumw_state + q[j], WA);
                mi_load(a.mean_state + q[j], meanA);
                if constexpr (kHasStd) mi_load(a.var_state + q[j], varA);
            }
#pragma unroll
            for (int e = 0; e < G; ++e) {
                const int k = j * G + e;
                res[k] = mi_epilogue<WEIGHT, STD>(sum[k], p[k], B, first, WA[e], meanA[e], varA[e], sv2);
                any_bad |= res[k].bad;
            }
        }
        // an ill-conditioned pivot anywhere in the wavefront: repeat the batch once with those elements' pivot at the now
        // known mean; the others recompute bit-identically, so an element's result does not depend on its neighbours
        if (pass_no == 0 && __any(any_bad)) {
#pragma unroll
            for (int k = 0; k < NE; ++k) p[k] = res[k].bad ? res[k].mb : p[k];
            continue;
        }
        break;
    }

#pragma unroll
    for (int j = 0; j < NP; ++j) {
        double mean[G];
        float var[G], wt[G], sd[G];
#pragma unroll
        for (int e = 0; e < G; ++e) {
            mean[e] = res[j * G + e].mean;
            var[e] = res[j * G + e].var;
            wt[e] = res[j * G + e].Wt;
            sd[e] = __builtin_amdgcn_sqrtf(var[e]);
        }
        if (keep_state) {
            mi_store<false>(a.mean_state + q[j], mean);
            mi_store<false>(a.sumw_state + q[j], wt);
            if constexpr (kHasStd) mi_store<false>(a.var_state + q[j], var);
        }
        if (finalize) {
            if (a.flags & CT_MERGE_MEAN_OUT_F32) {
                float m32[G];
#pragma unroll
                for (int e = 0; e < G; ++e) m32[e] = (float)mean[e];
                mi_store<true>(static_cast<float *>(a.mean_out) + q[j], m32);
            } else {
                mi_store<true>(static_cast<double *>(a.mean_out) + q[j], mean);
            }
            if constexpr (kHasStd) mi_store<true>(a.std_out + q[j], sd);
        }
    }
}

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
        mi_run<T, PACKED, (int)kG, INTERP, WEIGHT, STD>(a, lds, inv_t, cq, c0, p0, dsub, ddiv);
        return;
    }
    // a plane's head and tail (at most kG - 1 elements each): one lane, one element (pixel) after the other, each with its
    // own walk over the batch -- a few serial batches of latency in two lanes per plane, nothing next to a plane's packets
#pragma unroll 1
    for (uint32_t k = 0; k < n; ++k) mi_run<T, PACKED, 1, INTERP, WEIGHT, STD>(a, lds, inv_t, cq, c0, p0 + k, dsub, ddiv);
}

template <typename T, bool PACKED, int INTERP, int WEIGHT, int STD>
static int mi_launch(const MergeIngestArgs &a, hipStream_t s)
{
    if constexpr (INTERP == CT_INTERP_LOOKUP && WEIGHT == CT_WEIGHT_NONE && STD != CT_STD_NONE) {
        return CT_ERR_NO_GRADIENT_PATH;  // (refused by the entry point before it gets here)
    } else {
        const size_t lds = (INTERP == CT_INTERP_NONE ? 0 : (size_t)a.channels * a.n_points * lut_entry_bytes(INTERP)) +
                           2 * sizeof(float) * (size_t)a.batch;
        constexpr uint64_t kG = PACKED ? kMiPackedGroup : kMiGroup;
        const uint64_t slots = 1 + ((uint64_t)a.plane + kG - 1) / kG;
        const dim3 grid((uint32_t)((slots + kBlock - 1) / kBlock), PACKED ? 1u : (uint32_t)a.channels);
        hipLaunchKernelGGL((merge_ingest_kernel<T, PACKED, INTERP, WEIGHT, STD>), grid, dim3(kBlock), lds, s, a);
        return hipGetLastError() == hipSuccess ? CT_OK : CT_ERR_LAUNCH;
    }
}

template <typename T, bool PACKED>
static int mi_dispatch(const MergeIngestArgs &a, int interp, int weight_mode, int std_mode, hipStream_t s)
{
    return with_enum<CT_INTERP_LOOKUP, CT_INTERP_LINEAR, CT_INTERP_CATMULL, CT_INTERP_NONE>(interp, [&](auto I) {
        return with_enum<CT_WEIGHT_NONE, CT_WEIGHT_GAUSS>(weight_mode, [&](auto W) {
            return with_enum<CT_STD_NONE, CT_STD_CONSTANT, CT_STD_MULTIPLIER, CT_STD_EXPLICIT>(
                std_mode, [&](auto S) { return mi_launch<T, PACKED, I, W, S>(a, s); });
        });
    });
}

}  // namespace ct

extern "C" int ct_hdr_merge_ingest_batch(const void *frames_dev, int32_t dtype, int32_t batch, const ct_geometry *geom,
                                         const ct_ingest_stage *stages, int32_t n_stages, const float *consts_dev,
                                         const float *std_dev, int32_t std_mode, float std_value, const double *exposure_dev,
                                         const ct_icrf *icrf, int32_t weight_mode, double *mean_state_dev, float *sumw_state_dev,
                                         float *var_state_dev, void *mean_out_dev, float *std_out_dev, uint32_t flags, void *stream)
{
    using namespace ct;
    // everything that needs no pointer into device memory first: geometry and modes (as ct_hdr_merge_batch), the stack and
    // the stage list (as ct_ingest_transform / _data), the flags this entry point does not take
    if (!geom || !icrf) return CT_ERR_INVALID_ARGUMENT;
    if (geom->channels <= 0 || geom->h_tile < 0 || geom->width < 0 || geom->h_global < geom->h_tile || geom->row_offset < 0 ||
        geom->row_offset + geom->h_tile > geom->h_global)
        return CT_ERR_INVALID_ARGUMENT;
    if (geom->layout < CT_LAYOUT_NCHW || geom->layout > CT_LAYOUT_NHWC_BGR) return CT_ERR_INVALID_ARGUMENT;
    if (geom->h_global * geom->width * geom->channels >= (int64_t)1 << 31) return CT_ERR_TOO_LARGE;
    const int64_t plane = geom->h_tile * geom->width;
    bool by_channel = false;
    int rc = ingest_validate(dtype, geom->layout, batch, geom->channels, plane, stages, n_stages, CT_INGEST_MAX_STAGES,
                             consts_dev ? 1 : 0, by_channel);
    if (rc != CT_OK) return rc;
    if (dtype == CT_DTYPE_F32) return CT_ERR_UNSUPPORTED;  // float32 pixels have no copy to save: ct_hdr_merge_batch takes them
    if (reinterpret_cast<uintptr_t>(consts_dev) % sizeof(float) != 0) return CT_ERR_INVALID_ARGUMENT;
    const int interp = icrf->interp;
    if (interp < CT_INTERP_LOOKUP || interp > CT_INTERP_NONE) return CT_ERR_INVALID_ARGUMENT;
    if (interp != CT_INTERP_NONE && (!icrf->lut_dev || icrf->n_points < 2)) return CT_ERR_INVALID_ARGUMENT;
    if (std_mode < CT_STD_NONE || std_mode > CT_STD_EXPLICIT) return CT_ERR_INVALID_ARGUMENT;
    if (weight_mode != CT_WEIGHT_NONE && weight_mode != CT_WEIGHT_GAUSS) return CT_ERR_INVALID_ARGUMENT;
    // hdr_merge.py:107-113: autograd.grad raises when nothing connects the mean to the image
    if (std_mode != CT_STD_NONE && interp == CT_INTERP_LOOKUP && weight_mode == CT_WEIGHT_NONE) return CT_ERR_NO_GRADIENT_PATH;
    if (flags & (CT_MERGE_F64_MOMENTS | CT_MERGE_REFERENCE_ORDER | CT_MERGE_OUT_AS_INPUT)) return CT_ERR_UNSUPPORTED;
    // what ct_hdr_merge_batch sends to the reference-order kernel (float64-VALU bound: its bytes are not what it waits for)
    if ((interp == CT_INTERP_CATMULL || interp == CT_INTERP_LOOKUP) && std_mode != CT_STD_NONE && !(flags & CT_MERGE_CLOSED_FORM))
        return CT_ERR_UNSUPPORTED;
    const bool has_state = mean_state_dev && sumw_state_dev && (std_mode == CT_STD_NONE || var_state_dev);
    if (!has_state && !((flags & CT_MERGE_FIRST_BATCH) && (flags & CT_MERGE_FINALIZE))) return CT_ERR_INVALID_ARGUMENT;
    if ((flags & CT_MERGE_FINALIZE) && (!mean_out_dev || (std_mode != CT_STD_NONE && !std_out_dev))) return CT_ERR_INVALID_ARGUMENT;
    if (geom->image_stride < plane * geom->channels) return CT_ERR_INVALID_ARGUMENT;
    const int n_points = interp == CT_INTERP_NONE ? 2 : icrf->n_points;
    if ((interp == CT_INTERP_NONE ? 0 : (size_t)geom->channels * (size_t)n_points * lut_entry_bytes(interp)) +
            2 * sizeof(float) * (size_t)batch > 160 * 1024)
        return CT_ERR_TOO_LARGE;
    if (batch == 0 || plane == 0) return CT_OK;
    auto aligned = [](const void *p, uintptr_t b) { return reinterpret_cast<uintptr_t>(p) % b == 0; };
    if (!frames_dev || !exposure_dev || (std_mode == CT_STD_EXPLICIT && !std_dev)) return CT_ERR_INVALID_ARGUMENT;
    if (!aligned(frames_dev, dtype == CT_DTYPE_U16 ? 2 : 1) || !aligned(exposure_dev, sizeof(double)) || !aligned(std_dev, sizeof(float)) ||
        !aligned(mean_state_dev, sizeof(double)) || !aligned(sumw_state_dev, sizeof(float)) || !aligned(var_state_dev, sizeof(float)) ||
        !aligned(mean_out_dev, (flags & CT_MERGE_MEAN_OUT_F32) ? sizeof(float) : sizeof(double)) || !aligned(std_out_dev, sizeof(float)))
        return CT_ERR_INVALID_ARGUMENT;
    MergeIngestArgs a = {};
    a.frames = frames_dev;
    a.std_stack = std_mode == CT_STD_EXPLICIT ? std_dev : nullptr;
    a.consts = consts_dev;
    a.exposure = exposure_dev;
    a.lut = icrf->lut_dev;
    a.mean_state = has_state ? mean_state_dev : nullptr;
    a.sumw_state = has_state ? sumw_state_dev : nullptr;
    a.var_state = has_state ? var_state_dev : nullptr;
    a.mean_out = mean_out_dev;
    a.std_out = std_out_dev;
    a.image_stride = geom->image_stride;
    a.plane = (uint32_t)plane;
    a.plane_global = (uint32_t)(geom->h_global * geom->width);
    a.base = (uint32_t)(geom->row_offset * geom->width);
    a.batch = batch;
    a.channels = geom->channels;
    a.n_points = n_points;
    a.reversed = geom->layout == CT_LAYOUT_NHWC_BGR ? 1u : 0u;
    a.by_channel = by_channel ? 1u : 0u;
    a.std_value = std_value;
    a.weight_scale = 30.0f;  // gaussian_value_weights default scale, hdr_merge.py:95
    a.flags = flags;
    a.n_stages = (uint32_t)n_stages;
    for (int32_t k = 0; k < n_stages; ++k) a.stage[k] = stages[k];
    const bool packed = geom->layout != CT_LAYOUT_NCHW;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == CT_DTYPE_U8)
        return packed ? mi_dispatch<uint8_t, true>(a, interp, weight_mode, std_mode, s) : mi_dispatch<uint8_t, false>(a, interp, weight_mode, std_mode, s);
    return packed ? mi_dispatch<uint16_t, true>(a, interp, weight_mode, std_mode, s) : mi_dispatch<uint16_t, false>(a, interp, weight_mode, std_mode, s);
}
