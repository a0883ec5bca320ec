// ct_merge_ingest_kernel.hpp -- what the kernels of ct_merge_ingest.hip (one batch per launch) and ct_merge_ingest_multi.hip
// (several batches per launch, the streaming state in registers in between) share: the argument blocks and mi_run, the walk of
// one thread over the batch(es) of the elements it owns.  The head of ct_merge_ingest.hip describes ownership, packets and
// the element-by-element walk.  MULTI is a template flag of that one body; everything it adds is behind `if constexpr`, and
// the order of the text is kept so that the single-batch kernels compile to the instructions they had without it; STRIDED
// (ct_merge_ingest_strided.hip: a StridedDownscale applied by the load) is a second such flag, under the same rule.  The
// workgroups around mi_run are written out in the two .hip files: shared as a function they compile to other instructions
// (profiles/merge_fused_refactor_ab.md).  Host side, what the three fused families (this one, ct_merge_dark_kernel.hpp and
// ct_merge_dark_ingest_kernel.hpp) have in front of a launch, one copy each: the dtype and mode dispatch (with_code_dtype,
// with_pixel_dtype, with_fused_merge_modes), the launch (merge_fused_launch) and the walk over a batch list (merge_batches).
#pragma once
#include "ct_args.hpp"
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

// MULTI (ct_hdr_merge_ingest_batches): batch b has batch[b] >= 1 exposures at frames[b] (explicit uncertainties at
// std_stack[b], the constants of a data-dependent Normalize at consts[b] or NULL); the exposure times of all batches follow
// each other in MergeIngestArgs::exposure and MergeIngestArgs::batch is their total.  MergeIngestArgs::frames, std_stack and
// consts are not read.
constexpr int kMaxFusedBatches = 16;  // of every fused family: the lists of the three entry points are one size
constexpr int kMaxIngestBatches = kMaxFusedBatches;
struct MergeIngestBatches {
    const void *frames[kMaxIngestBatches];
    const float *std_stack[kMaxIngestBatches];
    const float *consts[kMaxIngestBatches];
    int32_t batch[kMaxIngestBatches];
    int32_t n_batches;  // 2 .. kMaxIngestBatches
};

// ct_merge_ingest_multi.hip: the several-batches launch, dispatched on dtype / layout / interpolation / weight / std mode.
// Returns a CT_* status (CT_ERR_TOO_LARGE: the LUT and the scales of all exposures exceed the LDS).
int merge_ingest_multi(const MergeIngestArgs &a, const MergeIngestBatches &mb, int dtype, bool packed, int interp, int weight_mode,
                       int std_mode, hipStream_t stream);

// LDS of a launch over `batch` exposures: the LUT, 1 / t_n and the derivative scales
inline size_t mi_lds_bytes(int interp, int channels, int n_points, int64_t batch)
{
    return lut_lds_bytes(interp, channels, n_points) + 2 * sizeof(float) * (size_t)batch;
}

// ct_merge_ingest_strided.hip: a StridedDownscale(step) in front of the chain, applied by the load.  MergeIngestArgs then
// describes the OUTPUT (plane = plane_global = ho * wo, base = 0; image_stride stays the source's) and this block the source.
struct MergeIngestStride {
    uint32_t wo;            // output columns
    uint32_t row_stride;    // source elements between selected rows: step * W (interleaved: step * 3 W)
    uint32_t pixel_stride;  // ... between selected pixels of a row: step (interleaved: 3 step)
    uint32_t src_plane;     // planar: source elements per plane, H * W
};

// ct_merge_ingest_strided.hip: 1 .. kMaxIngestBatches batches behind a downscale in one launch of the STRIDED kernels
int merge_ingest_strided(const MergeIngestArgs &a, const MergeIngestBatches &mb, const MergeIngestStride &sd, int dtype, bool packed,
                         int interp, int weight_mode, int std_mode, hipStream_t stream);

constexpr int kMiGroup = 4;        // PLANAR: output elements per thread, one 16-byte packet
constexpr int kMiPackedGroup = 2;  // PACKED3: pixels per thread (see the head of ct_merge_ingest.hip)
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

// G consecutive elements of every plane the thread owns, from local pixel p0: the whole batch, state and outputs.
// MULTI: batch 0 .. mb->n_batches - 1 in turn, each exactly as a launch of its own would run it -- pivot, sample loop,
// epilogue, conditioning test and one repeat -- with (mean, sum of weights, variance) in registers in between: the state
// arrays are read once, before batch 0 (unless it starts the merge), and written once, after the last batch; FIRST_BATCH
// is batch 0's and FINALIZE the last one's.  inv_t and cq hold the scales of all batches, concatenated.
// STRIDED (ct_merge_ingest_strided.hip): p0 and everything in `a` but image_stride are OUTPUT coordinates of a downscale; the
// source of output element p = i * wo + j is row i * step, column j * step of the same plane (frame), so the one dense load
// per exposure becomes one load per selected element (pixel) from offsets computed once -- nothing else changes.
template <typename T, bool PACKED, int G, int INTERP, int WEIGHT, int STD, bool MULTI, bool STRIDED = false>
__device__ __forceinline__ void mi_run(const MergeIngestArgs &a, const MergeIngestBatches *mb, const char *lds, const float *inv_t,
                                       const float *cq, uint32_t c0, uint32_t p0, float dsub, float ddiv,
                                       const MergeIngestStride *sd = nullptr)
{
    constexpr int NP = PACKED ? 3 : 1;  // planes per thread
    constexpr int NE = NP * G;
    constexpr bool kHasStd = STD != CT_STD_NONE;
    constexpr bool kGauss = WEIGHT == CT_WEIGHT_GAUSS;
    constexpr int kEntry = lut_entry_bytes(INTERP);
    const int C = a.channels, L = a.n_points;
    int B = a.batch;
    const float top = INTERP == CT_INTERP_NONE ? 1.0f : (float)(L - 1);
    const float kk = sqrtf(a.weight_scale * 1.4426950408889634f);
    const float K = -2.0f * a.weight_scale;
    const float dk_mul = kk, dk_add = -0.5f * kk;
    bool first = a.flags & CT_MERGE_FIRST_BATCH;
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
    // STRIDED: (i, j) of element p0 with one division, carried over the end of an output row; i < ho and j < wo for all G
    // elements (the caller hands over whole groups inside the plane), so every offset lies inside the source plane (frame)
    [[maybe_unused]] uint32_t off[STRIDED ? G : 1];
    if constexpr (STRIDED) {
        uint32_t i = p0 / sd->wo, j = p0 - i * sd->wo;
#pragma unroll
        for (int e = 0; e < G; ++e) {
            off[e] = i * sd->row_stride + j * sd->pixel_stride;
            if (++j == sd->wo) {
                j = 0;
                ++i;
            }
        }
    }
    const int64_t src_off = STRIDED ? (PACKED ? (int64_t)0 : (int64_t)c0 * sd->src_plane) : PACKED ? (int64_t)p0 * NP : (int64_t)c0 * a.plane + p0;
    const T *src = static_cast<const T *>(a.frames) + src_off;
    const float *std_multi = nullptr;  // MULTI: the batch's explicit uncertainties
    const int64_t std_stride = (int64_t)C * a.plane;  // the explicit uncertainties are planar and dense

    auto load_raw = [&](int64_t frame_offset) {
        MiRaw<T, NE> r;
        if constexpr (STRIDED) {
#pragma unroll
            for (int e = 0; e < G; ++e) __builtin_memcpy(&r.v[e * NP], src + frame_offset + off[e], NP * sizeof(T));  // one selected pixel
        } else {
            __builtin_memcpy(&r, src + frame_offset, sizeof(r));  // any alignment: planes are only element-aligned in general
        }
        return r;
    };
    // the G pixels of plane j behind the chain
    auto pixels = [&](const MiRaw<T, NE> &raw, int j, float (&x)[G]) {
#pragma unroll
        for (int e = 0; e < G; ++e) x[e] = (float)raw.v[e * NP + j];
        ingest_stages<true>(x, a, a.by_channel ? cj[j] : 0u, dsub, ddiv);
    };

    // MULTI: batch b's frames, uncertainties, size and constants take the place of the launch's
    int b = 0;
    auto select_batch = [&]() {
        B = mb->batch[b];
        src = static_cast<const T *>(mb->frames[b]) + src_off;
        std_multi = mb->std_stack[b];
        const float *consts = mb->consts[b];  // wave-uniform
        dsub = consts ? consts[0] : 0.0f;
        ddiv = consts ? consts[1] : 1.0f;
    };
    // ... and the state between the batches is in registers: what a launch per batch would have stored and read again
    constexpr int NS = MULTI ? NE : 1;
    double st_mean[NS] = {};
    float st_w[NS] = {}, st_var[NS] = {};
    if constexpr (MULTI) select_batch();

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
            if constexpr (MULTI) {  // the one read of the state
                float w[G], v[G] = {};
                mi_load(a.sumw_state + q[j], w);
                if constexpr (kHasStd) mi_load(a.var_state + q[j], v);
#pragma unroll
                for (int e = 0; e < G; ++e) {
                    st_mean[j * G + e] = m[e];
                    st_w[j * G + e] = w[e];
                    st_var[j * G + e] = v[e];
                }
            }
        }
    }

    // scale of the folded second moments back to true units
    double fs = 1.0;
    if constexpr (kGauss) fs = (double)K / (double)kk;
    if constexpr (STD == CT_STD_CONSTANT || STD == CT_STD_MULTIPLIER) fs *= (double)a.std_value;
    const double sv2 = fs * fs;

    MiResult res[NE];
    do {  // MULTI: once per batch
        for (int pass_no = 0;; ++pass_no) {
            MiSums sum[NE];
#pragma unroll
            for (int k = 0; k < NE; ++k) sum[k] = MiSums{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

            // software pipeline, as merge_kernel's: kMiPF loads in flight per thread ahead of the sample being reduced
            MiRaw<T, NE> ring[kMiPF];
            float sring[STD == CT_STD_EXPLICIT ? kMiPF : 1][NE];
            auto load_std = [&](int64_t nn, float (&sg)[NE]) {
#pragma unroll
                for (int j = 0; j < NP; ++j) __builtin_memcpy(&sg[j * G], (MULTI ? std_multi : a.std_stack) + nn * std_stride + q[j], G * sizeof(float));
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
                if constexpr (MULTI) {
#pragma unroll
                    for (int e = 0; e < G; ++e) {
                        WA[e] = st_w[j * G + e];
                        meanA[e] = st_mean[j * G + e];
                        varA[e] = st_var[j * G + e];
                    }
                } else if (!first) {
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

        if constexpr (MULTI) {
            if (++b == mb->n_batches) break;
            // what the next batch finds as its state; its pivot is the running mean, its scales follow this batch's
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                st_mean[k] = res[k].mean;
                st_w[k] = res[k].Wt;
                st_var[k] = res[k].var;
                p[k] = (float)res[k].mean;
            }
            inv_t += B;
            cq += B;
            first = false;
            select_batch();
        }
    } while (MULTI);

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

// grid of a launch: one slot per packet of a plane and one for what precedes the first
template <bool PACKED>
inline dim3 mi_grid(const MergeIngestArgs &a)
{
    constexpr uint64_t kG = PACKED ? kMiPackedGroup : kMiGroup;
    const uint64_t slots = 1 + ((uint64_t)a.plane + kG - 1) / kG;
    return dim3((uint32_t)((slots + kBlock - 1) / kBlock), PACKED ? 1u : (uint32_t)a.channels);
}

// ---- host: dispatch and launch of the three fused families, one copy ----------------------------------------------------
// f(T{}) for the element type of raw codes (validated: CT_DTYPE_U8 or CT_DTYPE_U16) ...
template <typename F>
static int with_code_dtype(int dtype, F &&f)
{
    return dtype == CT_DTYPE_U8 ? f(uint8_t{}) : f(uint16_t{});
}

// ... and of a stack that may also hold float32 pixels
template <typename F>
static int with_pixel_dtype(int dtype, F &&f)
{
    return dtype == CT_DTYPE_U8 || dtype == CT_DTYPE_U16 ? with_code_dtype(dtype, f) : f(float{});
}

// with_merge_modes for a fused family.  hdr_merge.py:107-113 (nothing connects the mean to the image) is refused HERE, not in
// the launch: a kernel named as the launch's argument is instantiated whether or not it is launched, and no family has one
// for that combination.  (The entry points refuse such a call before it gets here.)
template <int... STDS, typename F>
static int with_fused_merge_modes(int interp, int weight_mode, int std_mode, F &&f)
{
    return with_merge_modes<STDS...>(interp, weight_mode, std_mode, [&](auto I, auto W, auto S) {
        if constexpr (I == CT_INTERP_LOOKUP && W == CT_WEIGHT_NONE && S != CT_STD_NONE)
            return (int)CT_ERR_NO_GRADIENT_PATH;
        else
            return f(I, W, S);
    });
}

// the scales of `exposures` exposures fit the LDS beside the LUT of a (validated) model
static inline bool merge_scales_fit(const ct_icrf *icrf, int channels, int64_t exposures)
{
    return mi_lds_bytes(icrf->interp, channels, icrf_points(icrf), exposures) <= kLdsBudget;
}

// kernel(args...) on `grid` with the LUT and the scales of `batch` exposures in LDS.  (CT_ERR_TOO_LARGE cannot fire for one
// batch, which validation has refused, nor for a list, which the entry points walk batch by batch instead.)
template <typename Kernel, typename... Args>
static int merge_fused_launch(Kernel kernel, dim3 grid, int interp, int channels, int n_points, int64_t batch, hipStream_t s,
                              const Args &...args)
{
    const size_t lds = mi_lds_bytes(interp, channels, n_points, batch);
    if (lds > kLdsBudget) return CT_ERR_TOO_LARGE;
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, s, args...);
    return hipGetLastError() == hipSuccess ? CT_OK : CT_ERR_LAUNCH;
}

// ---- host: the batch list of ct_hdr_merge_ingest_batches, ct_hdr_merge_dark_batches and ct_hdr_merge_dark_ingest_batches -------
// element b of an optional list of pointers
template <typename P>
static inline P batch_item(P const *list, int b)
{
    return list ? list[b] : nullptr;
}

// ... which holds a pointer for every one of the n batches or for none
template <typename P>
static inline bool all_or_none(P const *list, int n)
{
    for (int b = 1; b < n; ++b)
        if ((batch_item(list, b) != nullptr) != (batch_item(list, 0) != nullptr)) return false;
    return true;
}

// the list itself: 1 to kMaxFusedBatches batches, their sizes and every array that is not optional
template <typename... Lists>
static inline bool batch_list_ok(int32_t n_batches, const int32_t *batch_sizes, Lists... required)
{
    return n_batches >= 1 && n_batches <= kMaxFusedBatches && batch_sizes && (... && (required != nullptr));
}

// the batches a call works on, in order: which batch of the arguments, and where its exposure times start
struct MergeBatchList {
    int n;
    int index[kMaxFusedBatches];
    int64_t offset[kMaxFusedBatches];
    int64_t total;  // exposures of all batches
};

// What the three entry points do differently on purpose ("Host-side argument checks").
struct MergeBatchPolicy {
    bool skip_empty;         // a batch of size 0 is skipped and the list compacted; else the validator judges it like any other
    int no_state;            // one launch per batch, but no state to carry between them
    int require_one_launch;  // one launch per batch, but CT_MERGE_REQUIRE_ONE_LAUNCH
};

constexpr int kMergePerBatch = 1;  // one_launch's answer where the list is not one launch (no CT_* status is positive)

// Every batch judged as the single-batch entry point would judge it -- nothing has touched the device when one of them is
// refused -- then ONE launch where the list allows it, else one launch per batch with the state in memory, exactly what the
// caller would have done.
//   validate(b, offset)          the status of batch b of the arguments, whose exposure times start at `offset`
//   one_launch(list)             the status of the call, or kMergePerBatch: what besides the validators' verdict stands
//                                between the list and one launch is the entry point's, in its order
//   single(b, flags, offset)     batch b alone, with merge_batch_flags of its place in the list
template <typename Validate, typename OneLaunch, typename Single>
static int merge_batches(const int32_t *batch_sizes, int32_t n_batches, uint32_t flags, bool has_state, MergeBatchPolicy policy,
                         Validate &&validate, OneLaunch &&one_launch, Single &&single)
{
    MergeBatchList list = {};
    for (int b = 0; b < n_batches; ++b) {
        if (const int rc = validate(b, list.total); rc != CT_OK) return rc;
        if (policy.skip_empty && batch_sizes[b] == 0) continue;
        list.index[list.n] = b;
        list.offset[list.n] = list.total;
        ++list.n;
        list.total += batch_sizes[b];
    }
    if (const int rc = one_launch(list); rc != kMergePerBatch) return rc;
    if (list.n > 1 && (flags & CT_MERGE_REQUIRE_ONE_LAUNCH)) return policy.require_one_launch;  // (tests: make the route explicit)
    if (list.n > 1 && !has_state) return policy.no_state;
    for (int k = 0; k < list.n; ++k)
        if (const int rc = single(list.index[k], merge_batch_flags(flags, k == 0, k == list.n - 1), list.offset[k]); rc != CT_OK) return rc;
    return CT_OK;
}

}  // namespace ct
