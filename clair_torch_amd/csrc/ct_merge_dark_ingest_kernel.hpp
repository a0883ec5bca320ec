// ct_merge_dark_ingest_kernel.hpp -- what ct_merge_dark_ingest.hip (the entry point and the planar kernels) and
// ct_merge_dark_ingest_packed.hip (the interleaved kernels) share: the argument blocks, mdi_run -- the walk of one thread over
// the batches of the elements it owns -- the workgroup around it and its dispatch.  The head of ct_merge_dark_ingest.hip
// describes ownership, the window and the byte counts.  mdi_run is md_run (ct_merge_dark_kernel.hpp) with the state always in registers
// (one batch is a list of one) and a sample step that sends the raw window taps through the chain before the blur.
#pragma once
#include "ct_merge_dark_kernel.hpp"

namespace ct {

struct MergeDarkIngestArgs {
    MergeDarkArgs d;       // geometry, blur parameters, model, state and outputs (stack, halo, std_stack, dark, dark_std and
                           // dark_stride are not read: MergeDarkIngestBatches holds those of every batch; norm is not read)
    uint32_t reversed;     // PACKED3: memory channel cm feeds plane 2 - cm (BGR)
    uint32_t by_channel;   // some clamp holds different pairs for different channels; else every channel takes pair 0
    uint32_t n_stages;
    ct_ingest_stage stage[CT_INGEST_MAX_STAGES];
};

// Batch b has batch[b] >= 1 exposures at frames[b] -- raw, MergeDarkArgs::image_stride elements apart -- with the raw halo
// rows, the explicit sigma (planar, dense), the dark field and dark std of its own (dark_stride[b]: 0 for one shared dark
// field, C * H_tile * W for one per frame) and the constants of a CT_INGEST_AFFINE_DATA stage (or NULL); its exposure times
// start at offset[b] of MergeDarkArgs::exposure, where those of all batches follow each other, and MergeDarkArgs::batch is
// their total.
struct MergeDarkIngestBatches {
    const void *frames[kMaxDarkBatches];
    const void *halo[kMaxDarkBatches];
    const float *std_stack[kMaxDarkBatches];
    const float *dark[kMaxDarkBatches];
    const float *dark_std[kMaxDarkBatches];
    const float *consts[kMaxDarkBatches];
    int64_t dark_stride[kMaxDarkBatches];
    int32_t batch[kMaxDarkBatches];
    int32_t offset[kMaxDarkBatches];
    int32_t n_batches;  // 1 .. kMaxDarkBatches
};

// ct_merge_dark_ingest_packed.hip: the launch on interleaved (B, H, W, 3) frames, dispatched like the planar one.
// Returns a CT_* status.
int merge_dark_ingest_packed(const MergeDarkIngestArgs &a, const MergeDarkIngestBatches &mb, int dtype, int interp, int weight_mode,
                             bool has_std, hipStream_t stream);

constexpr int kMdiPlanarPF = kMdPF;  // samples in flight ahead of the one being reduced: planar as md_run,
constexpr int kMdiPackedPF = 1;      // ... interleaved one (a window is 3 x 12 elements and 6 dark-field pairs: see the resources)

// what one frame contributes to the NP * G elements of a thread, as loaded: per row the pixels {left, w0 .. w0 + G - 1, right}
// with NP memory channels each, and per plane j the dark field, its std and the explicit sigma of its G elements at [j * G]
template <typename T, int NP, int G>
struct MdiRaw {
    T up[(G + 2) * NP], mid[(G + 2) * NP], dn[(G + 2) * NP];
    float d[NP * G], ds[NP * G], sg[NP * G];
};

template <typename T, int NP, int G>
__device__ __forceinline__ void mdi_load_row(const T *row, const DarkRows<T> &rw, T (&v)[(G + 2) * NP])
{
    __builtin_memcpy(&v[0], row + (int64_t)rw.cl * NP, NP * sizeof(T));  // any alignment: rows are only element-aligned in general
    __builtin_memcpy(&v[NP], row + (int64_t)rw.w0 * NP, G * NP * sizeof(T));
    __builtin_memcpy(&v[(G + 1) * NP], row + (int64_t)rw.cr * NP, NP * sizeof(T));
}

// PACKED3: the three rows of the window of pixels w0 .. w0 + G - 1 of row h in the interleaved frame at `frame` (the whole
// image: reflect at every edge, index -1 -> 1, H -> H - 2, W -> W - 2); the columns are PIXEL indices
template <typename T, int G>
__device__ __forceinline__ DarkRows<T> mdi_packed_rows(const MergeDarkArgs &d, const T *frame, uint32_t h, uint32_t w0)
{
    const uint32_t W = (uint32_t)d.width, H = (uint32_t)d.h_tile;
    const uint32_t hu = h > 0 ? h - 1 : 1, hd = h + 1 < H ? h + 1 : H - 2;
    DarkRows<T> rw;
    rw.up = frame + (int64_t)hu * W * 3;
    rw.mid = frame + (int64_t)h * W * 3;
    rw.dn = frame + (int64_t)hd * W * 3;
    rw.up_stride = rw.dn_stride = d.image_stride;
    rw.w0 = w0;
    rw.cl = w0 > 0 ? w0 - 1 : 1;
    rw.cr = w0 + G < W ? w0 + G : W - 2;
    return rw;
}

// Columns (NP == 1: of plane c0) or pixels (NP == 3: all three planes) w0 .. w0 + G - 1 of local row h: every batch of the
// launch in turn, each exactly as a launch of its own would run it -- pivot (the middle exposure on a first batch, else the
// running mean), sample loop with PF samples in flight, epilogue, conditioning test and one repeat -- with (mean, sum of
// weights, variance) in registers in between: the state arrays are read once, before batch 0 (unless it starts the merge), and
// written once, after the last batch; FIRST_BATCH is batch 0's and FINALIZE the last one's.  STD: CT_STD_EXPLICIT (a dark std:
// sigma_eff is propagated) or CT_STD_NONE; the std mode of the image behind the chain and a data-dependent stage are
// wave-uniform run-time branches.  inv_t_all and cq_all hold the scales of all batches, concatenated.
template <typename T, int NP, int G, int PF, int INTERP, int WEIGHT, int STD>
__device__ __forceinline__ void mdi_run(const MergeDarkIngestArgs &a, const MergeDarkIngestBatches &mb, const char *lds,
                                        const float *inv_t_all, const float *cq_all, uint32_t c0, uint32_t h, uint32_t w0)
{
    static_assert(STD == CT_STD_NONE || STD == CT_STD_EXPLICIT, "the merge sees sigma_eff or nothing");
    static_assert(NP == 1 || NP == 3, "one plane, or the three of an interleaved pixel");
    constexpr int NE = NP * G, N = G + 2;
    constexpr bool kHasStd = STD != CT_STD_NONE;
    constexpr bool kGauss = WEIGHT == CT_WEIGHT_GAUSS;
    constexpr int kEntry = lut_entry_bytes(INTERP);
    const MergeDarkArgs &d = a.d;
    const int C = d.channels, L = d.n_points;
    int B = 0;
    const uint32_t W = (uint32_t)d.width;
    const float top = INTERP == CT_INTERP_NONE ? 1.0f : (float)(L - 1);
    const float kk = sqrtf(d.weight_scale * 1.4426950408889634f);
    const float K = -2.0f * d.weight_scale;
    const float dk_mul = kk, dk_add = -0.5f * kk;
    bool first = d.flags & CT_MERGE_FIRST_BATCH;
    const bool finalize = d.flags & CT_MERGE_FINALIZE;
    const bool keep_state = d.mean_state != nullptr;
    [[maybe_unused]] const bool explicit_sigma = d.std_mode == CT_STD_EXPLICIT;

    const uint32_t p0 = h * W + w0;  // first element inside a plane
    uint32_t cj[NP];                 // plane of the state / outputs / dark fields (wave-uniform)
    uint32_t q[NP];                  // index of the first element in the planar (C, plane) arrays
    int row_off[NE];                 // byte offset of each element's LUT row inside the LDS table
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        cj[j] = NP == 3 ? (a.reversed ? (uint32_t)(NP - 1 - j) : (uint32_t)j) : c0;
        q[j] = cj[j] * d.plane + p0;
        const uint32_t qg = cj[j] * d.plane_global + d.base + p0;  // global flat NCHW index (< 2^31)
        int r = (int)(qg % (uint32_t)C);
#pragma unroll
        for (int e = 0; e < G; ++e) {
            row_off[j * G + e] = (INTERP == CT_INTERP_LOOKUP ? (int)cj[j] : r) * L * kEntry;
            ++r;
            r = r >= C ? r - C : r;
        }
    }
    const int64_t std_stride = (int64_t)C * d.plane;  // the explicit uncertainties are planar and dense

    // the batch in hand: its window rows in frame 0, dark field, uncertainties, scales and constants
    DarkRows<T> rw;
    const float *dark = nullptr, *dark_std = nullptr, *sigma = nullptr, *inv_t = nullptr, *cq = nullptr;
    int64_t dark_stride = 0;
    float dsub = 0.0f, ddiv = 1.0f;
    int b = 0;
    auto select_batch = [&]() {
        B = mb.batch[b];
        if constexpr (NP == 1) {
            const MdBand band{mb.halo[b], d.image_stride, d.width, d.h_tile, d.channels, d.at_top, d.at_bottom};
            rw = dark_rows<T, G, true>(band, static_cast<const T *>(mb.frames[b]) + (int64_t)c0 * d.plane, c0, h, w0);
        } else {
            rw = mdi_packed_rows<T, G>(d, static_cast<const T *>(mb.frames[b]), h, w0);
        }
        dark = mb.dark[b];
        dark_std = mb.dark_std[b];
        sigma = mb.std_stack[b];
        dark_stride = mb.dark_stride[b];
        inv_t = inv_t_all + mb.offset[b];
        cq = cq_all + mb.offset[b];
        const float *consts = mb.consts[b];  // wave-uniform
        dsub = consts ? consts[0] : 0.0f;
        ddiv = consts ? consts[1] : 1.0f;
    };
    auto load_raw = [&](int64_t n) {
        MdiRaw<T, NP, G> r{};
        mdi_load_row<T, NP, G>(rw.up + n * rw.up_stride, rw, r.up);
        mdi_load_row<T, NP, G>(rw.mid + n * d.image_stride, rw, r.mid);
        mdi_load_row<T, NP, G>(rw.dn + n * rw.dn_stride, rw, r.dn);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int64_t dq = n * dark_stride + q[j];
            __builtin_memcpy(&r.d[j * G], dark + dq, G * sizeof(float));
            if constexpr (kHasStd) {
                __builtin_memcpy(&r.ds[j * G], dark_std + dq, G * sizeof(float));
                if (explicit_sigma) __builtin_memcpy(&r.sg[j * G], sigma + n * std_stride + q[j], G * sizeof(float));
            }
        }
        return r;
    };
    // xb and sigma_eff of the NE elements: the 3 x N taps of every plane through the chain with the plane's channel, then
    // dark_blur_kernel's expressions on them
    auto blur = [&](const MdiRaw<T, NP, G> &r, float (&xb)[NE], float (&sig)[NE]) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            float v[3 * N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                v[k] = (float)r.up[k * NP + j];
                v[N + k] = (float)r.mid[k * NP + j];
                v[2 * N + k] = (float)r.dn[k * NP + j];
            }
            ingest_stages<true>(v, a, a.by_channel ? cj[j] : 0u, dsub, ddiv);
            dark_blur_staged<G, kHasStd>(d, v, v + N, v + 2 * N, &r.d[j * G], &r.ds[j * G], &r.sg[j * G], explicit_sigma, &xb[j * G],
                                         &sig[j * G]);
        }
    };

    double st_mean[NE] = {};
    float st_w[NE] = {}, st_var[NE] = {};
    select_batch();

    // ---- pivot: the middle exposure's sample on a first batch, else the running mean ----
    float p[NE];
    if (first) {
        const int probe = B / 2;
        const MdiRaw<T, NP, G> raw = load_raw(probe);
        const float itp = inv_t[probe];
        float xb[NE], sig[NE];
        blur(raw, xb, sig);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            float lin, dfds;
            mi_sample<INTERP>(xb[e], lds + row_off[e], top, lin, dfds);
            p[e] = lin * itp;
        }
    } else {  // the one read of the state
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            double m[G];
            float w[G], v[G] = {};
            mi_load(d.mean_state + q[j], m);
            mi_load(d.sumw_state + q[j], w);
            if constexpr (kHasStd) mi_load(d.var_state + q[j], v);
#pragma unroll
            for (int e = 0; e < G; ++e) {
                p[j * G + e] = (float)m[e];
                st_mean[j * G + e] = m[e];
                st_w[j * G + e] = w[e];
                st_var[j * G + e] = v[e];
            }
        }
    }

    // scale of the folded second moments back to true units (explicit uncertainties carry their own)
    double fs = 1.0;
    if constexpr (kGauss) fs = (double)K / (double)kk;
    const double sv2 = fs * fs;

    MiResult res[NE];
    for (;;) {  // once per batch
        for (int pass_no = 0;; ++pass_no) {
            MiSums sum[NE];
#pragma unroll
            for (int k = 0; k < NE; ++k) sum[k] = MiSums{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

            // software pipeline, as md_run's: PF exposures in flight per thread ahead of the one being reduced
            MdiRaw<T, NP, G> ring[PF];
#pragma unroll
            for (int k = 0; k < PF; ++k) ring[k] = load_raw(k < B ? k : B - 1);
#pragma unroll PF
            for (int n = 0; n < B; ++n) {
                const int nn = n + PF < B ? n + PF : B - 1;  // the tail re-loads the last exposure (cache hit, unused)
                // (the exposure index is laundered through an empty asm, as in merge_kernel: otherwise the compiler re-loads the
                //  sample at its point of use and the prefetch is gone)
                int64_t opaque_zero = 0;
                asm volatile("" : "+s"(opaque_zero));
                const MdiRaw<T, NP, G> incoming = load_raw((int64_t)nn + opaque_zero);
                const MdiRaw<T, NP, G> raw = ring[0];
#pragma unroll
                for (int k = 0; k + 1 < PF; ++k) ring[k] = ring[k + 1];
                ring[PF - 1] = incoming;
                const float it = inv_t[n];
                const float cqn = cq[n];
                float xb[NE], sig[NE], lin[NE], dfds[NE];
                blur(raw, xb, sig);
#pragma unroll
                for (int e = 0; e < NE; ++e) mi_sample<INTERP>(xb[e], lds + row_off[e], top, lin[e], dfds[e]);  // the gathers issue together
#pragma unroll
                for (int e = 0; e < NE; ++e)
                    mi_accumulate<INTERP, WEIGHT, STD>(xb[e], lin[e], dfds[e], sig[e], it, cqn, p[e], dk_mul, dk_add, sum[e]);
            }

            bool any_bad = false;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                res[e] = mi_epilogue<WEIGHT, STD>(sum[e], p[e], B, first, st_w[e], st_mean[e], st_var[e], sv2);
                any_bad |= res[e].bad;
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
        if (++b == mb.n_batches) break;
        // what the next batch finds as its state; its pivot is the running mean
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            st_mean[k] = res[k].mean;
            st_w[k] = res[k].Wt;
            st_var[k] = res[k].var;
            p[k] = (float)res[k].mean;
        }
        first = false;
        select_batch();
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
            mi_store<false>(d.mean_state + q[j], mean);
            mi_store<false>(d.sumw_state + q[j], wt);
            if constexpr (kHasStd) mi_store<false>(d.var_state + q[j], var);
        }
        if (finalize) {
            if (d.flags & CT_MERGE_MEAN_OUT_F32) {
                float m32[G];
#pragma unroll
                for (int e = 0; e < G; ++e) m32[e] = (float)mean[e];
                mi_store<true>(static_cast<float *>(d.mean_out) + q[j], m32);
            } else {
                mi_store<true>(static_cast<double *>(d.mean_out) + q[j], mean);
            }
            if constexpr (kHasStd) mi_store<true>(d.std_out + q[j], sd);
        }
    }
}

// merge_dark_multi_kernel's workgroup (ct_merge_dark_multi.hip): the LUT and the scales of all batches staged once, one slot
// per group of every row; a workgroup row (blockIdx.y) is one channel plane, or with PACKED the whole frame
template <typename T, bool PACKED, int INTERP, int WEIGHT, int STD>
__global__ __launch_bounds__(kBlock) void merge_dark_ingest_kernel(const MergeDarkIngestArgs a, const MergeDarkIngestBatches mb)
{
    extern __shared__ __align__(16) char lds[];
    constexpr bool kGauss = WEIGHT == CT_WEIGHT_GAUSS;
    constexpr int NP = PACKED ? 3 : 1, kG = PACKED ? kMiPackedGroup : kMdGroup, PF = PACKED ? kMdiPackedPF : kMdiPlanarPF;
    const int C = a.d.channels, L = a.d.n_points, B = a.d.batch;  // B: the exposures of all batches
    const int lut_bytes = INTERP == CT_INTERP_NONE ? 0 : C * L * lut_entry_bytes(INTERP);
    float *inv_t = reinterpret_cast<float *>(lds + lut_bytes);  // 1 / t_n
    float *cq = inv_t + B;                                      // derivative scale per exposure
    const float top = INTERP == CT_INTERP_NONE ? 1.0f : (float)(L - 1);
    const float kk = sqrtf(a.d.weight_scale * 1.4426950408889634f);
    const float K = -2.0f * a.d.weight_scale;
    stage_lut<INTERP, true>(lds, a.d.lut, C, L);
    for (int n = threadIdx.x; n < B; n += blockDim.x) {
        const float it = (float)(1.0 / a.d.exposure[n]);
        inv_t[n] = it;
        cq[n] = kGauss ? kk * top * it / K : top * it;
    }
    __syncthreads();

    const uint32_t W = (uint32_t)a.d.width;
    const uint32_t gpr = groups_per_row<kG>(W);
    const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (slot >= (uint64_t)gpr * (uint32_t)a.d.h_tile) return;
    const uint32_t h = (uint32_t)(slot / gpr);
    const uint32_t w0 = ((uint32_t)slot - h * gpr) * kG;
    const uint32_t c0 = PACKED ? 0u : blockIdx.y;
    if (W - w0 >= (uint32_t)kG) {
        mdi_run<T, NP, kG, PF, INTERP, WEIGHT, STD>(a, mb, lds, inv_t, cq, c0, h, w0);
        return;
    }
    // the end of a row whose width is no multiple of the group (at most kG - 1 columns / pixels): one lane, one after the
    // other, each with its own walk over the batches
#pragma unroll 1
    for (uint32_t w = w0; w < W; ++w) mdi_run<T, NP, 1, PF, INTERP, WEIGHT, STD>(a, mb, lds, inv_t, cq, c0, h, w);
}

// the launch of one layout, dispatched on dtype / interpolation / weight / dark std (has_std: CT_STD_EXPLICIT, else none)
template <bool PACKED>
static int mdi_dispatch(const MergeDarkIngestArgs &a, const MergeDarkIngestBatches &mb, int dtype, int interp, int weight_mode, bool has_std,
                        hipStream_t s)
{
    constexpr int kG = PACKED ? kMiPackedGroup : kMdGroup;
    return with_pixel_dtype(dtype, [&](auto t) {
        return with_dark_merge_modes(interp, weight_mode, has_std, [&](auto I, auto W, auto S) {
            return merge_fused_launch(merge_dark_ingest_kernel<decltype(t), PACKED, I, W, S>, md_grid<kG>(a.d, PACKED ? 1u : (uint32_t)a.d.channels), I,
                                      a.d.channels, a.d.n_points, a.d.batch, s, a, mb);
        });
    });
}

}  // namespace ct
