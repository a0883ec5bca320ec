// ct_merge.hip -- fused HDR merge + propagated uncertainty for one batch of exposures (gfx950).
//
// Replaces the interior of compute_hdr_image's loop body (clair_torch/inference/hdr_merge.py:61-128) and,
// with CT_MERGE_FINALIZE, its return statement (hdr_merge.py:155).  The reference runs ~50 full-tensor eager
// kernels plus an autograd backward per batch; here each thread owns V consecutive output elements, streams
// the B samples of those elements once from HBM (16-byte coalesced loads), looks the ICRF up in an LDS copy
// of the LUT, and keeps five running sums per element in registers:
//
//     W   = sum w_n                      (float32, as torch.sum over the batch dim of the float32 weights)
//     Swy = sum w_n y_n                  y_n = f(x_n) / t_n
//     Saa = sum a_n^2, Sab = sum a_n b_n, Sbb = sum b_n^2          (float64)
//         a_n = w'_n sigma_n,  b_n = (w'_n y_n + w_n y'_n) sigma_n
//
// from which the closed form of the reference's autograd variance follows (oracle/ct_oracle.c):
//     m_b  = Swy / (W + 1e-6)                     mean = mean_A + (W/Wt)(m_b - mean_A),  Wt = W_A + W
//     dmean/dx_n = alpha w'_n + beta (w'_n y_n + w_n y'_n)
//         beta  = (W/Wt) / (W + 1e-6),   alpha = (W_A/Wt^2)(m_b - mean_A) - beta m_b
//     var += alpha^2 Saa + 2 alpha beta Sab + beta^2 Sbb
// The three second moments are accumulated in float64: the quadratic form cancels by up to ~100x where
// w'(y - m) and w y' nearly cancel, which float32 sums cannot carry at the 1e-5 parity bar.
//
// Roofline: HBM.  Algorithmic bytes per output element = B * sizeof(T) (+ 4 B with an explicit std stack)
// read + 12 written (float64 mean + float32 std).  No MFMA: this is a gather/reduce, not a contraction.
//
// This file: the generic kernel (any dtype, float LUT coordinate), the one-batch instantiations of the pivoted kernel for
// raw integer codes (ct_merge_pivot.hpp), the route between them and the exported entry points.  The several-batches
// instantiations of the pivoted kernel are a translation unit of their own (ct_merge_multi.hip) so that the two build in parallel.
#include "ct_merge_pivot.hpp"

namespace ct {

// Arithmetic of one sample, written so that every constant factor is folded out of the loop:
//   dk  = kk (x - 1/2),  kk = sqrt(scale log2 e)          w = exp2(-dk^2)            (= exp(-scale (x-1/2)^2))
//   av  = dk w s'                                           true a = w' sigma           = av * (K / kk) * sig_scale
//   bv  = av y + (w s' f'_u) cq_n,  cq_n = kk top / (K t_n) true b = (w' y + w y') sigma = bv * (K / kk) * sig_scale
// with K = -2 scale, f'_u = df/ds (per unit of LUT coordinate), s' = sigma / sig_scale (the code u, the pixel x,
// 1, or the explicit std), so the loop body has no multiply by scale, top, 1/max_code or std_value.
// FOLD (integer codes only): the pixel value x is never formed; s and dk come straight from the code.
// PIVOT (the default since round 3): the second moments are float32 sums about a per-pixel pivot p ~ m_b, exactly as in
// merge_pivot_kernel (ct_merge_pivot.hpp: c_n = b_n - p a_n; Saa, Sac, Scc; conditioning check and one repeat about the known mean) --
// the float64 moments Saa, Sab, Sbb of round 1 remain behind CT_MERGE_F64_MOMENTS as the independent comparand of the
// tests.  Besides being cheaper, the pivoted form is the more accurate one where it matters: b_n = a_n y_n is rounded to
// float32 before the float64 sums ever see it, and for LOOKUP (b = a y exactly) the whole variance is the cancelling
// part; y_n - p by one FMA does not lose those bits (LOOKUP against the recorded vectors: 1.25e-5 -> ~5e-6).
template <typename T, int V, int INTERP, int WEIGHT, int STD, bool FOLD, int PF = 2, bool PIVOT = true>
__global__ __launch_bounds__(kBlock) void merge_kernel(const MergeArgs a)
{
    extern __shared__ __align__(16) char lds[];
    constexpr bool kInt = sizeof(T) != 4;
    constexpr bool kRanged = kInt;
    constexpr bool kHasStd = STD != CT_STD_NONE;
    constexpr bool kGauss = WEIGHT == CT_WEIGHT_GAUSS;
    constexpr int kEntry = lut_entry_bytes(INTERP);
    static_assert(!FOLD || kInt, "FOLD is for integer codes");
    using Moment = std::conditional_t<PIVOT, float, double>;
    const int C = a.channels, L = a.n_points, B = a.batch;
    const int lut_bytes = INTERP == CT_INTERP_NONE ? 0 : C * L * kEntry;
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

    const uint32_t vec = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (vec * (uint32_t)V >= a.q_count) return;
    const uint32_t q0 = a.q_begin + vec * (uint32_t)V;

    int row_off[V];  // byte offset of each element's LUT row inside the LDS table
    if (a.tile.layout == CT_LAYOUT_NCHW) {
        // planar input: one division and one modulo per packet; the next element's global index is one further (plus
        // the rows of the other bands when the packet runs into the next channel plane), so its row follows by an add
        // and a conditional subtract
        int ch;
        uint32_t qg;
        a.tile.locate(q0, ch, qg);
        uint32_t off = q0 - (uint32_t)ch * a.tile.plane_local;
        int r = (int)(qg % (uint32_t)C);
        const int skip_mod = (int)(a.tile.chan_skip % (uint32_t)C);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            row_off[e] = (INTERP == CT_INTERP_LOOKUP ? ch : r) * L * kEntry;
            int inc = 1;
            if (++off == a.tile.plane_local) {
                off = 0;
                ++ch;
                inc += skip_mod;
            }
            r += inc;
            r = r >= C ? r - C : r;
        }
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            int ch;
            uint32_t qg;
            a.tile.locate(a.tile.planar_index(q0 + e), ch, qg);
            row_off[e] = lut_row<INTERP>(qg, ch, C) * L * kEntry;
        }
    }

    const T *src = static_cast<const T *>(a.stack) + q0;
    const float *ssrc = STD == CT_STD_EXPLICIT ? a.std_stack + q0 : nullptr;
    const float dk_mul = FOLD ? kk * a.inv_max_code : kk, dk_add = -0.5f * kk;
    const bool first = a.flags & CT_MERGE_FIRST_BATCH;
    const bool finalize = a.flags & CT_MERGE_FINALIZE;
    const bool keep_state = a.mean_state != nullptr;

    // one sample: pixel (or raw code when FOLD), f(x), df/ds per unit of LUT coordinate
    auto sample = [&](T code, int roff, float &px, float &lin, float &dfds) {
        float s;
        if constexpr (FOLD) {
            px = (float)code;
            s = __builtin_fmaf(px, a.index.hi, px * a.index.lo);
        } else {
            px = to_pixel<T>(code, a.norm);
            s = px * top;
        }
        if constexpr (INTERP == CT_INTERP_NONE) {
            lin = FOLD ? px * a.inv_max_code : px;
            dfds = 1.0f;
        } else if constexpr (INTERP == CT_INTERP_LOOKUP) {
            float r = rintf(s);
            r = kRanged ? fminf(r, top) : fminf(fmaxf(r, 0.0f), top);  // codes are >= 0: only the upper clamp can act
            lin = reinterpret_cast<const float *>(lds + roff)[(int)r];
            dfds = 0.0f;
        } else {
            float pass = 1.0f;
            if constexpr (!kRanged) {
                pass = (s >= 0.0f && s <= top) ? 1.0f : 0.0f;
                s = fminf(fmaxf(s, 0.0f), top);
            } else {
                // a code above max_code: clamp to the top of the LUT like the reference (base.py:166,190); LINEAR's
                // last staged interval has zero slope, CATMULL needs the explicit gradient mask
                if constexpr (INTERP == CT_INTERP_CATMULL) pass = s <= top ? 1.0f : 0.0f;
                s = fminf(s, top);
            }
            const int i0 = (int)s;  // s >= 0: truncation is floor
            const float fr = __builtin_amdgcn_fractf(s);
            if constexpr (INTERP == CT_INTERP_LINEAR) {
                const float2 g = reinterpret_cast<const float2 *>(lds + roff)[i0];  // {g[i], g[i+1] - g[i]}
                dfds = g.y;
                lin = __builtin_fmaf(dfds, fr, g.x);
                if constexpr (!kRanged) dfds *= pass;
            } else {
                const float4 g = reinterpret_cast<const float4 *>(lds + roff)[i0];
                const float t = fr, t2 = t * t, t3 = t2 * t;
                const float w0 = -0.5f * t3 + t2 - 0.5f * t, w1 = 1.5f * t3 - 2.5f * t2 + 1.0f;
                const float w2 = -1.5f * t3 + 2.0f * t2 + 0.5f * t, w3 = 0.5f * t3 - 0.5f * t2;
                lin = ((w0 * g.x + w1 * g.y) + w2 * g.z) + w3 * g.w;
                const float d0 = __builtin_fmaf(__builtin_fmaf(-1.5f, t, 2.0f), t, -0.5f);
                const float d2 = __builtin_fmaf(__builtin_fmaf(-4.5f, t, 4.0f), t, 0.5f);
                const float d3 = __builtin_fmaf(1.5f, t, -1.0f) * t;
                dfds = __builtin_fmaf(d0, g.x - g.y, __builtin_fmaf(d2, g.z - g.y, d3 * (g.w - g.y)));
                dfds *= pass;
            }
        }
    };

    // ---- pivot (PIVOT): the running mean of the earlier batches, else the middle exposure's sample ----
    [[maybe_unused]] float p[V];
    if constexpr (PIVOT) {
        if (first) {
            const int probe = B / 2;
            const Packet<T, V> pk = *reinterpret_cast<const Packet<T, V> *>(src + (int64_t)probe * a.image_stride);
            const float itp = inv_t[probe];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float px, lin, dfds;
                sample(pk.v[e], row_off[e], px, lin, dfds);
                p[e] = lin * itp;
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) p[e] = (float)a.mean_state[a.out_index(q0 + e)];
        }
    }

    double mean_o[V];
    float std_o[V];
    for (int pass_no = 0;; ++pass_no) {
    float W[V], Swy[V];
    Moment Saa[V], Sab[V], Sbb[V];  // PIVOT: Saa, Sac, Scc about the pivot (float32); else the raw float64 moments
#pragma unroll
    for (int e = 0; e < V; ++e) {
        W[e] = 0.0f;
        Swy[e] = 0.0f;
        Saa[e] = 0;
        Sab[e] = 0;
        Sbb[e] = 0;
    }

    // Software pipeline: PF packets (16-byte loads) are in flight per thread ahead of the one being reduced.
    Packet<T, V> ring[PF];  // ring[0] is the packet being reduced; rotation is by register renaming after unroll
    Packet<float, V> sring[STD == CT_STD_EXPLICIT ? PF : 1];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        const int nn = k < B ? k : B - 1;
        ring[k] = *reinterpret_cast<const Packet<T, V> *>(src + (int64_t)nn * a.image_stride);
        if constexpr (STD == CT_STD_EXPLICIT)
            sring[k] = *reinterpret_cast<const Packet<float, V> *>(ssrc + (int64_t)nn * a.image_stride);
    }
#pragma unroll PF
    for (int n = 0; n < B; ++n) {
        const int nn = n + PF < B ? n + PF : B - 1;  // tail re-loads the last exposure (cache hit, unused)
        // The exposure offset is laundered through an empty asm each iteration: otherwise LLVM proves that the packet
        // consumed in iteration n equals a fresh load of exposure n and re-loads it at the point of use, which
        // deletes the prefetch (seen in the ISA: load, s_waitcnt vmcnt(0), use).
        int64_t opaque_zero = 0;
        asm volatile("" : "+s"(opaque_zero));
        const int64_t eoff = (int64_t)nn * a.image_stride + opaque_zero;
        const Packet<T, V> incoming = *reinterpret_cast<const Packet<T, V> *>(src + eoff);
        Packet<float, V> sincoming;
        if constexpr (STD == CT_STD_EXPLICIT) sincoming = *reinterpret_cast<const Packet<float, V> *>(ssrc + eoff);
        const Packet<T, V> pk = ring[0];
        const Packet<float, V> sp = sring[0];
#pragma unroll
        for (int k = 0; k + 1 < PF; ++k) {
            ring[k] = ring[k + 1];
            if constexpr (STD == CT_STD_EXPLICIT) sring[k] = sring[k + 1];
        }
        ring[PF - 1] = incoming;
        if constexpr (STD == CT_STD_EXPLICIT) sring[PF - 1] = sincoming;
        const float it = inv_t[n];
        const float cqn = cq[n];
        float pxv[V], linv[V], dfv[V];
#pragma unroll
        for (int e = 0; e < V; ++e) sample(pk.v[e], row_off[e], pxv[e], linv[e], dfv[e]);  // the V LDS gathers issue together
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float px = pxv[e], lin = linv[e], dfds = dfv[e];
            const float y = PIVOT ? __builtin_fmaf(lin, it, -p[e]) : lin * it;  // PIVOT: y_n - p
            float sg = 1.0f;
            if constexpr (STD == CT_STD_EXPLICIT) sg = sp.v[e];
            if constexpr (STD == CT_STD_MULTIPLIER) sg = px;
            if constexpr (kGauss) {
                const float dk = __builtin_fmaf(px, dk_mul, dk_add);
                const float w = __builtin_amdgcn_exp2f(-dk * dk);
                W[e] += w;
                Swy[e] = __builtin_fmaf(w, y, Swy[e]);
                if constexpr (kHasStd) {
                    const float wu = (STD == CT_STD_CONSTANT) ? w : w * sg;
                    const float av = dk * wu;
                    float bv;  // PIVOT: c_n = b_n - p a_n
                    if constexpr (INTERP == CT_INTERP_LOOKUP)
                        bv = av * y;
                    else if constexpr (INTERP == CT_INTERP_NONE)
                        bv = __builtin_fmaf(av, y, wu * cqn);
                    else
                        bv = __builtin_fmaf(av, y, (wu * dfds) * cqn);
                    if constexpr (PIVOT) {
                        Saa[e] = __builtin_fmaf(av, av, Saa[e]);
                        Sab[e] = __builtin_fmaf(av, bv, Sab[e]);
                        Sbb[e] = __builtin_fmaf(bv, bv, Sbb[e]);
                    } else {
                        // float64 FMAs: the quadratic form below cancels by 1e2..1e4 (LOOKUP: b = a y exactly)
                        const double ad = (double)av, bd = (double)bv;
                        Saa[e] = __builtin_fma(ad, ad, Saa[e]);
                        Sab[e] = __builtin_fma(ad, bd, Sab[e]);
                        Sbb[e] = __builtin_fma(bd, bd, Sbb[e]);
                    }
                }
            } else {
                Swy[e] += y;
                if constexpr (kHasStd) {
                    const float bv = (INTERP == CT_INTERP_NONE ? sg : dfds * sg) * cqn;
                    if constexpr (PIVOT) {
                        Sbb[e] = __builtin_fmaf(bv, bv, Sbb[e]);
                    } else {
                        const double bd = (double)bv;
                        Sbb[e] = __builtin_fma(bd, bd, Sbb[e]);
                    }
                }
            }
        }
    }

    // scale of the folded second moments back to true units
    double fs = 1.0;
    if constexpr (kGauss) fs = (double)K / (double)kk;
    if constexpr (STD == CT_STD_CONSTANT) fs *= (double)a.std_value;
    if constexpr (STD == CT_STD_MULTIPLIER) fs *= (double)a.std_value * (FOLD ? (double)a.inv_max_code : 1.0);
    const double sv2 = fs * fs;
    bool any_bad = false;
    [[maybe_unused]] float mb_f[V];
    [[maybe_unused]] bool bad[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const uint32_t q = a.out_index(q0 + e);  // state and outputs are planar (C, H, W) unless CT_MERGE_OUT_AS_INPUT
        float Wb = W[e];
        if constexpr (!kGauss) Wb = (float)B;
        const float Df = Wb + 1e-6f;  // float32 tensor + python float stays float32 (statistics.py:79-80)
        const float WA = first ? 0.0f : a.sumw_state[q];
        const double meanA = first ? 0.0 : a.mean_state[q];
        const float Wt = WA + Wb;
        const float frac = Wb / Wt;  // float32 division (statistics.py:105)
        double mean;
        float var = 0.0f;
        if constexpr (PIVOT) {
            // as merge_pivot_kernel's epilogue: m_b - p from the sums about the pivot, variance from the three float32 moments
            float r = __builtin_amdgcn_rcpf(Df);
            r = r * __builtin_fmaf(-Df, r, 2.0f);
            const float num = __builtin_fmaf(-p[e], 1e-6f, Swy[e]);  // sum w y - p (W + 1e-6)
            float qd = num * r;
            qd = __builtin_fmaf(__builtin_fmaf(-qd, Df, num), r, qd);  // m_b - p
            const double diff = ((double)p[e] - meanA) + (double)qd;   // m_b - mean_A
            mean = __builtin_fma((double)frac, diff, meanA);
            mb_f[e] = p[e] + qd;
            bad[e] = false;
            if constexpr (kHasStd) {
                const float gam = first ? 0.0f : (WA / (Wt * Wt)) * (float)diff;
                const float beta = frac * r;
                const float kap = __builtin_fmaf(-beta, qd, gam);
                const float t1 = beta * beta * Sbb[e];
                const float t2 = 2.0f * beta * kap * Sab[e];
                const float t3 = kap * kap * Saa[e];
                const float upd = (t1 + t2) + t3;
                if constexpr (kGauss) bad[e] = (t1 + fabsf(t2)) + t3 > kPivotCondLimit * upd;
                var = (first ? 0.0f : a.var_state[q]) + fmaxf(upd, 0.0f) * (float)sv2;
            }
            any_bad |= bad[e];
        } else {
            const double D = (double)Df;
            const double mb = (double)Swy[e] / D;
            mean = meanA + (double)frac * (mb - meanA);
            if constexpr (kHasStd) {
                const double beta = (double)frac / D;
                const double alpha = ((double)WA / ((double)Wt * (double)Wt)) * (mb - meanA) - beta * mb;
                const double upd = (alpha * alpha * (double)Saa[e] + 2.0 * alpha * beta * (double)Sab[e] + beta * beta * (double)Sbb[e]) * sv2;
                var = (first ? 0.0f : a.var_state[q]) + (float)upd;
            }
        }
        mean_o[e] = mean;
        std_o[e] = var;  // the variance until the stores below
        W[e] = Wt;       // (re-used as the output total weight)
    }
    if constexpr (PIVOT) {
        // an ill-conditioned pivot anywhere in the wavefront: repeat the batch once with those elements' pivot at the now
        // known mean; the others recompute bit-identically, so an element's result does not depend on its neighbours
        if (pass_no == 0 && __any(any_bad)) {
#pragma unroll
            for (int e = 0; e < V; ++e) p[e] = bad[e] ? mb_f[e] : p[e];
            continue;
        }
    }
    if (keep_state) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const uint32_t q = a.out_index(q0 + e);
            a.mean_state[q] = mean_o[e];
            a.sumw_state[q] = W[e];
            if constexpr (kHasStd) a.var_state[q] = std_o[e];
        }
    }
    break;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) std_o[e] = __builtin_amdgcn_sqrtf(std_o[e]);
    if (finalize && a.tile.layout != CT_LAYOUT_NCHW && !(a.flags & CT_MERGE_OUT_AS_INPUT)) {
        // interleaved input: the V elements of this thread belong to different planes -> element-wise stores
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const uint32_t q = a.tile.planar_index(q0 + e);
            if (a.flags & CT_MERGE_MEAN_OUT_F32)
                static_cast<float *>(a.mean_out)[q] = (float)mean_o[e];
            else
                static_cast<double *>(a.mean_out)[q] = mean_o[e];
            if constexpr (kHasStd) a.std_out[q] = std_o[e];
        }
    } else if (finalize) {
        if (a.flags & CT_MERGE_MEAN_OUT_F32) {
            Packet<float, V> o;
#pragma unroll
            for (int e = 0; e < V; ++e) o.v[e] = (float)mean_o[e];
            store_stream(reinterpret_cast<Packet<float, V> *>(static_cast<float *>(a.mean_out) + q0), o);
        } else {
            Packet<double, V> o;
#pragma unroll
            for (int e = 0; e < V; ++e) o.v[e] = mean_o[e];
            store_stream(reinterpret_cast<Packet<double, V> *>(static_cast<double *>(a.mean_out) + q0), o);
        }
        if constexpr (kHasStd) {
            Packet<float, V> o;
#pragma unroll
            for (int e = 0; e < V; ++e) o.v[e] = std_o[e];
            store_stream(reinterpret_cast<Packet<float, V> *>(a.std_out + q0), o);
        }
    }
}

template <typename T, int V, int INTERP, int WEIGHT, int STD, bool CLAMP>
static int launch_pivot(const MergeArgs &a, PivotArgs x, hipStream_t stream)
{
    if (a.q_count == 0) return CT_OK;
    if constexpr (INTERP == CT_INTERP_LOOKUP && WEIGHT == CT_WEIGHT_NONE && STD != CT_STD_NONE) {
        return CT_ERR_NO_GRADIENT_PATH;  // (refused by ct_hdr_merge_batch before it gets here)
    } else {
        x.n_tiles = (a.q_count + (uint32_t)(kBlock * V) - 1) / (uint32_t)(kBlock * V);  // a.q_count is a multiple of V
        size_t lds = pivot_lds_bytes(a, x, INTERP);
        x.rgb252 = 0;
        if constexpr (V == 4) {
            // interleaved RGB / BGR, the whole image in this launch, outputs only (no streaming state): packet stores
            if (a.tile.layout != CT_LAYOUT_NCHW && !(a.flags & CT_MERGE_OUT_AS_INPUT) && a.channels == 3 && a.tile.plane_local % 4 == 0 && !a.mean_state &&
                (a.flags & CT_MERGE_FINALIZE) && !(a.flags & CT_MERGE_MEAN_OUT_F32) && a.q_begin == 0 &&
                a.q_count == 3u * a.tile.plane_local && aligned(a.mean_out, 16) && aligned(a.std_out, 16)) {
                x.rgb252 = 1;
                lds = (lds + 15) & ~(size_t)15;
                x.stage_off = (uint32_t)lds;
                lds += 4 * 3072;
            }
        }
        if (lds > kLdsBudget) return CT_ERR_TOO_LARGE;
        if constexpr (V == 4) {
            if (x.rgb252)
                return (a.flags & CT_MERGE_FIRST_BATCH)
                           ? launch_pivot_grid<merge_pivot_kernel<T, V, INTERP, WEIGHT, STD, true, CLAMP, false, true>>(a, x, lds, stream)
                           : CT_ERR_INVALID_ARGUMENT;  // (no state and not the first batch: refused earlier)
        }
        return (a.flags & CT_MERGE_FIRST_BATCH)
                   ? launch_pivot_grid<merge_pivot_kernel<T, V, INTERP, WEIGHT, STD, true, CLAMP>>(a, x, lds, stream)
                   : launch_pivot_grid<merge_pivot_kernel<T, V, INTERP, WEIGHT, STD, false, CLAMP>>(a, x, lds, stream);
    }
}

// CLAMP (codes above max_code exist: max_code below the container's range) costs one v_min per sample, so it is its own
// instantiation for uint16 packets; the one-element launch of a ragged tail always carries it (its cost is irrelevant);
// uint8 packets with max_code < 255 are left to the generic kernel (merge_route).  Without a model there is no table and
// nothing to clamp.
template <typename T, int V>
static int dispatch_pivot(const MergeArgs &a, const PivotArgs &x, int interp, int weight_mode, int std_mode, bool clamp, hipStream_t s)
{
    return with_merge_modes(interp, weight_mode, std_mode, [&](auto I, auto W, auto S) {
        if constexpr (I == CT_INTERP_NONE) {
            return launch_pivot<T, V, I, W, S, false>(a, x, s);
        } else if constexpr (V == 1) {
            return launch_pivot<T, V, I, W, S, true>(a, x, s);
        } else if constexpr (sizeof(T) == 2) {
            return clamp ? launch_pivot<T, V, I, W, S, true>(a, x, s) : launch_pivot<T, V, I, W, S, false>(a, x, s);
        } else {
            return launch_pivot<T, V, I, W, S, false>(a, x, s);
        }
    });
}

template <typename T, int V, int INTERP, int WEIGHT, int STD>
static int launch_one(const MergeArgs &a, hipStream_t stream, bool fold)
{
    if (a.q_count == 0) return CT_OK;
    const uint32_t vecs = a.q_count / V;
    const uint32_t grid = (vecs + kBlock - 1) / kBlock;
    const size_t lds = lut_lds_bytes(INTERP, a.channels, a.n_points) +
                       2 * sizeof(float) * (size_t)a.batch;
    if (lds > kLdsBudget) return CT_ERR_TOO_LARGE;
    const bool f64 = a.flags & CT_MERGE_F64_MOMENTS;  // diagnostic: the round-1 float64 moments
    if constexpr (sizeof(T) != 4) {
        if (fold && f64)
            hipLaunchKernelGGL((merge_kernel<T, V, INTERP, WEIGHT, STD, true, 2, false>), dim3(grid), dim3(kBlock), lds, stream, a);
        else if (fold)
            hipLaunchKernelGGL((merge_kernel<T, V, INTERP, WEIGHT, STD, true, 2, true>), dim3(grid), dim3(kBlock), lds, stream, a);
        else if (f64)
            hipLaunchKernelGGL((merge_kernel<T, V, INTERP, WEIGHT, STD, false, 2, false>), dim3(grid), dim3(kBlock), lds, stream, a);
        else
            hipLaunchKernelGGL((merge_kernel<T, V, INTERP, WEIGHT, STD, false, 2, true>), dim3(grid), dim3(kBlock), lds, stream, a);
    } else if (f64) {
        hipLaunchKernelGGL((merge_kernel<T, V, INTERP, WEIGHT, STD, false, 2, false>), dim3(grid), dim3(kBlock), lds, stream, a);
    } else {
        hipLaunchKernelGGL((merge_kernel<T, V, INTERP, WEIGHT, STD, false, 2, true>), dim3(grid), dim3(kBlock), lds, stream, a);
    }
    return hipGetLastError() == hipSuccess ? CT_OK : CT_ERR_LAUNCH;
}

template <typename T, int V>
static int dispatch_generic(const MergeArgs &a, int interp, int weight_mode, int std_mode, hipStream_t s, bool fold)
{
    return with_merge_modes(interp, weight_mode, std_mode, [&](auto I, auto W, auto S) { return launch_one<T, V, I, W, S>(a, s, fold); });
}

// Elements per thread.  Measured on MI355X (tools/merge_bench.hip, C2 shape, Gaussian + MULTIPLIER std, PF = 2):
// uint16 V=8 (16-byte packets) and V=4 (8-byte) tie within device-to-device noise with the uncertainty on
// (1.20-1.26 ms vs 1.18-1.30 ms: VALU-bound either way) and V=8 is 7 % faster without it (0.72-0.75 vs 0.78-0.81 ms,
// HBM-bound), so 16-byte packets are used.  Rejected on measurement (profiles/r01_harness_*.log): float32 block
// moments (7 % faster, 1.3e-4 parity error), a two-phase variant caching every sample's (a_n, b_n) in registers to
// drop the float64 FMAs (exact, but 256 VGPRs and 4-byte loads: 2.4 ms), auto-SLP packed float32 (10 % slower).

template <typename T>
struct VecWidth {
    // uint8: 8 codes (8-byte loads); uint16: 4 codes (8-byte loads) -- measured 6 % faster than 8 codes per thread
    // in sustained runs (1.21 vs 1.28 ms on C2: 71 instead of 160 VGPRs); float32: 4 pixels (16-byte loads)
    static constexpr int value = sizeof(T) == 1 ? 8 : 4;
};

// The packet path needs every packet of V elements naturally aligned in every exposure: base pointers and the image stride
// multiples of the packet (a null pointer is not used, hence aligned).  `with_state`: the state arrays are moved in packets
// too (the generic kernel; the pivoted one addresses its state element by element).
static bool packets_aligned(const MergeArgs &a, size_t elem_bytes, int V, bool with_state)
{
    auto ok = [V](const void *p, size_t bytes) { return aligned(p, bytes * V); };
    return ok(a.stack, elem_bytes) && a.image_stride % V == 0 && ok(a.std_stack, 4) && ok(a.mean_out, 8) && ok(a.std_out, 4) &&
           (!with_state || (ok(a.mean_state, 8) && ok(a.sumw_state, 4) && ok(a.var_state, 4)));
}

// One batch of Q elements: packets where the alignment allows; anything else (odd widths, ragged tiles) goes through the
// V = 1 kernel, and a ragged tail of an otherwise aligned stack is a second, tiny V = 1 launch.  `pivot`: through the
// pivoted float32 kernel whole -- per-element arithmetic is identical in its packet and one-element forms, so how a stack
// is cut into tiles does not change a single bit of the result.
template <typename T>
static int merge_typed(MergeArgs a, uint32_t Q, int interp, int weight_mode, int std_mode, hipStream_t s, bool fold,
                       const PivotArgs *pivot = nullptr, bool pivot_clamp = false)
{
    constexpr int V = VecWidth<T>::value;
    int rc = CT_OK;
    if constexpr (sizeof(T) != 4) {
        if (pivot) {
            const uint32_t q_pv = packets_aligned(a, sizeof(T), kPivotV, false) ? (Q / kPivotV) * kPivotV : 0;
            a.q_begin = 0;
            a.q_count = q_pv;
            if (q_pv) rc = dispatch_pivot<T, kPivotV>(a, *pivot, interp, weight_mode, std_mode, pivot_clamp, s);
            a.q_begin = q_pv;
            a.q_count = Q - q_pv;
            if (rc == CT_OK && q_pv < Q) rc = dispatch_pivot<T, 1>(a, *pivot, interp, weight_mode, std_mode, pivot_clamp, s);
            return rc;
        }
    }
    const uint32_t q_vec = packets_aligned(a, sizeof(T), V, true) ? (Q / V) * V : 0;
    a.q_begin = 0;
    a.q_count = q_vec;
    if (q_vec) rc = dispatch_generic<T, V>(a, interp, weight_mode, std_mode, s, fold);
    a.q_begin = q_vec;
    a.q_count = Q - q_vec;
    if (rc == CT_OK && q_vec < Q) rc = dispatch_generic<T, 1>(a, interp, weight_mode, std_mode, s, fold);
    return rc;
}

}  // namespace ct

// Host check that fma(u, hi, u*lo) == u / max_code for every code (see NormConst in ct_device.hpp).
extern "C" int ct_norm_constants(float max_code, float *hi, float *lo);
extern "C" int ct_index_constants(float max_code, int n_points, float *hi, float *lo);
// Host proof behind the pivoted kernel's table addressing (ct_api.cpp).
extern "C" int ct_pivot_interval_constants(float max_code, int n_points, int lookup, int dtype_max, float *scale);

// Diagnostics (not part of the data path): device counter that merge_pivot_kernel bumps once per wavefront that ran
// its fallback pass.  NULL (the default) disables counting.  Process-global; set it only around a measurement.
static unsigned long long *g_merge_retry_counter = nullptr;
extern "C" void ct_merge_set_retry_counter(unsigned long long *counter_dev) { g_merge_retry_counter = counter_dev; }

enum class MergeRoute {
    ReferenceOrder,  // ct_merge_exact.hip: the reference's float32 autograd order
    Pivot,           // merge_pivot_kernel: closed form, raw integer codes
    Generic          // merge_kernel: closed form, any dtype
};

// Which kernel family merges these arguments.
// ReferenceOrder: LOOKUP and CATMULL with uncertainties by default -- their reference results are dominated by float32
// cancellation (CATMULL in the cubic-basis backward, LOOKUP, whose variance is the weight path alone, in y_n - m_b with m_b
// formed from the float32-rounded sum of weights), so a closed form, however accurate, differs from the reference by the
// reference's own noise (up to 2e-5 / 4e-5 on single elements).  CT_MERGE_REFERENCE_ORDER asks for that path in any mode,
// CT_MERGE_CLOSED_FORM keeps the fast closed-form kernels.
// Pivot: raw integer codes whose table entry is an exact function of the code by one round-down FMA -- verified on the host
// for every code the container can hold, also above max_code (12- and 14-bit data in uint16) and for LUT steps that are
// not a whole number of codes; fills *px, and *clamp says that codes above max_code exist and must clamp to the last entry
// (uint8 packets have no CLAMP instantiation).  CT_MERGE_F64_MOMENTS opts out.
static MergeRoute merge_route(int32_t dtype, float max_code, int interp, int n_points, int std_mode, uint32_t flags,
                              ct::PivotArgs *px, bool *clamp)
{
    if (flags & CT_MERGE_REFERENCE_ORDER) return MergeRoute::ReferenceOrder;
    if ((interp == CT_INTERP_CATMULL || interp == CT_INTERP_LOOKUP) && std_mode != CT_STD_NONE &&
        !(flags & (CT_MERGE_CLOSED_FORM | CT_MERGE_F64_MOMENTS)))
        return MergeRoute::ReferenceOrder;
    if ((dtype != CT_DTYPE_U8 && dtype != CT_DTYPE_U16) || (flags & CT_MERGE_F64_MOMENTS)) return MergeRoute::Generic;
    const int dtype_max = dtype == CT_DTYPE_U8 ? 255 : 65535;
    if (!(max_code >= 1.0f) || max_code > (float)dtype_max || floorf(max_code) != max_code) return MergeRoute::Generic;
    if (interp < CT_INTERP_LOOKUP || interp > CT_INTERP_NONE) return MergeRoute::Generic;
    const bool lookup = interp == CT_INTERP_LOOKUP;
    *clamp = interp != CT_INTERP_NONE && max_code < (float)dtype_max;
    px->step = 1.0f;
    px->index_rcp = 1.0f;
    px->max_code = max_code;
    px->n_entries = 0;
    px->tf_max = ct::kFloorMagic;
    if (interp == CT_INTERP_NONE) return MergeRoute::Pivot;
    if (*clamp && dtype == CT_DTYPE_U8) return MergeRoute::Generic;
    if (ct_pivot_interval_constants(max_code, n_points, lookup, dtype_max, &px->index_rcp) != CT_OK) return MergeRoute::Generic;
    px->step = (float)((double)max_code / (double)(n_points - 1));
    px->n_entries = lookup ? 2u * (uint32_t)n_points : (uint32_t)n_points;
    px->tf_max = ct::kFloorMagic + (float)(lookup ? 2 * (n_points - 1) : n_points - 1);
    return MergeRoute::Pivot;
}

// Which kernel ct_hdr_merge_batch dispatches for these arguments (bench.py records it next to its numbers).
extern "C" const char *ct_hdr_merge_kernel_name(int32_t dtype, float max_code, int32_t interp, int32_t n_points,
                                                uint32_t flags)
{
    ct::PivotArgs px{};
    bool clamp = false;
    // (std mode unknown here: CT_MERGE_STD_HINT in flags says uncertainties are propagated)
    switch (merge_route(dtype, max_code, interp, n_points, (flags & CT_MERGE_STD_HINT) ? CT_STD_CONSTANT : CT_STD_NONE, flags, &px, &clamp)) {
        case MergeRoute::ReferenceOrder:
            return "ct::merge_reference_order_kernel (the reference's float32 autograd order, two passes, float64 exp and divisions)";
        case MergeRoute::Pivot:
            return (flags & CT_MERGE_FIRST_BATCH)
                       ? "ct::merge_pivot_kernel (float32 moments about a per-pixel pivot, persistent workgroups, 4 codes per "
                         "thread through typed buffer loads, 7 wavefronts per SIMD, first batch)"
                       : "ct::merge_pivot_kernel (float32 moments about the running mean, persistent workgroups, 4 codes per "
                         "thread, streaming state)";
        case MergeRoute::Generic: break;
    }
    if (flags & CT_MERGE_F64_MOMENTS)
        return dtype == CT_DTYPE_F32 ? "ct::merge_kernel (float64 moments, float32 pixels, 4 per thread)"
                                     : "ct::merge_kernel (float64 moments, integer codes)";
    return dtype == CT_DTYPE_F32 ? "ct::merge_kernel (float32 moments about a per-pixel pivot, float32 pixels, 4 per thread)"
                                 : "ct::merge_kernel (float32 moments about a per-pixel pivot, integer codes through the float LUT coordinate)";
}

// What ct_hdr_merge_batch and ct_hdr_merge_batches have in common besides the stack(s).
struct MergeCall {
    const ct_geometry *geom;
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
    bool state_ok() const { return has_state() || ((flags & CT_MERGE_FIRST_BATCH) && (flags & CT_MERGE_FINALIZE)); }
    // hdr_merge.py:107-113: autograd.grad raises when nothing connects the mean to the image
    bool no_gradient_path() const { return std_mode != CT_STD_NONE && icrf->interp == CT_INTERP_LOOKUP && weight_mode == CT_WEIGHT_NONE; }
};

// The argument checks of a merge, in the order their status codes are documented; nothing is launched before they pass.
static int validate_merge(const MergeCall &c)
{
    using namespace ct;
    const ct_geometry *geom = c.geom;
    if (!geom || !c.icrf || !c.exposure) return CT_ERR_INVALID_ARGUMENT;
    if (!shape_positive(geom) || !band_fits(geom) || !layout_ok(geom) || !icrf_ok(c.icrf)) return CT_ERR_INVALID_ARGUMENT;
    if (!std_mode_in_range(c.std_mode) || (c.weight_mode != CT_WEIGHT_NONE && c.weight_mode != CT_WEIGHT_GAUSS)) return CT_ERR_INVALID_ARGUMENT;
    if (c.no_gradient_path()) return CT_ERR_NO_GRADIENT_PATH;
    if (!c.state_ok()) return CT_ERR_INVALID_ARGUMENT;
    if ((c.flags & CT_MERGE_FINALIZE) && (!c.mean_out || (c.std_mode != CT_STD_NONE && !c.std_out))) return CT_ERR_INVALID_ARGUMENT;
    if (!global_below_2_31(geom)) return CT_ERR_TOO_LARGE;
    if (!stride_holds_image(geom)) return CT_ERR_INVALID_ARGUMENT;
    // last, as the fused forms do (ct_merge_dark_kernel.hpp, ct_merge_ingest.hip): every pointer at a multiple of its element --
    // the one-element launches that packets_aligned leaves to any other address still load and store whole elements
    return aligned(c.exposure, sizeof(double)) && aligned(c.mean_state, sizeof(double)) && aligned(c.sumw_state, sizeof(float)) &&
                   aligned(c.var_state, sizeof(float)) &&
                   aligned(c.mean_out, (c.flags & CT_MERGE_MEAN_OUT_F32) ? sizeof(float) : sizeof(double)) && aligned(c.std_out, sizeof(float))
               ? CT_OK
               : CT_ERR_INVALID_ARGUMENT;
}

// ... and the stack of a batch with its explicit uncertainties (a null pointer is not used, hence aligned)
static bool batch_pointers_aligned(const void *stack, const float *std_stack, int32_t dtype)
{
    return ct::aligned(stack, ct::dtype_bytes(dtype)) && ct::aligned(std_stack, sizeof(float));
}

// The kernels' argument block for `batch` exposures at `stack` (explicit uncertainties at `std_stack`).  q_begin / q_count
// are the launcher's; norm, index and inv_max_code are set by the integer-code routes.
static ct::MergeArgs fill_merge_args(const MergeCall &c, const void *stack, const float *std_stack, int32_t batch)
{
    using namespace ct;
    const ct_geometry *geom = c.geom;
    const bool has_state = c.has_state();
    MergeArgs a{};
    a.stack = stack;
    a.std_stack = c.std_mode == CT_STD_EXPLICIT ? std_stack : nullptr;
    a.exposure = c.exposure;
    a.lut = c.icrf->lut_dev;
    a.mean_state = has_state ? c.mean_state : nullptr;
    a.sumw_state = has_state ? c.sumw_state : nullptr;
    a.var_state = has_state ? c.var_state : nullptr;
    a.mean_out = c.mean_out;
    a.std_out = c.std_out;
    a.image_stride = geom->image_stride;
    a.tile = make_tile(geom);
    a.batch = batch;
    a.channels = geom->channels;
    a.n_points = icrf_points(c.icrf);
    a.std_value = c.std_value;
    a.weight_scale = 30.0f;  // gaussian_value_weights default scale, hdr_merge.py:95
    a.inv_max_code = 1.0f;
    a.flags = c.flags;
    return a;
}

extern "C" int ct_hdr_merge_batch(const void *stack_dev, int32_t dtype, float max_code, int32_t batch,
                                  const ct_geometry *geom, const float *std_dev, int32_t std_mode, float std_value,
                                  const double *exposure_dev, const ct_icrf *icrf, int32_t weight_mode,
                                  double *mean_state_dev, float *sumw_state_dev, float *var_state_dev,
                                  void *mean_out_dev, float *std_out_dev, uint32_t flags, void *stream)
{
    using namespace ct;
    const MergeCall c{geom, std_mode, std_value, exposure_dev, icrf, weight_mode, mean_state_dev, sumw_state_dev, var_state_dev,
                      mean_out_dev, std_out_dev, flags};
    if (!stack_dev || batch <= 0 || (std_mode == CT_STD_EXPLICIT && !std_dev)) return CT_ERR_INVALID_ARGUMENT;
    if (const int rc = validate_merge(c); rc != CT_OK) return rc;
    if (!batch_pointers_aligned(stack_dev, std_mode == CT_STD_EXPLICIT ? std_dev : nullptr, dtype)) return CT_ERR_INVALID_ARGUMENT;
    MergeArgs a = fill_merge_args(c, stack_dev, std_dev, batch);
    const uint32_t Ql = (uint32_t)local_elements(geom);
    const int interp = icrf->interp;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PivotArgs px{};
    bool clamp = false;
    const MergeRoute route = merge_route(dtype, max_code, interp, a.n_points, std_mode, flags, &px, &clamp);
    if (dtype != CT_DTYPE_F32 && ct_norm_constants(max_code, &a.norm.hi, &a.norm.lo) != CT_OK) return CT_ERR_UNSUPPORTED;
    if (route == MergeRoute::ReferenceOrder) return merge_reference_order(a, dtype, Ql, interp, weight_mode, std_mode, s);
    if (dtype == CT_DTYPE_F32) return merge_typed<float>(a, Ql, interp, weight_mode, std_mode, s, false);
    if (dtype != CT_DTYPE_U8 && dtype != CT_DTYPE_U16) return CT_ERR_UNSUPPORTED;
    // FOLD needs the LUT index formed from the code to equal the reference's float32 index for every code
    const bool fold = ct_index_constants(max_code, a.n_points, &a.index.hi, &a.index.lo) == CT_OK;
    a.inv_max_code = (float)(1.0 / (double)max_code);
    px.probe = batch / 2;
    px.retry_count = g_merge_retry_counter;
    const PivotArgs *pivot = route == MergeRoute::Pivot ? &px : nullptr;
    return dtype == CT_DTYPE_U8 ? merge_typed<uint8_t>(a, Ql, interp, weight_mode, std_mode, s, fold, pivot, clamp)
                                : merge_typed<uint16_t>(a, Ql, interp, weight_mode, std_mode, s, fold, pivot, clamp);
}

// Several consecutive batches of one merge in ONE launch (hdr_merge.py:61-128 for k iterations of the loop) where a
// kernel walks batches -- the pivoted one (whole packets everywhere) and the reference-order one (any dtype); otherwise one
// launch per batch with the state in memory, exactly what the caller would have done.
extern "C" int ct_hdr_merge_batches(const void *const *stack_devs, const float *const *std_devs, const int32_t *batch_sizes,
                                    int32_t n_batches, int32_t dtype, float max_code, const ct_geometry *geom, int32_t std_mode,
                                    float std_value, const double *exposure_dev, const ct_icrf *icrf, int32_t weight_mode,
                                    double *mean_state_dev, float *sumw_state_dev, float *var_state_dev, void *mean_out_dev,
                                    float *std_out_dev, uint32_t flags, void *stream)
{
    using namespace ct;
    if (!stack_devs || !batch_sizes || n_batches <= 0 || !geom || !icrf || !exposure_dev) return CT_ERR_INVALID_ARGUMENT;
    if (std_mode == CT_STD_EXPLICIT && !std_devs) return CT_ERR_INVALID_ARGUMENT;
    int64_t total = 0;
    for (int b = 0; b < n_batches; ++b) {
        if (!stack_devs[b] || batch_sizes[b] <= 0 || (std_mode == CT_STD_EXPLICIT && !std_devs[b])) return CT_ERR_INVALID_ARGUMENT;
        total += batch_sizes[b];
    }
    const MergeCall c{geom, std_mode, std_value, exposure_dev, icrf, weight_mode, mean_state_dev, sumw_state_dev, var_state_dev,
                      mean_out_dev, std_out_dev, flags};
    const int valid = validate_merge(c);  // of the whole sequence (FIRST: before its first batch, FINALIZE: after its last)
    // a batch off its element is refused here, before the first batch is launched (a one-launch route would read it as it is)
    for (int b = 0; valid == CT_OK && b < n_batches; ++b)
        if (!batch_pointers_aligned(stack_devs[b], std_mode == CT_STD_EXPLICIT ? std_devs[b] : nullptr, dtype)) return CT_ERR_INVALID_ARGUMENT;
    const int interp = icrf->interp;
    const int64_t Ql = local_elements(geom);
    hipStream_t s = static_cast<hipStream_t>(stream);
    MergeArgs a = fill_merge_args(c, stack_devs[0], std_mode == CT_STD_EXPLICIT ? std_devs[0] : nullptr, (int32_t)total);
    PivotArgs px{};
    bool clamp = false;
    const MergeRoute route = merge_route(dtype, max_code, interp, a.n_points, std_mode, flags, &px, &clamp);

    if (route == MergeRoute::ReferenceOrder && valid == CT_OK && n_batches >= 2 && n_batches <= kMaxMergeBatches && total <= 65536 &&
        (dtype == CT_DTYPE_U8 || dtype == CT_DTYPE_U16 || dtype == CT_DTYPE_F32)) {
        if (dtype != CT_DTYPE_F32 && ct_norm_constants(max_code, &a.norm.hi, &a.norm.lo) != CT_OK) return CT_ERR_UNSUPPORTED;
        MergeBatches mb{};
        mb.n_batches = n_batches;
        for (int b = 0; b < n_batches; ++b) {
            mb.batch_size[b] = batch_sizes[b];
            mb.batch_ptr[b] = stack_devs[b];
            mb.std_ptr[b] = std_mode == CT_STD_EXPLICIT ? std_devs[b] : nullptr;
        }
        return merge_reference_order(a, dtype, (uint32_t)Ql, interp, weight_mode, std_mode, s, &mb);
    }
    // the pivoted kernel in one launch: a well-formed problem in whole packets; what else may be wrong with the call is
    // reported from here, before anything is launched
    bool fast = route == MergeRoute::Pivot && n_batches >= 2 && n_batches <= kMaxMultiBatches && total <= 0x7fffffff && c.state_ok() &&
                shape_positive(geom) && !c.no_gradient_path() && Ql % kPivotV == 0;
    for (int b = 0; fast && b < n_batches; ++b) {
        a.stack = stack_devs[b];
        a.std_stack = std_mode == CT_STD_EXPLICIT ? std_devs[b] : nullptr;
        fast = packets_aligned(a, dtype == CT_DTYPE_U8 ? 1 : 2, kPivotV, false);
    }
    if (fast) {
        if (valid != CT_OK) return valid;
        if (ct_norm_constants(max_code, &a.norm.hi, &a.norm.lo) != CT_OK) return CT_ERR_UNSUPPORTED;
        a.stack = stack_devs[0];
        a.std_stack = std_mode == CT_STD_EXPLICIT ? std_devs[0] : nullptr;
        a.q_begin = 0;
        a.q_count = (uint32_t)Ql;
        a.inv_max_code = (float)(1.0 / (double)max_code);
        px.n_batches = n_batches;
        px.fresh = (flags & CT_MERGE_FIRST_BATCH) ? 1 : 0;
        px.probe = batch_sizes[0] / 2;
        px.retry_count = g_merge_retry_counter;
        for (int b = 0; b < n_batches; ++b) {
            px.batch_size[b] = batch_sizes[b];
            px.batch_ptr[b] = stack_devs[b];
            px.std_ptr[b] = std_mode == CT_STD_EXPLICIT ? std_devs[b] : nullptr;
        }
        return merge_pivot_multi(a, px, dtype, clamp, interp, weight_mode, std_mode, s);
    }
    if (flags & CT_MERGE_REQUIRE_ONE_LAUNCH) return CT_ERR_UNSUPPORTED;  // (tests: make the route explicit)
    if (n_batches > 1 && !c.has_state()) return CT_ERR_INVALID_ARGUMENT;
    int64_t n0 = 0;
    for (int b = 0; b < n_batches; ++b) {
        const int rc = ct_hdr_merge_batch(stack_devs[b], dtype, max_code, batch_sizes[b], geom, std_devs ? std_devs[b] : nullptr,
                                          std_mode, std_value, exposure_dev + n0, icrf, weight_mode, mean_state_dev,
                                          sumw_state_dev, var_state_dev, mean_out_dev, std_out_dev,
                                          merge_batch_flags(flags, b == 0, b == n_batches - 1), stream);
        if (rc != CT_OK) return rc;
        n0 += batch_sizes[b];
    }
    return CT_OK;
}
