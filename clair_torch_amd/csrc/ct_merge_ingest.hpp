// ct_merge_ingest.hpp -- the per-sample and per-element arithmetic of the generic merge kernel
// (merge_kernel<float, V, INTERP, WEIGHT, STD, /*FOLD*/ false> in ct_merge.hip: float32 pixel, float LUT coordinate with the
// clamp and its gradient mask, float32 moments about a per-pixel pivot) as device functions of ONE element, for
// ct_merge_ingest.hip, whose pixel is a raw code behind a gpu_transforms chain and never reaches memory.  Every expression is
// that kernel's, operation for operation (-ffp-contract=off; the fused multiply-adds are the spelled ones), so the two
// give the same bits for the same pixel; tests/test_gpu_merge_ingest.py compares them.  ct_merge.hip does not include this.
#pragma once
#include "ct_merge.hpp"

namespace ct {

// f(x) and df/ds per unit of LUT coordinate of a float32 pixel; `row` is the element's LUT row in LDS (stage_lut<INTERP, true>)
template <int INTERP>
__device__ __forceinline__ void mi_sample(float px, const char *row, float top, float &lin, float &dfds)
{
    if constexpr (INTERP == CT_INTERP_NONE) {
        lin = px;
        dfds = 1.0f;
    } else if constexpr (INTERP == CT_INTERP_LOOKUP) {
        float r = rintf(px * top);
        r = fminf(fmaxf(r, 0.0f), top);
        lin = reinterpret_cast<const float *>(row)[(int)r];
        dfds = 0.0f;
    } else {
        float s = px * top;
        const float pass = (s >= 0.0f && s <= top) ? 1.0f : 0.0f;  // the clamp's gradient mask (base.py:166,190)
        s = fminf(fmaxf(s, 0.0f), top);
        const int i0 = (int)s;  // s >= 0: truncation is floor
        const float fr = __builtin_amdgcn_fractf(s);
        if constexpr (INTERP == CT_INTERP_LINEAR) {
            const float2 g = reinterpret_cast<const float2 *>(row)[i0];  // {g[i], g[i+1] - g[i]}
            dfds = g.y;
            lin = __builtin_fmaf(dfds, fr, g.x);
            dfds *= pass;
        } else {
            const float4 g = reinterpret_cast<const float4 *>(row)[i0];
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
}

// the running sums of one element: W = sum w, Swy = sum w (y - p), and the float32 moments Saa, Sac, Scc about the pivot p
struct MiSums {
    float W, Swy, Saa, Sab, Sbb;
};

// one sample into the sums: y = lin / t - p; sg = the explicit sigma (EXPLICIT only); it = 1 / t_n, cqn = the derivative
// scale of exposure n; dk_mul / dk_add = kk and -kk / 2 (see the comment above merge_kernel for the folded constants)
template <int INTERP, int WEIGHT, int STD>
__device__ __forceinline__ void mi_accumulate(float px, float lin, float dfds, float sg_explicit, float it, float cqn, float p,
                                              float dk_mul, float dk_add, MiSums &s)
{
    constexpr bool kHasStd = STD != CT_STD_NONE;
    const float y = __builtin_fmaf(lin, it, -p);
    float sg = 1.0f;
    if constexpr (STD == CT_STD_EXPLICIT) sg = sg_explicit;
    if constexpr (STD == CT_STD_MULTIPLIER) sg = px;
    if constexpr (WEIGHT == CT_WEIGHT_GAUSS) {
        const float dk = __builtin_fmaf(px, dk_mul, dk_add);
        const float w = __builtin_amdgcn_exp2f(-dk * dk);
        s.W += w;
        s.Swy = __builtin_fmaf(w, y, s.Swy);
        if constexpr (kHasStd) {
            const float wu = (STD == CT_STD_CONSTANT) ? w : w * sg;
            const float av = dk * wu;
            float bv;  // c_n = b_n - p a_n
            if constexpr (INTERP == CT_INTERP_LOOKUP)
                bv = av * y;
            else if constexpr (INTERP == CT_INTERP_NONE)
                bv = __builtin_fmaf(av, y, wu * cqn);
            else
                bv = __builtin_fmaf(av, y, (wu * dfds) * cqn);
            s.Saa = __builtin_fmaf(av, av, s.Saa);
            s.Sab = __builtin_fmaf(av, bv, s.Sab);
            s.Sbb = __builtin_fmaf(bv, bv, s.Sbb);
        }
    } else {
        s.Swy += y;
        if constexpr (kHasStd) {
            const float bv = (INTERP == CT_INTERP_NONE ? sg : dfds * sg) * cqn;
            s.Sbb = __builtin_fmaf(bv, bv, s.Sbb);
        }
    }
}

// what a batch leaves of one element: the new mean, variance and total weight; mb is the batch mean (the pivot of a
// repeat), bad says that the pivot was ill-conditioned for this element
struct MiResult {
    double mean;
    float var, Wt, mb;
    bool bad;
};

// the epilogue of merge_kernel's PIVOT form: WBOMean.update_values (statistics.py:64-109) and the closed-form variance.
// WA, meanA, varA: the state before this batch (ignored on a first batch); sv2: the scale of the folded moments, squared
template <int WEIGHT, int STD>
__device__ __forceinline__ MiResult mi_epilogue(const MiSums &s, float p, int B, bool first, float WA_state, double meanA_state,
                                                float varA_state, double sv2)
{
    MiResult o;
    float Wb = s.W;
    if constexpr (WEIGHT != CT_WEIGHT_GAUSS) Wb = (float)B;
    const float Df = Wb + 1e-6f;  // float32 tensor + python float stays float32 (statistics.py:79-80)
    const float WA = first ? 0.0f : WA_state;
    const double meanA = first ? 0.0 : meanA_state;
    const float Wt = WA + Wb;
    const float frac = Wb / Wt;  // float32 division (statistics.py:105)
    float var = 0.0f;
    float r = __builtin_amdgcn_rcpf(Df);
    r = r * __builtin_fmaf(-Df, r, 2.0f);
    const float num = __builtin_fmaf(-p, 1e-6f, s.Swy);  // sum w y - p (W + 1e-6)
    float qd = num * r;
    qd = __builtin_fmaf(__builtin_fmaf(-qd, Df, num), r, qd);  // m_b - p
    const double diff = ((double)p - meanA) + (double)qd;      // m_b - mean_A
    o.mean = __builtin_fma((double)frac, diff, meanA);
    o.mb = p + qd;
    o.bad = false;
    if constexpr (STD != CT_STD_NONE) {
        const float gam = first ? 0.0f : (WA / (Wt * Wt)) * (float)diff;
        const float beta = frac * r;
        const float kap = __builtin_fmaf(-beta, qd, gam);
        const float t1 = beta * beta * s.Sbb;
        const float t2 = 2.0f * beta * kap * s.Sab;
        const float t3 = kap * kap * s.Saa;
        const float upd = (t1 + t2) + t3;
        if constexpr (WEIGHT == CT_WEIGHT_GAUSS) o.bad = (t1 + fabsf(t2)) + t3 > kPivotCondLimit * upd;
        var = (first ? 0.0f : varA_state) + fmaxf(upd, 0.0f) * (float)sv2;
    }
    o.var = var;
    o.Wt = Wt;
    return o;
}

}  // namespace ct
