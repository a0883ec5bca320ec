// ct_merge_pivot.hpp -- the pivoted float32 merge kernel for raw integer codes, its argument block and its persistent
// launch; shared by ct_merge.hip (one batch per launch) and ct_merge_multi.hip (several batches per launch).
#pragma once
#include "ct_merge.hpp"
#include <type_traits>

namespace ct {

// Kernel for raw integer codes (round 2; LOOKUP and CATMULL since round 3): single-precision moments about a per-pixel pivot.
//
// Why: ct::merge_kernel (ct_merge.hip) is VALU-bound on the 2 B/sample headline form (profiles/r01_merge_c2_sq_counters.md), and 45 %
// of its loop is the float64 moments plus the float -> index conversions; another 20 % of all VALU work sat outside
// the loop (per-workgroup LUT staging with integer divides, three IEEE float64 divisions per output element).  Here:
//   * moments about a pivot p ~ m_b:   c_n = b_n - p a_n = w'_n sigma_n (y_n - p) + w_n y'_n sigma_n   (float32)
//       sum (alpha a_n + beta b_n)^2 = beta^2 Scc + 2 beta kappa Sac + kappa^2 Saa,   kappa = gamma - beta (m_b - p),
//       gamma = (W_A / Wt^2)(m_b - mean_A).  With |m_b - p| << m_b the expansion no longer cancels (for LINEAR
//       |a_n (m_b - p)| <= 13.6 |m_b - p| / m_b times the y' term), so float32 sums carry it.  The pivot is the running
//       mean of the earlier batches, or for a first batch the sample of the middle exposure.  Every output element
//       checks its own conditioning (sum of |terms| against the result); a wavefront with an ill-conditioned element
//       runs the batch a second time about the now known mean (explicit fallback, exact to float32 rounding).
//   * the batch mean is accumulated about the same pivot: sum w (y - p), mean = p + ..., in float64 only at the end;
//   * the codes reach the registers as floats through typed buffer loads (conversion in the texture-data path, not on
//     the VALU; ct_device.hpp), the LUT interval floor(code / step) is the mantissa of ONE FMA that rounds toward minus
//     infinity (host-verified for every code against the reference's float32 index), and the 8-byte LUT entry {A, S}
//     gives f = A + S * code in one more FMA: no float coordinate, no fract, no float -> int, no integer -> float;
//   * persistent workgroups: the table and 1/t are staged once per workgroup, not once per 1024 elements;
//   * the epilogue has no float64 division (one v_rcp_f32 + Newton step, shared by the mean and the variance).
// The raw-load build (codes unpacked on the VALU) was measured and rejected: profiles/r02_typed_load_ab.log.

// One packet through a buffer descriptor based at `base` (wave-uniform) + a 32-bit per-thread byte offset:
// buffer_load_* v, v_offset, s[descriptor], 0 offen.  The descriptor spans 4 GiB from the base, so the offset (an
// element index inside ONE image times the element size) must stay below that -- the callers check.
constexpr int kStackLoadAux = 0;  // MUBUF cache-policy bits of the stack loads (bit 0 sc0, bit 1 nt, bit 4 sc1)
template <typename P>
__device__ __forceinline__ P load_buffer(uint64_t base, uint32_t offset)
{
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(base), 0, 0xffffffff, 0x00020000 /* gfx9 raw dword format */);
    P out;
    if constexpr (sizeof(P) == 1) {
        const uint8_t v = __builtin_amdgcn_raw_buffer_load_b8(rsrc, offset, 0, kStackLoadAux);
        __builtin_memcpy(&out, &v, sizeof(P));
    } else if constexpr (sizeof(P) == 2) {
        const uint16_t v = __builtin_amdgcn_raw_buffer_load_b16(rsrc, offset, 0, kStackLoadAux);
        __builtin_memcpy(&out, &v, sizeof(P));
    } else if constexpr (sizeof(P) == 4) {
        const uint32_t v = __builtin_amdgcn_raw_buffer_load_b32(rsrc, offset, 0, kStackLoadAux);
        __builtin_memcpy(&out, &v, sizeof(P));
    } else if constexpr (sizeof(P) == 8) {
        typedef uint32_t vec_t __attribute__((ext_vector_type(2)));
        const vec_t v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, offset, 0, kStackLoadAux);
        __builtin_memcpy(&out, &v, sizeof(P));
    } else {
        static_assert(sizeof(P) == 16, "packets are at most 16 bytes");
        typedef uint32_t vec_t __attribute__((ext_vector_type(4)));
        const vec_t v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, offset, 0, kStackLoadAux);
        __builtin_memcpy(&out, &v, sizeof(P));
    }
    return out;
}

// Typed buffer loads (load_codes_as_float, ct_device.hpp): the codes reach the registers as floats, converted in the
// texture-data path instead of by one half-rate conversion per sample on the VALU this kernel is bound by.
template <typename T, int V>
__device__ __forceinline__ Packet<float, V> load_codes_as_float(uint64_t base, uint32_t offset)
{
    Packet<float, V> out;
    load_codes_as_float<T, V, kStackLoadAux>(base, offset, out.v);
    return out;
}

// (floor_index_bits, lds_row_constant, lds_entry_address: ct_device.hpp -- shared with the training kernels)

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(<N-1>)
template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

struct PivotArgs {
    uint32_t index_mul;  // reserved (unused; keeps the kernel-argument layout): always 0
    float step;          // max_code / (L-1): codes per LUT interval (any positive value; a whole number on the headline shapes)
    uint32_t n_tiles;    // tiles of kBlock * V elements
    int32_t probe;       // exposure whose sample seeds the pivot of a first batch
    float index_rcp;     // table entry of a code = floor(code * index_rcp) by one round-down FMA: (L-1) / max_code
                         // for LINEAR, 2 (L-1) / max_code for LOOKUP (half intervals), rounded so that EVERY code the container
                         // can hold lands in the reference's entry (ct_pivot_interval_constants)
    float max_code;      // what Normalize divides by
    float tf_max;        // CLAMP: 1.5 * 2^23 + last table entry (codes above max_code clamp to the top of the LUT, base.py:166)
    uint32_t n_entries;  // table entries per LUT row: L (LINEAR), 2 L (LOOKUP)
    unsigned long long *retry_count;  // diagnostics: wavefronts that ran the fallback pass (may be NULL)
    // MULTI (ct_hdr_merge_batches): several consecutive batches per launch, the streaming state in registers in between
    int32_t n_batches;                          // 1 .. kMaxMultiBatches
    int32_t fresh;                              // the first batch starts a merge (no state to read)
    int32_t batch_size[16];                     // exposures per batch; a.batch = their sum, a.exposure in the same order
    const void *batch_ptr[16];                  // each batch's (B_b, C, H_tile, W) stack
    const float *std_ptr[16];                   // CT_STD_EXPLICIT: each batch's std stack
    // interleaved RGB / BGR input with planar packet stores (see the kernel's epilogue): the results of a wavefront are
    // regrouped by channel plane through its 3 KB staging area at `stage_off`
    int32_t rgb252;
    uint32_t stage_off;                         // LDS byte offset of the 4 x 3072-byte staging areas
};
constexpr int kMaxMultiBatches = 16;
constexpr int kPivotV = 4;  // elements per thread of merge_pivot_kernel (uint16: 8-byte loads, uint8: 4-byte)

constexpr int kPivotDepth = 2;  // exposures in flight per thread
constexpr float kRoughLimit = 64.0f;  // |A| / max(|g[i]|, |g[i+1]|) above which the table keeps {g[i], S}: error bound 2^-25 * 64 = 2e-6

// The weight is one v_exp_f32 per sample.  Two table-based evaluations (a fine linear weight table in LDS; 16-byte LUT
// entries with a degree-4 polynomial) were measured and rejected: profiles/r03_merge_weight_variants.md.

// The first-batch kernels (no state carried through the loop): 7 wavefronts per SIMD (72 VGPRs).  With the codes held as
// four floats per packet instead of two packed dwords the 64-VGPR build spills 19 registers (1.24 ms); 7 and 6
// wavefronts measure the same within 1 % (0.856 / 0.865 ms sustained, profiles/r02_typed_load_ab.log).  The RGB252
// instantiations (the regrouping costs registers) get 6; the state-carrying kernels keep the default allocation.
constexpr int kRgb252Waves = 6;
// MULTI: the launch walks x.n_batches consecutive batches per element with (mean, sum of weights, variance) in registers and
// the per-batch recurrence of WBOMean (statistics.py:64-109, state detached after every batch, hdr_merge.py:128) applied
// between them -- bit for bit what one launch per batch gives (the first-batch arithmetic with zero state IS the
// state-carrying arithmetic: W_A = 0 makes frac = 1 and gamma = 0 exactly), without the 32 B per element and batch of
// state traffic the reference's default batch_size: 4 costs beside 8 B of samples.
template <typename T, int V, int INTERP, int WEIGHT, int STD, bool FIRST, bool CLAMP = false, bool MULTI = false, bool RGB252 = false>
__global__ __launch_bounds__(kBlock)
__attribute__((amdgpu_waves_per_eu(FIRST && V <= 4 && STD != CT_STD_EXPLICIT ? (RGB252 ? kRgb252Waves : 7) : 4, 8)))
void merge_pivot_kernel(const MergeArgs a, const PivotArgs x)
{
    static_assert(!MULTI || !FIRST, "MULTI carries state");
    static_assert(!RGB252 || (V == 4 && FIRST && !MULTI), "RGB252: single-batch packets");
    extern __shared__ __align__(16) char lds[];
    static_assert(sizeof(T) != 4, "raw integer codes only");
    constexpr bool kLut = INTERP != CT_INTERP_NONE;  // a table in LDS
    constexpr bool kLookup = INTERP == CT_INTERP_LOOKUP;  // piecewise constant: entry j = half interval j, slope 0, row = channel
    // CATMULL (r03): entry i holds the interval's cubic in the code offset, f = d + o (c + o (b + o a)), o = code - i step --
    // the Catmull-Rom basis of base.py:199-224 on the taps g[i-1..i+2] (edges replicated) collected by powers of t = o / step
    // in float64 and rounded once; three FMAs for the value, four more instructions for df/dcode.  The closed-form kernel
    // for CATMULL stacks WITHOUT uncertainties (and with CT_MERGE_CLOSED_FORM); the default with uncertainties stays
    // the reference-order kernel.
    constexpr bool kCat = INTERP == CT_INTERP_CATMULL;
    constexpr bool kHasStd = STD != CT_STD_NONE;
    constexpr bool kGauss = WEIGHT == CT_WEIGHT_GAUSS;
    using CodePk = Packet<float, V>;  // codes arrive as floats from typed buffer loads
    const int C = a.channels, L = a.n_points, B = a.batch;
    constexpr int kEntryShift = kCat ? 4 : 3;
    const int E = kLut ? (int)x.n_entries : 0;  // table entries per row
    const int lut_bytes = C * E * (1 << kEntryShift);
    float2 *expo = reinterpret_cast<float2 *>(lds + lut_bytes);  // per exposure {1 / t_n, chain factor of the y' term}
    const float kk = sqrtf(a.weight_scale * 1.4426950408889634f);
    const float dk_mul = kk * a.inv_max_code, dk_add = -0.5f * kk;
    const float K = -2.0f * a.weight_scale;
    // y' = (df/dcode) max_code / t_n;  the loop forms (w s' df/dcode) * cq_n with cq_n = max_code (kk / K) / t_n
    const float max_code = kLut ? x.max_code : 1.0f;  // (no model: df/dcode * max_code = 1, folded)
    const float ce = kGauss ? max_code * kk / K : max_code;

    bool rough = false;
    if constexpr (kLookup) {
        // entry j of row c covers LUT coordinates [j / 2, (j + 1) / 2): the reference's round-half-even index is (j + 1) / 2
        // for every code (host-verified), so f = g[c][(j + 1) >> 1] and the slope is zero
        const int total = C * E;
        for (int k = threadIdx.x; k < total; k += kBlock) {
            const int r = k / E, j = k - r * E;
            const int idx = (j + 1) >> 1;
            reinterpret_cast<float2 *>(lds)[k] = make_float2(a.lut[(size_t)r * L + (idx < L ? idx : L - 1)], 0.0f);
        }
    } else if constexpr (kCat) {
        const int total = C * L;
        const double st = (double)x.step;
        for (int k = threadIdx.x; k < total; k += kBlock) {
            const int r = k / L, i = k - r * L;
            const float *row = a.lut + (size_t)r * L;
            const double p0 = row[i > 0 ? i - 1 : 0], p1 = row[i], p2 = row[i + 1 < L ? i + 1 : L - 1], p3 = row[i + 2 < L ? i + 2 : L - 1];
            // w0 p0 + w1 p1 + w2 p2 + w3 p3 with the basis of base.py:199-224 = p1 + t c + t^2 b + t^3 a
            const double c1 = 0.5 * (p2 - p0), b1 = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3), a1 = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3);
            // (entry L - 1 is met at offset 0 only -- code == max_code, where the reference's clamp still passes the gradient
            // -- or, with CLAMP, by codes above max_code, whose offset and slope are zeroed in the loop)
            reinterpret_cast<float4 *>(lds)[k] = make_float4((float)p1, (float)(c1 / st), (float)(b1 / (st * st)), (float)(a1 / (st * st * st)));
        }
    } else if constexpr (kLut) {
        // entry i of row r: f(code) = A + S * code on [i * step, (i + 1) * step):  S = (g[i+1] - g[i]) / step (the
        // reference backward's g1 - g0), A = g[i] - S * i * step formed in float64 and rounded once.  One FMA per
        // sample, but A carries an absolute rounding error of 2^-25 |A|, and |A| <= |g[i]| + i |g[i+1] - g[i]| exceeds
        // the LUT values themselves when the curve is steep: a factor 1 + p for g = x^p, unbounded for a LUT with a
        // jump.  A workgroup that meets |A| > kRoughLimit max(|g[i]|, |g[i+1]|) anywhere therefore stages {g[i], S}
        // instead and evaluates f = g[i] + S (code - i * step) with the offset formed exactly when the step is a whole
        // number of codes (two more instructions per sample); every workgroup sees the same LUT, so all take the same branch.
        const int total = C * L;
        const double stepd = (double)x.max_code / (double)(L - 1);
        bool viol = false;
        for (int k = threadIdx.x; k < total; k += kBlock) {
            const int r = k / L, i = k - r * L;
            const float *row = a.lut + (size_t)r * L;
            const float g0 = row[i], g1 = row[i + 1 < L ? i + 1 : L - 1];
            const float slope = (g1 - g0) / x.step;
            const float A = (float)((double)g0 - (double)slope * ((double)i * stepd));
            viol |= !(fabsf(A) <= kRoughLimit * fmaxf(fmaxf(fabsf(g0), fabsf(g1)), 1e-30f));
        }
        rough = __syncthreads_or(viol);
        for (int k = threadIdx.x; k < total; k += kBlock) {
            const int r = k / L, i = k - r * L;
            const float *row = a.lut + (size_t)r * L;
            const float g0 = row[i], g1 = row[i + 1 < L ? i + 1 : L - 1];
            const float slope = (g1 - g0) / x.step;
            const float A = (float)((double)g0 - (double)slope * ((double)i * stepd));
            reinterpret_cast<float2 *>(lds)[k] = make_float2(rough ? g0 : A, slope);
        }
    }
    for (int n = threadIdx.x; n < B; n += kBlock) {
        const float it = (float)(1.0 / a.exposure[n]);
        expo[n] = make_float2(it, ce * it);
    }
    __syncthreads();  // the only barrier: everything below is per wavefront

    const bool finalize = a.flags & CT_MERGE_FINALIZE;
    const bool keep_state = a.mean_state != nullptr;
    const bool planar = a.tile.layout == CT_LAYOUT_NCHW;
    const bool planar_out = planar || (a.flags & CT_MERGE_OUT_AS_INPUT);  // state / outputs at the memory index itself
    float fsf = 1.0f;  // scale of the folded moments back to true units
    if constexpr (kGauss) fsf = K / kk;
    if constexpr (STD == CT_STD_CONSTANT) fsf *= a.std_value;
    if constexpr (STD == CT_STD_MULTIPLIER) fsf *= a.std_value * a.inv_max_code;
    const float sv2 = fsf * fsf;
    [[maybe_unused]] const float index_rcp = x.index_rcp;
    [[maybe_unused]] float floor_magic = kFloorMagic;
    asm volatile("" : "+v"(floor_magic));  // one VGPR for the whole kernel (a VOP3 FMA cannot carry a literal)

    constexpr bool rgb252 = RGB252;  // interleaved RGB / BGR with packet stores: its own instantiation (the regrouping costs
                                     // registers the planar headline kernel, capped at 72, does not have)
    for (uint32_t tile = blockIdx.x; tile < x.n_tiles; tile += gridDim.x) {
        const uint32_t vec = tile * (uint32_t)kBlock + threadIdx.x;
        if (vec * (uint32_t)V >= a.q_count) continue;  // ragged last tile (no barrier below: lanes may leave)
        const uint32_t q0 = a.q_begin + vec * (uint32_t)V;

        int row_off[V];  // byte offset of each element's LUT row inside the LDS table
        if constexpr (kLut) {
            if (planar) {
                // channel by comparisons, row by a constant-divisor modulo when C == 3: a runtime 32-bit division costs
                // ~30 instructions, and this runs once per tile per thread
                int ch = 0;
                for (int c = 1; c < C; ++c) ch += q0 >= (uint32_t)c * a.tile.plane_local ? 1 : 0;
                const uint32_t qg = q0 + (uint32_t)ch * a.tile.chan_skip + a.tile.base;
                uint32_t off = q0 - (uint32_t)ch * a.tile.plane_local;
                int r = C == 3 ? (int)(qg % 3u) : (int)(qg % (uint32_t)C);
                const int skip_mod = (int)(a.tile.chan_skip % (uint32_t)C);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    row_off[e] = (kLookup ? ch : r) * E * 8;  // LOOKUP: the true channel (base.py:149-155)
                    int inc = 1;
                    if (++off == a.tile.plane_local) {
                        off = 0;
                        ++ch;
                        inc += skip_mod;
                    }
                    r += inc;
                    r = r >= C ? r - C : r;
                }
            } else if (C == 3) {
                // interleaved RGB / BGR: constant divisors (channel = m % 3, pixel = m / 3, row = global index % 3)
                const uint32_t plane_g = a.tile.plane_local + a.tile.chan_skip;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    uint32_t c, pixel;
                    a.tile.interleaved3(q0 + e, c, pixel);
                    const uint32_t qg = c * plane_g + a.tile.base + pixel;
                    row_off[e] = (int)(kLookup ? c : qg % 3u) * E * 8;
                }
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    int ch;
                    uint32_t qg;
                    a.tile.locate(a.tile.planar_index(q0 + e), ch, qg);
                    row_off[e] = (kLookup ? ch : (int)(qg % (uint32_t)C)) * E * 8;
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) row_off[e] = 0;
        }
        [[maybe_unused]] uint32_t rowc[V];  // the row offset as the addend of lds_entry_address
        if constexpr (kLut) {
#pragma unroll
            for (int e = 0; e < V; ++e) rowc[e] = lds_row_constant<kEntryShift>(row_off[e] << (kEntryShift - 3));
        }

        // loads are addressed as (wave-uniform exposure base) + (32-bit per-thread byte offset): no 64-bit VALU address math
        const uint32_t voff = q0 * (uint32_t)sizeof(T), svoff = q0 * 4u;
        // planar (state / output) index of memory element m: the identity for planar stacks, constant divisors for RGB / BGR
        auto planar_of = [&](uint32_t m) -> uint32_t {
            if (planar_out) return m;
            if (C == 3) {
                uint32_t c, pixel;
                a.tile.interleaved3(m, c, pixel);
                return c * a.tile.plane_local + pixel;
            }
            return a.tile.planar_index(m);
        };

        // ---- pivot: the running mean of the earlier batches, else the middle exposure's sample ----
        constexpr int VS = FIRST ? 1 : V;  // state registers exist only when there is state
        float p[V], WA[VS], varA[VS];
        double meanA[VS];
        [[maybe_unused]] auto probe_pivot = [&](uint64_t stack_base) {  // p = the probe exposure's y
            const Packet<float, V> pk = load_codes_as_float<T, V>(
                stack_base + (uint64_t)((int64_t)x.probe * a.image_stride * (int64_t)sizeof(T)), voff);
            const float itp = expo[x.probe].x;
            float tf[V];
            if constexpr (kLut) floor_index_bits<V>(pk.v, index_rcp, floor_magic, tf);
            if constexpr (kLut && CLAMP) {
#pragma unroll
                for (int e = 0; e < V; ++e) tf[e] = fminf(tf[e], x.tf_max);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float px = pk.v[e];
                float lin = px * a.inv_max_code;
                if constexpr (kCat) {
                    const float4 g = *reinterpret_cast<const float4 *>(lds + lds_entry_address<kEntryShift>(tf[e], rowc[e]));
                    float o = __builtin_fmaf(tf[e] - floor_magic, -x.step, px);
                    if constexpr (CLAMP) o = px > x.max_code ? 0.0f : o;
                    lin = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(g.w, o, g.z), o, g.y), o, g.x);
                } else if constexpr (kLut) {
                    const float2 g = *reinterpret_cast<const float2 *>(lds + lds_entry_address<kEntryShift>(tf[e], rowc[e]));
                    lin = __builtin_fmaf(g.y, rough ? __builtin_fmaf(tf[e] - floor_magic, -x.step, px) : px, g.x);
                }
                p[e] = lin * itp;
            }
        };
        if constexpr (FIRST) {
            probe_pivot(reinterpret_cast<uint64_t>(a.stack));
        } else {
            bool fresh = false;
            if constexpr (MULTI) fresh = x.fresh != 0;
            if (fresh) {  // a new merge: WBOMean starts at mean 0, weight 0 (statistics.py:30-31)
                if constexpr (MULTI) {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        meanA[e] = 0.0;
                        WA[e] = 0.0f;
                        varA[e] = 0.0f;
                    }
                    probe_pivot(reinterpret_cast<uint64_t>(x.batch_ptr[0]));
                }
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const uint32_t q = planar_of(q0 + e);
                    meanA[e] = a.mean_state[q];
                    WA[e] = a.sumw_state[q];
                    if constexpr (kHasStd) varA[e] = a.var_state[q];
                    p[e] = (float)meanA[e];
                }
            }
        }

        double mean_o[V];
        float var_o[V], Wt_o[V];
        const int n_batches = MULTI ? x.n_batches : 1;
        int n0 = 0;  // first exposure of the current batch within the launch (a.exposure / the LDS constants)
        for (int bi = 0; bi < n_batches; ++bi) {
        const int Bb = MULTI ? x.batch_size[bi] : B;  // exposures of this batch
        const uint64_t batch_base = MULTI ? reinterpret_cast<uint64_t>(x.batch_ptr[bi]) : reinterpret_cast<uint64_t>(a.stack);
        [[maybe_unused]] const uint64_t batch_std_base = MULTI ? reinterpret_cast<uint64_t>(x.std_ptr[bi]) : reinterpret_cast<uint64_t>(a.std_stack);
        for (int pass = 0;; ++pass) {
            float W[V], Swy[V], Saa[V], Sac[V], Scc[V];
#pragma unroll
            for (int e = 0; e < V; ++e) W[e] = Swy[e] = Saa[e] = Sac[e] = Scc[e] = 0.0f;

            auto run_batch = [&](auto rough_c, auto moments_c) {
            constexpr bool kRough = decltype(rough_c)::value;  // see the staging: exact but slower interval arithmetic
            constexpr bool kMoments = decltype(moments_c)::value;  // false: sum of weights and weighted sum only (kMeanFirst)
            // one exposure of this thread's V elements
            auto reduce = [&](const CodePk &pk, const Packet<float, V> &sp, uint32_t expo_adr) {
                const float2 ex = *reinterpret_cast<const float2 *>(lds + expo_adr);  // {1 / t_n, chain factor} of this exposure
                const float it = ex.x, cqn = ex.y;
                float pxv[V], ga[V], gs[V];
                [[maybe_unused]] float pxl[V];
                [[maybe_unused]] float dkv[V], wv[V];
                [[maybe_unused]] float tf[V];
#pragma unroll
                for (int e = 0; e < V; ++e) pxv[e] = pk.v[e];
                if constexpr (kLut) floor_index_bits<V>(pxv, index_rcp, floor_magic, tf);
                if constexpr (kLut && CLAMP) {  // a code above max_code: the last entry (top of the LUT, zero slope)
#pragma unroll
                    for (int e = 0; e < V; ++e) tf[e] = fminf(tf[e], x.tf_max);
                }
                static_for<V>([&](auto ec) {  // stage A: the V table gathers and the V transcendentals, each issued together
                    constexpr int e = decltype(ec)::value;
                    if constexpr (kCat) {
                        const float4 g = *reinterpret_cast<const float4 *>(lds + lds_entry_address<4>(tf[e], rowc[e]));
                        float o = __builtin_fmaf(tf[e] - floor_magic, -x.step, pxv[e]);  // code - i * step
                        [[maybe_unused]] bool above = false;  // a code above max_code: the model clamps it to the top, gradient 0
                        if constexpr (CLAMP) {
                            above = pxv[e] > x.max_code;
                            o = above ? 0.0f : o;
                        }
                        ga[e] = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(g.w, o, g.z), o, g.y), o, g.x);   // f
                        gs[e] = 0.0f;
                        if constexpr (kHasStd) {
                            gs[e] = __builtin_fmaf(__builtin_fmaf(3.0f * g.w, o, g.z + g.z), o, g.y);   // df / dcode
                            if constexpr (CLAMP) gs[e] = above ? 0.0f : gs[e];
                        }
                    } else if constexpr (kLut) {
                        const float2 g = *reinterpret_cast<const float2 *>(lds + lds_entry_address(tf[e], rowc[e]));
                        ga[e] = g.x;
                        gs[e] = g.y;
                        if constexpr (kRough) pxl[e] = __builtin_fmaf(tf[e] - floor_magic, -x.step, pxv[e]);  // code - i * step, exact
                    }
                    if constexpr (kGauss) {
                        dkv[e] = __builtin_fmaf(pxv[e], dk_mul, dk_add);
                        wv[e] = __builtin_amdgcn_exp2f(-dkv[e] * dkv[e]);
                    }
                });
                if constexpr (kGauss) {
                    // pins the four v_exp_f32 ahead of the dependent arithmetic: measured 4 % faster than letting the
                    // scheduler sink each one next to its first use (profiles/r02_merge_ablation.md)
#pragma unroll
                    for (int e = 0; e < V; ++e) asm volatile("" : "+v"(wv[e]));
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {  // stage B: f, weight, running sums
                    const float px = pxv[e];
                    const float lin = (kLookup || kCat) ? ga[e] : kLut ? __builtin_fmaf(gs[e], kRough ? pxl[e] : px, ga[e]) : px * a.inv_max_code;
                    const float yd = __builtin_fmaf(lin, it, -p[e]);  // y_n - p
                    if constexpr (kGauss) {
                        const float dk = dkv[e], w = wv[e];
                        W[e] += w;
                        Swy[e] = __builtin_fmaf(w, yd, Swy[e]);
                        if constexpr (kHasStd && kMoments) {
                            float wu = w;
                            if constexpr (STD == CT_STD_MULTIPLIER) wu = w * px;
                            if constexpr (STD == CT_STD_EXPLICIT) wu = w * sp.v[e];
                            const float av = dk * wu;
                            float cv;
                            if constexpr (kLookup) {
                                cv = av * yd;  // no gradient through the index: the whole variance is the weight path
                            } else {
                                const float ev = kLut ? (wu * gs[e]) * cqn : wu * cqn;
                                cv = __builtin_fmaf(av, yd, ev);
                            }
                            Saa[e] = __builtin_fmaf(av, av, Saa[e]);
                            Sac[e] = __builtin_fmaf(av, cv, Sac[e]);
                            Scc[e] = __builtin_fmaf(cv, cv, Scc[e]);
                        }
                    } else {
                        Swy[e] += yd;
                        if constexpr (kHasStd) {
                            float ev = kLut ? gs[e] * cqn : cqn;
                            if constexpr (STD == CT_STD_MULTIPLIER) ev *= px;
                            if constexpr (STD == CT_STD_EXPLICIT) ev *= sp.v[e];
                            Scc[e] = __builtin_fmaf(ev, ev, Scc[e]);
                        }
                    }
                }
            };

            // Software pipeline: kDepth exposures in flight per thread, kDepth + 1 per trip through rotating registers
            // (the slot freed by one step is re-filled by the next), so that no packet is ever copied -- a copy would
            // make the wavefront wait for the load it has just issued.
            auto fetch = [&](int n, CodePk &pk, Packet<float, V> &sp) {
                const int nn = n < Bb ? n : Bb - 1;  // past the end: re-load the last exposure (cache hit, unused)
                // Buffer loads: (scalar descriptor rebased to the exposure) + (32-bit per-thread byte offset) -- no vector
                // address arithmetic.  The base is laundered through an empty asm so LLVM cannot prove the prefetched
                // packet equal to a fresh load at its use (it would re-load there and drop the prefetch).
                uint64_t base = batch_base + (uint64_t)((int64_t)nn * a.image_stride * (int64_t)sizeof(T));
                asm volatile("" : "+s"(base));
                pk = load_codes_as_float<T, V>(base, voff);
                if constexpr (STD == CT_STD_EXPLICIT) {
                    uint64_t sbase = batch_std_base + (uint64_t)((int64_t)nn * a.image_stride * 4);
                    asm volatile("" : "+s"(sbase));
                    sp = load_buffer<Packet<float, V>>(sbase, svoff);
                }
            };
            constexpr int kRing = kPivotDepth + 1;
            CodePk ring[kRing];
            Packet<float, V> sring[STD == CT_STD_EXPLICIT ? kRing : 1];
            static_for<kPivotDepth>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                fetch(j, ring[j], sring[STD == CT_STD_EXPLICIT ? j : 0]);
            });
            uint32_t expo_adr = (uint32_t)lut_bytes + 8u * (uint32_t)n0;  // LDS byte address of this trip's per-exposure constants
            for (int n = 0; n < Bb; n += kRing) {
                static_for<kRing>([&](auto jc) {
                    constexpr int j = decltype(jc)::value, slot = (j + kPivotDepth) % kRing;
                    fetch(n + j + kPivotDepth, ring[slot], sring[STD == CT_STD_EXPLICIT ? slot : 0]);
                    if (j == 0 || n + j < Bb) reduce(ring[j], sring[STD == CT_STD_EXPLICIT ? j : 0], expo_adr + 8u * j);
                });
                expo_adr += 8u * kRing;
            }
            };
            // LOOKUP's closed-form variance is the weight path alone, sum a_n^2 (y_n - m)^2: about any pivot that is not the
            // mean it cancels, and every wavefront of C2 used to repeat its batch (tools/debug/retry_rate.py: 196 608 of
            // 196 608).  So its first pass computes the mean only (9 instead of 17 instructions per sample) and the second,
            // about that mean, the moments.
            constexpr bool kMeanFirst = kLookup && kHasStd;
            if constexpr (kMeanFirst) {
                if (pass == 0)
                    run_batch(std::false_type{}, std::false_type{});
                else
                    run_batch(std::false_type{}, std::true_type{});
            } else {
                if (rough)
                    run_batch(std::true_type{}, std::true_type{});
                else
                    run_batch(std::false_type{}, std::true_type{});
            }

            // ---- epilogue: WBOMean update (statistics.py:64-109) and the closed-form variance, division-free ----
            bool bad[V];
            float mb_f[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float Wb = kGauss ? W[e] : (float)Bb;
                const float Df = Wb + 1e-6f;  // float32 tensor + python float stays float32 (statistics.py:79-80)
                // v_rcp_f32 (1 ulp) as it comes: the quotient q is corrected against D below, and a last-bit error of
                // beta = frac / D or of frac moves the variance / the mean update by 1e-7 of themselves.  (Newton steps on
                // both reciprocals and the term-by-term quadratic form cost 8 of this epilogue's ~45 instructions, and
                // with several batches per launch the epilogue runs once per batch and element.)
                const float r = __builtin_amdgcn_rcpf(Df);
                const float num = __builtin_fmaf(-p[e], 1e-6f, Swy[e]);  // sum w y - p (W + 1e-6)
                float q = num * r;
                q = __builtin_fmaf(__builtin_fmaf(-q, Df, num), r, q);  // m_b - p
                float Wt = Wb, frac = 1.0f, var = 0.0f, gam = 0.0f;
                bad[e] = false;
                if constexpr (FIRST) {
                    mean_o[e] = (double)p[e] + (double)q;
                } else {
                    Wt = WA[e] + Wb;
                    const float rw = __builtin_amdgcn_rcpf(Wt);  // statistics.py:105, division-free
                    frac = WA[e] == 0.0f ? 1.0f : Wb * rw;  // (a fresh merge inside a MULTI launch: W_A = 0, W_B / W_B = 1 exactly)
                    const double diff = ((double)p[e] - meanA[e]) + (double)q;  // m_b - mean_A
                    mean_o[e] = __builtin_fma((double)frac, diff, meanA[e]);
                    gam = ((WA[e] * rw) * rw) * (float)diff;
                    var = varA[e];
                }
                Wt_o[e] = Wt;
                mb_f[e] = p[e] + q;
                if constexpr (kHasStd) {
                    const float beta = frac * r;
                    const float kap = __builtin_fmaf(-beta, q, gam);
                    // beta^2 Scc + 2 beta kappa Sac + kappa^2 Saa: the two squares first (S >= 0), then the cross term.
                    // Cancellation test: t1 + |t2| + t3 > kPivotCondLimit * upd  <=>  t2 < 0 and upd < S * 2 / (limit + 1)
                    const float bk = beta * kap;
                    const float S = __builtin_fmaf(kap * kap, Saa[e], (beta * beta) * Scc[e]);
                    const float upd = __builtin_fmaf(bk + bk, Sac[e], S);
                    if constexpr (kGauss) bad[e] = upd * (0.5f * (kPivotCondLimit + 1.0f)) < S;
                    if constexpr (kMeanFirst) bad[e] = bad[e] || pass == 0;  // (the first pass had no moments: go on about the mean)
                    var += fmaxf(upd, 0.0f) * sv2;
                }
                var_o[e] = var;
            }
            bool any_bad = false;
#pragma unroll
            for (int e = 0; e < V; ++e) any_bad |= bad[e];
            if (pass == 1 || !__any(any_bad)) break;
            if (x.retry_count && (threadIdx.x & 63) == 0) atomicAdd(x.retry_count, 1ull);
            // only the ill-conditioned elements move their pivot: the others recompute exactly what they had, so an
            // element's result does not depend on which other elements share its wavefront (tiles == whole, bit for bit)
#pragma unroll
            for (int e = 0; e < V; ++e) p[e] = bad[e] ? mb_f[e] : p[e];
        }
        if constexpr (MULTI) {  // internal_detach (hdr_merge.py:128): the batch's result is the next batch's state and pivot
#pragma unroll
            for (int e = 0; e < V; ++e) {
                meanA[e] = mean_o[e];
                WA[e] = Wt_o[e];
                varA[e] = var_o[e];
                p[e] = (float)mean_o[e];
            }
            n0 += Bb;
        }
        }  // batches

        if (keep_state) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const uint32_t q = planar_of(q0 + e);
                a.mean_state[q] = mean_o[e];
                a.sumw_state[q] = Wt_o[e];
                if constexpr (kHasStd) a.var_state[q] = var_o[e];
            }
        }
        if (finalize && rgb252) {
            if constexpr (RGB252) {
                // Regroup the WORKGROUP's results by channel plane through LDS: a full tile's 1024 consecutive memory
                // elements contain 84-85 whole groups of 12 elements = 4 pixels x 3 channels; thread 3 i + c takes plane c of
                // group i and writes its four consecutive pixels as 16-byte packets.  Only the <= 11 elements before the first
                // and after the last whole group of the TILE are stored one by one (1 % of the elements; regrouping per
                // wavefront left 4 % of them to such partial-line stores: FETCH_SIZE +11 %, WRITE_SIZE +8 %,
                // profiles/r03_layout_ingest.md).  Two workgroup barriers per tile; the ragged last tile of the image, where
                // threads have left the loop, stores element by element.  (A mapping that gives every wavefront 252 elements
                // = 84 whole pixels was measured first: its 504-byte wave loads cost 11 % more HBM fetch.)
                const uint32_t tile_first = tile * (uint32_t)(kBlock * V);     // relative to q_begin (0 in this mode)
                const bool tile_full = tile_first + (uint32_t)(kBlock * V) <= a.q_count;   // workgroup-uniform
                float sdv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) sdv[e] = kHasStd ? __builtin_amdgcn_sqrtf(var_o[e]) : 0.0f;
                if (tile_full) {
                    char *stage = lds + x.stage_off;
                    double *sm = reinterpret_cast<double *>(stage);            // 1024 means in memory order
                    float *ss = reinterpret_cast<float *>(stage + 8192);       // 1024 standard uncertainties
                    typedef double d2 __attribute__((ext_vector_type(2)));
                    typedef float f4 __attribute__((ext_vector_type(4)));
                    __syncthreads();  // the previous tile's readers are done with the stage
                    d2 m01 = {mean_o[0], mean_o[1]}, m23 = {mean_o[2], mean_o[3]};
                    *reinterpret_cast<d2 *>(sm + 4u * threadIdx.x) = m01;
                    *reinterpret_cast<d2 *>(sm + 4u * threadIdx.x + 2) = m23;
                    if constexpr (kHasStd) {
                        f4 sv = {sdv[0], sdv[1], sdv[2], sdv[3]};
                        *reinterpret_cast<f4 *>(ss + 4u * threadIdx.x) = sv;
                    }
                    __syncthreads();
                    const uint32_t g_first = (tile_first + 11u) / 12u, g_end = (tile_first + (uint32_t)(kBlock * V)) / 12u;   // whole groups
#pragma unroll
                    for (int e = 0; e < 4; ++e) {   // the ragged ends of the tile
                        const uint32_t m = q0 + (uint32_t)e - a.q_begin;
                        if (m < 12u * g_first || m >= 12u * g_end) {
                            const uint32_t q = planar_of(q0 + e);
                            static_cast<double *>(a.mean_out)[q] = mean_o[e];
                            if constexpr (kHasStd) a.std_out[q] = sdv[e];
                        }
                    }
                    // plane-major: threads 0 .. n-1 take plane 0 of the tile's n groups, the next n plane 1, ... -- consecutive
                    // lanes then store consecutive 32-byte packets of ONE plane (whole lines per wavefront; group-major
                    // threads 3 i + c alternated between the planes: WRITE_SIZE +20 %)
                    const uint32_t n_groups = g_end - g_first;               // 84 or 85: 3 n <= 256 threads
                    const uint32_t c = (threadIdx.x >= n_groups ? 1u : 0u) + (threadIdx.x >= 2u * n_groups ? 1u : 0u);
                    const uint32_t tri = threadIdx.x - c * n_groups;
                    if (threadIdx.x < 3u * n_groups) {
                        const uint32_t g = g_first + tri;                      // global group: pixels 4 g .. 4 g + 3
                        const uint32_t cm = a.tile.layout == CT_LAYOUT_NHWC_BGR ? 2u - c : c;
                        const uint32_t local = 12u * g - tile_first + cm;     // index of (pixel 4 g, memory channel cm) in the stage
                        Packet<double, 4> mo;
                        Packet<float, 4> so;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            mo.v[j] = sm[local + 3u * (uint32_t)j];
                            if constexpr (kHasStd) so.v[j] = ss[local + 3u * (uint32_t)j];
                        }
                        const size_t dst = (size_t)c * a.tile.plane_local + 4u * (size_t)g;
                        store_stream(reinterpret_cast<Packet<double, 4> *>(static_cast<double *>(a.mean_out) + dst), mo);
                        if constexpr (kHasStd) store_stream(reinterpret_cast<Packet<float, 4> *>(a.std_out + dst), so);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t q = planar_of(q0 + e);
                        static_cast<double *>(a.mean_out)[q] = mean_o[e];
                        if constexpr (kHasStd) a.std_out[q] = sdv[e];
                    }
                }
            }
        } else if (finalize && !planar_out) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const uint32_t q = planar_of(q0 + e);
                if (a.flags & CT_MERGE_MEAN_OUT_F32)
                    static_cast<float *>(a.mean_out)[q] = (float)mean_o[e];
                else
                    static_cast<double *>(a.mean_out)[q] = mean_o[e];
                if constexpr (kHasStd) a.std_out[q] = __builtin_amdgcn_sqrtf(var_o[e]);
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
                for (int e = 0; e < V; ++e) o.v[e] = __builtin_amdgcn_sqrtf(var_o[e]);
                store_stream(reinterpret_cast<Packet<float, V> *>(a.std_out + q0), o);
            }
        }
    }
}

// Workgroups of `kernel` that fit one compute unit (registers, LDS, waves), cached per instantiation.
template <typename KernelT>
static int pivot_blocks_per_cu(KernelT kernel, size_t lds)
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kBlock, lds) != hipSuccess || n < 1) n = 1;
    return n < 8 ? n : 8;
}

// Persistent grid: as many workgroups as are resident at once (so every workgroup walks the same number of tiles, +-1).
template <auto kernel>
static int launch_pivot_grid(const MergeArgs &a, const PivotArgs &x, size_t lds, hipStream_t stream)
{
    // residency per kernel (the kernel is a template argument, so these statics are per kernel); it is re-derived when
    // a later call needs more LDS (a larger LUT)
    static int per_cu = 0;
    static size_t per_cu_lds = 0;
    if (per_cu == 0 || lds > per_cu_lds) {
        per_cu = pivot_blocks_per_cu(kernel, lds);
        per_cu_lds = lds;
    }
    uint32_t grid = (uint32_t)(compute_units() * per_cu);
    if (grid > x.n_tiles) grid = x.n_tiles;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, stream, a, x);
    return hipGetLastError() == hipSuccess ? CT_OK : CT_ERR_LAUNCH;
}

// Dynamic LDS of merge_pivot_kernel: the table (16-byte entries for CATMULL, 8-byte otherwise; none without a model) and
// {1 / t_n, chain factor} per exposure.
static size_t pivot_lds_bytes(const MergeArgs &a, const PivotArgs &x, int interp)
{
    const size_t table = interp == CT_INTERP_NONE ? 0 : (size_t)a.channels * x.n_entries * (interp == CT_INTERP_CATMULL ? 16 : 8);
    return table + 2 * sizeof(float) * (size_t)a.batch;
}

// (with_merge_modes, the dispatch on the three modes of a merge, is in ct_merge.hpp)

// The several-batches launch of ct_hdr_merge_batches (ct_merge_multi.hip): packets of kPivotV, state-carrying instantiations.
int merge_pivot_multi(const MergeArgs &a, const PivotArgs &px, int dtype, bool clamp, int interp, int weight_mode, int std_mode,
                      hipStream_t s);

}  // namespace ct
