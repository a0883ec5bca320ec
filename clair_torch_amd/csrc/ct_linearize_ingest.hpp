// ct_linearize_ingest.hpp -- what the fused chain + linearization kernels share (ct_linearize_ingest.hip on dense frames,
// ct_linearize_ingest_strided.hip on every step-th row and column of them): the argument block, the slot / span scheme of
// a thread's 4 output elements, the sample step behind the chain (li_sample4: four linearize_sample of ct_device.hpp, the
// step ct_linearize.hip runs, and their `tiny` fix-up), the flat-field epilogue of the FLAT instantiations behind it (li_flat1 /
// li_flat4, which ct_linearize.hip shares), the packet store, and the host-side launch loop and dispatch over
// element type, interpolation and uncertainty mode (with_enum, with_linearize_std).  One copy of each: the outputs of the
// two files agree bit for bit because they run the same device functions.
#pragma once
#include <type_traits>
#include "ct_args.hpp"
#include "ct_ingest_stages.hpp"

namespace ct {

struct LinIngestArgs {
    const void *src;
    const float *std_in;   // EXPLICIT: planar (F, C, plane) float32, like the outputs
    const float *lut;
    const float *consts;   // (F, 4) per-frame {sub, div, min, max} of a CT_INGEST_AFFINE_DATA stage, or NULL
    float *lin_out;
    float *std_out;
    int64_t image_stride;  // source elements between consecutive frames
    int64_t plane;         // H_tile * W
    uint32_t first;        // first plane / frame of this launch (a grid's y extent is 65535)
    uint32_t channels, n_points;
    uint32_t plane_global;  // H_global * W: global flat index of (c, local p) = c * plane_global + base + p
    uint32_t base;          // row_offset * W
    uint32_t reversed;      // PACKED3: memory channel cm feeds plane 2 - cm (BGR)
    uint32_t by_channel;    // some clamp holds different pairs for different channels (then C <= CT_INGEST_MAX_CHANNELS);
                            // else every channel takes pair 0, whatever C is
    float std_value;
    uint32_t n_stages;
    ct_ingest_stage stage[CT_INGEST_MAX_STAGES];
};

struct alignas(16) LinIngestPacket {
    float v[4];
};

// The flat field of the FLAT instantiations (ct_linearize*_flat): planar (C, plane) float32 of the OUTPUT's shape -- the
// downscaled one behind a step, the band's rows for a row band -- and the C channel means, a constant of the run
struct LinFlat {
    const float *flat;
    const float *flat_std;  // or NULL
    const float *mean;      // (C) float32 in device memory
};

// The argument block of a kernel family with the flat field BEHIND it: the FLAT = false instantiations take the family's own
// block, unchanged, so every offset they load from is the one they had
template <typename Base>
struct WithFlat : Base {
    LinFlat ff;
};
template <typename Base, bool FLAT>
using flat_args_t = std::conditional_t<FLAT, WithFlat<Base>, Base>;

constexpr int kLiGroup = 4;     // output elements per packet
constexpr int kLiSlots = 4;     // slots per thread
constexpr uint32_t kLiMaxRows = 65535;

// slot 0 -> the elements in front of the first aligned packet, slot s >= 1 -> packet s - 1; false when there is nothing
__device__ __forceinline__ bool li_span(int64_t head, int64_t slot, int64_t plane, int64_t &p0, int &n)
{
    if (slot == 0) {
        p0 = 0;
        n = (int)(head < plane ? head : plane);
        return n > 0;
    }
    p0 = head + (slot - 1) * kLiGroup;
    if (p0 >= plane) return false;
    n = plane - p0 < kLiGroup ? (int)(plane - p0) : kLiGroup;
    return true;
}

// four samples behind the chain -> (lin, std); `r` is the LINEAR / CATMULL row of the first one, `c` the channel
template <int INTERP, int STD, bool WRITE_STD>
__device__ __forceinline__ void li_sample4(const float (&x)[kLiGroup], const float (&sg)[kLiGroup], const char *lds, int L, int C,
                                           int c, int r, float std_value, LinIngestPacket &lo, LinIngestPacket &so)
{
    constexpr int kEntry = lut_entry_bytes(INTERP);
    const float top = (float)(L - 1);
    [[maybe_unused]] bool tiny = false;  // some 0 < |grad * std| < 1e-18 among these
#pragma unroll
    for (int e = 0; e < kLiGroup; ++e) {
        // RANGED = false: x is a float behind the chain (and so is the x of MULTIPLIER)
        const LinSample s = linearize_sample<INTERP, STD, WRITE_STD, false>(x[e], lds + (INTERP == CT_INTERP_LOOKUP ? c : r) * L * kEntry,
                                                                            top, sg[e], std_value);
        lo.v[e] = s.lin;
        so.v[e] = s.sd;
        tiny |= s.tiny;
        ++r;
        r = r >= C ? r - C : r;
    }
    if constexpr (WRITE_STD && STD != CT_STD_NONE) {
        if (__builtin_expect(__any(tiny), 0)) {  // wave-uniform, practically never taken (linearize_sample)
#pragma unroll
            for (int e = 0; e < kLiGroup; ++e)
                if (so.v[e] < 1e-18f && so.v[e] != 0.0f) so.v[e] = sqrtf(so.v[e] * so.v[e]);
        }
    }
}

// n <= 4 results to dp[0..n): one packet when all four are there and dp is 16-byte aligned, else element by element
__device__ __forceinline__ void li_store(float *dp, const LinIngestPacket &v, int n)
{
    if (n == kLiGroup && (reinterpret_cast<uintptr_t>(dp) & 15u) == 0) {
        store_stream(reinterpret_cast<LinIngestPacket *>(dp), v);
        return;
    }
#pragma unroll
    for (int k = 0; k < kLiGroup; ++k)
        if (k < n) dp[k] = v.v[k];
}

// n <= 4 floats from sp[0..n) (any alignment), zeros behind them
__device__ __forceinline__ void li_load_std(const float *sp, int n, float (&sg)[kLiGroup])
{
    if (n == kLiGroup) {
        __builtin_memcpy(sg, sp, sizeof(sg));
        return;
    }
#pragma unroll
    for (int k = 0; k < kLiGroup; ++k) sg[k] = k < n ? sp[k] : 0.0f;
}

// ---- the flat-field epilogue ------------------------------------------------------------------------------------------------
// linearization.py:48-57,118-130 on one sample the unfused launch would have stored (behind the `tiny` fix-up): exactly the
// expressions of flatfield_apply_kernel<float, false> (ct_flatfield.hip) with the mean a constant -- same float32 types, same
// order, every operation rounded on its own (-ffp-contract=off) -- so the results are those of ct_flatfield_apply on the
// stored pair, bit for bit.  `fs` is read with WITH_STD only.
template <bool WITH_STD>
__device__ __forceinline__ void li_flat1(float &lin, float &sd, float flat, float fs, float M)
{
    const float den = flat + 1e-6f;
    const float v = lin;
    lin = (v / den) * M;
    float var = sd * sd;
    if constexpr (WITH_STD) {
        const float grad = -(M * v) / (den * den);
        const float gs = grad * fs;
        var = var + gs * gs;
    }
    sd = sqrtf(var);
}

// ... on the n <= 4 (lin, sd) of a packet at element p0 of a channel plane whose flat field starts at `flat` (`flat_std`: its
// uncertainty or NULL, a wave-uniform branch) and whose mean is M.  The loads are li_load_std's: one 16-byte packet for a
// whole group, element by element otherwise; lanes k >= n compute on zeros and are never stored.
__device__ __forceinline__ void li_flat4(LinIngestPacket &lo, LinIngestPacket &so, const float *flat, const float *flat_std, int64_t p0,
                                         int n, float M)
{
    float fl[kLiGroup], fs[kLiGroup];
    li_load_std(flat + p0, n, fl);
    if (flat_std) {
        li_load_std(flat_std + p0, n, fs);
#pragma unroll
        for (int e = 0; e < kLiGroup; ++e) li_flat1<true>(lo.v[e], so.v[e], fl[e], fs[e], M);
    } else {
#pragma unroll
        for (int e = 0; e < kLiGroup; ++e) li_flat1<false>(lo.v[e], so.v[e], fl[e], 0.0f, M);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// `rows` workgroup rows (planes or frames) of `kernel`, at most kLiMaxRows per launch; Args is LinIngestArgs or derives from it
template <typename Args>
static int li_launch_rows(void (*kernel)(const Args), Args a, int interp, int64_t rows, hipStream_t s)
{
    const int64_t slots = 1 + (a.plane + kLiGroup - 1) / kLiGroup;
    const int64_t per_block = (int64_t)kBlock * kLiSlots;
    const size_t lds = lut_lds_bytes(interp, a.channels, a.n_points);
    const dim3 block(kBlock);
    for (int64_t first = 0; first < rows; first += kLiMaxRows) {
        a.first = (uint32_t)first;
        const dim3 grid((uint32_t)((slots + per_block - 1) / per_block), (uint32_t)(rows - first < kLiMaxRows ? rows - first : kLiMaxRows));
        hipLaunchKernelGGL(kernel, grid, block, lds, s, a);
        if (hipGetLastError() != hipSuccess) return CT_ERR_LAUNCH;
    }
    return CT_OK;
}

// dtype / interp / std_mode / write_std -> template arguments; Launch<T, INTERP, STD, WRITE_STD>::run(a, packed, rows, s) picks
// the kernel of a file.  LOOKUP with uncertainties has no gradient path (refused by the caller) and no kernel.
template <template <typename, int, int, bool> class Launch, typename T, typename Args>
static int li_dispatch_typed(const Args &a, bool packed, int64_t rows, int interp, int std_mode, bool write_std, hipStream_t s)
{
    return with_enum<CT_INTERP_LOOKUP, CT_INTERP_LINEAR, CT_INTERP_CATMULL, CT_INTERP_NONE>(interp, [&](auto I) {
        auto run = [&](auto S, auto W) { return Launch<T, I, S, W>::run(a, packed, rows, s); };
        if constexpr (I == CT_INTERP_LOOKUP)
            return with_linearize_std<>(std_mode, write_std, run);
        else
            return with_linearize_std<CT_STD_CONSTANT, CT_STD_MULTIPLIER, CT_STD_EXPLICIT>(std_mode, write_std, run);
    });
}

template <template <typename, int, int, bool> class Launch, typename Args>
static int li_dispatch(const Args &a, int32_t dtype, bool packed, int64_t rows, int interp, int std_mode, bool write_std, hipStream_t s)
{
    if (dtype == CT_DTYPE_U8) return li_dispatch_typed<Launch, uint8_t>(a, packed, rows, interp, std_mode, write_std, s);
    if (dtype == CT_DTYPE_U16) return li_dispatch_typed<Launch, uint16_t>(a, packed, rows, interp, std_mode, write_std, s);
    return li_dispatch_typed<Launch, float>(a, packed, rows, interp, std_mode, write_std, s);
}

// What the entry points check in this order, before any pointer into device memory: the stack and the stage list
// (ingest_validate over `plane` elements per channel; AFFINE_DATA only with constants), the constants' alignment, the model and
// the uncertainty mode, LOOKUP with uncertainties (linearization.py:100-105: autograd.grad raises, no gradient path), the LDS
// budget, the row count.  `rows`: workgroup rows of the launch.
static inline int li_check_call(int32_t dtype, int64_t n_frames, const ct_geometry *geom, int64_t plane, const ct_ingest_stage *stages,
                                int32_t n_stages, const float *std_dev, int32_t std_mode, const ct_icrf *icrf, const float *consts_dev,
                                bool &by_channel, int64_t &rows)
{
    int rc = ingest_validate(dtype, geom->layout, n_frames, geom->channels, plane, stages, n_stages, CT_INGEST_MAX_STAGES,
                             consts_dev ? 1 : 0, by_channel);
    if (rc != CT_OK) return rc;
    if (!aligned(consts_dev, sizeof(float))) return CT_ERR_INVALID_ARGUMENT;
    if (!icrf_ok(icrf) || !std_mode_ok(std_mode, std_dev)) return CT_ERR_INVALID_ARGUMENT;
    if (std_mode != CT_STD_NONE && icrf->interp == CT_INTERP_LOOKUP) return CT_ERR_NO_GRADIENT_PATH;
    if (lut_lds_bytes(icrf->interp, geom->channels, icrf->n_points) > kLdsBudget) return CT_ERR_TOO_LARGE;
    rows = n_frames;
    if ((geom->layout == CT_LAYOUT_NCHW && __builtin_mul_overflow(n_frames, (int64_t)geom->channels, &rows)) || rows > 0x7fffffff)
        return CT_ERR_TOO_LARGE;
    return CT_OK;
}

// ... and after them the pointers: frames and lin_out are required, everything is aligned to its element
static inline bool li_pointers_ok(const void *frames_dev, int32_t dtype, const float *std_dev, const float *lin_out_dev,
                                  const float *std_out_dev)
{
    return frames_dev && lin_out_dev && aligned(frames_dev, dtype_bytes(dtype)) && aligned(lin_out_dev, sizeof(float)) &&
           aligned(std_out_dev, sizeof(float)) && aligned(std_dev, sizeof(float));
}

// ... and behind those, in the _flat entry points: the flat field and its means are required, everything is aligned to its
// element, and the correction writes a std
static inline bool li_flat_ok(const LinFlat &ff, const float *std_out_dev)
{
    return ff.flat && ff.mean && std_out_dev && aligned(ff.flat, sizeof(float)) && aligned(ff.flat_std, sizeof(float)) &&
           aligned(ff.mean, sizeof(float));
}

}  // namespace ct
