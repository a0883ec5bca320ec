// ct_extrema.hip -- the bounds of a data-dependent Normalize, taken on the device (gfx950).
//
// Normalize() with max_val and / or min_val None normalises a batch by its own extrema (normalize_tensor,
// clair_torch/common/general_functions.py:373-376): x.max() / x.min() of the whole tensor the transform receives, i.e. of
// a raw frame (or stack) after the constant stages that stand in front of it.  ingest_extrema_kernel is that reduction as a
// read-only streaming pass, with one set of constants PER FRAME of a dense stack: it evaluates the prefix per element with
// the ingest kernels' own ingest_stages, and reduces min, max and "any NaN" (torch's extrema propagate NaN, v_min_f32 /
// v_max_f32 drop it).  The frame is the grid's y index, so it is workgroup-uniform; a frame's gridDim.x workgroups walk that
// frame alone and leave partial[frame][blockIdx.x].  ingest_extrema_fold_kernel, one workgroup per frame, folds the frame's
// partials -- no atomics, so the result does not depend on the order the workgroups ran in -- and forms sub, top and
// div = fl32(top - sub) for the CT_INGEST_AFFINE_DATA stage of ct_ingest.hip: two launches whatever the number of frames.
// ct_ingest_extrema_frames gives every frame of its stack constants of its own (a consumer whose frames are batches of their
// own: linearize_dataset_generator); ct_ingest_extrema is the same call with the whole stack as its one frame (grid y = 1),
// and since min, max and the NaN flag are exact and order-independent, the four floats of frame f are those
// ct_ingest_extrema gives for that frame alone.
//
// Roofline: HBM, sizeof(T) bytes read per sample, every byte once; nothing written but 16 bytes per workgroup.
//
// A span is a run of elements that share the clamp pair.  When no prefix stage depends on the channel (the empty prefix
// included) a frame is ONE span, whatever its layout.  Otherwise: PLANES, each plane of the frame is a span (channel = plane
// index % channels, wave-uniform); PACKED3, the interleaved frame is one span whose element e belongs to memory channel
// e % 3 (BGR: plane 2 - e % 3).  A span is read as
//   head     the elements in front of the first 16-byte boundary                        (thread t of the grid: element t)
//   packets  16-byte aligned loads, kLoads per thread in flight; a workgroup owns kBlock * kLoads consecutive packets per
//            trip (lanes side by side in each of the kLoads rows), the frame's workgroups stride over the trips (persistent
//            workgroups)
//   rest     what follows the last whole packet (PACKED3: the last whole triple)         (thread t: element rest0 + t)
// The walk starts at the frame's own base address -- the head length and, for PACKED3, the channel phase of the registers
// follow from that address, so they are per frame (a frame's byte size need not be a multiple of 16).
// PACKED3 with channel-dependent stages reads three consecutive packets per thread: 3 * 16 bytes hold a whole number of
// pixels, so the channel of every register is the same for all lanes (it depends on head % 3 alone).
// Integer codes with an empty prefix are reduced as integers (packed 16-bit min / max: the cast to float32 is exact and
// monotone) and converted once per workgroup.
// Every load is that of an element of the workgroup's frame; nothing is written except the workgroup's partial.
#include <algorithm>

#include "ct_ingest_stages.hpp"

namespace ct {

constexpr int kExtremaGroups = 2048;  // most workgroups of a launch = partials in the workspace: 8 per CU, 32 waves
constexpr int kLoads = 4;             // 16-byte loads a thread has in flight

struct ExtremaPartial {  // 16 bytes
    float lo, hi;
    uint32_t nan, pad;
};

struct ExtremaArgs {
    const void *src;
    ExtremaPartial *partial;
    int64_t span;       // elements per span
    uint32_t n_spans;   // PLANES: planes of the stack; else 1
    uint32_t channels;  // PLANES: span index % channels selects the clamp pair
    uint32_t n_stages;
    ct_ingest_stage stage[CT_EXTREMA_MAX_PREFIX];
};

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint16_t u16x2_t __attribute__((ext_vector_type(2)));

enum ExtremaMode { kRawCodes = 0, kUniform = 1, kPlanes = 2, kPacked3 = 3, kPacked3Rev = 4 };

// float32 values: min / max that ignore NaN plus a flag for it
struct FloatAcc {
    float lo = INFINITY, hi = -INFINITY;
    uint32_t nan = 0;
    __device__ __forceinline__ void add(float v)
    {
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
        nan |= v != v ? 1u : 0u;
    }
};

// raw uint8 / uint16 codes: two 16-bit lanes per register (v_pk_min_u16 / v_pk_max_u16)
struct CodeAcc {
    u16x2_t lo = {0xffff, 0xffff}, hi = {0, 0};
    __device__ __forceinline__ void add_pair(u16x2_t p)
    {
        lo = __builtin_elementwise_min(lo, p);
        hi = __builtin_elementwise_max(hi, p);
    }
    __device__ __forceinline__ void add(uint32_t code) { add_pair(u16x2_t{(uint16_t)code, (uint16_t)code}); }
    template <typename T>
    __device__ __forceinline__ void add_packet(const u32x4_t w)
    {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t word = w[k];  // (a copy: __builtin_bit_cast of the vector's element itself reads element 0)
            if (sizeof(T) == 2) {
                add_pair(__builtin_bit_cast(u16x2_t, word));
            } else {  // bytes 0, 2 and bytes 1, 3 of the word as two pairs
                add_pair(__builtin_bit_cast(u16x2_t, word & 0x00ff00ffu));
                add_pair(__builtin_bit_cast(u16x2_t, (word >> 8) & 0x00ff00ffu));
            }
        }
    }
    __device__ __forceinline__ FloatAcc as_float() const
    {
        FloatAcc f;
        f.lo = (float)(lo[0] < lo[1] ? lo[0] : lo[1]);
        f.hi = (float)(hi[0] > hi[1] ? hi[0] : hi[1]);
        return f;
    }
};

template <typename T>
__device__ __forceinline__ void extrema_element(const ExtremaArgs &a, uint32_t c, T x, FloatAcc &acc)
{
    float v[1] = {(float)x};
    ingest_stages<false>(v, a, c);
    acc.add(v[0]);
}

template <typename T>
__device__ __forceinline__ void extrema_element(const ExtremaArgs &, uint32_t, T x, CodeAcc &acc)
{
    acc.add((uint32_t)x);
}

// one aligned packet of a span whose elements share the channel c
template <typename T>
__device__ __forceinline__ void extrema_packet(const ExtremaArgs &a, uint32_t c, const u32x4_t w, FloatAcc &acc)
{
    constexpr int E = 16 / (int)sizeof(T);
    T in[E];
    __builtin_memcpy(in, &w, 16);
    float v[E];
#pragma unroll
    for (int k = 0; k < E; ++k) v[k] = (float)in[k];
    ingest_stages<false>(v, a, c);
#pragma unroll
    for (int k = 0; k < E; ++k) acc.add(v[k]);
}

template <typename T>
__device__ __forceinline__ void extrema_packet(const ExtremaArgs &, uint32_t, const u32x4_t w, CodeAcc &acc)
{
    acc.add_packet<T>(w);
}

// three consecutive packets whose first element is element H3 (mod 3) of a pixel: memory channel m owns the registers
// (m - H3) mod 3, +3, +6, ...; plane REV ? 2 - m : m of the planar result selects the clamp pair
template <typename T, bool REV, int H3>
__device__ __forceinline__ void extrema_triple(const ExtremaArgs &a, const u32x4_t (&w)[3], FloatAcc &acc)
{
    constexpr int E = 16 / (int)sizeof(T);
    T in[3 * E];
    __builtin_memcpy(in, w, 48);
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        float v[E];
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = (float)in[(m + 3 - H3) % 3 + 3 * k];
        ingest_stages<false>(v, a, (uint32_t)(REV ? 2 - m : m));
#pragma unroll
        for (int k = 0; k < E; ++k) acc.add(v[k]);
    }
}

template <typename T, bool INTERLEAVED, bool REV, int U, typename Acc>
__device__ __forceinline__ void extrema_unit(const ExtremaArgs &a, uint32_t c, uint32_t h3, const u32x4_t (&w)[U], Acc &acc)
{
    if constexpr (INTERLEAVED) {
        if (h3 == 0)
            extrema_triple<T, REV, 0>(a, w, acc);
        else if (h3 == 1)
            extrema_triple<T, REV, 1>(a, w, acc);
        else
            extrema_triple<T, REV, 2>(a, w, acc);
    } else {
        extrema_packet<T>(a, c, w[0], acc);
    }
}

// A span of n elements at src.  INTERLEAVED: element e of the span has memory channel e % 3 (the span starts at a pixel);
// else every element has channel c.
template <typename T, bool INTERLEAVED, bool REV, typename Acc>
__device__ __forceinline__ void extrema_span(const ExtremaArgs &a, const T *src, int64_t n, uint32_t c, Acc &acc)
{
    constexpr int E = 16 / (int)sizeof(T);
    constexpr int kUnit = INTERLEAVED ? 3 : 1;       // packets a thread reads side by side
    constexpr int kRows = INTERLEAVED ? 2 : kLoads;  // units a thread has in flight
    const int64_t head0 = (int64_t)(((0 - reinterpret_cast<uintptr_t>(src)) & 15u) / sizeof(T));
    const int64_t head = head0 < n ? head0 : n;
    const int64_t units = (n - head) / (E * kUnit);
    const int64_t rest0 = head + units * (E * kUnit);
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    // the ragged ends: fewer than 16 elements in front, fewer than 4 packets behind (kBlock >= 64 threads cover both)
    if (t < head) {
        const uint32_t ce = INTERLEAVED ? (uint32_t)(REV ? 2 - t % 3 : t % 3) : c;
        extrema_element<T>(a, ce, src[t], acc);
    }
    if (rest0 + t < n) {
        const int64_t e = rest0 + t;
        const uint32_t ce = INTERLEAVED ? (uint32_t)(REV ? 2 - e % 3 : e % 3) : c;
        extrema_element<T>(a, ce, src[e], acc);
    }
    const u32x4_t *pk = reinterpret_cast<const u32x4_t *>(src + head);
    const uint32_t h3 = (uint32_t)(head % 3);  // wave-uniform
    constexpr int64_t kTrip = (int64_t)kBlock * kRows;
    for (int64_t base = (int64_t)blockIdx.x * kTrip; base < units; base += (int64_t)gridDim.x * kTrip) {
        if (base + kTrip <= units) {  // workgroup-uniform: every load of the trip is issued before the first use
            u32x4_t w[kRows][kUnit];
#pragma unroll
            for (int r = 0; r < kRows; ++r)
#pragma unroll
                for (int j = 0; j < kUnit; ++j) w[r][j] = pk[(base + r * kBlock + threadIdx.x) * kUnit + j];
#pragma unroll
            for (int r = 0; r < kRows; ++r) extrema_unit<T, INTERLEAVED, REV>(a, c, h3, w[r], acc);
        } else {  // the last, partial trip of the span
            for (int64_t u = base + threadIdx.x; u < units; u += kBlock) {
                u32x4_t w[kUnit];
#pragma unroll
                for (int j = 0; j < kUnit; ++j) w[j] = pk[u * kUnit + j];
                extrema_unit<T, INTERLEAVED, REV>(a, c, h3, w, acc);
            }
        }
    }
}

__device__ __forceinline__ void fold(FloatAcc &a, const FloatAcc &b)
{
    a.lo = fminf(a.lo, b.lo);
    a.hi = fmaxf(a.hi, b.hi);
    a.nan |= b.nan;
}

// workgroup -> one FloatAcc (thread 0 returns true and holds it): wave shuffles, then LDS across the waves
__device__ __forceinline__ bool extrema_block_fold(FloatAcc &s)
{
    for (int off = 32; off > 0; off >>= 1) {
        FloatAcc o;
        o.lo = __shfl_down(s.lo, off, 64);
        o.hi = __shfl_down(s.hi, off, 64);
        o.nan = __shfl_down(s.nan, off, 64);
        fold(s, o);
    }
    __shared__ ExtremaPartial part[kBlock / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ExtremaPartial{s.lo, s.hi, s.nan, 0u};
    __syncthreads();
    if (threadIdx.x != 0) return false;
    for (int w = 1; w < kBlock / 64; ++w) {
        s.lo = fminf(s.lo, part[w].lo);
        s.hi = fmaxf(s.hi, part[w].hi);
        s.nan |= part[w].nan;
    }
    return true;
}

// Frame blockIdx.y of a dense stack: a.span * a.n_spans elements per frame (PLANES: n_spans planes of a.span elements,
// plane q of channel q % a.channels; else one span).  Workgroup blockIdx.x of gridDim.x walks that frame and leaves
// partial[frame][blockIdx.x].
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void ingest_extrema_kernel(const ExtremaArgs a)
{
    const T *src = static_cast<const T *>(a.src) + (int64_t)blockIdx.y * ((int64_t)a.n_spans * a.span);
    FloatAcc acc;
    if constexpr (MODE == kRawCodes) {
        CodeAcc codes;
        extrema_span<T, false, false>(a, src, a.span, 0u, codes);
        acc = codes.as_float();
    } else if constexpr (MODE == kUniform) {
        extrema_span<T, false, false>(a, src, a.span, 0u, acc);
    } else if constexpr (MODE == kPlanes) {
        for (uint32_t q = 0; q < a.n_spans; ++q)
            extrema_span<T, false, false>(a, src + (int64_t)q * a.span, a.span, q % a.channels, acc);
    } else {
        extrema_span<T, true, MODE == kPacked3Rev>(a, src, a.span, 0u, acc);
    }
    if (extrema_block_fold(acc)) {
        u32x4_t out = {__float_as_uint(acc.lo), __float_as_uint(acc.hi), acc.nan, 0u};
        *reinterpret_cast<u32x4_t *>(&a.partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x]) = out;
    }
}

// workgroup f: the n_partials partials of frame f -> consts[4 f .. 4 f + 3] = {sub, div, data min, data max}
__global__ __launch_bounds__(kBlock) void ingest_extrema_fold_kernel(const ExtremaPartial *__restrict__ partial, int n_partials,
                                                                     int from_data, float fixed_min, float fixed_max,
                                                                     float *__restrict__ consts)
{
    partial += (int64_t)blockIdx.x * n_partials;
    consts += 4 * (int64_t)blockIdx.x;
    FloatAcc acc;
    for (int k = threadIdx.x; k < n_partials; k += kBlock) {
        FloatAcc p;
        p.lo = partial[k].lo;
        p.hi = partial[k].hi;
        p.nan = partial[k].nan;
        fold(acc, p);
    }
    if (!extrema_block_fold(acc)) return;
    const float lo = acc.nan ? __builtin_nanf("") : acc.lo, hi = acc.nan ? __builtin_nanf("") : acc.hi;
    const float sub = (from_data & CT_EXTREMA_MIN) ? lo : fixed_min;
    const float top = (from_data & CT_EXTREMA_MAX) ? hi : fixed_max;
    consts[0] = sub;
    consts[1] = top - sub;
    consts[2] = lo;
    consts[3] = hi;
}

template <typename T>
static void launch_extrema(const ExtremaArgs &a, int mode, dim3 grid, hipStream_t s)
{
    const dim3 block(kBlock);
    if (mode == kUniform)
        hipLaunchKernelGGL((ingest_extrema_kernel<T, kUniform>), grid, block, 0, s, a);
    else if (mode == kPlanes)
        hipLaunchKernelGGL((ingest_extrema_kernel<T, kPlanes>), grid, block, 0, s, a);
    else if (mode == kPacked3)
        hipLaunchKernelGGL((ingest_extrema_kernel<T, kPacked3>), grid, block, 0, s, a);
    else if (mode == kPacked3Rev)
        hipLaunchKernelGGL((ingest_extrema_kernel<T, kPacked3Rev>), grid, block, 0, s, a);
    else if constexpr (sizeof(T) < sizeof(float))  // kRawCodes: integer codes only
        hipLaunchKernelGGL((ingest_extrema_kernel<T, kRawCodes>), grid, block, 0, s, a);
}

// Partials (= most workgroups) per frame of an n_frames launch: together about kExtremaGroups, which is what fills the
// device (8 workgroups per CU) -- one 1080p uint8 frame alone has 380 trips and cannot
static inline int64_t extrema_groups_per_frame(int64_t n_frames)
{
    return n_frames >= kExtremaGroups ? 1 : (kExtremaGroups + n_frames - 1) / n_frames;
}

constexpr int64_t kExtremaMaxFrames = 65535;  // a grid's y extent

// bytes of the partials of an n_frames launch; 0: one call does not take that many frames
static inline int64_t extrema_workspace(int64_t n_frames)
{
    if (n_frames < 1 || n_frames > kExtremaMaxFrames) return 0;
    return n_frames * extrema_groups_per_frame(n_frames) * (int64_t)sizeof(ExtremaPartial);
}

// Both entry points.  per_frame: every image of the stack is a frame with constants of its own (consts_dev holds four floats
// per image); else the whole stack is the one frame.  The two test workspace and size in opposite orders, which decides the
// status of a call with both faults: the whole-stack call tests its workspace first, the per-frame call the size.
static int ingest_extrema(const void *src_dev, int32_t dtype, int32_t layout, int64_t n_images, bool per_frame, int32_t channels,
                          int64_t plane, const ct_ingest_stage *prefix, int32_t n_prefix, int32_t from_data, float fixed_min,
                          float fixed_max, void *workspace_dev, int64_t workspace_bytes, float *consts_dev, void *stream)
{
    bool by_channel = false;
    const int rc = ingest_validate(dtype, layout, n_images, channels, plane, prefix, n_prefix, CT_EXTREMA_MAX_PREFIX, 0, by_channel);
    if (rc != CT_OK) return rc;
    if (from_data < CT_EXTREMA_MIN || from_data > (CT_EXTREMA_MIN | CT_EXTREMA_MAX)) return CT_ERR_INVALID_ARGUMENT;
    if (n_images == 0 || plane == 0) return CT_ERR_INVALID_ARGUMENT;  // torch raises on the extrema of an empty tensor
    if (!src_dev || !aligned(src_dev, dtype_bytes(dtype))) return CT_ERR_INVALID_ARGUMENT;
    if (!consts_dev || !aligned(consts_dev, sizeof(float))) return CT_ERR_INVALID_ARGUMENT;
    const int64_t n_frames = per_frame ? n_images : 1;
    const bool workspace_ok = workspace_dev && workspace_bytes >= extrema_workspace(n_frames) && aligned(workspace_dev, 16);
    if (!per_frame && !workspace_ok) return CT_ERR_INVALID_ARGUMENT;
    int64_t rows, total;
    if (__builtin_mul_overflow(n_images, (int64_t)channels, &rows) || __builtin_mul_overflow(rows, plane, &total) ||
        total > (INT64_MAX >> 4) || rows > 0x7fffffff || n_frames > kExtremaMaxFrames)
        return CT_ERR_TOO_LARGE;
    if (!workspace_ok) return CT_ERR_INVALID_ARGUMENT;
    ExtremaArgs a = {};
    a.src = src_dev;
    a.partial = static_cast<ExtremaPartial *>(workspace_dev);
    a.n_stages = (uint32_t)n_prefix;
    for (int32_t k = 0; k < n_prefix; ++k) a.stage[k] = prefix[k];
    a.span = total / n_frames;  // a frame
    a.n_spans = 1;
    a.channels = 1;
    int mode = kUniform;
    if (by_channel && layout == CT_LAYOUT_NCHW) {
        mode = kPlanes;
        a.span = plane;
        a.n_spans = (uint32_t)(rows / n_frames);
        a.channels = (uint32_t)channels;
    } else if (by_channel) {
        mode = layout == CT_LAYOUT_NHWC_BGR ? kPacked3Rev : kPacked3;
    } else if (n_prefix == 0 && dtype != CT_DTYPE_F32) {
        mode = kRawCodes;
    }
    const int64_t elems_per_trip = (int64_t)kBlock * (16 / (int64_t)dtype_bytes(dtype)) * (mode >= kPacked3 ? 6 : kLoads);
    const int64_t trips = std::max<int64_t>(1, (a.span + elems_per_trip - 1) / elems_per_trip);
    const int groups = (int)std::min<int64_t>(extrema_groups_per_frame(n_frames), trips);
    const dim3 grid((uint32_t)groups, (uint32_t)n_frames);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == CT_DTYPE_U8)
        launch_extrema<uint8_t>(a, mode, grid, s);
    else if (dtype == CT_DTYPE_U16)
        launch_extrema<uint16_t>(a, mode, grid, s);
    else
        launch_extrema<float>(a, mode, grid, s);
    if (hipGetLastError() != hipSuccess) return CT_ERR_LAUNCH;
    hipLaunchKernelGGL(ingest_extrema_fold_kernel, dim3((uint32_t)n_frames), dim3(kBlock), 0, s, a.partial, groups, from_data,
                       fixed_min, fixed_max, consts_dev);
    return hipGetLastError() == hipSuccess ? CT_OK : CT_ERR_LAUNCH;
}

}  // namespace ct

extern "C" int64_t ct_ingest_extrema_workspace(void) { return ct::extrema_workspace(1); }

extern "C" int ct_ingest_extrema(const void *src_dev, int32_t dtype, int32_t layout, int64_t n_images, int32_t channels,
                                 int64_t plane, const ct_ingest_stage *prefix, int32_t n_prefix, int32_t from_data,
                                 float fixed_min, float fixed_max, void *workspace_dev, int64_t workspace_bytes,
                                 float *consts_dev, void *stream)
{
    return ct::ingest_extrema(src_dev, dtype, layout, n_images, false, channels, plane, prefix, n_prefix, from_data, fixed_min,
                              fixed_max, workspace_dev, workspace_bytes, consts_dev, stream);
}

extern "C" int64_t ct_ingest_extrema_frames_workspace(int64_t n_frames) { return ct::extrema_workspace(n_frames); }

extern "C" int ct_ingest_extrema_frames(const void *src_dev, int32_t dtype, int32_t layout, int64_t n_frames, int32_t channels,
                                        int64_t plane, const ct_ingest_stage *prefix, int32_t n_prefix, int32_t from_data,
                                        float fixed_min, float fixed_max, void *workspace_dev, int64_t workspace_bytes,
                                        float *consts_dev, void *stream)
{
    return ct::ingest_extrema(src_dev, dtype, layout, n_frames, true, channels, plane, prefix, n_prefix, from_data, fixed_min,
                              fixed_max, workspace_dev, workspace_bytes, consts_dev, stream);
}
