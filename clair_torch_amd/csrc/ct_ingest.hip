// ct_ingest.hip -- a recognised gpu_transforms chain in one pass: raw codes / pixels to a planar float32 stack (gfx950).
//
// The reference runs CastTo(float32), Normalize(max, min, range) (normalize_tensor,
// clair_torch/common/general_functions.py:359-388) and ClampAlongDims (clamp_along_dims, general_functions.py:392-436;
// the transform classes are clair_torch/common/transforms.py:108-157) as separate float32 tensor ops on the CPU.  Here
// the chain is evaluated per sample in registers, with the reference's arithmetic: float32 throughout, every operation
// rounded on its own (-ffp-contract=off), subnormals kept.
//   AFFINE  t = x - sub;  t = t / div;  t = t * mul;  t = t + add     sub = fl32(min), div = fl32(max - min),
//           mul = fl32(hi - lo), add = fl32(lo).  All four always run (x * 1 + 0 still turns -0.0 into +0.0); the
//           division is the correctly rounded IEEE one (plain operator /, which hipcc expands to the div_scale / div_fmas
//           / div_fixup sequence; tests/test_gpu_ingest.py compares every uint16 code against the CPU).
//   CLAMP   t = x < lo ? lo : x;  t = t > hi ? hi : t   -- torch.clamp's min(max(x, lo), hi): NaN stays NaN (both
//           comparisons are false), and a bound that equals x keeps x (so -0.0 against a bound of +0.0 stays -0.0, as
//           std::max / MAXPS give it on the CPU).  One (lo, hi) pair per channel of the planar result.
//
// Roofline: HBM, sizeof(T) bytes read and 4 written per sample, every byte once.
//
// PLANAR (any C): a workgroup row (blockIdx.y) is one plane, so the channel -- the clamp pair -- is wave-uniform.  A
//   thread owns 4 consecutive output elements whose store is one 16-byte aligned packet and fetches their 4 inputs with
//   one 4 / 8 / 16-byte load (any alignment: planes are only element-aligned in general).  When no stage depends on the
//   channel the host passes the whole stack as one plane.
// PACKED3 (interleaved (B,H,W,3), RGB or BGR): a workgroup row is one image.  A thread owns 4 pixels: it reads their 12
//   elements with dense loads, regroups in registers and writes one packet per plane -- the mirror image of
//   export_packed_kernel.  The pixel count in front of the first group aligns plane 0; the other planes are aligned with
//   it iff H*W is a multiple of 4, else their packets are stored element by element.
// What precedes the first aligned packet of a plane / image (slot 0) and what follows the last whole one goes element by
// element.  Every load is that of an element of the thread's own pixels, every store lies in the thread's own [p0, p0+n).
// The stage list travels by value in the kernel arguments; the stage loop is wave-uniform.
//
// AFFINE_DATA (ct_ingest_transform_data) is AFFINE whose sub and div are not known when the launch is queued: a
// data-dependent Normalize (max_val and / or min_val None) takes them from the batch, and ct_ingest_extrema leaves them in
// consts_dev[0..1].  The *_data_kernel twins read the two floats once per thread through a wave-uniform load; the kernels
// of the constant chains take no such pointer and are the code they were.
#include "ct_ingest_stages.hpp"

namespace ct {

struct IngestArgs {
    const void *src;
    float *dst;
    int64_t plane;      // elements per plane (PLANAR) / pixels per image (PACKED3)
    uint32_t first;     // first plane / image of this launch (a grid's y extent is 65535)
    uint32_t channels;  // PLANAR: plane index % channels selects the clamp pair (1 when no stage depends on it)
    uint32_t n_stages;
    ct_ingest_stage stage[CT_INGEST_MAX_STAGES];
};

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
constexpr int kGroup = 4;        // output elements per packet
constexpr uint32_t kMaxRows = 65535;

// slot 0 -> the elements in front of the first aligned packet, slot s >= 1 -> packet s - 1; false when there is nothing
__device__ __forceinline__ bool ingest_span(const float *dst, int64_t plane, int64_t &p0, int64_t &n, bool &whole)
{
    const int64_t head = (int64_t)(((0 - reinterpret_cast<uintptr_t>(dst)) & 15u) / sizeof(float));
    const int64_t slot = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (slot == 0) {
        p0 = 0;
        n = head < plane ? head : plane;
        whole = false;
        return n > 0;
    }
    p0 = head + (slot - 1) * kGroup;
    if (p0 >= plane) return false;
    n = plane - p0 < kGroup ? plane - p0 : kGroup;
    whole = n == kGroup;
    return true;
}

__device__ __forceinline__ void ingest_store_packet(float *dp, const float (&v)[kGroup])
{
    u32x4_t w;
    __builtin_memcpy(&w, v, 16);
    *reinterpret_cast<u32x4_t *>(dp) = w;
}

template <typename T, bool DATA>
__device__ __forceinline__ void ingest_planar(const IngestArgs &a, const float *consts)
{
    const float dsub = DATA ? consts[0] : 0.0f, ddiv = DATA ? consts[1] : 1.0f;
    const uint32_t q = a.first + blockIdx.y;
    const uint32_t c = q % a.channels;
    const T *src = static_cast<const T *>(a.src) + (int64_t)q * a.plane;
    float *dst = a.dst + (int64_t)q * a.plane;
    int64_t p0, n;
    bool whole;
    if (!ingest_span(dst, a.plane, p0, n, whole)) return;
    if (whole) {
        T in[kGroup];
        __builtin_memcpy(in, src + p0, sizeof(in));
        float v[kGroup];
#pragma unroll
        for (int k = 0; k < kGroup; ++k) v[k] = (float)in[k];
        ingest_stages<DATA>(v, a, c, dsub, ddiv);
        ingest_store_packet(dst + p0, v);
        return;
    }
    for (int64_t k = 0; k < n; ++k) {
        float v[1] = {(float)src[p0 + k]};
        ingest_stages<DATA>(v, a, c, dsub, ddiv);
        dst[p0 + k] = v[0];
    }
}

template <typename T, bool REV, bool DATA>
__device__ __forceinline__ void ingest_packed3(const IngestArgs &a, const float *consts)
{
    constexpr int C = 3;
    const float dsub = DATA ? consts[0] : 0.0f, ddiv = DATA ? consts[1] : 1.0f;
    const uint32_t f = a.first + blockIdx.y;
    const T *src = static_cast<const T *>(a.src) + (int64_t)f * C * a.plane;
    float *dst = a.dst + (int64_t)f * C * a.plane;
    int64_t p0, n;
    bool whole;
    if (!ingest_span(dst, a.plane, p0, n, whole)) return;
    if (whole) {
        T in[kGroup * C];
        __builtin_memcpy(in, src + p0 * C, sizeof(in));
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float v[kGroup];
#pragma unroll
            for (int k = 0; k < kGroup; ++k) v[k] = (float)in[k * C + (REV ? C - 1 - c : c)];
            ingest_stages<DATA>(v, a, (uint32_t)c, dsub, ddiv);
            float *dp = dst + c * a.plane + p0;
            if ((reinterpret_cast<uintptr_t>(dp) & 15u) == 0) {  // plane 0 always; the others iff plane % 4 == 0
                ingest_store_packet(dp, v);
            } else {
#pragma unroll
                for (int k = 0; k < kGroup; ++k) dp[k] = v[k];
            }
        }
        return;
    }
    for (int64_t k = 0; k < n; ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float v[1] = {(float)src[(p0 + k) * C + (REV ? C - 1 - c : c)]};
            ingest_stages<DATA>(v, a, (uint32_t)c, dsub, ddiv);
            dst[c * a.plane + p0 + k] = v[0];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void ingest_planar_kernel(const IngestArgs a)
{
    ingest_planar<T, false>(a, nullptr);
}

template <typename T, bool REV>
__global__ __launch_bounds__(kBlock) void ingest_packed3_kernel(const IngestArgs a)
{
    ingest_packed3<T, REV, false>(a, nullptr);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void ingest_planar_data_kernel(const IngestArgs a, const float *__restrict__ consts)
{
    ingest_planar<T, true>(a, consts);
}

template <typename T, bool REV>
__global__ __launch_bounds__(kBlock) void ingest_packed3_data_kernel(const IngestArgs a, const float *__restrict__ consts)
{
    ingest_packed3<T, REV, true>(a, consts);
}

template <typename T>
static int launch_ingest(IngestArgs a, int32_t layout, int64_t rows, const float *consts, hipStream_t s)
{
    const int64_t slots = 1 + (a.plane + kGroup - 1) / kGroup;
    const dim3 block(kBlock);
    for (int64_t first = 0; first < rows; first += kMaxRows) {
        a.first = (uint32_t)first;
        const dim3 grid((uint32_t)((slots + kBlock - 1) / kBlock), (uint32_t)(rows - first < kMaxRows ? rows - first : kMaxRows));
        if (consts) {
            if (layout == CT_LAYOUT_NCHW)
                hipLaunchKernelGGL((ingest_planar_data_kernel<T>), grid, block, 0, s, a, consts);
            else if (layout == CT_LAYOUT_NHWC_BGR)
                hipLaunchKernelGGL((ingest_packed3_data_kernel<T, true>), grid, block, 0, s, a, consts);
            else
                hipLaunchKernelGGL((ingest_packed3_data_kernel<T, false>), grid, block, 0, s, a, consts);
        } else if (layout == CT_LAYOUT_NCHW)
            hipLaunchKernelGGL((ingest_planar_kernel<T>), grid, block, 0, s, a);
        else if (layout == CT_LAYOUT_NHWC_BGR)
            hipLaunchKernelGGL((ingest_packed3_kernel<T, true>), grid, block, 0, s, a);
        else
            hipLaunchKernelGGL((ingest_packed3_kernel<T, false>), grid, block, 0, s, a);
        if (hipGetLastError() != hipSuccess) return CT_ERR_LAUNCH;
    }
    return CT_OK;
}

// consts_dev NULL: the constant chains of ct_ingest_transform (no AFFINE_DATA stage); else ct_ingest_transform_data
static int ingest_transform(const void *src_dev, int32_t dtype, int32_t layout, int64_t n_images, int32_t channels, int64_t plane,
                            const ct_ingest_stage *stages, int32_t n_stages, float *dst_dev, const float *consts_dev, bool data,
                            void *stream)
{
    bool by_channel = false;
    const int rc = ingest_validate(dtype, layout, n_images, channels, plane, stages, n_stages, CT_INGEST_MAX_STAGES, data ? 1 : 0,
                                   by_channel);
    if (rc != CT_OK) return rc;
    if (data && (!consts_dev || !aligned(consts_dev, sizeof(float)))) return CT_ERR_INVALID_ARGUMENT;
    if (n_images == 0 || plane == 0) return CT_OK;
    if (!src_dev || !dst_dev || !aligned(src_dev, dtype_bytes(dtype)) || !aligned(dst_dev, sizeof(float)))
        return CT_ERR_INVALID_ARGUMENT;
    // elements and byte offsets are 64-bit; planes / images are counted with 32 bits, a plane's packets with a grid's x
    int64_t rows, total;
    if (__builtin_mul_overflow(n_images, (int64_t)channels, &rows) || __builtin_mul_overflow(rows, plane, &total) ||
        total > (INT64_MAX >> 4) || rows > 0x7fffffff)
        return CT_ERR_TOO_LARGE;
    IngestArgs a = {};
    a.src = src_dev;
    a.dst = dst_dev;
    a.n_stages = (uint32_t)n_stages;
    for (int32_t k = 0; k < n_stages; ++k) a.stage[k] = stages[k];
    if (layout != CT_LAYOUT_NCHW) {
        rows = n_images;
        a.plane = plane;
        a.channels = 3;
    } else if (by_channel) {
        a.plane = plane;
        a.channels = (uint32_t)channels;
    } else {  // the channel plays no role: the stack is one long plane
        rows = 1;
        a.plane = total;
        a.channels = 1;
    }
    if (a.plane / kGroup / kBlock + 2 > 0x7fffffff) return CT_ERR_TOO_LARGE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == CT_DTYPE_U8) return launch_ingest<uint8_t>(a, layout, rows, consts_dev, s);
    if (dtype == CT_DTYPE_U16) return launch_ingest<uint16_t>(a, layout, rows, consts_dev, s);
    return launch_ingest<float>(a, layout, rows, consts_dev, s);
}

}  // namespace ct

extern "C" int ct_ingest_transform(const void *src_dev, int32_t dtype, int32_t layout, int64_t n_images, int32_t channels,
                                   int64_t plane, const ct_ingest_stage *stages, int32_t n_stages, float *dst_dev,
                                   void *stream)
{
    return ct::ingest_transform(src_dev, dtype, layout, n_images, channels, plane, stages, n_stages, dst_dev, nullptr, false, stream);
}

extern "C" int ct_ingest_transform_data(const void *src_dev, int32_t dtype, int32_t layout, int64_t n_images, int32_t channels,
                                        int64_t plane, const ct_ingest_stage *stages, int32_t n_stages, float *dst_dev,
                                        const float *consts_dev, void *stream)
{
    return ct::ingest_transform(src_dev, dtype, layout, n_images, channels, plane, stages, n_stages, dst_dev, consts_dev, true, stream);
}
