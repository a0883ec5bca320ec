// ct_export.hip -- planar (C, H, W) RGB results to the array an OpenCV writer takes (gfx950).
//
// save_image (clair_torch/common/data_io.py:228-234) casts a result to the file's dtype, transposes it to (H, W, C) and
// reverses a 3-channel image to BGR on the host.  Here that is one pass on the device, so the device-to-host copy
// already carries the final bytes:  dst[f][p][c'] = (dst type) src[f][c][p],  c' = C-1-c when reversed, p < plane = H*W.
// Both sides are contiguous in the pixel index p, so rows play no role.
//
// Roofline: HBM, (src + dst bytes) / bandwidth; every byte is touched once.
//
// Casts are the hardware's IEEE conversions, round to nearest even, subnormals kept (the library is not compiled with
// flush-to-zero): float64 -> float32 equals numpy's astype, float32 -> float64 is exact, and an export that keeps the
// type moves integer words, i.e. is a bit copy.
//
// PACKED (channels 1 or 3, compile-time): a thread owns one GROUP of G pixels of one image whose first output byte is
//   16-byte aligned in dst (a pixel count in front of it exists because 3 is invertible modulo the packet).  It fetches
//   the G elements of every plane with 16-byte loads (any alignment: planes are only element-aligned in general),
//   regroups and converts in registers and stores G * C elements as dense 16-byte packets.  What precedes the first
//   aligned pixel of an image (slot 0) and what follows its last whole group goes element by element.  A single channel
//   needs no regrouping and no per-image heads: the whole stack is one image.
// GENERIC (any other channel count): one thread per output element.
// Every load is that of an element src[f][c][p] with p < plane, every store lies in the thread's own pixels of dst[f].
#include "ct_device.hpp"

namespace ct {

struct ExportArgs {
    const void *src;
    void *dst;
    int64_t plane;     // pixels per image
    int64_t total;     // GENERIC: output elements
    uint32_t slots;    // PACKED: threads per image (slot 0 = head, then one per group)
    uint32_t threads;  // PACKED: n_images * slots
    uint32_t channels; // GENERIC
    uint32_t reverse;  // GENERIC
};

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

template <typename S, typename D>
__device__ __forceinline__ D export_cast(S v)
{
    return (D)v;
}

template <typename S, typename D, int C, bool REV>
__global__ __launch_bounds__(kBlock) void export_packed_kernel(const ExportArgs a)
{
    constexpr int SK = 16 / (int)sizeof(S), DK = 16 / (int)sizeof(D);  // elements per 16-byte packet
    constexpr int G = C == 1 ? 8 : 4;                                  // pixels per group: whole packets on both sides
    static_assert(G % SK == 0 && (G * C) % DK == 0, "a group is whole packets");

    const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (t >= a.threads) return;
    const uint32_t f = t / a.slots, slot = t - f * a.slots;
    const int64_t image = (int64_t)f * C * a.plane;
    const S *src = static_cast<const S *>(a.src) + image;
    D *dst = static_cast<D *>(a.dst) + image;

    // pixels in front of the first group: up to the first pixel whose output is 16-byte aligned
    const uint32_t to_aligned = (uint32_t)((0 - reinterpret_cast<uintptr_t>(dst)) & 15u) / (uint32_t)sizeof(D);
    const int64_t head = C == 3 ? ((to_aligned * 11u) & (DK - 1)) : to_aligned;  // 3 * 11 = 1 (mod 16)
    int64_t p0, n;
    if (slot == 0) {
        p0 = 0;
        n = head < a.plane ? head : a.plane;
    } else {
        p0 = head + (int64_t)(slot - 1) * G;
        if (p0 >= a.plane) return;
        n = a.plane - p0 < G ? a.plane - p0 : G;
    }

    if (slot != 0 && n == G) {
        D o[G * C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            S in[G];
            const S *sp = src + c * a.plane + p0;
#pragma unroll
            for (int l = 0; l < G / SK; ++l) {
                u32x4_t v;
                __builtin_memcpy(&v, sp + l * SK, 16);
                __builtin_memcpy(&in[l * SK], &v, 16);
            }
#pragma unroll
            for (int k = 0; k < G; ++k) o[k * C + (REV ? C - 1 - c : c)] = export_cast<S, D>(in[k]);
        }
        D *dp = dst + p0 * C;
#pragma unroll
        for (int pk = 0; pk < G * C / DK; ++pk) {
            u32x4_t v;
            __builtin_memcpy(&v, &o[pk * DK], 16);
            *reinterpret_cast<u32x4_t *>(dp + pk * DK) = v;
        }
        return;
    }
    for (int64_t k = 0; k < n; ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c) dst[(p0 + k) * C + (REV ? C - 1 - c : c)] = export_cast<S, D>(src[c * a.plane + p0 + k]);
    }
}

template <typename S, typename D>
__global__ __launch_bounds__(kBlock) void export_generic_kernel(const ExportArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.total) return;
    const int64_t pixel = i / a.channels;  // over all images
    const uint32_t cd = (uint32_t)(i - pixel * a.channels);
    const int64_t f = pixel / a.plane, p = pixel - f * a.plane;
    const uint32_t c = a.reverse ? a.channels - 1u - cd : cd;
    static_cast<D *>(a.dst)[i] = export_cast<S, D>(static_cast<const S *>(a.src)[(f * a.channels + c) * a.plane + p]);
}

template <typename S, typename D>
static int launch_export(ExportArgs a, int64_t n_images, int32_t channels, bool reverse, hipStream_t s)
{
    constexpr int64_t kMaxThreads = 0xffffffffll - kBlock;  // a grid's threads are counted with 32 bits
    if (channels == 1 || channels == 3) {
        if (channels == 1) {  // no regrouping: the stack is one long image
            a.plane *= n_images;
            n_images = 1;
        }
        const int64_t group = channels == 1 ? 8 : 4;
        const int64_t slots = 1 + (a.plane + group - 1) / group;
        if (slots > kMaxThreads || n_images > kMaxThreads / slots) return CT_ERR_TOO_LARGE;
        a.slots = (uint32_t)slots;
        a.threads = (uint32_t)(n_images * slots);
        const dim3 grid((a.threads + kBlock - 1) / kBlock);
        if (channels == 1)
            hipLaunchKernelGGL((export_packed_kernel<S, D, 1, false>), grid, dim3(kBlock), 0, s, a);
        else if (reverse)
            hipLaunchKernelGGL((export_packed_kernel<S, D, 3, true>), grid, dim3(kBlock), 0, s, a);
        else
            hipLaunchKernelGGL((export_packed_kernel<S, D, 3, false>), grid, dim3(kBlock), 0, s, a);
    } else {
        if (a.total > kMaxThreads) return CT_ERR_TOO_LARGE;
        a.channels = (uint32_t)channels;
        a.reverse = reverse ? 1u : 0u;
        hipLaunchKernelGGL((export_generic_kernel<S, D>), dim3((uint32_t)((a.total + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           s, a);
    }
    return hipGetLastError() == hipSuccess ? CT_OK : CT_ERR_LAUNCH;
}

}  // namespace ct

extern "C" int ct_export_cv(const void *src_dev, int32_t src_is_f64, void *dst_dev, int32_t dst_is_f64, int64_t n_images,
                            int32_t channels, int64_t plane, int32_t reverse_channels, void *stream)
{
    using namespace ct;
    if (channels < 1 || n_images < 0 || plane < 0) return CT_ERR_INVALID_ARGUMENT;
    if (n_images == 0 || plane == 0) return CT_OK;
    const uintptr_t src_align = src_is_f64 ? 8 : 4, dst_align = dst_is_f64 ? 8 : 4;
    if (!src_dev || !dst_dev || reinterpret_cast<uintptr_t>(src_dev) % src_align != 0 ||
        reinterpret_cast<uintptr_t>(dst_dev) % dst_align != 0)
        return CT_ERR_INVALID_ARGUMENT;
    // elements and byte offsets are 64-bit; the element count itself has to fit with room for the byte size
    int64_t per_image, total;
    if (__builtin_mul_overflow(plane, (int64_t)channels, &per_image) || __builtin_mul_overflow(per_image, n_images, &total) ||
        total > (INT64_MAX >> 4))
        return CT_ERR_TOO_LARGE;
    ExportArgs a = {};
    a.src = src_dev;
    a.dst = dst_dev;
    a.plane = plane;
    a.total = total;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool rev = reverse_channels != 0;
    // an export that keeps the type moves integer words: a bit copy, whatever the payload
    if (src_is_f64 && dst_is_f64) return launch_export<uint64_t, uint64_t>(a, n_images, channels, rev, s);
    if (!src_is_f64 && !dst_is_f64) return launch_export<uint32_t, uint32_t>(a, n_images, channels, rev, s);
    if (src_is_f64) return launch_export<double, float>(a, n_images, channels, rev, s);
    return launch_export<float, double>(a, n_images, channels, rev, s);
}
