// ct_downscale.hip -- x[..., ::step, ::step] on a contiguous stack of raw codes / pixels (gfx950).
//
// StridedDownscale (clair_torch/common/transforms.py:194-216) in front of the code-domain kernels: the selected pixels
// are compacted in their own element type and memory layout (planar, or interleaved with the channels of a pixel kept
// together), so everything downstream runs on a dense, smaller stack and gives the bits it would give on a stack that
// was sliced on the host.
//
// Roofline: HBM.  Only every step-th source row is touched; within such a row whole 128-byte lines arrive whenever
// step * pixel_bytes is below the line size, so the floor is (selected rows at full width) + output.
//
// One kernel, two ways to fetch.  A thread owns one GROUP of an output row: 16 / elem_bytes output pixels, i.e.
// pixel_elems packets of 16 bytes whose first byte is 16-byte aligned in dst (a pixel count exists for every odd
// pixel_elems because pixel_elems is then invertible modulo the packet).  What precedes the first aligned pixel of a
// row (slot 0) and what follows the last whole group is copied element by element.
//   WIDE   (step 2..4, pixel_elems 1 or 3: compile-time): the source span of the group is fetched with consecutive
//          16-byte loads (any alignment: the rows of a stack are not 16-byte aligned in general), the elements are picked
//          from the registers at compile-time offsets, and the packets are stored.  A span that would read past the end
//          of src (the last groups of the stack) falls back to:
//   GATHER (any step, any pixel_elems): one load per element, skipping the lines between selected pixels, the same
//          dense 16-byte stores.  With an even pixel_elems a group is one packet of elements instead of whole pixels.
// Every load address is that of a selected element (or, WIDE, inside a span checked against src's size); every store
// lies inside the thread's own [x0, x0 + n) of its output row.
#include <algorithm>
#include "ct_device.hpp"

namespace ct {

template <int EB> struct ElemOf;
template <> struct ElemOf<1> { typedef uint8_t type; };
template <> struct ElemOf<2> { typedef uint16_t type; };
template <> struct ElemOf<4> { typedef uint32_t type; };

struct DownscaleArgs {
    const unsigned char *src;
    unsigned char *dst;
    int64_t src_bytes;   // size of the source stack
    uint32_t rows;       // n_planes * ho output rows
    uint32_t h, ho;      // source / output rows per plane
    uint32_t row_in;     // elements per source row  (w * pixel_elems)
    uint32_t row_out;    // elements per output row  (wo * pixel_elems)
    uint32_t pe, step;   // pixel_elems, step (GATHER; WIDE has them as template arguments)
    uint32_t slot_bits;  // a workgroup covers 2^slot_bits slots of 256 >> slot_bits rows
};

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// element at compile-time byte offset `off` of the words loaded for a span
template <int EB, int NW>
__device__ __forceinline__ uint32_t span_element(const uint32_t (&w)[NW], int off)
{
    if constexpr (EB == 4)
        return w[off >> 2];
    else
        return (w[off >> 2] >> ((off & 3) * 8)) & (EB == 2 ? 0xffffu : 0xffu);
}

template <int EB, int PE_T, int STEP_T>
__global__ __launch_bounds__(kBlock) void downscale_kernel(const DownscaleArgs a)
{
    typedef typename ElemOf<EB>::type T;
    constexpr bool WIDE = PE_T > 0;
    constexpr int K = 16 / EB;                   // elements per packet
    constexpr int PACKETS = WIDE ? PE_T : 1;     // packets per group
    constexpr uint32_t GE = K * PACKETS;         // elements per group
    const uint32_t pe = WIDE ? (uint32_t)PE_T : a.pe, step = WIDE ? (uint32_t)STEP_T : a.step;

    const uint32_t row = blockIdx.x * (kBlock >> a.slot_bits) + (threadIdx.x >> a.slot_bits);
    const uint32_t slot = (blockIdx.y << a.slot_bits) + (threadIdx.x & ((1u << a.slot_bits) - 1u));
    if (row >= a.rows) return;
    const uint32_t p = row / a.ho, i = row - p * a.ho;
    const int64_t src_row = ((int64_t)p * a.h + (int64_t)i * step) * a.row_in;  // first element of the selected source row
    const T *srow = reinterpret_cast<const T *>(a.src) + src_row;
    T *drow = reinterpret_cast<T *>(a.dst) + (int64_t)row * a.row_out;

    // elements in front of the first group: up to the first pixel (WIDE) / element (GATHER) that is 16-byte aligned in dst
    const uint32_t to_aligned = (uint32_t)((0 - reinterpret_cast<uintptr_t>(drow)) & 15u) / EB;
    const uint32_t head = WIDE ? ((to_aligned * (PE_T == 3 ? 11u : 1u)) & (K - 1)) * PE_T : to_aligned;  // 3 * 11 = 1 (mod 16)
    uint32_t x0, n;
    if (slot == 0) {
        x0 = 0;
        n = min(head, a.row_out);
    } else {
        const uint64_t xs = head + (uint64_t)(slot - 1) * GE;
        if (xs >= a.row_out) return;
        x0 = (uint32_t)xs;
        n = min(GE, a.row_out - x0);
    }
    const uint32_t pixel_stride = step * pe;  // source elements between two selected pixels
    uint32_t j = x0 / pe, ch = x0 - j * pe;   // output pixel and channel of element x0

    if (slot != 0 && n == GE) {
        if constexpr (WIDE) {
            // ch == 0: the group is K whole pixels j .. j + K - 1
            constexpr int SPAN = ((K - 1) * STEP_T + 1) * PE_T * EB, LOADS = (SPAN + 15) / 16;
            const int64_t first = src_row + (int64_t)j * pixel_stride;
            if (first * EB + LOADS * 16 <= a.src_bytes) {
                const unsigned char *sp = a.src + first * EB;
                uint32_t w[LOADS * 4];
#pragma unroll
                for (int l = 0; l < LOADS; ++l) {
                    u32x4_t v;
                    __builtin_memcpy(&v, sp + 16 * l, 16);
                    w[4 * l + 0] = v.x;
                    w[4 * l + 1] = v.y;
                    w[4 * l + 2] = v.z;
                    w[4 * l + 3] = v.w;
                }
                constexpr int PER_WORD = 4 / EB;
#pragma unroll
                for (int pk = 0; pk < PACKETS; ++pk) {
                    uint32_t o[4];
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        o[m] = 0;
#pragma unroll
                        for (int t = 0; t < PER_WORD; ++t) {
                            const int e = (pk * 4 + m) * PER_WORD + t;  // output element of the group
                            const int off = ((e / PE_T) * STEP_T * PE_T + e % PE_T) * EB;
                            o[m] |= span_element<EB>(w, off) << (t * EB * 8 & 31);
                        }
                    }
                    u32x4_t v;
                    v.x = o[0];
                    v.y = o[1];
                    v.z = o[2];
                    v.w = o[3];
                    *reinterpret_cast<u32x4_t *>(drow + x0 + pk * K) = v;
                }
                return;
            }
        }
#pragma unroll
        for (int pk = 0; pk < PACKETS; ++pk) {
            T e[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                e[k] = srow[j * pixel_stride + ch];
                if (++ch == pe) {
                    ch = 0;
                    ++j;
                }
            }
            u32x4_t v;
            __builtin_memcpy(&v, e, 16);
            *reinterpret_cast<u32x4_t *>(drow + x0 + pk * K) = v;
        }
        return;
    }
    for (uint32_t k = 0; k < n; ++k) {
        drow[x0 + k] = srow[j * pixel_stride + ch];
        if (++ch == pe) {
            ch = 0;
            ++j;
        }
    }
}

template <int EB, int PE_T, int STEP_T>
static void launch_downscale(const DownscaleArgs &a, hipStream_t s)
{
    constexpr uint32_t GE = (16 / EB) * (PE_T > 0 ? PE_T : 1);
    const uint32_t slots = 1 + (a.row_out + GE - 1) / GE;
    const uint32_t per_block = 1u << a.slot_bits;
    const dim3 grid((a.rows + (kBlock >> a.slot_bits) - 1) / (kBlock >> a.slot_bits), (slots + per_block - 1) / per_block);
    hipLaunchKernelGGL((downscale_kernel<EB, PE_T, STEP_T>), grid, dim3(kBlock), 0, s, a);
}

template <int EB>
static void dispatch_downscale(const DownscaleArgs &a, hipStream_t s)
{
#define CT_DOWNSCALE_WIDE(PE, STEP)                      \
    if (a.pe == PE && a.step == STEP) {                  \
        launch_downscale<EB, PE, STEP>(a, s);            \
        return;                                          \
    }
    CT_DOWNSCALE_WIDE(1, 2)
    CT_DOWNSCALE_WIDE(1, 3)
    CT_DOWNSCALE_WIDE(1, 4)
    CT_DOWNSCALE_WIDE(3, 2)
    CT_DOWNSCALE_WIDE(3, 3)
    CT_DOWNSCALE_WIDE(3, 4)
#undef CT_DOWNSCALE_WIDE
    launch_downscale<EB, 0, 0>(a, s);
}

}  // namespace ct

extern "C" int ct_strided_downscale(const void *src_dev, void *dst_dev, int32_t elem_bytes, int64_t n_planes, int64_t h,
                                    int64_t w, int32_t pixel_elems, int32_t step, void *stream)
{
    using namespace ct;
    if (step < 1 || pixel_elems < 1 || (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4)) return CT_ERR_INVALID_ARGUMENT;
    if (n_planes < 0 || h < 0 || w < 0) return CT_ERR_INVALID_ARGUMENT;
    if (n_planes == 0 || h == 0 || w == 0) return CT_OK;
    if (!src_dev || !dst_dev || reinterpret_cast<uintptr_t>(src_dev) % elem_bytes != 0 ||
        reinterpret_cast<uintptr_t>(dst_dev) % elem_bytes != 0)
        return CT_ERR_INVALID_ARGUMENT;
    // rows are counted and elements of a row are indexed with 32 bits; a row takes at most 65535 * 256 slots
    constexpr int64_t kMax = 0x7fffffff;
    if (h > kMax || w > kMax || n_planes > kMax || w * pixel_elems > kMax || n_planes * h > kMax) return CT_ERR_TOO_LARGE;
    const int64_t ho = (h + step - 1) / step, wo = (w + step - 1) / step;
    const int elems_per_packet = 16 / elem_bytes;
    if (wo * pixel_elems / elems_per_packet + 2 > (int64_t)65535 * kBlock) return CT_ERR_TOO_LARGE;
    DownscaleArgs a;
    a.src = static_cast<const unsigned char *>(src_dev);
    a.dst = static_cast<unsigned char *>(dst_dev);
    a.src_bytes = n_planes * h * w * pixel_elems * elem_bytes;
    a.rows = (uint32_t)(n_planes * ho);
    a.h = (uint32_t)h;
    a.ho = (uint32_t)ho;
    a.row_in = (uint32_t)(w * pixel_elems);
    a.row_out = (uint32_t)(wo * pixel_elems);
    a.pe = (uint32_t)pixel_elems;
    a.step = (uint32_t)step;
    // slots of one row a workgroup covers: the power of two that holds a row's groups, at most the whole workgroup
    const bool wide = (pixel_elems == 1 || pixel_elems == 3) && step >= 2 && step <= 4;
    const int64_t group = (int64_t)elems_per_packet * (wide ? pixel_elems : 1);
    const int64_t slots = 1 + (a.row_out + group - 1) / group;
    a.slot_bits = 0;
    while (a.slot_bits < 8 && ((int64_t)1 << a.slot_bits) < slots) ++a.slot_bits;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (elem_bytes == 1)
        dispatch_downscale<1>(a, s);
    else if (elem_bytes == 2)
        dispatch_downscale<2>(a, s);
    else
        dispatch_downscale<4>(a, s);
    return hipGetLastError() == hipSuccess ? CT_OK : CT_ERR_LAUNCH;
}
