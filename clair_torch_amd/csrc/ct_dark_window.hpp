// ct_dark_window.hpp -- device code: the 3 x 3 dark-field window of G consecutive columns of one image row, as the fused
// kernels walk it (merge_dark_kernel of ct_merge_dark.hip, linearize_dark_kernel of ct_linearize_dark.hip): where its three
// rows lie, how they are loaded, and the conditional blur with its effective uncertainty.  The blur is dark_blur_kernel's
// expressions (ct_darkfield.hip) in its operation order; that kernel keeps its own plain statement of them, and the GPU
// tests hold both fused kernels to it bit for bit.  Templated on the argument block (norm, k0, k1, threshold, alpha, std_mode,
// std_value), so every kernel keeps the layout of its own.  The blur itself works on floats (dark_blur_staged), so a kernel
// that puts something between the load and the blur -- ct_linearize_dark_ingest.hip: a gpu_transforms chain -- runs the same
// expressions.
#pragma once
#include "ct_device.hpp"

namespace ct {

// what one frame contributes to the G elements of a thread, as loaded
template <typename T, int G>
struct DarkRaw {
    T up[G + 2], mid[G + 2], dn[G + 2];  // columns {left, w0 .. w0 + G - 1, right} of the rows h - 1, h, h + 1
    float d[G], ds[G], sg[G];            // dark field, its std, the explicit sigma
};

// the three rows of the window in frame 0, what lies between two frames of the outer ones (the middle one: the image
// stride), and the columns: the group's first, and its left and right taps
template <typename T>
struct DarkRows {
    const T *up, *mid, *dn;
    int64_t up_stride, dn_stride;
    uint32_t w0, cl, cr;
};

// Local row h of plane c0, which starts at `img` in frame 0 (a.width columns, a.h_tile rows).  Each outer row is the image
// row or, at the edge, the reflected one; with BANDS, where the band does not touch the global top / bottom (a.at_top,
// a.at_bottom), the row of a.halo ((B, C, 2, W)) instead.  Without BANDS the block has no such fields and none is read.
template <typename T, int G, bool BANDS, typename Args>
__device__ __forceinline__ DarkRows<T> dark_rows(const Args &a, const T *img, uint32_t c0, uint32_t h, uint32_t w0)
{
    const uint32_t W = (uint32_t)a.width;
    DarkRows<T> rw;
    rw.mid = img + (int64_t)h * W;
    rw.up_stride = rw.dn_stride = a.image_stride;
    if (h > 0) {
        rw.up = img + (int64_t)(h - 1) * W;
    } else {
        rw.up = img + (int64_t)1 * W;  // global top: reflect -1 -> 1
        if constexpr (BANDS) {
            if (!a.at_top) {
                rw.up = static_cast<const T *>(a.halo) + ((int64_t)c0 * 2 + 0) * W;
                rw.up_stride = (int64_t)a.channels * 2 * W;
            }
        }
    }
    if (h + 1 < (uint32_t)a.h_tile) {
        rw.dn = img + (int64_t)(h + 1) * W;
    } else {
        rw.dn = img + (int64_t)(a.h_tile - 2) * W;  // global bottom: reflect H -> H - 2
        if constexpr (BANDS) {
            if (!a.at_bottom) {
                rw.dn = static_cast<const T *>(a.halo) + ((int64_t)c0 * 2 + 1) * W;
                rw.dn_stride = (int64_t)a.channels * 2 * W;
            }
        }
    }
    // column taps with reflect padding (index -1 -> 1, W -> W - 2)
    rw.w0 = w0;
    rw.cl = w0 > 0 ? w0 - 1 : 1;
    rw.cr = w0 + G < W ? w0 + G : W - 2;
    return rw;
}

template <typename T, int G>
__device__ __forceinline__ void dark_load_row(const T *row, uint32_t w0, uint32_t cl, uint32_t cr, T (&v)[G + 2])
{
    v[0] = row[cl];
    __builtin_memcpy(&v[1], row + w0, G * sizeof(T));  // any alignment: rows are only element-aligned in general
    v[G + 1] = row[cr];
}

// Frame n of the window into r (zeroed by the caller).  q: the group's first element inside a frame of the planar arrays --
// the dark field and its std, dark_stride between two frames, and the explicit sigma, laid out like the image.
template <typename T, int G, bool HAS_STD>
__device__ __forceinline__ void dark_load(DarkRaw<T, G> &r, const DarkRows<T> &rw, int64_t n, int64_t image_stride, const float *dark,
                                          const float *dark_std, int64_t dark_stride, bool explicit_sigma, const float *sigma, uint32_t q)
{
    dark_load_row<T, G>(rw.up + n * rw.up_stride, rw.w0, rw.cl, rw.cr, r.up);
    dark_load_row<T, G>(rw.mid + n * image_stride, rw.w0, rw.cl, rw.cr, r.mid);
    dark_load_row<T, G>(rw.dn + n * rw.dn_stride, rw.w0, rw.cl, rw.cr, r.dn);
    const int64_t dq = n * dark_stride + q;
    __builtin_memcpy(r.d, dark + dq, G * sizeof(float));
    if constexpr (HAS_STD) {
        __builtin_memcpy(r.ds, dark_std + dq, G * sizeof(float));
        if (explicit_sigma) __builtin_memcpy(r.sg, sigma + n * image_stride + q, G * sizeof(float));
    }
}

// xb and sigma_eff of the G elements from the window as floats -- ru, rm, rd: the G + 2 pixel values of the rows h - 1, h,
// h + 1; d, ds, sg: the dark field, its std and the explicit sigma of the G elements -- dark_blur_kernel, expression for
// expression.  The std mode of the raw image is a wave-uniform run-time branch; without a dark std (HAS_STD false) nothing is
// propagated and sig is 1.  Of the argument block only k0, k1, threshold, alpha, std_mode and std_value are read.
template <int G, bool HAS_STD, typename Args>
__device__ __forceinline__ void dark_blur_staged(const Args &a, const float *ru, const float *rm, const float *rd, const float *d,
                                                 const float *ds, const float *sgx, bool explicit_sigma, float *xb, float *sig)
{
#pragma unroll
    for (int e = 0; e < G; ++e) {
        const float bu = (a.k1 * ru[e] + a.k0 * ru[e + 1]) + a.k1 * ru[e + 2];
        const float bm = (a.k1 * rm[e] + a.k0 * rm[e + 1]) + a.k1 * rm[e + 2];
        const float bd = (a.k1 * rd[e] + a.k0 * rd[e + 1]) + a.k1 * rd[e + 2];
        const float x = rm[e + 1];
        const float blurred = (a.k1 * bu + a.k0 * bm) + a.k1 * bd;
        const float dv = d[e];
        const float m = 1.0f / (1.0f + expf(-(dv - a.threshold) * a.alpha));  // torch.sigmoid
        xb[e] = m * blurred + (1.0f - m) * x;
        sig[e] = 1.0f;
        if constexpr (HAS_STD) {
            float sg = 0.0f;
            if (explicit_sigma) sg = sgx[e];
            if (a.std_mode == CT_STD_CONSTANT) sg = a.std_value;
            if (a.std_mode == CT_STD_MULTIPLIER) sg = a.std_value * x;  // the dataset derives sigma from the RAW image
            const float dterm = (blurred - x) * (a.alpha * m * (1.0f - m));
            const float dsv = dterm * ds[e];
            sig[e] = sqrtf(sg * sg + dsv * dsv);
        }
    }
}

// ... of the window as loaded: every element to its pixel value (to_pixel with a.norm), then the blur above
template <typename T, int G, bool HAS_STD, typename Args>
__device__ __forceinline__ void dark_blur(const Args &a, const DarkRaw<T, G> &r, bool explicit_sigma, float *xb, float *sig)
{
    float ru[G + 2], rm[G + 2], rd[G + 2];
#pragma unroll
    for (int j = 0; j < G + 2; ++j) {
        ru[j] = to_pixel<T>(r.up[j], a.norm);
        rm[j] = to_pixel<T>(r.mid[j], a.norm);
        rd[j] = to_pixel<T>(r.dn[j], a.norm);
    }
    dark_blur_staged<G, HAS_STD>(a, ru, rm, rd, r.d, r.ds, r.sg, explicit_sigma, xb, sig);
}

}  // namespace ct
