// ct_linearize_ingest.hip -- a recognised gpu_transforms chain and the ICRF linearization in ONE pass (gfx950): raw codes /
// pixels in, planar float32 (lin, std) out.  The outputs are bit for bit those of ct_ingest_transform (ct_ingest.hip)
// followed by ct_linearize_std (ct_linearize.hip) on its float32 result -- the same two device functions run here on a
// value that never leaves the registers: ct::ingest_stages (ct_ingest_stages.hpp) and linearize_sample (ct_device.hpp:
// icrf_sample<INTERP, true, false> -- RANGED = false, the clamp mask, the reference-order CATMULL derivative -- then
// std = |f'(x) * sigma|), with the sqrtf of the rounded square behind a wave-uniform branch where the square underflows
// (linearization.py:106,132; li_sample4 of ct_linearize_ingest.hpp).
//
// Roofline: HBM, sizeof(T) bytes read and 4 or 8 written per sample (+ 4 read with explicit uncertainties), every byte
// once: 10 B per uint16 sample where the two launches move 18.
//
// Ownership is that of the ingest kernels, the LUT is staged in LDS by stage_lut<INTERP> as in ct_linearize.hip:
// PLANAR (any C): a workgroup row (blockIdx.y) is one plane of one frame, so the channel -- the clamp pair, the LOOKUP
//   row -- is wave-uniform.  A thread owns 4 consecutive output elements whose stores are one 16-byte aligned packet in
//   lin_out and in std_out, and fetches their inputs with one 4 / 8 / 16-byte load of any alignment.  The LINEAR / CATMULL
//   row is the reference's flat NCHW index modulo C (base.py:173-176): one modulo for the first element, an add and a
//   conditional subtract for the next three.  It depends on the position, so the stack is never passed as one plane.
// PACKED3 (interleaved (F,H,W,3), RGB or BGR): a workgroup row is one frame.  A thread owns 4 pixels: it reads their 12
//   elements with dense loads, regroups in registers and writes one packet per plane and output.  The pixel count in front
//   of the first group aligns plane 0; the other planes are aligned with it iff H*W is a multiple of 4, else their
//   packets are stored element by element.  BGR is a wave-uniform output plane index (2 - memory channel), not a variant.
// A workgroup walks kSlots slots per thread, a workgroup apart, so one staging of the LUT serves kSlots * 1024 elements.
// What precedes the first aligned packet of a plane (slot 0) and what follows the last whole one goes element by element.
// Every load is that of an element of the thread's own pixels, every store lies in the thread's own [p0, p0 + n).  The
// stage list travels by value in the kernel arguments; the stage loop is wave-uniform.  No atomics.
//
// ct_linearize_ingest_data: the chain may hold one CT_INGEST_AFFINE_DATA stage -- a data-dependent Normalize -- whose sub
// and div are PER FRAME: consts[4 f], consts[4 f + 1] as ct_ingest_extrema_frames left them.  The frame of a workgroup row
// is known before the slot loop (planar: (first + blockIdx.y) / channels; interleaved: first + blockIdx.y), so the two
// floats are one wave-uniform load per workgroup and the select against the stage's own constants is scalar.  The kernels
// are the same instantiations (as in ct_merge_ingest_kernel.hpp): a NULL consts is the constant chain.
#include "ct_linearize_ingest.hpp"

namespace ct {

template <typename T, int INTERP, int STD, bool WRITE_STD, bool FLAT>
__global__ __launch_bounds__(kBlock) void linearize_ingest_planar_kernel(const flat_args_t<LinIngestArgs, FLAT> a)
{
    extern __shared__ __align__(16) char lds[];
    const int C = (int)a.channels, L = (int)a.n_points;
    stage_lut<INTERP>(lds, a.lut, C, L);
    __syncthreads();
    const uint32_t q = a.first + blockIdx.y;  // plane of the (F, C, plane) outputs
    const uint32_t f = q / a.channels, c = q - f * a.channels;
    const T *src = static_cast<const T *>(a.src) + (int64_t)f * a.image_stride + (int64_t)c * a.plane;
    float *lin = a.lin_out + (int64_t)q * a.plane;
    [[maybe_unused]] float *sdo = WRITE_STD ? a.std_out + (int64_t)q * a.plane : nullptr;
    [[maybe_unused]] const float *sdi = STD == CT_STD_EXPLICIT ? a.std_in + (int64_t)q * a.plane : nullptr;
    const int64_t head = (int64_t)(((0 - reinterpret_cast<uintptr_t>(lin)) & 15u) / sizeof(float));
    const uint32_t row0 = c * a.plane_global + a.base;  // global flat index of this plane's first local element (< 2^31)
    const float dsub = a.consts ? a.consts[4 * (int64_t)f] : 0.0f, ddiv = a.consts ? a.consts[4 * (int64_t)f + 1] : 1.0f;
    // FLAT: this plane of the flat field, of its uncertainty (or NULL) and its mean -- wave-uniform
    [[maybe_unused]] const float *fl = nullptr, *fls = nullptr;
    [[maybe_unused]] float M = 0.0f;
    if constexpr (FLAT) {
        fl = a.ff.flat + (int64_t)c * a.plane;
        fls = a.ff.flat_std ? a.ff.flat_std + (int64_t)c * a.plane : nullptr;
        M = a.ff.mean[c];
    }
#pragma unroll 1
    for (int k = 0; k < kLiSlots; ++k) {
        const int64_t slot = ((int64_t)blockIdx.x * kLiSlots + k) * kBlock + threadIdx.x;
        int64_t p0;
        int n;
        if (!li_span(head, slot, a.plane, p0, n)) continue;
        float v[kLiGroup], sg[kLiGroup] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (n == kLiGroup) {
            T in[kLiGroup];
            __builtin_memcpy(in, src + p0, sizeof(in));
#pragma unroll
            for (int e = 0; e < kLiGroup; ++e) v[e] = (float)in[e];
        } else {
#pragma unroll
            for (int e = 0; e < kLiGroup; ++e) v[e] = e < n ? (float)src[p0 + e] : 0.0f;
        }
        if constexpr (STD == CT_STD_EXPLICIT) li_load_std(sdi + p0, n, sg);
        ingest_stages<true>(v, a, a.by_channel ? c : 0u, dsub, ddiv);
        const uint32_t qg = row0 + (uint32_t)p0;
        const int r = C == 3 ? (int)(qg % 3u) : (int)(qg % a.channels);
        LinIngestPacket lo, so;
        li_sample4<INTERP, STD, WRITE_STD>(v, sg, lds, L, C, (int)c, r, a.std_value, lo, so);
        if constexpr (FLAT) li_flat4(lo, so, fl, fls, p0, n, M);
        li_store(lin + p0, lo, n);
        if constexpr (WRITE_STD) li_store(sdo + p0, so, n);
    }
}

template <typename T, int INTERP, int STD, bool WRITE_STD, bool FLAT>
__global__ __launch_bounds__(kBlock) void linearize_ingest_packed3_kernel(const flat_args_t<LinIngestArgs, FLAT> a)
{
    extern __shared__ __align__(16) char lds[];
    constexpr int C = 3;
    const int L = (int)a.n_points;
    stage_lut<INTERP>(lds, a.lut, C, L);
    __syncthreads();
    const uint32_t f = a.first + blockIdx.y;
    const T *src = static_cast<const T *>(a.src) + (int64_t)f * a.image_stride;
    float *lin = a.lin_out + (int64_t)f * C * a.plane;
    [[maybe_unused]] float *sdo = WRITE_STD ? a.std_out + (int64_t)f * C * a.plane : nullptr;
    [[maybe_unused]] const float *sdi = STD == CT_STD_EXPLICIT ? a.std_in + (int64_t)f * C * a.plane : nullptr;
    const int64_t head = (int64_t)(((0 - reinterpret_cast<uintptr_t>(lin)) & 15u) / sizeof(float));
    const uint32_t pg3 = a.plane_global % 3u;
    const float dsub = a.consts ? a.consts[4 * (int64_t)f] : 0.0f, ddiv = a.consts ? a.consts[4 * (int64_t)f + 1] : 1.0f;
#pragma unroll 1
    for (int k = 0; k < kLiSlots; ++k) {
        const int64_t slot = ((int64_t)blockIdx.x * kLiSlots + k) * kBlock + threadIdx.x;
        int64_t p0;
        int n;
        if (!li_span(head, slot, a.plane, p0, n)) continue;
        T in[kLiGroup * C];
        if (n == kLiGroup) {
            __builtin_memcpy(in, src + p0 * C, sizeof(in));
        } else {
#pragma unroll
            for (int e = 0; e < kLiGroup * C; ++e) in[e] = e < n * C ? src[p0 * C + e] : (T)0;
        }
        const uint32_t m3 = (a.base + (uint32_t)p0) % 3u;
#pragma unroll
        for (int cm = 0; cm < C; ++cm) {
            const uint32_t c = a.reversed ? (uint32_t)(C - 1 - cm) : (uint32_t)cm;  // plane of the outputs (wave-uniform)
            float v[kLiGroup], sg[kLiGroup] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int e = 0; e < kLiGroup; ++e) v[e] = (float)in[e * C + cm];
            const int64_t po = (int64_t)c * a.plane + p0;
            if constexpr (STD == CT_STD_EXPLICIT) li_load_std(sdi + po, n, sg);
            ingest_stages<true>(v, a, a.by_channel ? c : 0u, dsub, ddiv);
            // row of (plane c, pixel p0): (c * plane_global + base + p0) % 3 (base.py:173-176)
            const int r = (int)((c * pg3 + m3) % 3u);
            LinIngestPacket lo, so;
            li_sample4<INTERP, STD, WRITE_STD>(v, sg, lds, L, C, (int)c, r, a.std_value, lo, so);
            if constexpr (FLAT) li_flat4(lo, so, a.ff.flat, a.ff.flat_std, po, n, a.ff.mean[c]);  // (C, plane): po of plane 0
            li_store(lin + po, lo, n);
            if constexpr (WRITE_STD) li_store(sdo + po, so, n);
        }
    }
}

template <typename T, int INTERP, int STD, bool WRITE_STD>
struct LinIngestLaunch {
    static int run(const LinIngestArgs &a, bool packed, int64_t rows, hipStream_t s)
    {
        return li_launch_rows(packed ? linearize_ingest_packed3_kernel<T, INTERP, STD, WRITE_STD, false>
                                     : linearize_ingest_planar_kernel<T, INTERP, STD, WRITE_STD, false>,
                              a, INTERP, rows, s);
    }
    // the flat-field epilogue always writes a std (li_flat_ok): no kernel without one
    static int run(const WithFlat<LinIngestArgs> &a, bool packed, int64_t rows, hipStream_t s)
    {
        if constexpr (WRITE_STD)
            return li_launch_rows(packed ? linearize_ingest_packed3_kernel<T, INTERP, STD, true, true>
                                         : linearize_ingest_planar_kernel<T, INTERP, STD, true, true>,
                                  a, INTERP, rows, s);
        return CT_ERR_INVALID_ARGUMENT;
    }
};

// consts_dev NULL: the constant chains of ct_linearize_ingest (no AFFINE_DATA stage); else ct_linearize_ingest_data.
// ff NULL: no flat field; else ct_linearize_ingest_flat
static int linearize_ingest(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                            const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode, float std_value,
                            const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev, const float *consts_dev, void *stream,
                            const LinFlat *ff = nullptr)
{
    // everything that needs no pointer into device memory first: geometry (check_ingest_geometry, no empty plane), then the
    // stack, the stage list, the model and the uncertainty mode (li_check_call)
    if (!geom || !icrf) return CT_ERR_INVALID_ARGUMENT;
    int rc = check_ingest_geometry(geom, false);
    if (rc != CT_OK) return rc;
    if (!stride_holds_image(geom)) return CT_ERR_INVALID_ARGUMENT;
    bool by_channel = false;
    int64_t rows = 0;
    rc = li_check_call(dtype, n_frames, geom, geom->h_tile * geom->width, stages, n_stages, std_dev, std_mode, icrf, consts_dev,
                       by_channel, rows);
    if (rc != CT_OK) return rc;
    if (n_frames == 0) return CT_OK;
    if (!li_pointers_ok(frames_dev, dtype, std_dev, lin_out_dev, std_out_dev)) return CT_ERR_INVALID_ARGUMENT;
    if (ff && !li_flat_ok(*ff, std_out_dev)) return CT_ERR_INVALID_ARGUMENT;
    WithFlat<LinIngestArgs> a = {};
    a.src = frames_dev;
    a.std_in = std_mode == CT_STD_EXPLICIT ? std_dev : nullptr;
    a.lut = icrf->lut_dev;
    a.consts = consts_dev;
    a.lin_out = lin_out_dev;
    a.std_out = std_out_dev;
    fill_ingest_args(a, geom, icrf_points(icrf), by_channel, stages, n_stages);
    a.std_value = std_value;
    const bool packed = geom->layout != CT_LAYOUT_NCHW;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!ff) return li_dispatch<LinIngestLaunch>(static_cast<const LinIngestArgs &>(a), dtype, packed, rows, icrf->interp, std_mode, std_out_dev != nullptr, s);
    a.ff = *ff;
    return li_dispatch<LinIngestLaunch>(a, dtype, packed, rows, icrf->interp, std_mode, true, s);
}

}  // namespace ct

extern "C" int ct_linearize_ingest_flat(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                                        const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                                        float std_value, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev,
                                        const float *consts_dev, const float *flat_dev, const float *flat_std_dev,
                                        const float *flat_mean_dev, void *stream)
{
    const ct::LinFlat ff = {flat_dev, flat_std_dev, flat_mean_dev};
    return ct::linearize_ingest(frames_dev, dtype, n_frames, geom, stages, n_stages, std_dev, std_mode, std_value, icrf, lin_out_dev,
                                std_out_dev, consts_dev, stream, &ff);
}

extern "C" int ct_linearize_ingest(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                                   const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                                   float std_value, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev, void *stream)
{
    return ct::linearize_ingest(frames_dev, dtype, n_frames, geom, stages, n_stages, std_dev, std_mode, std_value, icrf, lin_out_dev,
                                std_out_dev, nullptr, stream);
}

extern "C" int ct_linearize_ingest_data(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                                        const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                                        float std_value, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev,
                                        const float *consts_dev, void *stream)
{
    return ct::linearize_ingest(frames_dev, dtype, n_frames, geom, stages, n_stages, std_dev, std_mode, std_value, icrf, lin_out_dev,
                                std_out_dev, consts_dev, stream);
}
