// ct_linearize_ingest_strided.hip -- StridedDownscale, a recognised gpu_transforms chain and the ICRF linearization in ONE
// pass (gfx950): every step-th row and column of the raw frames in, dense planar float32 (lin, std) of shape
// (F, C, ho, wo), ho = ceil(H / step), wo = ceil(W / step), out.  Bit for bit ct_strided_downscale (ct_downscale.hip)
// followed by ct_linearize_ingest / ct_linearize_ingest_data (ct_linearize_ingest.hip) on the compacted frames: selecting
// pixels commutes with the per-sample chain, and the sample step is the same code (ct_linearize_ingest.hpp: ingest_stages,
// li_sample4 = linearize_sample of ct_device.hpp four times and the wave-uniform sqrtf branch of the `tiny` corner).
//
// Roofline: HBM.  Only every step-th source row is touched; within such a row whole 128-byte lines arrive whenever
// step * pixel_bytes is below the line size, so the floor is (selected rows at full width) + 4 or 8 bytes written per output
// sample (+ 4 read with explicit uncertainties).  The compacted copy of the two launches -- written once, read once -- is gone.
//
// Ownership is that of ct_linearize_ingest.hip in OUTPUT coordinates: a workgroup row (blockIdx.y) is one output plane
// (planar) or one frame (interleaved (F,H,W,3), RGB or BGR: three output planes); a thread owns 4 consecutive elements
// p0 .. p0 + 3 of an output plane and stores one aligned 16-byte packet per output (and, interleaved, per plane); slot 0 --
// what precedes the first aligned packet -- and the tail go element by element.  Output element p is row i = p / wo, column
// j = p % wo: one division for the first element, then (i, j) is carried, across an output-row boundary where the group
// straddles one.  Its source is row i * step, column j * step: one load per selected element (interleaved: one pixel =
// 3 elements), never a neighbour.  The LINEAR / CATMULL LUT row is the flat NCHW index OF THE DOWNSCALED FRAME modulo C,
// (c * ho * wo + p) % C (base.py:173-176 on the tensor the reference's transform list hands to the model); source
// coordinates do not enter it.  Explicit uncertainties are planar and already (F, C, ho, wo): gpu_transforms never touch them.
// Every load is that of a selected element of the thread's own pixels, every store lies in the thread's own [p0, p0 + n).
// No atomics.
//
// step == 1 is ct_linearize_ingest / _data itself, row band included (h_global, row_offset as there).  With step > 1 a
// row band is refused: which of its rows a downscale selects depends on row_offset % step, a phase that is not carried.
#include "ct_linearize_ingest.hpp"

namespace ct {

struct LinIngestStridedArgs : LinIngestArgs {  // plane, plane_global, base: of the OUTPUT (ho * wo; step 1: the row band's)
    uint32_t step;
    uint32_t wo;         // output columns
    uint32_t row_in;     // source elements per source row: W, interleaved 3 W
    uint32_t src_plane;  // planar: source elements per plane, H * W
};

template <typename T, int INTERP, int STD, bool WRITE_STD, bool PACKED, bool FLAT>
__global__ __launch_bounds__(kBlock) void linearize_ingest_strided_kernel(const flat_args_t<LinIngestStridedArgs, FLAT> a)
{
    extern __shared__ __align__(16) char lds[];
    constexpr int PE = PACKED ? 3 : 1;  // elements of a source pixel = output planes of a workgroup row
    const int C = PACKED ? 3 : (int)a.channels, L = (int)a.n_points;
    stage_lut<INTERP>(lds, a.lut, C, L);
    __syncthreads();
    const uint32_t q = a.first + blockIdx.y;  // PACKED: frame; else plane of the (F, C, plane) outputs
    const uint32_t f = PACKED ? q : q / a.channels, c0 = PACKED ? 0u : q - f * a.channels;
    const T *src = static_cast<const T *>(a.src) + (int64_t)f * a.image_stride + (int64_t)c0 * a.src_plane;
    const int64_t out0 = ((int64_t)f * C + c0) * a.plane;
    float *lin = a.lin_out + out0;
    [[maybe_unused]] float *sdo = WRITE_STD ? a.std_out + out0 : nullptr;
    [[maybe_unused]] const float *sdi = STD == CT_STD_EXPLICIT ? a.std_in + out0 : nullptr;
    const int64_t head = (int64_t)(((0 - reinterpret_cast<uintptr_t>(lin)) & 15u) / sizeof(float));
    const uint32_t row_stride = a.step * a.row_in, pixel_stride = a.step * PE;  // source elements between selected rows / pixels
    const uint32_t pg3 = a.plane_global % 3u;
    const float dsub = a.consts ? a.consts[4 * (int64_t)f] : 0.0f, ddiv = a.consts ? a.consts[4 * (int64_t)f + 1] : 1.0f;
#pragma unroll 1
    for (int k = 0; k < kLiSlots; ++k) {
        const int64_t slot = ((int64_t)blockIdx.x * kLiSlots + k) * kBlock + threadIdx.x;
        int64_t p0;
        int n;
        if (!li_span(head, slot, a.plane, p0, n)) continue;
        // source offsets of the group's pixels: (i, j) of element p0, carried over the end of an output row
        uint32_t i = (uint32_t)p0 / a.wo, j = (uint32_t)p0 - i * a.wo;
        uint32_t off[kLiGroup];
#pragma unroll
        for (int e = 0; e < kLiGroup; ++e) {
            off[e] = i * row_stride + j * pixel_stride;  // (used for e < n only: then i < ho, j < wo, inside the frame)
            if (++j == a.wo) {
                j = 0;
                ++i;
            }
        }
        T in[kLiGroup * PE];
        if (n == kLiGroup) {
#pragma unroll
            for (int e = 0; e < kLiGroup; ++e) __builtin_memcpy(in + e * PE, src + off[e], PE * sizeof(T));
        } else {
#pragma unroll
            for (int e = 0; e < kLiGroup; ++e)
#pragma unroll
                for (int cm = 0; cm < PE; ++cm) in[e * PE + cm] = e < n ? src[off[e] + cm] : (T)0;
        }
        const uint32_t m3 = (a.base + (uint32_t)p0) % 3u;
#pragma unroll
        for (int cm = 0; cm < PE; ++cm) {
            // plane of the outputs (wave-uniform); BGR: memory channel cm feeds plane 2 - cm
            const uint32_t c = PACKED ? (a.reversed ? (uint32_t)(PE - 1 - cm) : (uint32_t)cm) : c0;
            float v[kLiGroup], sg[kLiGroup] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int e = 0; e < kLiGroup; ++e) v[e] = (float)in[e * PE + cm];
            const int64_t po = (PACKED ? (int64_t)c * a.plane : 0) + p0;
            if constexpr (STD == CT_STD_EXPLICIT) li_load_std(sdi + po, n, sg);
            ingest_stages<true>(v, a, a.by_channel ? c : 0u, dsub, ddiv);
            // row of (plane c, output element p0): (c * plane_global + base + p0) % C (base.py:173-176), below 2^31
            int r;
            if constexpr (PACKED) {
                r = (int)((c * pg3 + m3) % 3u);
            } else {
                const uint32_t qg = c * a.plane_global + a.base + (uint32_t)p0;
                r = C == 3 ? (int)(qg % 3u) : (int)(qg % a.channels);
            }
            LinIngestPacket lo, so;
            li_sample4<INTERP, STD, WRITE_STD>(v, sg, lds, L, C, (int)c, r, a.std_value, lo, so);
            // the flat field is (C, plane) of the OUTPUT: element po of plane c0 (interleaved: c0 = 0, po holds the plane)
            if constexpr (FLAT) li_flat4(lo, so, a.ff.flat + (int64_t)c0 * a.plane, a.ff.flat_std ? a.ff.flat_std + (int64_t)c0 * a.plane : nullptr, po, n, a.ff.mean[c]);
            li_store(lin + po, lo, n);
            if constexpr (WRITE_STD) li_store(sdo + po, so, n);
        }
    }
}

template <typename T, int INTERP, int STD, bool WRITE_STD>
struct LinIngestStridedLaunch {
    static int run(const LinIngestStridedArgs &a, bool packed, int64_t rows, hipStream_t s)
    {
        return li_launch_rows(packed ? linearize_ingest_strided_kernel<T, INTERP, STD, WRITE_STD, true, false>
                                     : linearize_ingest_strided_kernel<T, INTERP, STD, WRITE_STD, false, false>,
                              a, INTERP, rows, s);
    }
    // the flat-field epilogue always writes a std (li_flat_ok): no kernel without one
    static int run(const WithFlat<LinIngestStridedArgs> &a, bool packed, int64_t rows, hipStream_t s)
    {
        if constexpr (WRITE_STD)
            return li_launch_rows(packed ? linearize_ingest_strided_kernel<T, INTERP, STD, true, true, true>
                                         : linearize_ingest_strided_kernel<T, INTERP, STD, true, false, true>,
                                  a, INTERP, rows, s);
        return CT_ERR_INVALID_ARGUMENT;
    }
};

// ff NULL: ct_linearize_ingest_strided; else ct_linearize_ingest_strided_flat
static int linearize_ingest_strided(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom, int32_t step,
                                    const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                                    float std_value, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev,
                                    const float *consts_dev, void *stream, const LinFlat *ff)
{
    // everything that needs no pointer into device memory first, as in ct_linearize_ingest: the step, the geometry of the
    // SOURCE frames (no empty plane), no row band behind a downscale, then li_check_call on the output plane
    if (!geom || !icrf || step < 1) return CT_ERR_INVALID_ARGUMENT;
    int rc = check_ingest_geometry(geom, false);
    if (rc != CT_OK) return rc;
    if (step > 1 && (geom->row_offset != 0 || geom->h_tile != geom->h_global)) return CT_ERR_INVALID_ARGUMENT;
    if (!stride_holds_image(geom)) return CT_ERR_INVALID_ARGUMENT;
    const int64_t ho = (geom->h_tile + step - 1) / step, wo = (geom->width + step - 1) / step;
    bool by_channel = false;
    int64_t rows = 0;
    rc = li_check_call(dtype, n_frames, geom, ho * wo, stages, n_stages, std_dev, std_mode, icrf, consts_dev, by_channel, rows);
    if (rc != CT_OK) return rc;
    if (n_frames == 0) return CT_OK;
    if (!li_pointers_ok(frames_dev, dtype, std_dev, lin_out_dev, std_out_dev)) return CT_ERR_INVALID_ARGUMENT;
    if (ff && !li_flat_ok(*ff, std_out_dev)) return CT_ERR_INVALID_ARGUMENT;
    WithFlat<LinIngestStridedArgs> a = {};
    a.src = frames_dev;
    a.std_in = std_mode == CT_STD_EXPLICIT ? std_dev : nullptr;
    a.lut = icrf->lut_dev;
    a.consts = consts_dev;
    a.lin_out = lin_out_dev;
    a.std_out = std_out_dev;
    fill_ingest_args(a, geom, icrf_points(icrf), by_channel, stages, n_stages);  // plane, plane_global, base: of step 1
    a.std_value = std_value;
    const bool packed = geom->layout != CT_LAYOUT_NCHW;
    if (step > 1) {  // untiled (checked above): the downscaled frame is the whole image
        a.plane = ho * wo;
        a.plane_global = (uint32_t)(ho * wo);
    }
    a.step = (uint32_t)step;
    a.wo = (uint32_t)wo;
    a.row_in = (uint32_t)(geom->width * (packed ? 3 : 1));
    a.src_plane = (uint32_t)(geom->h_tile * geom->width);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!ff)
        return li_dispatch<LinIngestStridedLaunch>(static_cast<const LinIngestStridedArgs &>(a), dtype, packed, rows, icrf->interp, std_mode,
                                                   std_out_dev != nullptr, s);
    a.ff = *ff;
    return li_dispatch<LinIngestStridedLaunch>(a, dtype, packed, rows, icrf->interp, std_mode, true, s);
}

}  // namespace ct

extern "C" int ct_linearize_ingest_strided(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                                           int32_t step, const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev,
                                           int32_t std_mode, float std_value, const ct_icrf *icrf, float *lin_out_dev,
                                           float *std_out_dev, const float *consts_dev, void *stream)
{
    return ct::linearize_ingest_strided(frames_dev, dtype, n_frames, geom, step, stages, n_stages, std_dev, std_mode, std_value, icrf,
                                        lin_out_dev, std_out_dev, consts_dev, stream, nullptr);
}

extern "C" int ct_linearize_ingest_strided_flat(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                                                int32_t step, const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev,
                                                int32_t std_mode, float std_value, const ct_icrf *icrf, float *lin_out_dev,
                                                float *std_out_dev, const float *consts_dev, const float *flat_dev,
                                                const float *flat_std_dev, const float *flat_mean_dev, void *stream)
{
    const ct::LinFlat ff = {flat_dev, flat_std_dev, flat_mean_dev};
    return ct::linearize_ingest_strided(frames_dev, dtype, n_frames, geom, step, stages, n_stages, std_dev, std_mode, std_value, icrf,
                                        lin_out_dev, std_out_dev, consts_dev, stream, &ff);
}
