// ct_linearize_dark_ingest.hip -- a recognised gpu_transforms chain, the dark-field conditional blur and the ICRF linearization of
// F independent RAW frames in ONE pass (gfx950).  For every frame the outputs are bit for bit those of ct_ingest_transform
// (ct_ingest.hip) on it into a planar float32 stack x, ct_dark_field_blur (ct_darkfield.hip) on x as a batch of one with its
// own matched dark field into xb and sigma_eff, and ct_linearize_std (ct_linearize.hip) on (xb, CT_DTYPE_F32, std = sigma_eff,
// CT_STD_EXPLICIT): the same device functions run here on values that never leave the registers.  The 9 taps of a sample's
// window go through ct::ingest_stages<false> (ct_ingest_stages.hpp) with the tap's PLANE channel, the blur is dark_blur_staged
// (ct_dark_window.hpp: dark_blur_kernel's expressions in its order, on floats), the sample step is li_sample4<INTERP,
// CT_STD_EXPLICIT, true> (ct_linearize_ingest.hpp).  float32 throughout, every operation rounded on its own
// (-ffp-contract=off).  tests/test_gpu_linearize_dark_ingest.py holds the kernels to the three launches bit for bit.
//
// Roofline: HBM.  Per sample sizeof(T) bytes of the frame (window neighbours are L1 / L2 hits), 4 of the dark field and 4 of
// its std (+ 4 with explicit image uncertainties), 8 written: 18 B per uint16 sample with derived uncertainties (22 explicit)
// where the three launches move 2 + 4, then 4 + 8 + 8, then 8 + 8 = 42 (46), and the three float32 stacks of a group never
// exist.  (Byte counts from the shapes; what was timed: profiles/linearize_dark_ingest.md.)
//
// Ownership: the slot walk of ct_linearize_dark_launch.hpp.  The stage list travels in the argument block like the frames'
// dark-field pointers; the stage loop is wave-uniform.
// PLANAR (CT_LAYOUT_NCHW, any C): a workgroup row (blockIdx.y) is one (frame, channel) plane, so the clamp pair is
//   wave-uniform; 3 x (1 + 4 + 1) window loads per thread.
// PACKED3 (CT_LAYOUT_NHWC / NHWC_BGR, raw (F, H, W, 3) frames): a workgroup row is one frame.  A thread owns 4 consecutive
//   PIXELS of one image row with all 3 channels: on each of the three rows the 12 contiguous elements of its pixels and the
//   3 of the pixel left and of the pixel right of them (or the reflected ones) -- neighbours of a sample lie 3 elements apart
//   in a row and 3 * W apart between rows.  It regroups in registers and writes one packet per plane and output, so the frame
//   is read once; memory channel cm feeds plane 2 - cm with BGR (a wave-uniform index, not a variant).  This is the only
//   interleaved walk built: three stride-3 walks, one per plane, would read every frame three times through the caches and
//   were neither built nor timed.
// The dark field, its std and explicit image uncertainties are planar (C, H, W) float32 in plane (RGB) order whatever the
// layout of the frames; frames, dark fields and uncertainties are read only.  No LOOKUP (no gradient path: refused, no
// kernel).
//
// ct_linearize_dark_ingest_data: the chain may hold one CT_INGEST_AFFINE_DATA stage -- a data-dependent Normalize -- whose sub
// and div are PER FRAME: consts[4 f], consts[4 f + 1] as ct_ingest_extrema_frames left them and as ct_linearize_ingest_data reads
// them.  The frame of a workgroup row is known before the slot loop (blockIdx.y), so the two floats are one wave-uniform load per
// workgroup row; ingest_stages<true> takes them for all 9 taps of a window -- a reflected border tap is an element of the same
// frame.  The walks are the same templates with DATA = true (18 more kernels, their block the constant chains' with the pointer
// behind it); the DATA = false instantiations are the kernels of ct_linearize_dark_ingest, instruction for instruction
// (profiles/linearize_dark_ingest_data.md), and a call whose chain has no such stage launches those whether or not it brought
// constants.  ct_linearize_dark_ingest itself still refuses the kind.  Per uint16 sample the extrema pass adds 2 B to the 18.
//
// Resources (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; scratch is 0 bytes for all 36 kernels),
// VGPRs for LINEAR / CATMULL / no LUT:
//   planar   uint8, uint16, float32: 73 / 73 / 71 each (6 to 7 wavefronts per SIMD); DATA the same
//   packed3  uint8 111 / 111 / 109, uint16 115 / 115 / 114 (4 wavefronts per SIMD), float32 148 / 148 / 147 (3);
//            DATA the same but uint16 116 / 116 / 114 (4 wavefronts per SIMD still)
// Measured on 16 x 3 x 1080 x 1920 (profiles/linearize_dark_ingest.md): 0.55 to 0.63 of the time of the three launches, 2.8 to
// 3.5 TB/s of the bytes counted above; the packed3 walk's occupancy is the first thing to look at for more.  DATA, with the
// extrema pass in front (profiles/linearize_dark_ingest_data.md): 0.48 to 0.55 of the time of the four launches, 3.1 to 3.8 TB/s.
#include "ct_linearize_dark_launch.hpp"

namespace ct {

struct LinDarkIngestArgs {
    const void *frames;      // (F, C, H, W) or (F, H, W, 3) T, image_stride between frames
    const float *std_in;     // explicit sigma of the raw image: planar (F, C, H, W) float32, dense, or NULL
    const float *lut;
    float *lin_out;          // (F, C, H, W) dense
    float *std_out;
    const float *dark[CT_LINEARIZE_DARK_MAX_FRAMES];      // (C, H, W) each, one per frame of this launch
    const float *dark_std[CT_LINEARIZE_DARK_MAX_FRAMES];
    int64_t image_stride;
    uint32_t plane;          // H * W
    uint32_t width, h_tile;
    uint32_t channels, n_points;
    uint32_t reversed;       // PACKED3: memory channel cm feeds plane 2 - cm (BGR)
    uint32_t by_channel;     // some clamp holds different pairs for different channels; else every channel takes pair 0
    NormConst norm;          // (fill_blur_args; the chain stands where the code normalisation would)
    int32_t std_mode;        // of the image behind the chain: how sigma enters sigma_eff
    float std_value, threshold, alpha;
    float k0, k1;            // the two distinct taps of the normalised 1-D kernel: k0 (centre), k1 (sides)
    uint32_t n_stages;
    ct_ingest_stage stage[CT_INGEST_MAX_STAGES];
};

// The argument block of the DATA instantiations: the constants pointer appended BEHIND the block, so every member keeps its
// offset, and in a derived block (as WithFlat of ct_linearize_ingest.hpp), so the constant-chain instantiations take their own
// block unchanged -- a member more in it moves the hidden arguments behind the block, one s_load_dword offset in 12 of them
struct LinDarkIngestDataArgs : LinDarkIngestArgs {
    const float *consts;     // (frames of this launch, 4) per-frame {sub, div, min, max} of the CT_INGEST_AFFINE_DATA stage
};
template <bool DATA>
using ldi_args_t = std::conditional_t<DATA, LinDarkIngestDataArgs, LinDarkIngestArgs>;

// PLANAR: xb and sigma_eff of columns w0 .. w0 + G - 1 of row h of plane c0 of the frame at `frame` (its dark field: dark,
// dark_std; its explicit sigma: sigma or NULL, planar like the dark field)
template <typename T, int G, bool DATA>
__device__ __forceinline__ void ldi_planar(const LinDarkIngestArgs &a, const T *frame, const float *sigma, const float *dark,
                                           const float *dark_std, uint32_t c0, uint32_t h, uint32_t w0, float dsub, float ddiv,
                                           float *xb, float *sig)
{
    constexpr int N = G + 2;
    const uint32_t q = c0 * a.plane + h * a.width + w0;  // first element inside the (C, H, W) frame
    const DarkRows<T> rw = dark_rows<T, G, false>(a, frame + (int64_t)c0 * a.plane, c0, h, w0);
    const bool explicit_sigma = a.std_mode == CT_STD_EXPLICIT;
    DarkRaw<T, G> raw{};
    dark_load<T, G, true>(raw, rw, 0, 0, dark, dark_std, 0, explicit_sigma, sigma, q);
    float v[3 * N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        v[j] = (float)raw.up[j];
        v[N + j] = (float)raw.mid[j];
        v[2 * N + j] = (float)raw.dn[j];
    }
    ingest_stages<DATA>(v, a, a.by_channel ? c0 : 0u, dsub, ddiv);  // all 9 taps: reflected ones are the frame's own
    dark_blur_staged<G, true>(a, v, v + N, v + 2 * N, raw.d, raw.ds, raw.sg, explicit_sigma, xb, sig);
}

template <typename T, int INTERP, bool DATA>
__global__ __launch_bounds__(kBlock) void linearize_dark_ingest_planar_kernel(const ldi_args_t<DATA> a)
{
    extern __shared__ __align__(16) char lds[];
    const int C = (int)a.channels, L = (int)a.n_points;
    stage_lut<INTERP>(lds, a.lut, C, L);
    __syncthreads();
    const uint32_t f = blockIdx.y / a.channels, c0 = blockIdx.y - f * a.channels;  // frame of this launch, channel
    const T *frame = static_cast<const T *>(a.frames) + (int64_t)f * a.image_stride;
    const int64_t out0 = (int64_t)f * C * a.plane;  // the frame inside the dense planar arrays
    const float *sigma = a.std_in ? a.std_in + out0 : nullptr;
    const float *dark = a.dark[f], *dark_std = a.dark_std[f];
    // DATA: the frame's pair, one wave-uniform load per workgroup row (f comes from blockIdx.y)
    [[maybe_unused]] float dsub = 0.0f, ddiv = 1.0f;
    if constexpr (DATA) {
        dsub = a.consts[4 * (int64_t)f];
        ddiv = a.consts[4 * (int64_t)f + 1];
    }
    const uint32_t W = a.width;
    const uint32_t gpr = ld_groups_per_row(W);
    const uint64_t n_slots = (uint64_t)gpr * a.h_tile;
#pragma unroll 1
    for (int k = 0; k < kLdSlots; ++k) {
        const uint64_t slot = ((uint64_t)blockIdx.x * kLdSlots + k) * kBlock + threadIdx.x;
        if (slot >= n_slots) break;
        const uint32_t h = (uint32_t)(slot / gpr);
        const uint32_t w0 = ((uint32_t)slot - h * gpr) * kLdGroup;
        float xb[kLdGroup] = {0.0f, 0.0f, 0.0f, 0.0f}, sig[kLdGroup] = {0.0f, 0.0f, 0.0f, 0.0f};
        int n = kLdGroup;
        if (W - w0 >= (uint32_t)kLdGroup) {
            ldi_planar<T, kLdGroup, DATA>(a, frame, sigma, dark, dark_std, c0, h, w0, dsub, ddiv, xb, sig);
        } else {
            // the end of a row whose width is no multiple of the group (at most kLdGroup - 1 elements): one lane, one element
            // after the other, each with its own window
            n = (int)(W - w0);
#pragma unroll
            for (int e = 0; e < kLdGroup - 1; ++e)
                if (e < n) ldi_planar<T, 1, DATA>(a, frame, sigma, dark, dark_std, c0, h, w0 + e, dsub, ddiv, &xb[e], &sig[e]);
        }
        // the frame is batch element 0 of its own batch: the LINEAR / CATMULL row is the flat (C, H, W) index modulo C
        const uint32_t q = c0 * a.plane + h * W + w0;
        const int r = C == 3 ? (int)(q % 3u) : (int)(q % a.channels);
        LinIngestPacket lo, so;
        li_sample4<INTERP, CT_STD_EXPLICIT, true>(xb, sig, lds, L, C, (int)c0, r, 0.0f, lo, so);
        li_store(a.lin_out + out0 + q, lo, n);
        li_store(a.std_out + out0 + q, so, n);
    }
}

// PACKED3: xb and sigma_eff of pixels w0 .. w0 + G - 1 of row h of the interleaved frame at `frame`, all 3 channels, into
// elements E0 .. E0 + G - 1 of xb[cm] / sig[cm] (cm: the MEMORY channel; its plane is 2 - cm with a.reversed)
template <typename T, int G, int E0, bool DATA>
__device__ __forceinline__ void ldi_packed3(const LinDarkIngestArgs &a, const T *frame, const float *sigma, const float *dark,
                                            const float *dark_std, uint32_t h, uint32_t w0, float dsub, float ddiv,
                                            float (&xb)[3][kLdGroup], float (&sig)[3][kLdGroup])
{
    constexpr int C = 3, N = G + 2;
    const uint32_t W = a.width, H = a.h_tile;
    // rows and column taps with reflect padding (index -1 -> 1, H -> H - 2, W -> W - 2)
    const uint32_t hu = h > 0 ? h - 1 : 1, hd = h + 1 < H ? h + 1 : H - 2;
    const uint32_t cl = w0 > 0 ? w0 - 1 : 1, cr = w0 + G < W ? w0 + G : W - 2;
    T raw[3][N * C];  // rows h - 1, h, h + 1: pixels {left, w0 .. w0 + G - 1, right}, 3 elements each
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T *row = frame + (int64_t)(k == 0 ? hu : (k == 1 ? h : hd)) * W * C;
        __builtin_memcpy(&raw[k][0], row + (int64_t)cl * C, C * sizeof(T));  // any alignment: rows are only element-aligned
        __builtin_memcpy(&raw[k][C], row + (int64_t)w0 * C, G * C * sizeof(T));
        __builtin_memcpy(&raw[k][(G + 1) * C], row + (int64_t)cr * C, C * sizeof(T));
    }
    const bool explicit_sigma = a.std_mode == CT_STD_EXPLICIT;
#pragma unroll
    for (int cm = 0; cm < C; ++cm) {
        const uint32_t c = a.reversed ? (uint32_t)(C - 1 - cm) : (uint32_t)cm;  // plane (wave-uniform)
        const uint32_t q = c * a.plane + h * W + w0;                           // first element inside the planar (C, H, W) arrays
        float v[3 * N];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) v[k * N + j] = (float)raw[k][j * C + cm];
        ingest_stages<DATA>(v, a, a.by_channel ? c : 0u, dsub, ddiv);
        float d[G], ds[G], sg[G];
        __builtin_memcpy(d, dark + q, sizeof(d));
        __builtin_memcpy(ds, dark_std + q, sizeof(ds));
#pragma unroll
        for (int e = 0; e < G; ++e) sg[e] = 0.0f;
        if (explicit_sigma) __builtin_memcpy(sg, sigma + q, sizeof(sg));
        dark_blur_staged<G, true>(a, v, v + N, v + 2 * N, d, ds, sg, explicit_sigma, &xb[cm][E0], &sig[cm][E0]);
    }
}

template <typename T, int INTERP, bool DATA>
__global__ __launch_bounds__(kBlock) void linearize_dark_ingest_packed3_kernel(const ldi_args_t<DATA> a)
{
    extern __shared__ __align__(16) char lds[];
    constexpr int C = 3;
    const int L = (int)a.n_points;
    stage_lut<INTERP>(lds, a.lut, C, L);
    __syncthreads();
    const uint32_t f = blockIdx.y;  // frame of this launch
    const T *frame = static_cast<const T *>(a.frames) + (int64_t)f * a.image_stride;
    const int64_t out0 = (int64_t)f * C * a.plane;
    const float *sigma = a.std_in ? a.std_in + out0 : nullptr;
    const float *dark = a.dark[f], *dark_std = a.dark_std[f];
    [[maybe_unused]] float dsub = 0.0f, ddiv = 1.0f;  // DATA: the frame's pair, as in the planar kernel
    if constexpr (DATA) {
        dsub = a.consts[4 * (int64_t)f];
        ddiv = a.consts[4 * (int64_t)f + 1];
    }
    const uint32_t W = a.width;
    const uint32_t gpr = ld_groups_per_row(W);
    const uint64_t n_slots = (uint64_t)gpr * a.h_tile;
#pragma unroll 1
    for (int k = 0; k < kLdSlots; ++k) {
        const uint64_t slot = ((uint64_t)blockIdx.x * kLdSlots + k) * kBlock + threadIdx.x;
        if (slot >= n_slots) break;
        const uint32_t h = (uint32_t)(slot / gpr);
        const uint32_t w0 = ((uint32_t)slot - h * gpr) * kLdGroup;
        float xb[C][kLdGroup] = {}, sig[C][kLdGroup] = {};
        int n = kLdGroup;
        if (W - w0 >= (uint32_t)kLdGroup) {
            ldi_packed3<T, kLdGroup, 0, DATA>(a, frame, sigma, dark, dark_std, h, w0, dsub, ddiv, xb, sig);
        } else {
            // the end of a row whose width is no multiple of the group (1 to 3 pixels): one pixel after the other
            n = (int)(W - w0);
            ldi_packed3<T, 1, 0, DATA>(a, frame, sigma, dark, dark_std, h, w0, dsub, ddiv, xb, sig);
            if (n > 1) ldi_packed3<T, 1, 1, DATA>(a, frame, sigma, dark, dark_std, h, w0 + 1, dsub, ddiv, xb, sig);
            if (n > 2) ldi_packed3<T, 1, 2, DATA>(a, frame, sigma, dark, dark_std, h, w0 + 2, dsub, ddiv, xb, sig);
        }
#pragma unroll
        for (int cm = 0; cm < C; ++cm) {
            const uint32_t c = a.reversed ? (uint32_t)(C - 1 - cm) : (uint32_t)cm;
            const uint32_t q = c * a.plane + h * W + w0;
            LinIngestPacket lo, so;
            li_sample4<INTERP, CT_STD_EXPLICIT, true>(xb[cm], sig[cm], lds, L, C, (int)c, (int)(q % 3u), 0.0f, lo, so);
            li_store(a.lin_out + out0 + q, lo, n);
            li_store(a.std_out + out0 + q, so, n);
        }
    }
}

template <typename T, int INTERP, bool DATA>
static int ldi_launch(const ldi_args_t<DATA> &a, bool packed, int n_frames, hipStream_t s)
{
    if (packed) return ld_launch(linearize_dark_ingest_packed3_kernel<T, INTERP, DATA>, a, INTERP, (uint32_t)n_frames, s);
    return ld_launch(linearize_dark_ingest_planar_kernel<T, INTERP, DATA>, a, INTERP, (uint32_t)n_frames * a.channels, s);
}

// consts_dev NULL: the constant chains of ct_linearize_dark_ingest (no AFFINE_DATA stage); else ct_linearize_dark_ingest_data
static int linearize_dark_ingest(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                                 const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode, float std_value,
                                 const float *const *dark_devs, const float *const *dark_std_devs, float threshold, float alpha,
                                 const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev, const float *consts_dev, void *stream)
{
    // ---- what ct_linearize_dark refuses first: pointers, the frame count, a dark field per frame ----
    if (!ld_pointers_present(frames_dev, geom, dark_devs, dark_std_devs, lin_out_dev, std_out_dev, n_frames)) return CT_ERR_INVALID_ARGUMENT;
    // ---- the dark geometry, of the planar image the chain yields (the layout of the raw frames is the stage list's matter) ----
    ct_geometry planar = *geom;
    planar.layout = CT_LAYOUT_NCHW;
    if (int rc = ld_check_geometry(&planar, std_mode, std_dev)) return rc;
    // ---- the stack and the stage list: one AFFINE_DATA stage at most, and only with constants (li_check_call's rule) ----
    bool by_channel = false;
    if (int rc = ingest_validate(dtype, geom->layout, n_frames, geom->channels, geom->h_tile * geom->width, stages, n_stages,
                                 CT_INGEST_MAX_STAGES, consts_dev ? 1 : 0, by_channel))
        return rc;
    if (!aligned(consts_dev, sizeof(float))) return CT_ERR_INVALID_ARGUMENT;
    // constants without a data stage are not read: the constant chain's kernels
    bool data = false;
    for (int32_t k = 0; k < n_stages; ++k) data |= stages[k].kind == CT_INGEST_AFFINE_DATA;
    // ---- the model: float32 pixels with explicit uncertainties, as ct_linearize_std sees (xb, sigma_eff) ----
    if (!icrf || !icrf_ok(icrf)) return CT_ERR_INVALID_ARGUMENT;
    const int interp = icrf->interp;
    if (interp == CT_INTERP_LOOKUP) return CT_ERR_NO_GRADIENT_PATH;  // linearization.py:100-105
    const int n_points = icrf_points(icrf);
    if (lut_lds_bytes(interp, geom->channels, n_points) > kLdsBudget) return CT_ERR_TOO_LARGE;
    if (!global_below_2_31(geom)) return CT_ERR_TOO_LARGE;
    const bool packed = geom->layout != CT_LAYOUT_NCHW;
    const int64_t per_launch = ld_frames_per_launch(packed ? 1 : geom->channels);  // a workgroup row: a frame, or one of its planes
    if (per_launch < 1) return CT_ERR_TOO_LARGE;
    if (!li_pointers_ok(frames_dev, dtype, std_dev, lin_out_dev, std_out_dev) || !ld_darks_aligned(dark_devs, dark_std_devs, n_frames))
        return CT_ERR_INVALID_ARGUMENT;

    LinDarkIngestDataArgs a{};
    ld_fill_args(a, icrf, geom, n_points, NormConst{1.0f, 0.0f}, std_mode, std_value, threshold, alpha);
    a.reversed = geom->layout == CT_LAYOUT_NHWC_BGR ? 1u : 0u;
    a.by_channel = by_channel ? 1u : 0u;
    a.n_stages = (uint32_t)n_stages;
    for (int32_t k = 0; k < n_stages; ++k) a.stage[k] = stages[k];
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the explicit sigma is dense and planar, like the outputs.  (LOOKUP: refused above, no kernel).  b.consts: the DATA
    // instantiations, with the launch's rows of the constants
    return ld_launch_frames(a, frames_dev, dtype, std_mode == CT_STD_EXPLICIT ? std_dev : nullptr, geom->channels * (int64_t)a.plane,
                            lin_out_dev, std_out_dev, dark_devs, dark_std_devs, n_frames, per_launch,
                            [&](auto t, LinDarkIngestDataArgs &b, int64_t first, int nf) {
                                using T = decltype(t);
                                b.consts = data ? consts_dev + 4 * first : nullptr;
                                return with_enum<CT_INTERP_LINEAR, CT_INTERP_CATMULL, CT_INTERP_NONE>(interp, [&](auto I) {
                                    return b.consts ? ldi_launch<T, I, true>(b, packed, nf, s) : ldi_launch<T, I, false>(b, packed, nf, s);
                                });
                            });
}

}  // namespace ct

extern "C" int ct_linearize_dark_ingest(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                                        const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                                        float std_value, const float *const *dark_devs, const float *const *dark_std_devs,
                                        float threshold, float alpha, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev,
                                        void *stream)
{
    return ct::linearize_dark_ingest(frames_dev, dtype, n_frames, geom, stages, n_stages, std_dev, std_mode, std_value, dark_devs,
                                     dark_std_devs, threshold, alpha, icrf, lin_out_dev, std_out_dev, nullptr, stream);
}

extern "C" int ct_linearize_dark_ingest_data(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                                             const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                                             float std_value, const float *const *dark_devs, const float *const *dark_std_devs,
                                             float threshold, float alpha, const ct_icrf *icrf, float *lin_out_dev,
                                             float *std_out_dev, const float *consts_dev, void *stream)
{
    return ct::linearize_dark_ingest(frames_dev, dtype, n_frames, geom, stages, n_stages, std_dev, std_mode, std_value, dark_devs,
                                     dark_std_devs, threshold, alpha, icrf, lin_out_dev, std_out_dev, consts_dev, stream);
}
