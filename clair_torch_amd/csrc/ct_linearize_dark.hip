// ct_linearize_dark.hip -- the dark-field conditional blur and the ICRF linearization of F independent frames in ONE pass
// over the raw frames (gfx950).  For every frame the outputs are bit for bit those of ct_dark_field_blur (ct_darkfield.hip)
// on it as a batch of one with its own matched dark field, into float32 xb and sigma_eff, followed by ct_linearize_std
// (ct_linearize.hip) on (xb, CT_DTYPE_F32, std = sigma_eff, CT_STD_EXPLICIT): the blur is dark_blur_kernel's expressions in
// its operation order on values that never leave the registers, and the sample step is li_sample4<INTERP, CT_STD_EXPLICIT,
// true> of ct_linearize_ingest.hpp (linearize_sample with RANGED = false and its wave-uniform `tiny` fix-up), the step
// ct_linearize.hip runs on float32 pixels with explicit uncertainties.
//
// The window and the blur are those of md_run (ct_merge_dark.hip), from ct_dark_window.hpp; tests/test_gpu_linearize_dark.py
// and test_gpu_merge_dark.py hold each kernel to the pair of launches bit for bit.
//
// Roofline: HBM.  Per sample sizeof(T) bytes of the frame (its neighbours in the 3 x 3 window are L1 / L2 hits: the rows
// above and below belong to the wavefronts next door), 4 of the dark field and 4 of its std (+ 4 with explicit image
// uncertainties), 8 written.  The pair moves sizeof(T) + 8 (+ 4) read and 8 written by the blur, then 8 read and 8 written by
// the linearization: a uint16 frame with derived uncertainties costs 18 B per sample where the pair moves 34, and the two
// float32 stacks of a group never exist.  (Byte counts from the shapes; see profiles/linearize_dark.md for what was timed.)
//
// Ownership: the walk of ct_linearize_dark_launch.hpp with one (frame, channel) plane per workgroup row.  A thread's 4
// columns cost 3 x (1 + 4 + 1) window loads (the column left of the group or the reflected one, the group, the column right
// of it).  The frames and the dark fields are read only.
#include "ct_linearize_dark_launch.hpp"

namespace ct {

struct LinDarkArgs {
    const void *frames;      // (F, C, H, W) T, image_stride between frames
    const float *std_in;     // explicit sigma of the raw image, laid out like the frames, or NULL
    const float *lut;
    float *lin_out;          // (F, C, H, W) dense
    float *std_out;
    const float *dark[CT_LINEARIZE_DARK_MAX_FRAMES];      // (C, H, W) each, one per frame of this launch
    const float *dark_std[CT_LINEARIZE_DARK_MAX_FRAMES];
    int64_t image_stride;
    uint32_t plane;          // H * W
    uint32_t width, h_tile;
    uint32_t channels, n_points;
    NormConst norm;
    int32_t std_mode;        // of the RAW image: how sigma enters sigma_eff
    float std_value, threshold, alpha;
    float k0, k1;            // the two distinct taps of the normalised 1-D kernel: k0 (centre), k1 (sides)
};

// xb and sigma_eff of columns w0 .. w0 + G - 1 of row h of plane c0 of the frame at `frame` (its dark field: dark, dark_std;
// its explicit sigma: sigma or NULL): the window of ct_dark_window.hpp for one frame that is the whole image (no halo).
template <typename T, int G>
__device__ __forceinline__ void ld_blur(const LinDarkArgs &a, const T *frame, const float *sigma, const float *dark,
                                        const float *dark_std, uint32_t c0, uint32_t h, uint32_t w0, float *xb, float *sig)
{
    const uint32_t q = c0 * a.plane + h * a.width + w0;  // first element inside the (C, H, W) frame
    const DarkRows<T> rw = dark_rows<T, G, false>(a, frame + (int64_t)c0 * a.plane, c0, h, w0);
    const bool explicit_sigma = a.std_mode == CT_STD_EXPLICIT;
    DarkRaw<T, G> raw{};
    dark_load<T, G, true>(raw, rw, 0, 0, dark, dark_std, 0, explicit_sigma, sigma, q);
    dark_blur<T, G, true>(a, raw, explicit_sigma, xb, sig);
}

template <typename T, int INTERP>
__global__ __launch_bounds__(kBlock) void linearize_dark_kernel(const LinDarkArgs a)
{
    extern __shared__ __align__(16) char lds[];
    const int C = (int)a.channels, L = (int)a.n_points;
    stage_lut<INTERP>(lds, a.lut, C, L);
    __syncthreads();
    const uint32_t f = blockIdx.y / a.channels, c0 = blockIdx.y - f * a.channels;  // frame of this launch, channel
    const T *frame = static_cast<const T *>(a.frames) + (int64_t)f * a.image_stride;
    const float *sigma = a.std_in ? a.std_in + (int64_t)f * a.image_stride : nullptr;
    const float *dark = a.dark[f], *dark_std = a.dark_std[f];
    const int64_t out0 = (int64_t)f * C * a.plane;  // the frame inside the dense outputs
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
            ld_blur<T, kLdGroup>(a, frame, sigma, dark, dark_std, c0, h, w0, xb, sig);
        } else {
            // the end of a row whose width is no multiple of the group (at most kLdGroup - 1 elements): one lane, one element
            // after the other, each with its own window
            n = (int)(W - w0);
#pragma unroll
            for (int e = 0; e < kLdGroup - 1; ++e)
                if (e < n) ld_blur<T, 1>(a, frame, sigma, dark, dark_std, c0, h, w0 + e, &xb[e], &sig[e]);
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

}  // namespace ct

extern "C" int ct_linearize_dark(const void *frames_dev, int32_t dtype, float max_code, int64_t n_frames, const ct_geometry *geom,
                                 const float *std_dev, int32_t std_mode, float std_value, const float *const *dark_devs,
                                 const float *const *dark_std_devs, float threshold, float alpha, const ct_icrf *icrf,
                                 float *lin_out_dev, float *std_out_dev, void *stream)
{
    using namespace ct;
    if (!ld_pointers_present(frames_dev, geom, dark_devs, dark_std_devs, lin_out_dev, std_out_dev, n_frames)) return CT_ERR_INVALID_ARGUMENT;
    if (int rc = ld_check_geometry(geom, std_mode, std_dev)) return rc;
    NormConst norm;
    if (norm_for_dtype(dtype, max_code, &norm) != CT_OK) return CT_ERR_UNSUPPORTED;
    // ---- what ct_linearize_std refuses for (xb, sigma_eff): float32 pixels with explicit uncertainties ----
    if (!icrf || !icrf_ok(icrf)) return CT_ERR_INVALID_ARGUMENT;
    const int interp = icrf->interp;
    // linearization.py:100-105: uncertainties are always propagated here, and LOOKUP has no gradient path (li_check_call)
    if (interp == CT_INTERP_LOOKUP) return CT_ERR_NO_GRADIENT_PATH;
    if (!global_below_2_31(geom)) return CT_ERR_TOO_LARGE;
    const int n_points = icrf_points(icrf);
    if (lut_lds_bytes(interp, geom->channels, n_points) > kLdsBudget) return CT_ERR_TOO_LARGE;
    const int64_t per_launch = ld_frames_per_launch(geom->channels);  // a workgroup row is one (frame, channel) plane
    if (per_launch < 1) return CT_ERR_TOO_LARGE;
    if (!aligned(frames_dev, dtype_bytes(dtype)) || !aligned(std_dev, sizeof(float)) || !aligned(lin_out_dev, sizeof(float)) ||
        !aligned(std_out_dev, sizeof(float)) || !ld_darks_aligned(dark_devs, dark_std_devs, n_frames))
        return CT_ERR_INVALID_ARGUMENT;

    LinDarkArgs a{};
    ld_fill_args(a, icrf, geom, n_points, norm, std_mode, std_value, threshold, alpha);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the explicit sigma is laid out like the frames.  (LOOKUP: refused above, no kernel)
    return ld_launch_frames(a, frames_dev, dtype, std_mode == CT_STD_EXPLICIT ? std_dev : nullptr, geom->image_stride, lin_out_dev,
                            std_out_dev, dark_devs, dark_std_devs, n_frames, per_launch, [&](auto t, LinDarkArgs &b, int64_t, int nf) {
                                return with_enum<CT_INTERP_LINEAR, CT_INTERP_CATMULL, CT_INTERP_NONE>(interp, [&](auto I) {
                                    return ld_launch(linearize_dark_kernel<decltype(t), I>, b, I, (uint32_t)nf * b.channels, s);
                                });
                            });
}
