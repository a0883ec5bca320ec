// ct_stats_ingest.hip -- a recognised gpu_transforms chain and one batch of compute_video_mean_and_std's loop body in ONE
// pass (gfx950): B raw uint8 / uint16 frames in, the float32 planar (C, H, W) WBOMeanVar state (mean, m2) updated in place.
// The state is bit for bit that of ct_ingest_transform (or _data, ct_ingest.hip) into a dense planar float32 stack followed
// by ct_video_stats_batch (ct_stats.hip) on that stack -- the same device functions run here on a value that never leaves
// the registers: (float)code, ct::ingest_stages (ct_ingest_stages.hpp), icrf_sample<INTERP, true, false> (ct_device.hpp;
// RANGED = false: the second launch of the pair sees float32 pixels), then the sums in ct_stats.hip's order -- float32
// sum / B, sum (x - mean_b)^2 over the frames in order -- and ct::merge_state (ct_stats_merge.hpp, the one copy).
//
// Roofline: HBM.  sizeof(T) bytes read per sample, every byte once while B <= 32, plus 16 B of state per element and batch:
// 2 B per uint16 sample where the two launches move 10 (2 read + 4 written, then 4 read), 1 B against 9 for uint8.
//
// Both walks of ct_stats.hip are kept.  B <= 16 and B <= 32 are register-cached (BMAX = 16 / 32): all B loads of a thread
// are in flight together, every frame is loaded and the chain evaluated exactly once, the B values per element stay in
// registers between the mean and the m2 pass.  B > 32 (BMAX = 0) walks the frames twice and evaluates the chain in both
// passes: the same values again, so the result does not depend on the walk.
//
// Ownership.  The LUT is staged in LDS by stage_lut<INTERP> as in ct_stats.hip; the stage list travels by value in the
// kernel arguments and its loop is wave-uniform, as is the channel that selects a clamp pair and the LOOKUP row:
// PLANAR (any C): a workgroup row (blockIdx.y) is one channel plane.  G = 4: a thread owns 4 consecutive elements of the
//   plane whose state accesses are one 16-byte aligned packet each in mean and m2 (the host launches this only where the two
//   arrays are equally aligned), and fetches their codes with one 4- or 8-byte load of any alignment per frame.  What
//   precedes a plane's first aligned packet and what follows its last whole one -- at most 3 elements each -- goes to a
//   second launch of the G = 1 instantiation: the vector body plus scalar tail of ct_stats.hip, per plane.  The LINEAR /
//   CATMULL row is the reference's flat NCHW index modulo C (base.py:173-176) taken from the global position
//   c * H_global * W + row_offset * W + p: one modulo for the first element, an add and a conditional subtract for the rest.
// PACKED3 (interleaved (F, H, W, 3), RGB or BGR): a thread owns whole pixels, ONE of them (G = 1): consecutive memory
//   elements belong to different channels and ingest_stages takes one channel per call, so the three elements of a pixel
//   make three calls with a compile-time memory channel; BGR is a wave-uniform plane index (2 - memory channel), not a
//   variant.  Its 3 codes are one 3- / 6-byte load per frame, its state accesses one element per plane, dense across the
//   wavefront.  One pixel and not the four of linearize_ingest_packed3_kernel: the cached walk holds BMAX values per
//   element, and 12 elements x 32 frames do not fit the register file (the listing: DESIGN.md).  Calling ingest_stages
//   per element of a 4-element memory packet instead would make the clamp pair a per-lane choice inside the frame loop.
// Every load is that of a code of the thread's own elements (pixels) in one of the B frames, every store lies in the
// thread's own elements of mean_state and m2_state.  The consts of a CT_INGEST_AFFINE_DATA stage are read once per thread,
// before anything is stored.  No atomics, no LDS traffic besides the LUT, the frames are read only.
//
// Host: si_validate and si_pointers_ok are what the entry points refuse; dispatch, BMAX pick, launch and the walk over the
// batch list of ct_video_stats_ingest_batches are ct_stats_kernel.hpp's (si_dispatch, with_stats_bmax, stats_launch_grid,
// stats_batches), shared with the other three files.
#include "ct_ingest_stages.hpp"
#include "ct_stats_kernel.hpp"

namespace ct {

// One thread: G consecutive elements of every plane it owns, the whole batch and the state.  (Location, load, sample and walk
// stand in the kernel itself, here and in ct_stats_ingest_multi.hip: the thread's location as a function returning a struct
// changed the assembly of 128 of the 240 kernels of the two files, load_raw and sample as functions that of 180 -- no
// scratch, other instruction order and registers.  profiles/stats_refactor_ab.md.)
template <typename T, bool PACKED, int G, int INTERP, int BMAX, bool DATA>
__global__ __launch_bounds__(kBlock) void video_stats_ingest_kernel(const StatsIngestArgs a)
{
    extern __shared__ __align__(16) char lds[];
    static_assert(PACKED ? G == 1 : (G == 1 || G == kSiGroup), "one pixel, or one element / one packet of a plane");
    stage_lut<INTERP>(lds, a.lut, a.channels, a.n_points);
    // the constants of a data-dependent Normalize: one wave-uniform load, before anything is stored
    const float dsub = DATA ? a.consts[0] : 0.0f, ddiv = DATA ? a.consts[1] : 1.0f;
    __syncthreads();
    const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    uint32_t c0 = 0u, p0;  // plane (PLANAR) and first local pixel
    if constexpr (PACKED) {
        if (t >= a.plane) return;
        p0 = t;
    } else {
        c0 = blockIdx.y;
        uint32_t head, body_end;
        si_body(a, c0, head, body_end);
        if constexpr (G == kSiGroup) {
            const uint64_t at = (uint64_t)head + (uint64_t)t * kSiGroup;
            if (at >= body_end) return;
            p0 = (uint32_t)at;
        } else {  // the edges: [0, head) and [body_end, plane)
            const uint64_t at = t < head ? (uint64_t)t : (uint64_t)body_end + (t - head);
            if (at >= a.plane) return;
            p0 = (uint32_t)at;
        }
    }

    constexpr int NP = PACKED ? 3 : 1;  // planes per thread
    constexpr int NE = NP * G;
    constexpr int kEntry = lut_entry_bytes(INTERP);
    const int C = a.channels, L = a.n_points, B = a.batch;
    const float top = INTERP == CT_INTERP_NONE ? 1.0f : (float)(L - 1);

    uint32_t cj[NP];  // plane of the state (wave-uniform)
    uint32_t q[NP];   // index of the first element in the planar (C, plane) state
    int row_off[NE];  // byte offset of each element's LUT row inside the LDS table
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        cj[j] = PACKED ? (a.reversed ? (uint32_t)(NP - 1 - j) : (uint32_t)j) : c0;
        q[j] = cj[j] * a.plane + p0;
        // TileMap::locate's q_global for a channel that is known: the global flat NCHW index (< 2^31)
        const uint32_t qg = cj[j] * a.plane_global + a.base + p0;
        int r = lut_row<INTERP>(qg, (int)cj[j], PACKED ? 3 : C);  // (a constant divisor where the frames are interleaved)
#pragma unroll
        for (int e = 0; e < G; ++e) {
            row_off[j * G + e] = r * L * kEntry;
            if constexpr (INTERP != CT_INTERP_LOOKUP) {  // the next element's flat index is one further
                ++r;
                r = r >= C ? r - C : r;
            }
        }
    }
    const T *src = static_cast<const T *>(a.frames) + (PACKED ? (int64_t)p0 * NP : (int64_t)c0 * a.plane + p0);

    auto load_raw = [&](int n) __attribute__((always_inline)) {
        SiRaw<T, NE> r;
        __builtin_memcpy(&r, src + (int64_t)n * a.image_stride, sizeof(r));  // any alignment: frames are only element-aligned
        return r;
    };
    // the thread's NE samples of one frame: the chain, then the model
    auto sample = [&](const SiRaw<T, NE> &raw, float (&out)[NE]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            float x[G];
#pragma unroll
            for (int e = 0; e < G; ++e) x[e] = (float)raw.v[e * NP + j];
            ingest_stages<DATA>(x, a, a.by_channel ? cj[j] : 0u, dsub, ddiv);
#pragma unroll
            for (int e = 0; e < G; ++e) {
                float d;
                out[j * G + e] = icrf_sample<INTERP, true, false>(x[e], lds + row_off[j * G + e], top, d);
            }
        }
    };

    float sum[NE], m2[NE], mean_b[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) sum[k] = m2[k] = 0.0f;
    if constexpr (BMAX > 0) {  // the values stay in registers between the mean and the m2 pass
        SiRaw<T, NE> raw[BMAX];
#pragma unroll
        for (int n = 0; n < BMAX; ++n)
            if (n < B) raw[n] = load_raw(n);
        float xs[BMAX][NE];
#pragma unroll
        for (int n = 0; n < BMAX; ++n) {
            if (n < B) {
                sample(raw[n], xs[n]);
#pragma unroll
                for (int k = 0; k < NE; ++k) sum[k] += xs[n][k];
            }
        }
#pragma unroll
        for (int k = 0; k < NE; ++k) mean_b[k] = sum[k] / (float)B;  // torch.mean: float32 sum / count
#pragma unroll
        for (int n = 0; n < BMAX; ++n) {
            if (n < B) {
#pragma unroll
                for (int k = 0; k < NE; ++k) {
                    const float dv = xs[n][k] - mean_b[k];
                    m2[k] += dv * dv;
                }
            }
        }
    } else {
#pragma unroll 4
        for (int n = 0; n < B; ++n) {
            float x[NE];
            sample(load_raw(n), x);
#pragma unroll
            for (int k = 0; k < NE; ++k) sum[k] += x[k];
        }
#pragma unroll
        for (int k = 0; k < NE; ++k) mean_b[k] = sum[k] / (float)B;  // torch.mean: float32 sum / count
#pragma unroll 4
        for (int n = 0; n < B; ++n) {
            float x[NE];
            sample(load_raw(n), x);
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                const float dv = x[k] - mean_b[k];
                m2[k] += dv * dv;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        float mb[G], mm[G];
        uint32_t unused[G] = {};  // (the interleaved form of merge_state is not used: the state is addressed per plane)
#pragma unroll
        for (int e = 0; e < G; ++e) {
            mb[e] = mean_b[j * G + e];
            mm[e] = m2[j * G + e];
        }
        merge_state<G, false>(a, q[j], unused, mb, mm);
    }
}


// The launches of one batch: dtype / interp / layout / constants by ct::si_dispatch, then the walk that takes a.batch frames.
static int si_run(const StatsIngestArgs &a, int dtype, bool packed, int interp, hipStream_t s)
{
    return si_dispatch(a, dtype, packed, interp, [&](const StatsIngestArgs &part, dim3 grid, auto t, auto P, auto G, auto I, auto DATA) {
        return with_stats_bmax<true>(part.batch, [&](auto BMAX) {
            return stats_launch_grid(video_stats_ingest_kernel<decltype(t), P, G, I, BMAX, DATA>, grid, I, s, part);
        });
    });
}

// What ct_video_stats_ingest_batch refuses without looking at a pointer into device memory, in its order: geometry (an empty
// plane allowed), the stack and the stage list of 8-bit / 16-bit codes, the model (check_code_ingest, which
// ct_hdr_merge_ingest_batch shares), the count, the stride, the LDS and the grid.
static int si_validate(int32_t dtype, int32_t batch, const ct_geometry *geom, const ct_ingest_stage *stages, int32_t n_stages,
                       const float *consts_dev, const ct_icrf *icrf, float frames_before, bool &by_channel)
{
    if (const int rc = check_code_ingest(dtype, batch, geom, stages, n_stages, consts_dev, icrf, by_channel); rc != CT_OK) return rc;
    if (!(frames_before >= 0.0f) || !stride_holds_image(geom)) return CT_ERR_INVALID_ARGUMENT;
    if (lut_lds_bytes(icrf->interp, geom->channels, icrf->n_points) > kLdsBudget) return CT_ERR_TOO_LARGE;
    if (geom->layout == CT_LAYOUT_NCHW && geom->channels > 65535) return CT_ERR_TOO_LARGE;  // a plane is a row of the grid
    return CT_OK;
}

// the pointers of a batch that has something to do: present and aligned to their element
static bool si_pointers_ok(const void *frames_dev, int32_t dtype, const float *mean_state_dev, const float *m2_state_dev)
{
    if (!frames_dev || !mean_state_dev || !m2_state_dev) return false;
    return aligned(frames_dev, dtype == CT_DTYPE_U16 ? 2 : 1) && aligned(mean_state_dev, sizeof(float)) && aligned(m2_state_dev, sizeof(float));
}

}  // namespace ct

extern "C" int ct_video_stats_ingest_batch(const void *frames_dev, int32_t dtype, int32_t batch, const ct_geometry *geom,
                                           const ct_ingest_stage *stages, int32_t n_stages, const float *consts_dev,
                                           const ct_icrf *icrf, float frames_before, float *mean_state_dev, float *m2_state_dev,
                                           void *stream)
{
    using namespace ct;
    bool by_channel = false;
    if (const int rc = si_validate(dtype, batch, geom, stages, n_stages, consts_dev, icrf, frames_before, by_channel); rc != CT_OK) return rc;
    if (batch == 0 || geom->h_tile * geom->width == 0) return CT_OK;
    if (!si_pointers_ok(frames_dev, dtype, mean_state_dev, m2_state_dev)) return CT_ERR_INVALID_ARGUMENT;
    StatsIngestArgs a = {};
    a.frames = frames_dev;
    a.consts = consts_dev;
    a.lut = icrf->lut_dev;
    a.mean_state = mean_state_dev;
    a.m2_state = m2_state_dev;
    fill_ingest_args(a, geom, icrf_points(icrf), by_channel, stages, n_stages);
    a.batch = batch;
    a.count_before = frames_before;
    return si_run(a, dtype, geom->layout != CT_LAYOUT_NCHW, icrf->interp, static_cast<hipStream_t>(stream));
}

// Several consecutive batches behind one chain: ONE launch of the MULTI kernels (ct_stats_ingest_multi.hip) where every batch
// fits a register-cached walk and the batches agree on having constants; otherwise one launch per batch with the state in
// memory, exactly what the caller would have done.
extern "C" int ct_video_stats_ingest_batches(const void *const *frames_devs, const int32_t *batch_sizes, int32_t n_batches,
                                             int32_t dtype, const ct_geometry *geom, const ct_ingest_stage *stages,
                                             int32_t n_stages, const float *const *consts_devs, const ct_icrf *icrf,
                                             float frames_before, float *mean_state_dev, float *m2_state_dev, uint32_t flags,
                                             void *stream)
{
    using namespace ct;
    bool by_channel = false;
    return stats_batches(
        frames_devs, consts_devs, batch_sizes, n_batches, frames_before, flags, true,
        [&](int b, float count) {
            return si_validate(dtype, batch_sizes[b], geom, stages, n_stages, consts_devs ? consts_devs[b] : nullptr, icrf, count, by_channel);
        },
        [&](const StatsBatches &mb, bool cached) {
            if (geom->h_tile * geom->width == 0) return (int)CT_OK;
            int n_consts = 0;
            for (int b = 0; b < mb.n_batches; ++b) {
                if (!si_pointers_ok(mb.frames[b], dtype, mean_state_dev, m2_state_dev)) return (int)CT_ERR_INVALID_ARGUMENT;
                n_consts += mb.consts[b] ? 1 : 0;
            }
            if (!cached || (n_consts != 0 && n_consts != mb.n_batches)) return kStatsPerBatch;
            StatsIngestArgs a = {};
            a.consts = mb.consts[0];  // (only whether there are any: the kernel reads each batch's own)
            a.lut = icrf->lut_dev;
            a.mean_state = mean_state_dev;
            a.m2_state = m2_state_dev;
            fill_ingest_args(a, geom, icrf_points(icrf), by_channel, stages, n_stages);
            return stats_ingest_multi(a, mb, dtype, geom->layout != CT_LAYOUT_NCHW, icrf->interp, static_cast<hipStream_t>(stream));
        },
        [&](const void *frames, const float *consts, int32_t batch, float count) {
            return ct_video_stats_ingest_batch(frames, dtype, batch, geom, stages, n_stages, consts, icrf, count, mean_state_dev, m2_state_dev,
                                               stream);
        });
}
