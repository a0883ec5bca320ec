// ct_stats.hip -- streaming per-pixel mean and variance of video frames, gfx950.
//
// Replaces the loop body of compute_video_mean_and_std (clair_torch/inference/inferential_statistics.py:38-47):
// optional ICRF linearization of a batch of frames, then WBOMeanVar.update_values(frames, None)
// (clair_torch/common/statistics.py:213-259): batch mean, batch m2 = sum (x - mean_b)^2 and the pairwise merge
//   M = M_A + M_B + (W_A W_B / W)(mean_B - mean_A)^2,   mean = mean_A + (W_B / W)(mean_B - mean_A),   W = W_A + W_B
// with unit weights (W_B = batch size), all in float32 like the reference's float32 frames.
//
// One thread owns V consecutive elements.  The centred second moment needs the batch mean first, so the batch is
// walked twice -- out of registers when the batch has at most 32 frames (video_stats_cached_kernel: every frame is
// loaded and linearized exactly once, all loads in flight together), out of memory otherwise (video_stats_kernel).
// Both form the sums in the reference's order, so they agree bit for bit.  HBM-bound.
//
// Interleaved (F, H, W, C) frames as OpenCV decodes them (IL instantiations): a thread still owns V consecutive MEMORY
// elements -- the frame loads stay packets -- and only the LUT row and the position in the planar (C, H, W) state follow
// from TileMap::planar_index; the state is touched element by element, once per batch of frames.
//
// Host: stats_prepare is everything ct_video_stats_batch refuses and its argument block; dispatch, BMAX pick, launch and the
// walk over the batch list of ct_video_stats_batches are ct_stats_kernel.hpp's (stats_dispatch, with_stats_bmax,
// stats_launch_grid, stats_batches), shared with ct_stats_multi.hip and the two ingest files.
#include "ct_stats_kernel.hpp"

namespace ct {

template <typename T, int V, int INTERP, bool IL>
__global__ __launch_bounds__(kBlock) void video_stats_kernel(const StatsArgs a)
{
    extern __shared__ __align__(16) char lds[];
    constexpr bool kRanged = sizeof(T) != 4;
    const int C = a.channels, L = a.n_points, B = a.batch;
    stage_lut<INTERP>(lds, a.lut, C, L);
    __syncthreads();
    const uint32_t vec = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (vec * (uint32_t)V >= a.q_count) return;
    const uint32_t q0 = a.q_begin + vec * (uint32_t)V;
    const float top = INTERP == CT_INTERP_NONE ? 1.0f : (float)(L - 1);
    int row_off[V];
    uint32_t pq[V];  // position in the planar state (== q0 + e unless the frames are interleaved)
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const StatsOwn own = stats_own<INTERP, IL>(a.tile, q0 + e, C, L);
        pq[e] = own.pq;
        row_off[e] = own.row_off;
    }
    const T *src = static_cast<const T *>(a.frames) + q0;
    float sum[V], m2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) sum[e] = m2[e] = 0.0f;
    for (int n = 0; n < B; ++n) {
        const SPacket<T, V> pk = *reinterpret_cast<const SPacket<T, V> *>(src + (int64_t)n * a.image_stride);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float d;
            sum[e] += icrf_sample<INTERP, true, kRanged>(to_pixel<T>(pk.v[e], a.norm), lds + row_off[e], top, d);
        }
    }
    float mean_b[V];
#pragma unroll
    for (int e = 0; e < V; ++e) mean_b[e] = sum[e] / (float)B;  // torch.mean: float32 sum / count
    for (int n = 0; n < B; ++n) {
        const SPacket<T, V> pk = *reinterpret_cast<const SPacket<T, V> *>(src + (int64_t)n * a.image_stride);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float d;
            const float x = icrf_sample<INTERP, true, kRanged>(to_pixel<T>(pk.v[e], a.norm), lds + row_off[e], top, d);
            const float dv = x - mean_b[e];
            m2[e] += dv * dv;
        }
    }
    merge_state<V, IL>(a, q0, pq, mean_b, m2);
}

// Batch of at most BMAX frames: the linearized values stay in registers between the mean and the m2 pass.
template <typename T, int V, int INTERP, int BMAX, bool IL>
__global__ __launch_bounds__(kBlock) void video_stats_cached_kernel(const StatsArgs a)
{
    extern __shared__ __align__(16) char lds[];
    constexpr bool kRanged = sizeof(T) != 4;
    const int C = a.channels, L = a.n_points, B = a.batch;
    stage_lut<INTERP>(lds, a.lut, C, L);
    __syncthreads();
    const uint32_t vec = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (vec * (uint32_t)V >= a.q_count) return;
    const uint32_t q0 = a.q_begin + vec * (uint32_t)V;
    const float top = INTERP == CT_INTERP_NONE ? 1.0f : (float)(L - 1);
    int row_off[V];
    uint32_t pq[V];  // position in the planar state (== q0 + e unless the frames are interleaved)
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const StatsOwn own = stats_own<INTERP, IL>(a.tile, q0 + e, C, L);
        pq[e] = own.pq;
        row_off[e] = own.row_off;
    }
    const T *src = static_cast<const T *>(a.frames) + q0;
    SPacket<T, V> raw[BMAX];
#pragma unroll
    for (int n = 0; n < BMAX; ++n)
        if (n < B) raw[n] = *reinterpret_cast<const SPacket<T, V> *>(src + (int64_t)n * a.image_stride);
    float xs[BMAX][V], sum[V], m2[V], mean_b[V];
#pragma unroll
    for (int e = 0; e < V; ++e) sum[e] = m2[e] = 0.0f;
#pragma unroll
    for (int n = 0; n < BMAX; ++n) {
        if (n < B) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float d;
                xs[n][e] = icrf_sample<INTERP, true, kRanged>(to_pixel<T>(raw[n].v[e], a.norm), lds + row_off[e], top, d);
                sum[e] += xs[n][e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) mean_b[e] = sum[e] / (float)B;  // torch.mean: float32 sum / count
#pragma unroll
    for (int n = 0; n < BMAX; ++n) {
        if (n < B) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float dv = xs[n][e] - mean_b[e];
                m2[e] += dv * dv;
            }
        }
    }
    merge_state<V, IL>(a, q0, pq, mean_b, m2);
}

}  // namespace ct

extern "C" int ct_norm_constants(float max_code, float *hi, float *lo);

namespace ct {

// Everything ct_video_stats_batch refuses, in its order, and its argument block.  in_list: the batch is one of
// ct_video_stats_batches', where a size of 0 is a batch to skip (nothing of it is dereferenced, so neither its frames nor the
// state need to be there) and the LUT is tested against the LDS here, before any launch of the call.
static int stats_prepare(const void *frames_dev, int32_t dtype, float max_code, int32_t batch, const ct_geometry *geom,
                         const ct_icrf *icrf, float frames_before, float *mean_state_dev, float *m2_state_dev, bool in_list, StatsArgs &a)
{
    const bool skipped = in_list && batch == 0;
    if (!geom || !icrf || (!skipped && (!frames_dev || !mean_state_dev || !m2_state_dev || batch <= 0)) || frames_before < 0.0f)
        return CT_ERR_INVALID_ARGUMENT;
    if (!shape_positive(geom) || !band_fits(geom) || !icrf_ok(icrf)) return CT_ERR_INVALID_ARGUMENT;
    if (!global_below_2_31(geom)) return CT_ERR_TOO_LARGE;
    if (!stride_holds_image(geom) || !layout_ok(geom)) return CT_ERR_INVALID_ARGUMENT;
    a = StatsArgs{};
    a.frames = frames_dev;
    a.lut = icrf->lut_dev;
    a.mean_state = mean_state_dev;
    a.m2_state = m2_state_dev;
    a.image_stride = geom->image_stride;
    a.tile = make_tile(geom);  // frames planar or interleaved; the state is always planar (C, H, W)
    a.batch = batch;
    a.channels = geom->channels;
    a.n_points = icrf_points(icrf);
    a.count_before = frames_before;
    if (dtype == CT_DTYPE_U8 || dtype == CT_DTYPE_U16) {
        if (ct_norm_constants(max_code, &a.norm.hi, &a.norm.lo) != CT_OK) return CT_ERR_UNSUPPORTED;
    } else if (dtype != CT_DTYPE_F32) {
        return CT_ERR_UNSUPPORTED;
    }
    if (in_list && lut_lds_bytes(icrf->interp, a.channels, a.n_points) > kLdsBudget) return CT_ERR_TOO_LARGE;
    return CT_OK;
}

// The launches of one batch: dtype / V / interp / layout by ct::stats_dispatch, then the walk that takes a.batch frames.
static int stats_run(const StatsArgs &a, int32_t dtype, const ct_geometry *geom, int interp, hipStream_t s)
{
    return stats_dispatch(a, &a.frames, 1, dtype, (uint32_t)local_elements(geom), interp, [&](const StatsArgs &part, auto t, auto V, auto I, auto IL) {
        using T = decltype(t);
        return with_stats_bmax<true>(part.batch, [&](auto BMAX) {
            if constexpr (BMAX == 0)
                return stats_launch_grid(video_stats_kernel<T, V, I, IL>, stats_grid<V>(part), I, s, part);
            else
                return stats_launch_grid(video_stats_cached_kernel<T, V, I, BMAX, IL>, stats_grid<V>(part), I, s, part);
        });
    });
}

}  // namespace ct

extern "C" int ct_video_stats_batch(const void *frames_dev, int32_t dtype, float max_code, int32_t batch,
                                    const ct_geometry *geom, const ct_icrf *icrf, float frames_before,
                                    float *mean_state_dev, float *m2_state_dev, void *stream)
{
    using namespace ct;
    StatsArgs a;
    if (const int rc = stats_prepare(frames_dev, dtype, max_code, batch, geom, icrf, frames_before, mean_state_dev, m2_state_dev, false, a);
        rc != CT_OK)
        return rc;
    return stats_run(a, dtype, geom, icrf->interp, static_cast<hipStream_t>(stream));
}

// Several consecutive batches: ONE launch of the MULTI kernels (ct_stats_multi.hip) where every batch fits a register-cached
// walk; otherwise one launch per batch with the state in memory, exactly what the caller would have done.
extern "C" int ct_video_stats_batches(const void *const *frames_devs, const int32_t *batch_sizes, int32_t n_batches, int32_t dtype,
                                      float max_code, const ct_geometry *geom, const ct_icrf *icrf, float frames_before,
                                      float *mean_state_dev, float *m2_state_dev, uint32_t flags, void *stream)
{
    using namespace ct;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return stats_batches(
        frames_devs, nullptr, batch_sizes, n_batches, frames_before, flags, false,
        [&](int b, float count) {
            StatsArgs a;
            return stats_prepare(frames_devs[b], dtype, max_code, batch_sizes[b], geom, icrf, count, mean_state_dev, m2_state_dev, true, a);
        },
        [&](const StatsBatches &mb, bool cached) {
            if (!cached) return kStatsPerBatch;
            StatsArgs first;  // (judged above: the block of the first batch with frames)
            stats_prepare(mb.frames[0], dtype, max_code, mb.batch[0], geom, icrf, mb.count_before[0], mean_state_dev, m2_state_dev, true, first);
            return stats_multi(first, mb, dtype, (uint32_t)local_elements(geom), icrf->interp, s);
        },
        [&](const void *frames, const float *, int32_t batch, float count) {
            return ct_video_stats_batch(frames, dtype, max_code, batch, geom, icrf, count, mean_state_dev, m2_state_dev, stream);
        });
}
