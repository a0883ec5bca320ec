// ct_stats_multi.hip -- the several-batches-per-launch (MULTI) form of ct_stats.hip's register-cached kernel, behind
// ct::stats_multi (ct_video_stats_batches), gfx950.  A translation unit of its own, as ct_merge_multi.hip is for the merge:
// the instantiations compile next to ct_stats.hip's.
//
// One thread owns the V consecutive memory elements video_stats_cached_kernel gives it -- the V = 4 body and the V = 1 tail of
// ct::stats_split, planar or interleaved (IL), LUT row from the global flat index -- and owns them for EVERY batch of the
// call.  Per batch it runs that kernel's walk (all B <= BMAX loads in flight, every frame loaded and linearized once, float32
// sum / B, then sum (x - mean_b)^2 over the frames in order) inside a `#pragma unroll 1` loop over the batches, and merges
// with ct::merge_moments on registers: what a launch per batch stores and the next one reads again -- 16 B per element and
// batch -- stays in 2 * V registers.  The state arrays are read once, before batch 0 and only if frames came before it, and
// written once, after the last batch.  The count in front of every batch travels by value (StatsBatches::count_before, the
// float of the exact integer, formed on the host), so every merge_moments call sees the operands a launch of its own sees:
// the result is that of one launch per batch, bit for bit.  HBM-bound; no atomics, no LDS traffic besides the LUT.
// Host: ct::stats_multi is ct_stats.hip's dispatch and launch (ct_stats_kernel.hpp) with the batches as a second argument.
#include "ct_stats_kernel.hpp"

namespace ct {

template <typename T, int V, int INTERP, int BMAX, bool IL>
__global__ __launch_bounds__(kBlock) void video_stats_multi_kernel(const StatsArgs a, const StatsBatches mb)
{
    extern __shared__ __align__(16) char lds[];
    constexpr bool kRanged = sizeof(T) != 4;
    const int C = a.channels, L = a.n_points;
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

    // the one read of the state: what batch 0 merges into, unless it is the first of the video
    float st_mean[V], st_m2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) st_mean[e] = st_m2[e] = 0.0f;
    if (mb.count_before[0] != 0.0f) {
        if constexpr (IL) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                st_mean[e] = a.mean_state[pq[e]];
                st_m2[e] = a.m2_state[pq[e]];
            }
        } else {
            load_packet(a.mean_state + q0, st_mean);
            load_packet(a.m2_state + q0, st_m2);
        }
    }

#pragma unroll 1
    for (int b = 0; b < mb.n_batches; ++b) {
        const int B = mb.batch[b];
        const float WA = mb.count_before[b];
        const T *src = static_cast<const T *>(mb.frames[b]) + q0;
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
        // merge_state's two cases, on registers
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (WA != 0.0f) {
                merge_moments(WA, (float)B, st_mean[e], st_m2[e], mean_b[e], m2[e], st_mean[e], st_m2[e]);
            } else {
                st_mean[e] = mean_b[e];
                st_m2[e] = m2[e];
            }
        }
    }

    if constexpr (IL) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            a.mean_state[pq[e]] = st_mean[e];
            a.m2_state[pq[e]] = st_m2[e];
        }
    } else {
        store_packet(a.mean_state + q0, st_mean);
        store_packet(a.m2_state + q0, st_m2);
    }
}

int stats_multi(const StatsArgs &a, const StatsBatches &mb, int dtype, uint32_t Q, int interp, hipStream_t s)
{
    if (mb.n_batches < 2 || mb.n_batches > kMaxStatsBatches || mb.batch_max > kStatsCachedMax) return CT_ERR_INVALID_ARGUMENT;
    // packets of 4 elements only where every batch can be read as such: one ownership for the whole call
    return stats_dispatch(a, mb.frames, mb.n_batches, dtype, Q, interp, [&](const StatsArgs &part, auto t, auto V, auto I, auto IL) {
        return with_stats_bmax<false>(mb.batch_max, [&](auto BMAX) {
            return stats_launch_grid(video_stats_multi_kernel<decltype(t), V, I, BMAX, IL>, stats_grid<V>(part), I, s, part, mb);
        });
    });
}

}  // namespace ct
