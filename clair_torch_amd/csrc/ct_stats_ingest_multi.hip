// ct_stats_ingest_multi.hip -- the several-batches-per-launch (MULTI) form of ct_stats_ingest.hip's register-cached kernel,
// behind ct::stats_ingest_multi (ct_video_stats_ingest_batches), gfx950.  A translation unit of its own, as
// ct_merge_ingest_multi.hip is for the merge: the instantiations compile next to ct_stats_ingest.hip's.
//
// Ownership is video_stats_ingest_kernel's, word for word (the head of ct_stats_ingest.hip; the host side is ct::si_layout):
// PLANAR G = 4 packets of a plane with the G = 1 launch for what precedes the first aligned state packet and follows the last
// whole one, PACKED3 one pixel per thread, the LUT row from the global flat index -- and a thread owns its elements for EVERY
// batch of the call.  Per batch it runs that kernel's BMAX > 0 walk (all B loads in flight, every code loaded and the chain
// evaluated once, float32 sum / B, then sum (x - mean_b)^2 over the frames in order) inside a `#pragma unroll 1` loop over
// the batches, each batch with its own frames, size, count and -- DATA -- its own constants of a data-dependent Normalize
// (one wave-uniform load per batch), and merges with ct::merge_moments on registers: the 16 B of state per element and batch
// that a launch per batch moves stay in 2 * NE registers.  The state arrays are read once, before batch 0 and only if frames
// came before it, and written once, after the last batch.  The counts travel by value (StatsBatches::count_before, the float
// of the exact integer, formed on the host): the result is that of one launch per batch, bit for bit.  HBM-bound; no
// atomics, no LDS traffic besides the LUT, the frames are read only.
// Host: ct::stats_ingest_multi is ct_stats_ingest.hip's dispatch and launch (ct::si_dispatch, ct_stats_kernel.hpp) with the
// batches as a second argument.
#include "ct_ingest_stages.hpp"
#include "ct_stats_kernel.hpp"

namespace ct {

// (Location, load, sample and walk stand in the kernel itself, as in video_stats_ingest_kernel: see the remark there.)
template <typename T, bool PACKED, int G, int INTERP, int BMAX, bool DATA>
__global__ __launch_bounds__(kBlock) void video_stats_ingest_multi_kernel(const StatsIngestArgs a, const StatsBatches mb)
{
    extern __shared__ __align__(16) char lds[];
    static_assert(PACKED ? G == 1 : (G == 1 || G == kSiGroup), "one pixel, or one element / one packet of a plane");
    static_assert(BMAX > 0, "the register-cached walks only");
    stage_lut<INTERP>(lds, a.lut, a.channels, a.n_points);
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
    const int C = a.channels, L = a.n_points;
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
    const int64_t src_off = PACKED ? (int64_t)p0 * NP : (int64_t)c0 * a.plane + p0;

    // the one read of the state: what batch 0 merges into, unless it is the first of the video
    float st_mean[NE], st_m2[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) st_mean[k] = st_m2[k] = 0.0f;
    if (mb.count_before[0] != 0.0f) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            float ma[G], va[G];
            load_packet(a.mean_state + q[j], ma);
            load_packet(a.m2_state + q[j], va);
#pragma unroll
            for (int e = 0; e < G; ++e) {
                st_mean[j * G + e] = ma[e];
                st_m2[j * G + e] = va[e];
            }
        }
    }

#pragma unroll 1
    for (int b = 0; b < mb.n_batches; ++b) {
        const int B = mb.batch[b];
        const float WA = mb.count_before[b];
        const T *src = static_cast<const T *>(mb.frames[b]) + src_off;
        // the constants of this batch's data-dependent Normalize: one wave-uniform load
        const float *consts = mb.consts[b];
        const float dsub = DATA ? consts[0] : 0.0f, ddiv = DATA ? consts[1] : 1.0f;

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
        // merge_state's two cases, on registers
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            if (WA != 0.0f) {
                merge_moments(WA, (float)B, st_mean[k], st_m2[k], mean_b[k], m2[k], st_mean[k], st_m2[k]);
            } else {
                st_mean[k] = mean_b[k];
                st_m2[k] = m2[k];
            }
        }
    }

#pragma unroll
    for (int j = 0; j < NP; ++j) {
        float mo[G], vo[G];
#pragma unroll
        for (int e = 0; e < G; ++e) {
            mo[e] = st_mean[j * G + e];
            vo[e] = st_m2[j * G + e];
        }
        store_packet(a.mean_state + q[j], mo);
        store_packet(a.m2_state + q[j], vo);
    }
}

int stats_ingest_multi(const StatsIngestArgs &a, const StatsBatches &mb, int dtype, bool packed, int interp, hipStream_t s)
{
    if (mb.n_batches < 2 || mb.n_batches > kMaxStatsBatches || mb.batch_max > kStatsCachedMax) return CT_ERR_INVALID_ARGUMENT;
    return si_dispatch(a, dtype, packed, interp, [&](const StatsIngestArgs &part, dim3 grid, auto t, auto P, auto G, auto I, auto DATA) {
        return with_stats_bmax<false>(mb.batch_max, [&](auto BMAX) {
            return stats_launch_grid(video_stats_ingest_multi_kernel<decltype(t), P, G, I, BMAX, DATA>, grid, I, s, part, mb);
        });
    });
}

}  // namespace ct
