// ct_stats_kernel.hpp -- what the one-batch-per-launch statistics kernels (ct_stats.hip, ct_stats_ingest.hip) and their
// several-batches-per-launch forms (ct_stats_multi.hip, ct_stats_ingest_multi.hip) share: the argument blocks, the rules that
// say which thread owns which element (the host side of them: stats_split, si_layout) and the entry points of the MULTI
// translation units.  The kernels themselves stay in their .hip files; the MULTI kernels repeat the register-cached walk
// around a loop over the batches instead of sharing a device function with the single-batch kernels, whose code is left as
// it was (a walk in a callee costs ct_stats_ingest.hip's kernel a scratch copy of its argument block, see there).
#pragma once
#include "ct_args.hpp"
#include "ct_stats_merge.hpp"

namespace ct {

struct StatsArgs {
    const void *frames;
    const float *lut;
    float *mean_state, *m2_state;
    int64_t image_stride;
    uint32_t q_begin, q_count;
    TileMap tile;
    int32_t batch, channels, n_points;
    NormConst norm;
    float count_before;  // W_A (number of frames merged so far)
};

struct StatsIngestArgs {
    const void *frames;
    const float *consts;    // sub, div of a CT_INGEST_AFFINE_DATA stage (ct_ingest_extrema), or NULL
    const float *lut;
    float *mean_state, *m2_state;
    int64_t image_stride;   // source elements between consecutive frames
    uint32_t plane;         // H_tile * W
    uint32_t plane_global;  // H_global * W: global flat index of (c, local p) = c * plane_global + base + p
    uint32_t base;          // row_offset * W
    int32_t batch, channels, n_points;
    uint32_t reversed;      // PACKED3: memory channel cm feeds plane 2 - cm (BGR)
    uint32_t by_channel;    // some clamp holds different pairs for different channels (then C <= CT_INGEST_MAX_CHANNELS)
    uint32_t state_lead;    // PLANAR: (mean_state address / 4) % 4, or kSiNoPackets: every element goes through G = 1
    float count_before;     // W_A (number of frames merged so far)
    uint32_t n_stages;
    ct_ingest_stage stage[CT_INGEST_MAX_STAGES];
};

// MULTI (ct_video_stats_batches, ct_video_stats_ingest_batches): batch b is batch[b] >= 1 frames at frames[b], merged into a
// state of count_before[b] frames -- the float of the exact integer count, formed on the host as a caller of the single-batch
// entry point forms it, never summed in float32 on the device -- with the constants of a data-dependent Normalize at
// consts[b] (the ingest form with a CT_INGEST_AFFINE_DATA stage; else NULL).  The frames, batch, count_before and consts of
// the first argument block are not read.
constexpr int kMaxStatsBatches = CT_STATS_MAX_BATCHES;
constexpr int kStatsCachedMax = 32;  // frames of a batch the register-cached walks take (BMAX 16 / 32)
struct StatsBatches {
    const void *frames[kMaxStatsBatches];
    const float *consts[kMaxStatsBatches];
    int32_t batch[kMaxStatsBatches];
    float count_before[kMaxStatsBatches];
    int32_t n_batches;  // 2 .. kMaxStatsBatches
    int32_t batch_max;  // the largest batch[b], <= kStatsCachedMax: picks BMAX
};

// ct_stats_multi.hip / ct_stats_ingest_multi.hip: the several-batches launches (one, plus the scalar edge launch the
// single-batch entry points have), dispatched on dtype / layout / interpolation / BMAX.  `a` as the single-batch entry point
// fills it for any of the batches.  Return a CT_* status.
int stats_multi(const StatsArgs &a, const StatsBatches &mb, int dtype, uint32_t Q, int interp, hipStream_t stream);
int stats_ingest_multi(const StatsIngestArgs &a, const StatsBatches &mb, int dtype, bool packed, int interp, hipStream_t stream);

// ---- ct_stats.hip's ownership: V = 4 consecutive memory elements per thread, then a V = 1 tail --------------------------
constexpr int kStatsV = 4;  // 4 elements per thread: 32 frames x 4 values fit the register file

// the frames of a batch can be read as packets of V elements
template <typename T>
static inline bool stats_frames_vec_ok(const void *frames, int64_t image_stride)
{
    return aligned(frames, sizeof(T) * kStatsV) && (image_stride % kStatsV) == 0;
}

// The vector body [0, q_vec) and the scalar tail [q_vec, Q) of one call: dispatch(a, integral_constant<int, V>) launches the
// elements [a.q_begin, a.q_begin + a.q_count).  frames_vec_ok: stats_frames_vec_ok of every batch of the call.
template <typename Dispatch>
static int stats_split(StatsArgs a, uint32_t Q, bool frames_vec_ok, Dispatch &&dispatch)
{
    constexpr int V = kStatsV;
    const bool vec_ok = frames_vec_ok && aligned(a.mean_state, 4 * V) && aligned(a.m2_state, 4 * V);
    const uint32_t q_vec = vec_ok ? (Q / V) * V : 0;
    int rc = CT_OK;
    if (q_vec) {
        a.q_begin = 0;
        a.q_count = q_vec;
        rc = dispatch(a, std::integral_constant<int, V>{});
        if (rc != CT_OK) return rc;
    }
    if (q_vec < Q) {
        a.q_begin = q_vec;
        a.q_count = Q - q_vec;
        rc = dispatch(a, std::integral_constant<int, 1>{});
    }
    return rc;
}

// ---- ct_stats_ingest.hip's ownership (its head describes it) ------------------------------------------------------------
constexpr int kSiGroup = 4;  // PLANAR: elements per thread of the vector body, one 16-byte state packet
constexpr uint32_t kSiNoPackets = 4;

template <typename T, int N>
struct SiRaw {
    T v[N];
};

// elements in front of a plane's first aligned state packet, and the end of its last whole one
__device__ __forceinline__ void si_body(const StatsIngestArgs &a, uint32_t c, uint32_t &head, uint32_t &body_end)
{
    head = a.state_lead == kSiNoPackets ? a.plane : (0u - (a.state_lead + c * a.plane)) & (uint32_t)(kSiGroup - 1);
    head = head < a.plane ? head : a.plane;
    body_end = head + ((a.plane - head) & ~(uint32_t)(kSiGroup - 1));
}

// grid of a launch of threads_x threads per plane (PLANAR: a workgroup row per channel)
static inline dim3 si_grid(const StatsIngestArgs &a, bool packed, uint32_t threads_x)
{
    return dim3((threads_x + kBlock - 1) / kBlock, packed ? 1u : (uint32_t)a.channels);
}

// The launches of one call: launch(a, bool_constant<PACKED>, integral_constant<int, G>, threads_x).
template <typename Launch>
static int si_layout(StatsIngestArgs a, bool packed, Launch &&launch)
{
    using One = std::integral_constant<int, 1>;
    if (packed) return launch(a, std::true_type{}, One{}, a.plane);
    auto lead = [](const void *p) { return (uint32_t)((reinterpret_cast<uintptr_t>(p) / sizeof(float)) % kSiGroup); };
    // packets only where mean and m2 are equally aligned (always, for two allocations); else element by element
    const bool packets = lead(a.mean_state) == lead(a.m2_state) && a.plane >= (uint32_t)kSiGroup;
    a.state_lead = packets ? lead(a.mean_state) : kSiNoPackets;
    if (packets) {
        const int rc = launch(a, std::false_type{}, std::integral_constant<int, kSiGroup>{}, a.plane / kSiGroup);  // (a thread per possible packet)
        if (rc != CT_OK) return rc;
        if (a.state_lead == 0 && a.plane % kSiGroup == 0) return CT_OK;  // every plane is whole packets
        return launch(a, std::false_type{}, One{}, (uint32_t)(2 * (kSiGroup - 1)));
    }
    return launch(a, std::false_type{}, One{}, a.plane);
}

}  // namespace ct
