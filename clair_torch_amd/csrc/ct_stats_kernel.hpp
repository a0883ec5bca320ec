// ct_stats_kernel.hpp -- what the one-batch-per-launch statistics kernels (ct_stats.hip, ct_stats_ingest.hip) and their
// several-batches-per-launch forms (ct_stats_multi.hip, ct_stats_ingest_multi.hip) share: the argument blocks, the rules that
// say which thread owns which element (the host side of them: stats_split, si_layout), the entry points of the MULTI
// translation units and the one host path in front of every launch: the walk over a batch list (stats_batches), the dispatch
// on dtype / interpolation / layout (stats_dispatch, si_dispatch), the BMAX pick (with_stats_bmax) and the launch itself
// (stats_launch_grid).  The kernels stay in their .hip files.  Device code is shared only where every kernel's gfx950
// assembly stayed byte for byte what the copies gave (tools/compare_kernel_asm.py): stats_own below did.  The register-cached
// walk, the merge on registers, the ingest form's thread location and its load and sample step did not -- a shared form of
// each changed 128 to 207 of the 240 kernels that see it (instruction order, operand order, register numbers; no scratch) --
// so the MULTI kernels repeat them.  The table: profiles/stats_refactor_ab.md.
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

// ---- host: the launch, one copy for the four translation units ----------------------------------------------------------
// BMAX of the walk for batches of at most `batch` frames: f(integral_constant<int, BMAX>), the register-cached walks of 16 and
// of kStatsCachedMax frames.  STREAMED: the single-batch launches, which walk a larger batch out of memory (BMAX = 0).
template <bool STREAMED, typename F>
static int with_stats_bmax(int32_t batch, F &&f)
{
    if constexpr (STREAMED)
        if (batch > kStatsCachedMax) return f(std::integral_constant<int, 0>{});
    return batch <= 16 ? f(std::integral_constant<int, 16>{}) : f(std::integral_constant<int, kStatsCachedMax>{});
}

// kernel(a, mb...) on `grid`: an empty grid is nothing to do, the LUT has to fit the LDS (the ingest entry points have refused
// that one before they come here, si_validate: for them it cannot fire), the launch and its error.
template <typename Kernel, typename Args, typename... Batches>
static int stats_launch_grid(Kernel kernel, dim3 grid, int interp, hipStream_t s, const Args &a, const Batches &...mb)
{
    if (grid.x == 0) return CT_OK;
    const size_t lds = lut_lds_bytes(interp, a.channels, a.n_points);
    if (lds > kLdsBudget) return CT_ERR_TOO_LARGE;
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, s, a, mb...);
    return hipGetLastError() == hipSuccess ? CT_OK : CT_ERR_LAUNCH;
}

// ---- host: the batch list of ct_video_stats_batches and ct_video_stats_ingest_batches ---------------------------------------
constexpr int kStatsPerBatch = 1;  // one_launch's answer where the list is not one launch (no CT_* status is positive)

// Every batch judged as the single-batch entry point would judge it, with the frame count its caller would pass -- nothing has
// touched the device when one of them is refused -- then ONE launch where the list allows it, else one single-batch call per
// batch with frames, exactly what the caller would have done (CT_STATS_REQUIRE_ONE_LAUNCH: refused instead).
//   validate(b, count)                  the status of batch b of the arguments, with `count` frames in front of it
//   one_launch(mb, cached)              the batches with frames (at least one).  cached: two or more, each within a register-
//                                       cached walk.  The status of the call, or kStatsPerBatch
//   single(frames, consts, batch, count)   the single-batch entry point
// forward_lone_empty: a list of one batch of size 0 goes to `single` as a list of one batch with frames does; else it is a list.
template <typename Validate, typename OneLaunch, typename Single>
static int stats_batches(const void *const *frames_devs, const float *const *consts_devs, const int32_t *batch_sizes, int32_t n_batches,
                         float frames_before, uint32_t flags, bool forward_lone_empty, Validate &&validate, OneLaunch &&one_launch,
                         Single &&single)
{
    if (n_batches < 1 || n_batches > kMaxStatsBatches || !frames_devs || !batch_sizes) return CT_ERR_INVALID_ARGUMENT;
    if (n_batches == 1 && (forward_lone_empty || batch_sizes[0] != 0))
        return single(frames_devs[0], consts_devs ? consts_devs[0] : nullptr, batch_sizes[0], frames_before);
    StatsBatches mb = {};
    int64_t before = 0;
    int n = 0;
    for (int b = 0; b < n_batches; ++b) {
        // the float of the exact count (frames_before is one already; a sum of integers below 2^53 is exact in double)
        const float count = before == 0 ? frames_before : (float)((double)frames_before + (double)before);
        if (const int rc = validate(b, count); rc != CT_OK) return rc;
        if (batch_sizes[b] == 0) continue;
        mb.frames[n] = frames_devs[b];
        mb.consts[n] = consts_devs ? consts_devs[b] : nullptr;
        mb.batch[n] = batch_sizes[b];
        mb.count_before[n] = count;
        mb.batch_max = batch_sizes[b] > mb.batch_max ? batch_sizes[b] : mb.batch_max;
        before += batch_sizes[b];
        ++n;
    }
    mb.n_batches = n;
    if (n == 0) return CT_OK;
    if (const int rc = one_launch(mb, n >= 2 && mb.batch_max <= kStatsCachedMax); rc != kStatsPerBatch) return rc;
    if (n >= 2 && (flags & CT_STATS_REQUIRE_ONE_LAUNCH)) return CT_ERR_UNSUPPORTED;  // (tests: make the route explicit)
    for (int b = 0; b < n; ++b)
        if (const int rc = single(mb.frames[b], mb.consts[b], mb.batch[b], mb.count_before[b]); rc != CT_OK) return rc;
    return CT_OK;
}

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

// Memory element q of a tile of frames: its position in the planar state (== q unless the frames are interleaved) and the
// byte offset of its LUT row in the LDS table, from the global flat index.  One element, by value: the only shape of this
// rule that leaves the three kernels' assembly as it was (profiles/stats_refactor_ab.md).
struct StatsOwn {
    uint32_t pq;
    int row_off;
};

template <int INTERP, bool IL>
__device__ __forceinline__ StatsOwn stats_own(const TileMap &tile, uint32_t q, int C, int L)
{
    int ch;
    uint32_t qg;
    StatsOwn o;
    o.pq = IL ? tile.planar_index(q) : q;
    tile.locate(o.pq, ch, qg);
    o.row_off = lut_row<INTERP>(qg, ch, C) * L * lut_entry_bytes(INTERP);
    return o;
}

// grid of a launch of a.q_count elements, V of them per thread
template <int V>
static inline dim3 stats_grid(const StatsArgs &a)
{
    return dim3((a.q_count / V + kBlock - 1) / kBlock);
}

// dtype / V / interp / layout -> template arguments, for ct_stats.hip and ct_stats_multi.hip: launch(part, T{}, V, INTERP, IL)
// for the vector body and the scalar tail of the Q elements; packets where each of the n `frames` can be read as such.
template <typename Launch>
static int stats_dispatch(const StatsArgs &a, const void *const *frames, int n, int dtype, uint32_t Q, int interp, Launch &&launch)
{
    auto typed = [&](auto t) {
        using T = decltype(t);
        bool frames_vec_ok = true;
        for (int b = 0; b < n; ++b) frames_vec_ok = frames_vec_ok && stats_frames_vec_ok<T>(frames[b], a.image_stride);
        return stats_split(a, Q, frames_vec_ok, [&](const StatsArgs &part, auto V) {
            return with_enum<CT_INTERP_LOOKUP, CT_INTERP_LINEAR, CT_INTERP_CATMULL, CT_INTERP_NONE>(interp, [&](auto I) {
                return part.tile.layout == CT_LAYOUT_NCHW ? launch(part, T{}, V, I, std::false_type{}) : launch(part, T{}, V, I, std::true_type{});
            });
        });
    };
    if (dtype == CT_DTYPE_U8) return typed(uint8_t{});
    if (dtype == CT_DTYPE_U16) return typed(uint16_t{});
    if (dtype == CT_DTYPE_F32) return typed(float{});
    return CT_ERR_UNSUPPORTED;
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

// dtype / interp / layout / constants -> template arguments, for ct_stats_ingest.hip and ct_stats_ingest_multi.hip:
// launch(part, grid, T{}, PACKED, G, INTERP, DATA) for each launch of si_layout.
template <typename Launch>
static int si_dispatch(const StatsIngestArgs &a, int dtype, bool packed, int interp, Launch &&launch)
{
    auto typed = [&](auto t) {
        using T = decltype(t);
        return with_enum<CT_INTERP_LOOKUP, CT_INTERP_LINEAR, CT_INTERP_CATMULL, CT_INTERP_NONE>(interp, [&](auto I) {
            return si_layout(a, packed, [&](const StatsIngestArgs &part, auto P, auto G, uint32_t threads_x) {
                const dim3 grid = si_grid(part, P, threads_x);
                return a.consts ? launch(part, grid, T{}, P, G, I, std::true_type{}) : launch(part, grid, T{}, P, G, I, std::false_type{});
            });
        });
    };
    if (dtype == CT_DTYPE_U8) return typed(uint8_t{});
    if (dtype == CT_DTYPE_U16) return typed(uint16_t{});
    return CT_ERR_UNSUPPORTED;
}

}  // namespace ct
