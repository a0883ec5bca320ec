// ct_stats_merge.hpp -- the pairwise merge of a batch's (mean, m2) into the running WBOMeanVar state, shared by ct_stats.hip
// and ct_stats_ingest.hip (merge_state: the state in memory; Args: anything with mean_state, m2_state, count_before and batch)
// and by their several-batches forms ct_stats_multi.hip / ct_stats_ingest_multi.hip (merge_moments: the state in registers).
#pragma once
#include "ct_device.hpp"

namespace ct {

template <typename T, int V>
struct alignas(sizeof(T) * V) SPacket {
    T v[V];
};

// The merge itself on registers (statistics.py:250-251, the one copy): (ma, va) the running mean and m2 of WA > 0 frames,
// (mb, m2b) those of the WB frames of the batch; (mo, vo) may be (ma, va).
__device__ __forceinline__ void merge_moments(float WA, float WB, float ma, float va, float mb, float m2b, float &mo, float &vo)
{
    const float W = WA + WB;
    const float delta = mb - ma;
    vo = va + m2b + (WA * WB / W) * (delta * delta);  // statistics.py:250
    mo = ma + (WB / W) * delta;                       // statistics.py:251
}

// V consecutive floats as one aligned packet
template <int V>
__device__ __forceinline__ void load_packet(const float *p, float (&v)[V])
{
    const SPacket<float, V> t = *reinterpret_cast<const SPacket<float, V> *>(p);
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = t.v[e];
}

template <int V>
__device__ __forceinline__ void store_packet(float *p, const float (&v)[V])
{
    SPacket<float, V> t;
#pragma unroll
    for (int e = 0; e < V; ++e) t.v[e] = v[e];
    *reinterpret_cast<SPacket<float, V> *>(p) = t;
}

// Merge of the batch statistics into the running state in memory (statistics.py:245-251).
template <int V, bool IL, typename Args>
__device__ __forceinline__ void merge_state(const Args &a, uint32_t q0, const uint32_t (&pq)[V], const float (&mean_b)[V],
                                            const float (&m2)[V])
{
    const float WA = a.count_before, WB = (float)a.batch;
    if constexpr (IL) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float mo = mean_b[e], vo = m2[e];
            if (WA != 0.0f) {
                const float ma = a.mean_state[pq[e]], va = a.m2_state[pq[e]];
                merge_moments(WA, WB, ma, va, mean_b[e], m2[e], mo, vo);
            }
            a.mean_state[pq[e]] = mo;
            a.m2_state[pq[e]] = vo;
        }
        return;
    }
    SPacket<float, V> mo, vo;
    if (WA == 0.0f) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            mo.v[e] = mean_b[e];
            vo.v[e] = m2[e];
        }
    } else {
        const SPacket<float, V> ma = *reinterpret_cast<const SPacket<float, V> *>(a.mean_state + q0);
        const SPacket<float, V> va = *reinterpret_cast<const SPacket<float, V> *>(a.m2_state + q0);
#pragma unroll
        for (int e = 0; e < V; ++e) merge_moments(WA, WB, ma.v[e], va.v[e], mean_b[e], m2[e], mo.v[e], vo.v[e]);
    }
    *reinterpret_cast<SPacket<float, V> *>(a.mean_state + q0) = mo;
    *reinterpret_cast<SPacket<float, V> *>(a.m2_state + q0) = vo;
}

}  // namespace ct
