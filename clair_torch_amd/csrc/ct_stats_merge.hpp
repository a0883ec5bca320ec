// ct_stats_merge.hpp -- the pairwise merge of a batch's (mean, m2) into the running WBOMeanVar state, shared by ct_stats.hip
// and ct_stats_ingest.hip.  Args: anything with mean_state, m2_state, count_before and batch.
#pragma once
#include "ct_device.hpp"

namespace ct {

template <typename T, int V>
struct alignas(sizeof(T) * V) SPacket {
    T v[V];
};

// Merge of the batch statistics into the running state (statistics.py:245-251), shared by both kernels.
template <int V, bool IL, typename Args>
__device__ __forceinline__ void merge_state(const Args &a, uint32_t q0, const uint32_t (&pq)[V], const float (&mean_b)[V],
                                            const float (&m2)[V])
{
    const float WA = a.count_before, WB = (float)a.batch, W = WA + WB;
    if constexpr (IL) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float mo = mean_b[e], vo = m2[e];
            if (WA != 0.0f) {
                const float ma = a.mean_state[pq[e]], va = a.m2_state[pq[e]];
                const float delta = mean_b[e] - ma;
                vo = va + m2[e] + (WA * WB / W) * (delta * delta);  // statistics.py:250
                mo = ma + (WB / W) * delta;                          // statistics.py:251
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
        for (int e = 0; e < V; ++e) {
            const float delta = mean_b[e] - ma.v[e];
            vo.v[e] = va.v[e] + m2[e] + (WA * WB / W) * (delta * delta);  // statistics.py:250
            mo.v[e] = ma.v[e] + (WB / W) * delta;                          // statistics.py:251
        }
    }
    *reinterpret_cast<SPacket<float, V> *>(a.mean_state + q0) = mo;
    *reinterpret_cast<SPacket<float, V> *>(a.m2_state + q0) = vo;
}

}  // namespace ct
