// ct_merge_multi.hip -- the several-batches-per-launch (MULTI) instantiations of ct::merge_pivot_kernel, behind
// ct::merge_pivot_multi.  A translation unit of its own so that they compile next to ct_merge.hip's instantiations
// instead of after them (each of the two takes minutes of one core).
#include "ct_merge_pivot.hpp"

namespace ct {

template <typename T, int INTERP, int WEIGHT, int STD, bool CLAMP>
static int launch_pivot_multi(const MergeArgs &a, PivotArgs x, hipStream_t stream)
{
    if (a.q_count == 0) return CT_OK;
    if constexpr (INTERP == CT_INTERP_LOOKUP && WEIGHT == CT_WEIGHT_NONE && STD != CT_STD_NONE) {
        return CT_ERR_NO_GRADIENT_PATH;
    } else {
        constexpr int V = kPivotV;
        x.n_tiles = (a.q_count + (uint32_t)(kBlock * V) - 1) / (uint32_t)(kBlock * V);
        const size_t lds = pivot_lds_bytes(a, x, INTERP);
        // TODO: fall back to one launch per batch instead (the summed exposures of all batches need more LDS than one batch)
        if (lds > kLdsBudget) return CT_ERR_TOO_LARGE;
        return launch_pivot_grid<merge_pivot_kernel<T, V, INTERP, WEIGHT, STD, false, CLAMP, true>>(a, x, lds, stream);
    }
}

// CLAMP (codes above max_code) is its own instantiation for uint16 only; without a model there is nothing to clamp.
template <typename T>
static int dispatch_multi(const MergeArgs &a, const PivotArgs &x, bool clamp, int interp, int weight_mode, int std_mode, hipStream_t s)
{
    return with_merge_modes(interp, weight_mode, std_mode, [&](auto I, auto W, auto S) {
        if constexpr (sizeof(T) == 2 && I != CT_INTERP_NONE) {
            if (clamp) return launch_pivot_multi<T, I, W, S, true>(a, x, s);
        }
        return launch_pivot_multi<T, I, W, S, false>(a, x, s);
    });
}

int merge_pivot_multi(const MergeArgs &a, const PivotArgs &px, int dtype, bool clamp, int interp, int weight_mode, int std_mode,
                      hipStream_t s)
{
    return dtype == CT_DTYPE_U8 ? dispatch_multi<uint8_t>(a, px, clamp, interp, weight_mode, std_mode, s)
                                : dispatch_multi<uint16_t>(a, px, clamp, interp, weight_mode, std_mode, s);
}

}  // namespace ct
