// ct_ingest_stages.hpp -- the arithmetic of a recognised gpu_transforms chain, shared by ct_ingest.hip (which writes the
// result) and ct_extrema.hip (which reduces the value a data-dependent Normalize receives).  See ct_ingest.hip for the
// specification of the stages; float32 throughout, every operation rounded on its own (-ffp-contract=off).
#pragma once
#include <string.h>

#include "ct_args.hpp"

namespace ct {

// A stage list as the kernels take it by value: anything with n_stages and stage[].  DATA: a CT_INGEST_AFFINE_DATA
// stage takes sub / div from the caller (read once per thread from consts_dev); without DATA no such stage can occur
// (the host refuses it) and the code is that of the constant chains.
template <bool DATA, int N, typename Args>
__device__ __forceinline__ void ingest_stages(float (&v)[N], const Args &a, uint32_t c, float data_sub = 0.0f, float data_div = 1.0f)
{
    for (uint32_t s = 0; s < a.n_stages; ++s) {
        const ct_ingest_stage &st = a.stage[s];
        if (st.kind == CT_INGEST_AFFINE || (DATA && st.kind == CT_INGEST_AFFINE_DATA)) {
            const bool data = DATA && st.kind == CT_INGEST_AFFINE_DATA;
            const float sub = data ? data_sub : st.sub, div = data ? data_div : st.div, mul = st.mul, add = st.add;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                float t = v[k] - sub;
                t = t / div;
                t = t * mul;
                v[k] = t + add;
            }
        } else {
            const float lo = st.lo[c], hi = st.hi[c];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const float t = v[k] < lo ? lo : v[k];
                v[k] = t > hi ? hi : t;
            }
        }
    }
}

// Validation shared by ct_ingest_transform, ct_ingest_transform_data and ct_ingest_extrema: everything about the stack and
// the stage list that does not need a pointer.  by_channel: does a clamp hold different pairs for different channels?
// n_data: how many CT_INGEST_AFFINE_DATA stages the list holds (at most max_data are allowed).
static inline int ingest_validate(int32_t dtype, int32_t layout, int64_t n_images, int32_t channels, int64_t plane,
                                  const ct_ingest_stage *stages, int32_t n_stages, int32_t max_stages, int32_t max_data,
                                  bool &by_channel)
{
    if (dtype != CT_DTYPE_U8 && dtype != CT_DTYPE_U16 && dtype != CT_DTYPE_F32) return CT_ERR_INVALID_ARGUMENT;
    if (layout != CT_LAYOUT_NCHW && layout != CT_LAYOUT_NHWC && layout != CT_LAYOUT_NHWC_BGR) return CT_ERR_INVALID_ARGUMENT;
    if (channels < 1 || n_images < 0 || plane < 0) return CT_ERR_INVALID_ARGUMENT;
    if (n_stages < 0 || n_stages > max_stages || (n_stages > 0 && !stages)) return CT_ERR_INVALID_ARGUMENT;
    by_channel = false;
    int32_t n_data = 0;
    for (int32_t k = 0; k < n_stages; ++k) {
        if (stages[k].kind == CT_INGEST_AFFINE_DATA) {
            if (++n_data > max_data) return CT_ERR_INVALID_ARGUMENT;
            continue;
        }
        if (stages[k].kind != CT_INGEST_AFFINE && stages[k].kind != CT_INGEST_CLAMP) return CT_ERR_INVALID_ARGUMENT;
        if (stages[k].kind == CT_INGEST_CLAMP)
            for (int c = 1; c < CT_INGEST_MAX_CHANNELS; ++c)
                by_channel |= memcmp(&stages[k].lo[c], &stages[k].lo[0], sizeof(float)) != 0 ||
                              memcmp(&stages[k].hi[c], &stages[k].hi[0], sizeof(float)) != 0;
    }
    if (layout != CT_LAYOUT_NCHW && channels != 3) return CT_ERR_UNSUPPORTED;
    if (by_channel && channels > CT_INGEST_MAX_CHANNELS) return CT_ERR_UNSUPPORTED;
    return CT_OK;
}

// What ct_video_stats_ingest_batch and ct_hdr_merge_ingest_batch check first, in this order: the geometry (an empty plane is
// a call with nothing to do), a stack of `n_images` frames and the stage list, 8-bit / 16-bit codes (float32 pixels have no
// copy to save: ct_video_stats_batch / ct_hdr_merge_batch take them), the constants' alignment, the model.
static inline int check_code_ingest(int32_t dtype, int64_t n_images, const ct_geometry *geom, const ct_ingest_stage *stages,
                                    int32_t n_stages, const float *consts_dev, const ct_icrf *icrf, bool &by_channel)
{
    if (!geom || !icrf) return CT_ERR_INVALID_ARGUMENT;
    int rc = check_ingest_geometry(geom, true);
    if (rc != CT_OK) return rc;
    rc = ingest_validate(dtype, geom->layout, n_images, geom->channels, geom->h_tile * geom->width, stages, n_stages,
                         CT_INGEST_MAX_STAGES, consts_dev ? 1 : 0, by_channel);
    if (rc != CT_OK) return rc;
    if (dtype == CT_DTYPE_F32) return CT_ERR_UNSUPPORTED;
    return aligned(consts_dev, sizeof(float)) && icrf_ok(icrf) ? CT_OK : CT_ERR_INVALID_ARGUMENT;
}

}  // namespace ct
