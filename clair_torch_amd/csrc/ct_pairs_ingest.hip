// ct_pairs_ingest.hip -- a recognised gpu_transforms chain and the exposure-pair residual kernels in ONE pass over raw uint8 /
// uint16 frames (gfx950): ct_pair_residual_ingest_fwd and ct_pair_residual_ingest_bwd.  The kernels are those of
// ct_pairs_kernel.hpp instantiated with the extended argument block PairIngestArgs: phase 1 stages every sample as
//   x = (float)code -> ct::ingest_stages<true> (ct_ingest_stages.hpp) -> icrf_sample<INTERP, true, /*RANGED=*/false>
// -- the device functions ct_ingest_transform and then the float32 staging of ct_pair_residual_fwd / _bwd run -- so the staged
// (value, weight, coordinate, linearized std) have the bits of that two-launch route, and the pair phase is untouched.  Tile
// width and stager follow the same rule as there (pick_tile, vec_ok), so for contiguous allocations of one shape both routes
// walk the same tiles in the same column order and differ by the order of the float64 atomics alone.
//
// What it saves per launch: sizeof(code) bytes read per sample where the float32 stack costs 4, and per step the
// ct_ingest_transform pass (sizeof(code) read + 4 written per sample) and the (N, C, H, W) float32 buffer itself.  The chain is
// evaluated once per staged sample (about 4 .. 16 VALU operations), not per pair; the pair phase spends P / N pair evaluations
// on that sample.  The code-domain staging never applies here (a chain's output is not a code).
//
// Instantiations: uint8 and uint16 only (float32 frames have no copy to save: CT_ERR_UNSUPPORTED), every interpolation and std
// mode of ct_pairs.hip except LOOKUP with a std mode, which the entry points refuse (no gradient path).
#include "ct_pairs_kernel.hpp"

namespace ct {

// Everything that needs no pointer into device memory, in the siblings' order: geometry, stack and stage list, 8-bit /
// 16-bit codes, the constants' alignment and the model (check_code_ingest), then what ct_pair_residual_fwd / _bwd check
// (fill_common), then the alignment of the frames and of the planar std stack.
static int fill_ingest(PairIngestArgs &a, const void *frames_dev, int32_t dtype, const ct_ingest_stage *stages, int32_t n_stages,
                       const float *consts_dev, int32_t n_images, const ct_geometry *g, const float *std_dev, const ct_icrf *icrf,
                       const ct_pair_params *prm, int32_t n_pairs)
{
    bool by_channel = false;
    if (const int rc = check_code_ingest(dtype, n_images, g, stages, n_stages, consts_dev, icrf, by_channel); rc != CT_OK) return rc;
    if (const int rc = fill_common(a, frames_dev, n_images, g, std_dev, icrf, prm, n_pairs); rc != CT_OK) return rc;
    if (!aligned(frames_dev, dtype_bytes(dtype)) || !aligned(std_dev, sizeof(float))) return CT_ERR_INVALID_ARGUMENT;
    a.consts = consts_dev;
    a.std_stride = (int64_t)g->channels * g->h_tile * g->width;  // dense planar (N, C, H_tile, W)
    a.by_channel = by_channel ? 1u : 0u;
    a.n_stages = (uint32_t)n_stages;
    for (int32_t k = 0; k < n_stages; ++k) a.stage[k] = stages[k];
    return CT_OK;
}

template <typename F>
static int with_code_type(int32_t dtype, F &&f)
{
    return dtype == CT_DTYPE_U8 ? f(uint8_t{}) : f(uint16_t{});
}

}  // namespace ct

extern "C" int ct_pair_residual_ingest_fwd(const void *frames_dev, int32_t dtype, const ct_ingest_stage *stages, int32_t n_stages,
                                           const float *consts_dev, int32_t n_images, const ct_geometry *geom,
                                           const float *std_dev, const ct_icrf *icrf, const int32_t *i_idx_dev,
                                           const int32_t *j_idx_dev, const double *ratio_dev, int32_t n_pairs,
                                           const ct_pair_params *params, int32_t level, const double *center_dev,
                                           double *sums_dev, void *stream)
{
    using namespace ct;
    PairIngestArgs a{};
    int rc = fill_ingest(a, frames_dev, dtype, stages, n_stages, consts_dev, n_images, geom, std_dev, icrf, params, n_pairs);
    if (rc != CT_OK) return rc;
    if (n_pairs == 0) return CT_OK;
    if (!i_idx_dev || !j_idx_dev || !ratio_dev || !sums_dev || level < 0 || level > 1) return CT_ERR_INVALID_ARGUMENT;
    if (params->std_mode != CT_STD_NONE && icrf->interp == CT_INTERP_LOOKUP) return CT_ERR_NO_GRADIENT_PATH;
    a.i_idx = i_idx_dev;
    a.j_idx = j_idx_dev;
    a.ratio = ratio_dev;
    a.sums = sums_dev;
    a.center = center_dev;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_code_type(dtype, [&](auto t) { return fwd_dispatch<decltype(t)>(a, icrf->interp, params->std_mode, level, s); });
}

extern "C" int ct_pair_residual_ingest_bwd(const void *frames_dev, int32_t dtype, const ct_ingest_stage *stages, int32_t n_stages,
                                           const float *consts_dev, int32_t n_images, const ct_geometry *geom,
                                           const float *std_dev, const ct_icrf *icrf, const double *ratio_dev, int32_t n_pairs,
                                           const int32_t *partner_offsets_dev, const int32_t *partner_sample_dev,
                                           const int32_t *partner_pair_dev, const ct_pair_params *params, const double *coef_dev,
                                           const double *smean_dev, double *lut_grad_dev, void *workspace_dev,
                                           int64_t workspace_bytes, void *stream)
{
    using namespace ct;
    if (!params) return CT_ERR_INVALID_ARGUMENT;
    // uncertainties only matter to the backward through the weights: without uncertainty weighting they are ignored
    ct_pair_params prm = *params;
    if (!prm.use_uncertainty_weighting) prm.std_mode = CT_STD_NONE;
    PairIngestArgs a{};
    int rc = fill_ingest(a, frames_dev, dtype, stages, n_stages, consts_dev, n_images, geom, std_dev, icrf, &prm, n_pairs);
    if (rc != CT_OK) return rc;
    if (n_pairs == 0) return CT_OK;
    if (!ratio_dev || !partner_offsets_dev || !partner_sample_dev || !partner_pair_dev || !coef_dev || !lut_grad_dev ||
        workspace_bytes < 0)
        return CT_ERR_INVALID_ARGUMENT;
    if (icrf->interp == CT_INTERP_NONE) return CT_ERR_INVALID_ARGUMENT;
    if (prm.std_mode != CT_STD_NONE) {
        if (!smean_dev) return CT_ERR_INVALID_ARGUMENT;
        if (icrf->interp == CT_INTERP_LOOKUP) return CT_ERR_NO_GRADIENT_PATH;
    }
    a.ratio = ratio_dev;
    a.part_off = partner_offsets_dev;
    a.part_sample = partner_sample_dev;
    a.part_pair = partner_pair_dev;
    a.coef = coef_dev;
    a.smean = smean_dev;
    a.lut_grad = lut_grad_dev;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_code_type(dtype, [&](auto t) {
        return bwd_dispatch<decltype(t)>(a, icrf->interp, prm.std_mode, workspace_dev, (size_t)workspace_bytes, s);
    });
}
