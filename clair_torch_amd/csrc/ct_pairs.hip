// ct_pairs.hip -- the exposure-pair residual kernels (ct_pairs_kernel.hpp: structure, arithmetic, roofline) on stacks of
// uint8 / uint16 codes or float32 pixels: ct_pair_residual_fwd, ct_pair_residual_bwd and the backward's workspace size.
// This unit instantiates the kernels with their default argument block (PairArgs) and owns what only stacks of codes
// need: the normalisation constants and the code-domain staging decision.  ct_pairs_ingest.hip is the other unit.
#include "ct_pairs_kernel.hpp"

extern "C" int ct_norm_constants(float max_code, float *hi, float *lo);
extern "C" int ct_pivot_floor_constants(float max_code, int n_points, float *rcp_step);

namespace ct {

// Code-domain staging is taken for integer stacks at the type's full range with a LINEAR curve whose step is a whole
// number of codes (host-verified for every code: ct_pivot_floor_constants) and no uncertainties.  The reference's validity
// mask lower <= fl(u / max) <= upper (general_functions.py:302) becomes a code interval by bisection with the same float32
// division (monotone in u); an empty interval keeps the generic staging.
static void fill_code_domain(PairArgs &a, int32_t dtype, float max_code, int interp, int std_mode, float weight_scale)
{
    a.code_domain = 0;
    if (interp != CT_INTERP_LINEAR || std_mode != CT_STD_NONE) return;
    // (Extending this staging to max_code below the container's range and to LUT steps that are not whole numbers of codes
    // was built and measured in round 3 -- value and coordinate in the reference's order on the proven interval, bit-identical
    // to the generic staging -- and bought nothing: C3 with 12-bit codes 8.94 ms against 8.90 ms generic; at full range the
    // two stagings now differ by 0.5 %, the loads of the next tile being in flight behind the pair phase either way.)
    static const bool disabled = getenv("CT_PAIRS_NO_CODE_DOMAIN") != nullptr;  // diagnostics: time the generic staging
    if (disabled) return;
    if (max_code != (dtype == CT_DTYPE_U8 ? 255.0f : 65535.0f)) return;
    float rcp = 0.0f;
    if (ct_pivot_floor_constants(max_code, a.n_points, &rcp) != CT_OK) return;  // whole steps, verified for every code
    const float step = (float)((int)max_code / (a.n_points - 1));
    const int maxc = (int)max_code;
    auto norm = [&](int u) { const float uf = (float)u; return fmaf(uf, a.norm.hi, uf * a.norm.lo); };  // == fl(u / max), ct_norm_constants
    int lo = 0, hi = maxc + 1;  // first code with norm >= lower
    while (lo < hi) { const int mid = (lo + hi) / 2; if (norm(mid) >= a.lower) hi = mid; else lo = mid + 1; }
    const int code_lo = lo;
    lo = 0; hi = maxc + 1;      // first code with norm > upper
    while (lo < hi) { const int mid = (lo + hi) / 2; if (norm(mid) > a.upper) hi = mid; else lo = mid + 1; }
    const int code_hi = lo - 1;
    if (code_lo > code_hi) return;
    const double kk = sqrt((double)weight_scale * 1.4426950408889634);
    a.code_rcp = rcp;
    a.code_step = step;
    a.code_inv_step = (float)(1.0 / (double)step);
    a.code_lo = (float)code_lo;
    a.code_hi = (float)code_hi;
    a.code_dk_mul = (float)(kk / (double)max_code);
    a.code_dk_add = (float)(-0.5 * kk);
    a.code_domain = 1;
}

// The dtype step of both entry points: integer stacks get their normalisation constants and the code-domain decision,
// then f(T{}) runs with the element type (f dispatches on the remaining modes).
template <typename F>
static int with_pixel_type(PairArgs &a, int32_t dtype, float max_code, int interp, const ct_pair_params &prm, F &&f)
{
    if (dtype == CT_DTYPE_F32) return f(float{});
    if (dtype != CT_DTYPE_U8 && dtype != CT_DTYPE_U16) return CT_ERR_UNSUPPORTED;
    if (ct_norm_constants(max_code, &a.norm.hi, &a.norm.lo) != CT_OK) return CT_ERR_UNSUPPORTED;
    fill_code_domain(a, dtype, max_code, interp, prm.std_mode, prm.weight_scale);
    return dtype == CT_DTYPE_U8 ? f(uint8_t{}) : f(uint16_t{});
}
}  // namespace ct

extern "C" int ct_pair_residual_fwd(const void *stack_dev, int32_t dtype, float max_code, int32_t n_images,
                                    const ct_geometry *geom, const float *std_dev, const ct_icrf *icrf,
                                    const int32_t *i_idx_dev, const int32_t *j_idx_dev, const double *ratio_dev,
                                    int32_t n_pairs, const ct_pair_params *params, int32_t level,
                                    const double *center_dev, double *sums_dev, void *stream)
{
    using namespace ct;
    PairArgs a{};
    int rc = fill_common(a, stack_dev, n_images, geom, std_dev, icrf, params, n_pairs);
    if (rc != CT_OK) return rc;
    if (n_pairs == 0) return CT_OK;
    if (!i_idx_dev || !j_idx_dev || !ratio_dev || !sums_dev || level < 0 || level > 1) return CT_ERR_INVALID_ARGUMENT;
    // icrf_training.py:117-124 / measure_linearity.py:57-62: autograd.grad raises for LOOKUP when stds are given
    if (params->std_mode != CT_STD_NONE && icrf->interp == CT_INTERP_LOOKUP) return CT_ERR_NO_GRADIENT_PATH;
    a.i_idx = i_idx_dev;
    a.j_idx = j_idx_dev;
    a.ratio = ratio_dev;
    a.sums = sums_dev;
    a.center = center_dev;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_pixel_type(a, dtype, max_code, icrf->interp, *params, [&](auto t) {
        return fwd_dispatch<decltype(t)>(a, icrf->interp, params->std_mode, level, s);
    });
}

extern "C" int ct_pair_residual_bwd(const void *stack_dev, int32_t dtype, float max_code, int32_t n_images,
                                    const ct_geometry *geom, const float *std_dev, const ct_icrf *icrf,
                                    const double *ratio_dev, int32_t n_pairs, const int32_t *partner_offsets_dev,
                                    const int32_t *partner_sample_dev, const int32_t *partner_pair_dev,
                                    const ct_pair_params *params, const double *coef_dev, const double *smean_dev,
                                    double *lut_grad_dev, void *workspace_dev, int64_t workspace_bytes, void *stream)
{
    using namespace ct;
    if (!params) return CT_ERR_INVALID_ARGUMENT;
    // uncertainties only matter to the backward through the weights: without uncertainty weighting they are ignored
    ct_pair_params prm = *params;
    if (!prm.use_uncertainty_weighting) prm.std_mode = CT_STD_NONE;
    PairArgs a{};
    int rc = fill_common(a, stack_dev, n_images, geom, std_dev, icrf, &prm, n_pairs);
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
    return with_pixel_type(a, dtype, max_code, icrf->interp, prm, [&](auto t) {
        return bwd_dispatch<decltype(t)>(a, icrf->interp, prm.std_mode, workspace_dev, (size_t)workspace_bytes, s);
    });
}

extern "C" int64_t ct_pair_residual_bwd_workspace(int32_t n_images, int32_t n_pairs, int32_t channels)
{
    if (n_images < 0 || n_pairs < 0 || channels < 0) return 0;
    return (int64_t)ct::once_workspace_bytes(n_images, n_pairs, channels);
}
