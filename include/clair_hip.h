/*
 * clair_hip.h -- C ABI of the MI355X (gfx950) implementation of clair-torch's per-pixel hot path.
 *
 * The reference (samivout/clair-torch) is pure Python on eager PyTorch and has no FFI of its own; each entry
 * point below replaces the *interior* of one reference function (file:line cited per function, relative to
 * the reference repository).  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes, no torch / HIP types in the signatures; `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream);
 *   - every pointer named *_dev is DEVICE memory owned by the caller; nothing is allocated, freed or retained;
 *   - launches are asynchronous on `stream`; no hidden device synchronisation; re-entrant across streams;
 *   - return value: CT_OK (0) or a negative CT_ERR_* code; never throws.  ct_error_string() names a code.
 *   - image stacks are NCHW, contiguous inside one exposure; consecutive exposures are `image_stride`
 *     elements apart (= C*H_tile*W for a dense stack).
 *
 * Tiling (multi-GPU row bands): a rank holds rows [row_offset, row_offset + H_tile) of every channel plane of a
 * global (C, H_global, W) image.  The reference picks the LUT row for LINEAR/CATMULL interpolation from the flat
 * NCHW index modulo C (clair_torch/models/base.py:173-176, 216-219), so kernels need the GLOBAL geometry to
 * reproduce it on a tile; pass H_global = H_tile and row_offset = 0 for an untiled image.
 */
#ifndef CLAIR_HIP_H
#define CLAIR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CT_ABI_VERSION 3

/* status codes */
#define CT_OK 0
#define CT_ERR_INVALID_ARGUMENT (-1)
#define CT_ERR_UNSUPPORTED (-2)      /* dtype / mode combination not built */
#define CT_ERR_LAUNCH (-3)           /* HIP launch failure */
#define CT_ERR_NO_GRADIENT_PATH (-4) /* the reference raises RuntimeError here (no grad path to the image) */
#define CT_ERR_TOO_LARGE (-5)        /* a dimension exceeds what the kernels index */

/* element type of an image stack */
#define CT_DTYPE_U8 0  /* raw codes; x = code / max_code exactly as Normalize(0, max_code) on float32 */
#define CT_DTYPE_U16 1
#define CT_DTYPE_F32 2 /* already normalised float32 pixel values */

/* clair_torch/common/enums.py:10 InterpMode (+ "no model": icrf_model=None) */
#define CT_INTERP_LOOKUP 0
#define CT_INTERP_LINEAR 1
#define CT_INTERP_CATMULL 2
#define CT_INTERP_NONE 3

/* where the standard uncertainty of a sample comes from (clair_torch/datasets/base.py:128-135 MissingStdMode) */
#define CT_STD_NONE 0       /* no uncertainty propagated */
#define CT_STD_CONSTANT 1   /* sigma = std_value */
#define CT_STD_MULTIPLIER 2 /* sigma = std_value * x */
#define CT_STD_EXPLICIT 3   /* sigma read from std_dev (float32, same layout as the stack) */

/* weight_fn of compute_hdr_image: None -> ones, anything else -> Gaussian scale 30 (hdr_merge.py:95) */
#define CT_WEIGHT_NONE 0
#define CT_WEIGHT_GAUSS 1

/* flags of ct_hdr_merge_batch */
#define CT_MERGE_FIRST_BATCH 1u  /* state is not read (WBOMean starts at mean 0, weight 0) */
#define CT_MERGE_FINALIZE 2u     /* also write mean_out / std_out = sqrt(variance) after this batch */
#define CT_MERGE_MEAN_OUT_F32 4u /* mean_out is float32 instead of the reference's float64 */
#define CT_MERGE_F64_MOMENTS 8u  /* diagnostic: keep the float64-moment kernel where the pivoted float32 one would run */
#define CT_MERGE_REFERENCE_ORDER 16u /* evaluate the uncertainty in the reference's own float32 autograd order (two passes,
                                        float64 exp / divisions; ct_merge_exact.hip).  Default for LOOKUP and CATMULL with
                                        uncertainties, whose reference results are dominated by float32 cancellation */
#define CT_MERGE_CLOSED_FORM 32u     /* keep the fast closed-form kernels for LOOKUP / CATMULL with uncertainties as well */
#define CT_MERGE_REQUIRE_ONE_LAUNCH 128u /* ct_hdr_merge_batches, ct_hdr_merge_ingest_batches, ct_hdr_merge_dark_batches: CT_ERR_UNSUPPORTED instead of one launch per batch (ct_hdr_merge_dark_ingest_batches: CT_ERR_TOO_LARGE) */
#define CT_MERGE_STD_HINT 64u        /* ct_hdr_merge_kernel_name only: uncertainties are propagated */
#define CT_MERGE_OUT_AS_INPUT 256u   /* extension: state and outputs in the MEMORY ORDER OF THE INPUT stack instead of planar
                                        (C, H, W): an interleaved (H, W, C) RGB / BGR stack then gives (H, W, C) outputs in the
                                        same channel order -- what an OpenCV writer wants (the reference's save path permutes
                                        back, common/general_functions.py:338-358) -- and the merge stores dense packets
                                        without regrouping.  Use the same flag on every batch of a merge. */

/* ct_video_stats_batches, ct_video_stats_ingest_batches */
#define CT_STATS_MAX_BATCHES 16
#define CT_STATS_REQUIRE_ONE_LAUNCH 1u /* CT_ERR_UNSUPPORTED instead of one launch per batch */

/* Memory layout of one image of a stack.  Outputs and state are always planar (C, H, W) like the reference's tensors.
 * NHWC = the interleaved layout OpenCV decodes to (clair_torch/common/data_io.py:125-154); NHWC_BGR additionally
 * reverses the channel order on the fly, i.e. folds cv_to_torch (clair_torch/common/general_functions.py:315-335)
 * into the load.  Supported by ct_hdr_merge_batch(es), ct_linearize_std, ct_pair_residual_fwd / _bwd and
 * ct_video_stats_batch (an explicit std stack is then interleaved likewise); flat field, dark field and band
 * statistics work on planar data. */
#define CT_LAYOUT_NCHW 0
#define CT_LAYOUT_NHWC 1
#define CT_LAYOUT_NHWC_BGR 2

/* Geometry of a (tile of a) stack. */
typedef struct ct_geometry {
    int32_t channels;     /* C */
    int64_t h_tile;       /* rows held locally */
    int64_t width;        /* W */
    int64_t h_global;     /* rows of the full image (== h_tile when untiled) */
    int64_t row_offset;   /* first global row held locally */
    int64_t image_stride; /* elements between consecutive exposures / frames */
    int32_t layout;       /* CT_LAYOUT_* of the INPUT stack */
} ct_geometry;

/* ICRF model: LUT (C, L) float32 row-major as ICRFModelBase._icrf (clair_torch/models/base.py:69-71). */
typedef struct ct_icrf {
    const float *lut_dev; /* NULL with interp == CT_INTERP_NONE */
    int32_t n_points;     /* L */
    int32_t interp;       /* CT_INTERP_* */
} ct_icrf;

/* library / ABI */
int ct_abi_version(void);
const char *ct_error_string(int code);

/*
 * ct_hdr_merge_batch -- one batch of compute_hdr_image's loop body
 * (clair_torch/inference/hdr_merge.py:61-128: linearize, / exposure, weights, WBOMean.update_values
 *  [clair_torch/common/statistics.py:64-109], autograd variance [hdr_merge.py:107-115], internal_detach)
 * fused into one pass over the batch; with CT_MERGE_FINALIZE also hdr_merge.py:155 (squeeze + sqrt).
 *
 *   stack_dev      (B, C, H_tile, W) of `dtype`, exposures sorted as custom_collate does (datasets/collate.py:23)
 *   max_code       255 / 65535 / ... for integer dtypes (ignored for CT_DTYPE_F32)
 *   std_dev        explicit float32 std stack (CT_STD_EXPLICIT) else NULL; std_value for CONSTANT / MULTIPLIER
 *   exposure_dev   (B) float64 exposure times (collate.py:29 makes them float64)
 *   mean_state_dev (Q) float64, sumw_state_dev (Q) float32, var_state_dev (Q) float32, Q = C*H_tile*W:
 *                  WBOMean state + running variance, updated in place; may all be NULL when flags has both
 *                  FIRST_BATCH and FINALIZE (single-batch merge)
 *   mean_out_dev   (Q) float64 (or float32 with CT_MERGE_MEAN_OUT_F32), std_out_dev (Q) float32 or NULL when
 *                  std_mode == CT_STD_NONE; written only with CT_MERGE_FINALIZE
 * Returns CT_ERR_NO_GRADIENT_PATH for LOOKUP + CT_WEIGHT_NONE + std (the reference's autograd.grad raises).
 */
int ct_hdr_merge_batch(const void *stack_dev, int32_t dtype, float max_code, int32_t batch, const ct_geometry *geom,
                       const float *std_dev, int32_t std_mode, float std_value, const double *exposure_dev,
                       const ct_icrf *icrf, int32_t weight_mode, double *mean_state_dev, float *sumw_state_dev,
                       float *var_state_dev, void *mean_out_dev, float *std_out_dev, uint32_t flags, void *stream);

/*
 * ct_hdr_merge_batches -- n_batches consecutive iterations of compute_hdr_image's loop (hdr_merge.py:61-128) in one call:
 * exactly ct_hdr_merge_batch applied to batch 0 .. n_batches-1 in turn (CT_MERGE_FIRST_BATCH on batch 0 and
 * CT_MERGE_FINALIZE on the last one when set in `flags`), bit for bit.  Where the pivoted code-domain kernel applies and
 * every batch is packet-aligned (n_batches <= 16) it is ONE launch that keeps (mean, sum of weights, variance) in
 * registers between the batches -- the reference's default batch_size: 4 (scripts/config.yaml) otherwise moves 32 B of
 * state per element and batch beside 8 B of samples.  The reference-order kernel (CT_MERGE_REFERENCE_ORDER, the default
 * of LOOKUP / CATMULL with uncertainties) does the same for any dtype and alignment.  Anything else runs one launch per
 * batch.
 *   stack_devs / std_devs / batch_sizes  HOST arrays of n_batches device pointers / sizes (std_devs NULL unless EXPLICIT);
 *                                        every batch is (B_b, C, H_tile, W) with the common geometry, sorted as collate does
 *   exposure_dev                         the exposure times of all batches, concatenated in the same order (device)
 *   state / outputs / flags              as ct_hdr_merge_batch; the state may be NULL when flags has FIRST_BATCH and FINALIZE
 */
int ct_hdr_merge_batches(const void *const *stack_devs, const float *const *std_devs, const int32_t *batch_sizes,
                         int32_t n_batches, int32_t dtype, float max_code, const ct_geometry *geom, int32_t std_mode,
                         float std_value, const double *exposure_dev, const ct_icrf *icrf, int32_t weight_mode,
                         double *mean_state_dev, float *sumw_state_dev, float *var_state_dev, void *mean_out_dev,
                         float *std_out_dev, uint32_t flags, void *stream);

/*
 * Host-side proofs behind the folded integer paths (no device work; results cached per argument set):
 *   ct_norm_constants        fma(u, hi, u * lo) == the reference's float32 u / max_code for EVERY code
 *                            (clair_torch/common/general_functions.py:377) -- else CT_ERR_UNSUPPORTED
 *   ct_index_constants       the folded LUT coordinate has the reference's floor and round-half-even for every code
 *                            (clair_torch/models/base.py:146,166)
 *   ct_pivot_index_constants floor(u (L-1) / max_code) == (u * index_mul) >> 32 (or == u when *index_mul == 0) for every
 *                            code, with step = max_code / (L-1) an integer (what ct::merge_pivot_kernel addresses its
 *                            table with)
 *   ct_pivot_floor_constants the same interval from the code held as a float (typed buffer loads): mantissa of
 *                            fma(u, *rcp_step, 1.5 * 2^23) rounded toward minus infinity, for every code
 */
int ct_norm_constants(float max_code, float *hi, float *lo);
int ct_index_constants(float max_code, int n_points, float *hi, float *lo);
int ct_pivot_index_constants(float max_code, int n_points, uint32_t *index_mul, float *step);
int ct_pivot_floor_constants(float max_code, int n_points, float *rcp_step);
/*   ct_pivot_interval_constants  the general form of the above: table entry min(floor(u * *scale), last) equals the
 *                            reference's LINEAR interval (lookup = 0) / LOOKUP sample (entry j -> sample (j + 1) >> 1,
 *                            lookup = 1) for every code 0..dtype_max of the container, any max_code <= dtype_max, any L */
int ct_pivot_interval_constants(float max_code, int n_points, int lookup, int dtype_max, float *scale);

/* Diagnostics: a static string naming the kernel ct_hdr_merge_batch dispatches for these arguments. */
const char *ct_hdr_merge_kernel_name(int32_t dtype, float max_code, int32_t interp, int32_t n_points, uint32_t flags);

/* Diagnostics: device counter bumped once per wavefront of the pivoted merge kernel that had to repeat a batch about the
 * exact mean (ill-conditioned pivot); NULL disables.  Process-global, not part of the data path. */
void ct_merge_set_retry_counter(unsigned long long *counter_dev);

/*
 * ct_linearize_std -- body of linearize_dataset_generator for F independent frames
 * (clair_torch/inference/linearization.py:95-106,132): lin = f(x), std = sqrt((f'(x) * sigma)^2), float32,
 * bit-exact with the reference for LOOKUP / LINEAR.  std_out_dev may be NULL (value only).
 * Each frame is its own batch of one, as the reference requires (linearization.py:42).
 */
int ct_linearize_std(const void *frames_dev, int32_t dtype, float max_code, int64_t n_frames, const ct_geometry *geom,
                     const float *std_dev, int32_t std_mode, float std_value, const ct_icrf *icrf, float *lin_out_dev,
                     float *std_out_dev, void *stream);

/*
 * ct_linearize_fwd / ct_linearize_bwd -- ICRFModelBase.forward (clair_torch/models/base.py:135-226) on a
 * (N, C, H_tile, W) float32 tensor and its backward: grad wrt the image (analytic derivative of the LUT
 * interpolation incl. the clamp mask) and, when lut_grad_dev != NULL, the (C, L) float32 LUT gradient
 * accumulated (+=) with LDS-privatised scatter.  Used by the model's autograd wrapper.
 */
int ct_linearize_fwd(const float *x_dev, int64_t n_images, const ct_geometry *geom, const ct_icrf *icrf,
                     float *out_dev, void *stream);
int ct_linearize_bwd(const float *x_dev, const float *grad_out_dev, int64_t n_images, const ct_geometry *geom,
                     const ct_icrf *icrf, float *grad_x_dev, float *lut_grad_dev, void *stream);

/* Parameters of the exposure-pair linearity residual (train_icrf / measure_linearity). */
typedef struct ct_pair_params {
    float lower, upper;                 /* inclusive validity range of the raw pixel value (general_functions.py:302) */
    float weight_scale;                 /* Gaussian pair-weight scale, 10 in the reference (losses.py:212) */
    int32_t use_relative;               /* use_relative_linearity_loss */
    int32_t use_uncertainty_weighting;  /* add 1 / (err + 1e-6) to the weights (losses.py:96) */
    int32_t std_mode;                   /* CT_STD_*: source of sigma for the linearized std |f'(x) sigma| */
    float std_value;
    int32_t pair_band;                  /* backward only, a hint: 0 = nothing known; B > 0 = the caller promises that every
                                           pair (i, j) of the list has 0 < j - i <= B (get_valid_exposure_pairs on a sorted
                                           exposure series with a ratio limit gives such a band).  Enables the
                                           lane-per-sample backward for n_images <= 64; the promise is verified on the
                                           device and a broken one only costs the fast path. */
} ct_pair_params;

/*
 * ct_pair_residual_fwd -- spatial sums of the per-pixel linearity residual for P exposure pairs; replaces
 * get_pairwise_valid_pixel_mask + combined_gaussian_pair_weights + model forward + pixelwise_linearity_loss +
 * compute_spatial_linearity_loss of one train_icrf step (clair_torch/training/icrf_training.py:105-133) or of
 * measure_linearity (clair_torch/inference/measure_linearity.py:44-72).
 *   stack_dev (N, C, H_tile, W); i_idx_dev / j_idx_dev (P) int32, ratio_dev (P) float64 = t_i / t_j
 *   (get_valid_exposure_pairs, common/general_functions.py:242-272)
 *   level 0: sums 0..1 only (training), level 1: all five sums
 *   center_dev (P, C) float64 or NULL: value subtracted from v inside sum [2].  The weighted std needs
 *     sum (v - mean)^2 w m (general_functions.py:163-165); expanding it from raw moments cancels by (mean/std)^2, so
 *     callers run level 1 twice: once for the means, once with center = mean.
 *   sums_dev (P, C, 5) float64, ACCUMULATED (+=, caller zeroes; tiles / ranks add up):
 *     [0] sum w m   [1] sum v w m   [2] sum (v - center)^2 w m   [3] sum err m   [4] sum m
 *   with v the (relative) absolute residual, w the weight, m the validity mask, err the residual's uncertainty.
 *   spatial mean = [1] / max([0], 1e-8), etc. (general_functions.py:149-170).
 */
int ct_pair_residual_fwd(const void *stack_dev, int32_t dtype, float max_code, int32_t n_images,
                         const ct_geometry *geom, const float *std_dev, const ct_icrf *icrf, const int32_t *i_idx_dev,
                         const int32_t *j_idx_dev, const double *ratio_dev, int32_t n_pairs,
                         const ct_pair_params *params, int32_t level, const double *center_dev, double *sums_dev,
                         void *stream);

/*
 * ct_pair_residual_bwd -- gradient of the training loss's linearity term with respect to the (C, L) LUT
 * (what loss[c].backward() deposits in the model parameters, icrf_training.py:148-149, for that term).
 *   coef_dev (P, C) float64 = dL/d(spatial mean_pc) / max(sums[p][c][0], 1e-8)
 *   partner lists (CSR over samples): for sample n, entries partner_offsets[n] .. partner_offsets[n+1]-1 give the
 *   other sample of every pair containing n (partner_sample_dev) and the pair id (partner_pair_dev: p when n is
 *   the pair's first image i, ~p when it is the second image j)
 *   std_dev / params->std_mode: uncertainties, read only with params->use_uncertainty_weighting; the weights
 *   1/(err + 1e-6) then depend on the LUT (relative loss), and the backward needs smean_dev (P, C) float64 = the
 *   spatial means of the forward:  d mean = sum m [w dv + (v - mean) dw] / sum w m.  smean_dev may be NULL otherwise.
 *   lut_grad_dev (C, L) float64, ACCUMULATED (+=)
 *   workspace_dev: caller-owned scratch of at least ct_pair_residual_bwd_workspace(n_images, n_pairs, channels) bytes,
 *   32-byte aligned (the library allocates nothing): the per-channel partner tables the kernel reads with scalar loads
 *   are built there by a small preparatory launch on the same stream.  Contents are undefined afterwards.
 */
int64_t ct_pair_residual_bwd_workspace(int32_t n_images, int32_t n_pairs, int32_t channels);
int ct_pair_residual_bwd(const void *stack_dev, int32_t dtype, float max_code, int32_t n_images,
                         const ct_geometry *geom, const float *std_dev, const ct_icrf *icrf, const double *ratio_dev,
                         int32_t n_pairs, const int32_t *partner_offsets_dev, const int32_t *partner_sample_dev,
                         const int32_t *partner_pair_dev, const ct_pair_params *params, const double *coef_dev,
                         const double *smean_dev, double *lut_grad_dev, void *workspace_dev, int64_t workspace_bytes,
                         void *stream);

/*
 * Flat-field correction epilogues (clair_torch/inference/hdr_merge.py:131-153, linearization.py:48-57,118-130;
 * flat_field_mean / flatfield_correction, clair_torch/common/general_functions.py:182-238, whole-image ROI as both
 * call sites pass mid_area_side_fraction = 1.0).
 *
 * ct_flatfield_sums: sums_dev (C, 2) float64 += [sum flat, sum value / (flat + 1e-6)] over a (C, plane) band
 *   (value_dev may be NULL: only the first sum).  Additive over row bands: ranks all-reduce, then divide by the global
 *   pixel count to get M_c (float32) and the "through the mean" gradient term.
 * ct_flatfield_apply: value (F, C, plane) float64 or float32, in place: value / (flat + 1e-6) * M_c;
 *   var_or_std_dev (F, C, plane) float32 in place (or NULL): on entry the variance (input_is_variance != 0, merge)
 *   or the std (linearize) of the image term, on exit sqrt(var + (grad * flat_std)^2) with
 *   grad = -value * M_c / (flat + 1e-6)^2 + through_mean_dev[c]  (through_mean_dev NULL = 0, flat_std_dev NULL = no term),
 *   for both value types.  through_mean_dev[c] is one number per channel of ONE image, so with n_frames > 1 it is the
 *   caller's business what it means; ops.flatfield_correct refuses through_mean with several frames.
 */
int ct_flatfield_sums(const void *value_dev, int32_t value_is_f64, const float *flat_dev, int32_t channels,
                      int64_t plane, double *sums_dev, void *stream);
int ct_flatfield_apply(void *value_dev, int32_t value_is_f64, int64_t n_frames, float *var_or_std_dev,
                       int32_t input_is_variance, const float *flat_dev, const float *flat_std_dev,
                       const float *flat_mean_dev, const double *through_mean_dev, int32_t channels, int64_t plane,
                       void *stream);

/*
 * ct_band_stats -- per-channel statistics of one merged row band, the quantity BASELINE configuration C5 gathers over
 * RCCL ("tile-sharded ... merge + uncertainty, RCCL gather of per-tile stats"; the reference has no such function: its
 * script saves the merged image, scripts/run_hdr_merging.py:60-86).  One pass over the band:
 *   out_dev (6, C) float64 rows = min mean, max mean, sum mean, min std, max std, sum std   (std rows 0 when std_dev NULL)
 * mean_dev (C, plane) float64 and std_dev (C, plane) float32 are ct_hdr_merge_batch's outputs.  Deterministic (no
 * atomics); min / max / sum combine over bands.  workspace_dev: ct_band_stats_workspace(channels) bytes, 8-byte aligned.
 * Non-finite data: min / max are IEEE minNum / maxNum (fmin / fmax) -- a NaN is SKIPPED, +-inf is a number like any
 * other, and a channel that holds no number at all reports the identities (+inf, -inf).  The sums are plain additions
 * and carry NaN and inf, so a NaN anywhere in a channel always shows in that channel's sum row: a gather that must
 * notice NaN tests the sums.  (torch's amin / amax propagate NaN instead; the sign of a zero minimum or maximum is
 * unspecified when both zeros occur.)
 */
int64_t ct_band_stats_workspace(int32_t channels);
int ct_band_stats(const double *mean_dev, const float *std_dev, int32_t channels, int64_t plane, void *workspace_dev,
                  int64_t workspace_bytes, double *out_dev, void *stream);

/*
 * ct_dark_field_blur -- conditional_gaussian_blur(images, dark, threshold, 3, differentiable=True)
 * (clair_torch/common/general_functions.py:440-486) as compute_hdr_image (inference/hdr_merge.py:76-92,117-126) and
 * linearize_dataset_generator (inference/linearization.py:73-92,108-116) apply it, together with the per-sample
 * uncertainty that carries BOTH variance terms of those call sites through the unchanged merge / linearize kernels:
 *   xb_out      (B, C, H_tile, W) float32 = m blur3x3(x) + (1 - m) x,  m = sigmoid(alpha (dark - threshold))
 *   std_out     (B, C, H_tile, W) float32 = sqrt(sigma^2 + ((blur(x) - x) alpha m (1 - m) sigma_dark)^2), or NULL
 *   stack_dev   (B, C, H_tile, W) codes / float32 pixels (NCHW only); std_dev / std_mode / std_value: sigma of the RAW image
 *   dark_dev, dark_std_dev (dark_batch, C, H_tile, W) float32, dark_batch = 1 (shared) or B (one matched dark field per frame)
 *   halo_dev    (B, C, 2, W) in the stack's element type: the global rows just above and below the band; required unless
 *               the band is the whole image (at the global top / bottom the blur reflects instead and ignores that row)
 * PARITY UNPINNED: the blur is torchvision's GaussianBlur(3, sigma=1), restated from its published algorithm.
 */
int ct_dark_field_blur(const void *stack_dev, int32_t dtype, float max_code, int32_t batch, const ct_geometry *geom,
                       const void *halo_dev, const float *std_dev, int32_t std_mode, float std_value,
                       const float *dark_dev, const float *dark_std_dev, int32_t dark_batch, float threshold, float alpha,
                       float *xb_out_dev, float *std_out_dev, void *stream);

/*
 * ct_hdr_merge_dark_batch -- that blur and one batch of compute_hdr_image's loop body in ONE pass over B raw frames: state
 * and outputs are bit for bit those of ct_dark_field_blur into dense float32 (B, C, H_tile, W) stacks xb and sigma_eff
 * followed by ct_hdr_merge_batch on them with CT_DTYPE_F32, CT_STD_EXPLICIT, the same geometry (image_stride C*H_tile*W)
 * and the same flags with CT_MERGE_CLOSED_FORM -- without the two stacks: sizeof(code) + 8 bytes read per sample (+ 4 with
 * explicit image uncertainties) where the two launches move 16 B per sample more, and no float32 copy of the batch exists.
 *   stack_dev .. alpha   as ct_dark_field_blur takes them: codes or float32 pixels, CT_LAYOUT_NCHW only; std_dev (EXPLICIT)
 *                laid out like the stack (image_stride between frames); std_mode NONE / CONSTANT / MULTIPLIER / EXPLICIT only
 *                selects how the RAW image's sigma enters sigma_eff; dark_dev / dark_std_dev dense; halo_dev for a row band
 *   dark_std_dev NULL: there is no sigma_eff, as ct_dark_field_blur with std_out_dev == NULL: the merge then runs as
 *                ct_hdr_merge_batch with CT_STD_NONE on xb (std_dev / std_mode are still checked, var_state_dev and
 *                std_out_dev are not used)
 *   exposure_dev, icrf, weight_mode, state, outputs   as ct_hdr_merge_batch; state and outputs are planar (C, H_tile, W)
 *   flags        CT_MERGE_FIRST_BATCH, CT_MERGE_FINALIZE, CT_MERGE_MEAN_OUT_F32, CT_MERGE_CLOSED_FORM
 * Status: whatever ct_dark_field_blur refuses is refused with its status and in its order (a missing stack / geometry / dark
 * field, width < 2 or h_global < 2, a layout other than NCHW: CT_ERR_UNSUPPORTED, dark_batch outside {1, B}, one shared
 * dark field with its std for B > 1: CT_ERR_UNSUPPORTED, a bad std mode, a band without its halo, a one-row band at the
 * image's edge: CT_ERR_UNSUPPORTED, a short image_stride, an unknown dtype or max_code: CT_ERR_UNSUPPORTED), then whatever
 * ct_hdr_merge_batch refuses for (xb, sigma_eff) with its status (model, weight mode, CT_ERR_NO_GRADIENT_PATH for LOOKUP
 * with unit weights and a dark std, a missing state on a batch that is not first and final, missing outputs, CT_ERR_TOO_LARGE
 * for 2^31 elements).  CT_ERR_UNSUPPORTED besides: CT_MERGE_F64_MOMENTS, CT_MERGE_REFERENCE_ORDER, CT_MERGE_OUT_AS_INPUT, and
 * LOOKUP / CATMULL with a dark std and no CT_MERGE_CLOSED_FORM (ct_hdr_merge_batch sends those to the reference-order kernel,
 * which is not fused).  CT_ERR_TOO_LARGE: the LUT with 8 B per exposure exceeds 160 KiB of LDS.  Every argument is validated
 * before anything touches the device.  Allocates nothing, synchronises nothing, reads nothing back, never writes the frames,
 * touches nothing outside C*H_tile*W elements of the state and the outputs.
 */
int ct_hdr_merge_dark_batch(const void *stack_dev, int32_t dtype, float max_code, int32_t batch, const ct_geometry *geom,
                            const void *halo_dev, const float *std_dev, int32_t std_mode, float std_value,
                            const float *dark_dev, const float *dark_std_dev, int32_t dark_batch, float threshold, float alpha,
                            const double *exposure_dev, const ct_icrf *icrf, int32_t weight_mode, double *mean_state_dev,
                            float *sumw_state_dev, float *var_state_dev, void *mean_out_dev, float *std_out_dev, uint32_t flags,
                            void *stream);

/*
 * ct_hdr_merge_dark_batches -- n_batches consecutive dark-field batches of one merge in one call: exactly
 * ct_hdr_merge_dark_batch applied to batch 0 .. n_batches - 1 in turn on the same state, bit for bit -- but where it can, ONE
 * launch walks all of them with (mean, sum of weights, variance) in registers in between: the state arrays are read at most
 * once (not at all with CT_MERGE_FIRST_BATCH) and written at most once, and only if a state was passed, where a launch per batch
 * reads 16 B and writes 16 B per element and batch beside the samples and dark fields.
 *   stack_devs, batch_sizes, dark_devs, dark_batches   HOST arrays of n_batches (1 .. 16) entries: batch b is batch_sizes[b]
 *                frames at stack_devs[b] with dark_batches[b] (1 or batch_sizes[b]) dark fields at dark_devs[b], each as
 *                ct_hdr_merge_dark_batch takes it; one dtype, max_code and geometry (image_stride included) for all of them
 *   halo_devs    HOST array of n_batches device pointers, each the (B_b, C, 2, W) halo rows of that batch, or NULL as a whole;
 *                its entries are all NULL or all non-NULL
 *   std_devs     CT_STD_EXPLICIT: HOST array of n_batches device pointers, each laid out like its stack; else NULL as a whole
 *   dark_std_devs  HOST array of n_batches device pointers, or NULL as a whole; its entries are all NULL or all non-NULL
 *   exposure_dev the exposure times of all batches, concatenated (sum of batch_sizes doubles)
 *   flags        as ct_hdr_merge_dark_batch; CT_MERGE_FIRST_BATCH applies to the first and CT_MERGE_FINALIZE to the last batch.
 *                CT_MERGE_REQUIRE_ONE_LAUNCH: CT_ERR_UNSUPPORTED instead of one launch per batch.
 * n_batches outside 1 .. 16 (or a missing array) is CT_ERR_INVALID_ARGUMENT; n_batches == 1 is ct_hdr_merge_dark_batch.  A
 * mixture of NULL and non-NULL entries in dark_std_devs or in halo_devs is CT_ERR_INVALID_ARGUMENT.  Then every batch is judged
 * as ct_hdr_merge_dark_batch judges it (its checks in its order, the same status codes, the first refusal wins; the flags are
 * those of the whole call, so a state is needed unless both FIRST_BATCH and FINALIZE are set).  Every argument is validated
 * before anything touches the device.  One launch needs the LUT with 8 B per exposure of ALL batches to fit 160 KiB of LDS;
 * where only each batch alone fits, the batches are launched one by one on the state in memory -- not CT_ERR_TOO_LARGE --
 * which then must be given: without state arrays, or with CT_MERGE_REQUIRE_ONE_LAUNCH, that is CT_ERR_UNSUPPORTED and nothing
 * is launched.  Allocates nothing, synchronises nothing, reads nothing back, never writes the frames or the dark fields,
 * touches nothing outside C*H_tile*W elements of the state and the outputs.
 */
int ct_hdr_merge_dark_batches(const void *const *stack_devs, const int32_t *batch_sizes, int32_t n_batches, int32_t dtype,
                              float max_code, const ct_geometry *geom, const void *const *halo_devs, const float *const *std_devs,
                              int32_t std_mode, float std_value, const float *const *dark_devs, const float *const *dark_std_devs,
                              const int32_t *dark_batches, float threshold, float alpha, const double *exposure_dev,
                              const ct_icrf *icrf, int32_t weight_mode, double *mean_state_dev, float *sumw_state_dev,
                              float *var_state_dev, void *mean_out_dev, float *std_out_dev, uint32_t flags, void *stream);

/*
 * ct_linearize_dark --that blur and the body of linearize_dataset_generator in ONE pass over F independent raw frames, each
 * its own batch of one (linearization.py:42) with its own matched dark field: for every frame lin_out and std_out are bit for
 * bit those of ct_dark_field_blur on it (batch = 1, dark_batch = 1) into float32 xb and sigma_eff followed by
 * ct_linearize_std on (xb, CT_DTYPE_F32, std = sigma_eff, CT_STD_EXPLICIT) -- without the two stacks: sizeof(code) + 8 bytes
 * read per sample (+ 4 with explicit image uncertainties) and 8 written, where the two launches move 16 B per sample more.
 *   frames_dev   (F, C, H, W) codes (max_code) or float32 pixels, CT_LAYOUT_NCHW only, geom->image_stride between frames; the
 *                whole image (no row band: row_offset 0, h_tile == h_global)
 *   std_dev / std_mode / std_value   sigma of the RAW image as ct_dark_field_blur takes it (EXPLICIT: laid out like the
 *                frames; CT_STD_MULTIPLIER multiplies the raw x, not xb)
 *   dark_devs, dark_std_devs   HOST arrays of n_frames device pointers, read during the call: the (C, H, W) float32 dark field
 *                and its std matched to each frame; pointers may repeat.  They travel in the kernel's argument block,
 *                CT_LINEARIZE_DARK_MAX_FRAMES per launch; longer lists are walked in launches of that many
 *   lin_out_dev, std_out_dev   (F, C, H, W) float32, dense; both required (uncertainties are always propagated here)
 * Status: what ct_dark_field_blur refuses with its status and in its order (a missing pointer, n_frames <= 0 or a NULL entry
 * of either array, width < 2 or h_global < 2, a layout other than NCHW: CT_ERR_UNSUPPORTED, a bad std mode, a row band:
 * CT_ERR_UNSUPPORTED, a short image_stride, an unknown dtype or max_code: CT_ERR_UNSUPPORTED), then what ct_linearize_std
 * refuses for (xb, sigma_eff): the model, CT_ERR_NO_GRADIENT_PATH for LOOKUP, CT_ERR_TOO_LARGE for 2^31 elements per frame
 * or a LUT beyond 160 KiB of LDS; last, CT_ERR_INVALID_ARGUMENT for a pointer not aligned to its element.  Every argument is
 * validated before anything touches the device.  Allocates nothing, synchronises nothing, reads nothing back, never writes
 * the frames or the dark fields.
 */
#define CT_LINEARIZE_DARK_MAX_FRAMES 16
int ct_linearize_dark(const void *frames_dev, int32_t dtype, float max_code, int64_t n_frames, const ct_geometry *geom,
                      const float *std_dev, int32_t std_mode, float std_value, const float *const *dark_devs,
                      const float *const *dark_std_devs, float threshold, float alpha, const ct_icrf *icrf,
                      float *lin_out_dev, float *std_out_dev, void *stream);

/*
 * ct_video_stats_batch -- loop body of compute_video_mean_and_std
 * (clair_torch/inference/inferential_statistics.py:38-47): optional ICRF linearization of a batch of frames and the
 * unweighted WBOMeanVar update (clair_torch/common/statistics.py:213-259), float32 like the reference.
 *   frames_dev (B, C, H_tile, W); frames_before = number of frames already merged (0 for the first batch)
 *   mean_state_dev, m2_state_dev (C, H_tile, W) float32, updated in place.
 * After the last batch: mean = mean_state, std of the mean = sqrt(m2 / (n - 1)) / sqrt(n)  (SAMPLE_FREQUENCY).
 */
int ct_video_stats_batch(const void *frames_dev, int32_t dtype, float max_code, int32_t batch, const ct_geometry *geom,
                         const ct_icrf *icrf, float frames_before, float *mean_state_dev, float *m2_state_dev,
                         void *stream);

/*
 * ct_strided_downscale -- StridedDownscale (clair_torch/common/transforms.py:194-216), x[..., ::step, ::step], on a
 * contiguous stack in its own element type and layout, so that the code-domain kernels above run on the compacted codes:
 *   dst[p][i][j][e] = src[p][i*step][j*step][e],  i < ceil(h/step), j < ceil(w/step), e < pixel_elems
 * Planar (B, C, H, W): n_planes = B*C, pixel_elems = 1.  Interleaved (B, H, W, C): n_planes = B, pixel_elems = C (the
 * channel order is untouched).  elem_bytes 1, 2 or 4; src_dev / dst_dev aligned to it, dst_dev dense
 * (n_planes, ceil(h/step), ceil(w/step), pixel_elems).  Reads nothing outside src's n_planes*h*w*pixel_elems elements.
 */
int ct_strided_downscale(const void *src_dev, void *dst_dev, int32_t elem_bytes, int64_t n_planes, int64_t h, int64_t w,
                         int32_t pixel_elems, int32_t step, void *stream);

/*
 * ct_ingest_transform -- a gpu_transforms chain CastTo(float32), Normalize(max, min, range), ClampAlongDims in one pass
 * (normalize_tensor, clair_torch/common/general_functions.py:359-388; clamp_along_dims, general_functions.py:392-436; the
 * transform classes, clair_torch/common/transforms.py:108-157): raw codes or pixels to the planar float32 stack the
 * float32 kernels above take, bit for bit what those classes give on the CPU.  Up to CT_INGEST_MAX_STAGES stages, in
 * order, float32, every operation rounded on its own:
 *   CT_INGEST_AFFINE  t = x - sub; t = t / div; t = t * mul; t = t + add   (sub = fl32(min), div = fl32(max - min),
 *                     mul = fl32(hi - lo), add = fl32(lo); correctly rounded division; all four always run)
 *   CT_INGEST_CLAMP   t = min(max(x, lo[c]), hi[c]) as torch.clamp (NaN stays NaN), c = channel of the planar result;
 *                     one pair for all channels is that pair in all CT_INGEST_MAX_CHANNELS entries
 *   src_dev  CT_DTYPE_U8 / U16 / F32, dense, aligned to its element: (n_images, channels, plane) for CT_LAYOUT_NCHW,
 *            (n_images, plane, 3) for CT_LAYOUT_NHWC / NHWC_BGR (BGR: memory channel 2 - c feeds plane c)
 *   dst_dev  (n_images, channels, plane) float32, dense, aligned to 4 bytes (an interior slice of a buffer is fine)
 * n_stages = 0 is the cast alone.  CT_ERR_UNSUPPORTED: an interleaved layout with channels != 3; clamp pairs that differ
 * between channels with channels > CT_INGEST_MAX_CHANNELS.  Touches nothing outside n_images*channels*plane elements of
 * either side and never writes src; an empty input is CT_OK without a launch.
 */
#define CT_INGEST_AFFINE 0
#define CT_INGEST_CLAMP 1
#define CT_INGEST_MAX_STAGES 4
#define CT_INGEST_MAX_CHANNELS 4
typedef struct {
    int32_t kind;                       /* CT_INGEST_* */
    float sub, div, mul, add;           /* AFFINE */
    float lo[CT_INGEST_MAX_CHANNELS];   /* CLAMP, per channel */
    float hi[CT_INGEST_MAX_CHANNELS];
} ct_ingest_stage;
int ct_ingest_transform(const void *src_dev, int32_t dtype, int32_t layout, int64_t n_images, int32_t channels,
                        int64_t plane, const ct_ingest_stage *stages, int32_t n_stages, float *dst_dev, void *stream);

/*
 * ct_ingest_extrema / ct_ingest_transform_data -- a data-dependent Normalize (max_val and / or min_val None: the bound is
 * the batch's own extremum; normalize_tensor, clair_torch/common/general_functions.py:373-376, the class at
 * clair_torch/common/transforms.py:108-133) in such a chain, in two launches on one stream and without a readback.
 *
 * ct_ingest_extrema reads the raw stack once (src_dev, dtype, layout, n_images, channels, plane as ct_ingest_transform),
 * evaluates the n_prefix <= CT_EXTREMA_MAX_PREFIX constant stages that stand in front of the data-dependent Normalize per
 * element, reduces min, max and "any NaN" over ALL n_images*channels*plane values (torch's x.min() / x.max() of the whole
 * batch) and writes four floats to consts_dev:
 *   [0] sub = from_data & CT_EXTREMA_MIN ? min : fl32(fixed_min)      [2] the data minimum   (both NaN when any value is
 *   [1] div = fl32(top - sub), top = from_data & CT_EXTREMA_MAX ? max : fl32(fixed_max)       [3] the data maximum    NaN)
 * div == 0 is where the reference raises ValueError (general_functions.py:377-378): the caller reads consts_dev back if it
 * wants that check.  Deterministic (no atomics): one partial per workgroup in workspace_dev -- at least
 * ct_ingest_extrema_workspace() bytes, 16-byte aligned -- folded by a second one-workgroup kernel.  from_data = 0 and an
 * empty stack (torch raises on the extrema of an empty tensor) are CT_ERR_INVALID_ARGUMENT; otherwise the arguments are
 * validated as ct_ingest_transform's.  Reads nothing outside the stack, writes only the workspace and consts_dev.
 *
 * ct_ingest_transform_data is ct_ingest_transform with at most one stage of kind CT_INGEST_AFFINE_DATA: AFFINE whose sub
 * and div are consts_dev[0..1] (mul = fl32(hi - lo) and add = fl32(lo) still come from the struct).  consts_dev: non-NULL,
 * 4-byte aligned, read when the kernel runs.  ct_ingest_transform itself refuses that kind.
 * Neither function allocates, synchronises or reads anything back.
 */
#define CT_INGEST_AFFINE_DATA 2
#define CT_EXTREMA_MIN 1
#define CT_EXTREMA_MAX 2
#define CT_EXTREMA_MAX_PREFIX 3
int64_t ct_ingest_extrema_workspace(void);
int ct_ingest_extrema(const void *src_dev, int32_t dtype, int32_t layout, int64_t n_images, int32_t channels, int64_t plane,
                      const ct_ingest_stage *prefix, int32_t n_prefix, int32_t from_data, float fixed_min, float fixed_max,
                      void *workspace_dev, int64_t workspace_bytes, float *consts_dev, void *stream);
int ct_ingest_transform_data(const void *src_dev, int32_t dtype, int32_t layout, int64_t n_images, int32_t channels,
                             int64_t plane, const ct_ingest_stage *stages, int32_t n_stages, float *dst_dev,
                             const float *consts_dev, void *stream);

/*
 * ct_ingest_extrema_frames -- ct_ingest_extrema with one set of constants PER FRAME of a dense stack, for consumers whose
 * frames are batches of their own (linearize_dataset_generator: batch size 1, so Normalize() sees one frame at a time).
 * The n_frames frames lie channels*plane elements apart; consts_dev holds (n_frames, 4) floats and
 * consts_dev[4 f .. 4 f + 3] is bit for bit what ct_ingest_extrema writes when called with n_images = 1 on frame f alone:
 * {sub, div = fl32(top - sub), data min, data max}, both extrema NaN when THAT frame holds a NaN (its neighbours' constants
 * are untouched by it).  Two launches whatever n_frames is: the frame is a grid dimension of the reduction, the fold runs
 * one workgroup per frame; no atomics.  workspace_dev: at least ct_ingest_extrema_frames_workspace(n_frames) bytes,
 * 16-byte aligned.  Refusals as ct_ingest_extrema's (from_data = 0, an empty stack, NULL or misaligned pointers, a short
 * workspace: CT_ERR_INVALID_ARGUMENT); n_frames > 65535 is CT_ERR_TOO_LARGE (and its workspace size is 0).  Allocates
 * nothing, synchronises nothing, reads nothing outside the frames, writes only the workspace and consts_dev.
 */
int64_t ct_ingest_extrema_frames_workspace(int64_t n_frames);
int ct_ingest_extrema_frames(const void *src_dev, int32_t dtype, int32_t layout, int64_t n_frames, int32_t channels,
                             int64_t plane, const ct_ingest_stage *prefix, int32_t n_prefix, int32_t from_data,
                             float fixed_min, float fixed_max, void *workspace_dev, int64_t workspace_bytes,
                             float *consts_dev /* (n_frames, 4) */, void *stream);

/*
 * ct_linearize_ingest -- such a chain and the body of linearize_dataset_generator in ONE pass over F independent frames:
 * the outputs are bit for bit those of ct_ingest_transform followed by ct_linearize_std on its float32 result,
 *   x   = the stage list applied to (float)sample (CT_INGEST_AFFINE / CT_INGEST_CLAMP only, at most
 *         CT_INGEST_MAX_STAGES; n_stages = 0 is the cast alone; a CT_INGEST_AFFINE_DATA stage is
 *         CT_ERR_INVALID_ARGUMENT)
 *   lin = f(x), std = sqrt((f'(x) * sigma)^2) as ct_linearize_std computes them for a CT_DTYPE_F32 frame holding x;
 *         sigma = std_value (CONSTANT), std_value * x (MULTIPLIER, x behind the chain) or std_dev[...] (EXPLICIT)
 * without the float32 stack in between (10 bytes of memory traffic per uint16 sample instead of 18).
 *   frames_dev   CT_DTYPE_U8 / U16 / F32, aligned to its element; geom->layout CT_LAYOUT_NCHW (any C) or, with C == 3,
 *                CT_LAYOUT_NHWC / NHWC_BGR: the order of the SOURCE (a folded CvToTorch); frames image_stride elements apart
 *   geom         h_global / row_offset as for ct_linearize_std: a row band gives the same rows of the whole image (the
 *                LINEAR / CATMULL LUT row is the global flat NCHW index modulo C, the LOOKUP row the channel)
 *   lin_out_dev, std_out_dev   planar (F, C, H_tile, W) float32, dense, aligned to 4 bytes; std_out_dev may be NULL (value only)
 *   std_dev      EXPLICIT: planar (F, C, H_tile, W) float32, dense, like the OUTPUTS -- not like the stack, as
 *                ct_linearize_std's explicit std is: gpu_transforms never touch the uncertainty images, which are planar
 *                even where the frames are interleaved
 * CT_ERR_UNSUPPORTED: an interleaved layout with C != 3; clamp pairs that differ between channels with
 * C > CT_INGEST_MAX_CHANNELS.  LUT size limits, CT_ERR_NO_GRADIENT_PATH and CT_ERR_TOO_LARGE as ct_linearize_std.  Every
 * argument is validated before anything touches the device; n_frames == 0 is CT_OK without a launch.  Allocates nothing,
 * synchronises nothing, never writes the frames, touches nothing outside F*C*H_tile*W elements of the outputs.
 */
int ct_linearize_ingest(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                        const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                        float std_value, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev, void *stream);

/*
 * ct_linearize_ingest_data -- ct_linearize_ingest whose chain may hold at most one CT_INGEST_AFFINE_DATA stage with PER-FRAME
 * constants: sub and div of frame f are consts_dev[4 f] and consts_dev[4 f + 1] (consts_dev: (n_frames, 4) floats as
 * ct_ingest_extrema_frames leaves them, 4-byte aligned, read when the kernel runs).  For every frame the outputs are bit for
 * bit those of ct_ingest_transform_data on that frame with its four constants followed by ct_linearize_std on the float32
 * result.  A row band is normalised by the constants it is given (the band's own extrema on every route of the project).
 * consts_dev NULL: ct_linearize_ingest, which refuses that kind.  Everything else as ct_linearize_ingest.
 */
int ct_linearize_ingest_data(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                             const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                             float std_value, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev,
                             const float *consts_dev, void *stream);

/*
 * ct_linearize_ingest_strided -- StridedDownscale(step), such a chain and the linearization in ONE pass: every step-th row and
 * column of the raw frames in, dense planar float32 (F, C, ho, wo) out, ho = ceil(H_tile / step), wo = ceil(W / step).  Bit
 * for bit ct_strided_downscale followed by ct_linearize_ingest (consts_dev NULL) or ct_linearize_ingest_data on the
 * compacted frames, without the compacted copy; step == 1 is those two entry points themselves.
 *   geom         of the SOURCE frames (layout, H, W, image_stride) as ct_linearize_ingest takes it.  With step > 1 a row band
 *                (row_offset != 0 or h_tile != h_global) is CT_ERR_INVALID_ARGUMENT: which rows of a band a downscale selects
 *                depends on row_offset % step, a phase that is not carried
 *   step         >= 1, else CT_ERR_INVALID_ARGUMENT
 *   lin_out_dev, std_out_dev   planar (F, C, ho, wo) float32, dense, aligned to 4 bytes; std_out_dev may be NULL
 *   std_dev      EXPLICIT: planar (F, C, ho, wo) float32, dense -- already of the OUTPUT shape: gpu_transforms are applied to
 *                the value images only, so explicit uncertainties arrive at the downscaled size
 *   consts_dev   NULL, or (n_frames, 4) per-frame constants of one CT_INGEST_AFFINE_DATA stage as ct_linearize_ingest_data
 *                reads them (ct_ingest_extrema_frames on the FULL frames: a Normalize in front of the downscale)
 * The LINEAR / CATMULL LUT row is the flat NCHW index of the DOWNSCALED frame modulo C, (c * ho * wo + i * wo + j) % C.
 * Everything else -- stage checks, CT_ERR_UNSUPPORTED, CT_ERR_NO_GRADIENT_PATH, CT_ERR_TOO_LARGE, validation before anything
 * touches the device, n_frames == 0 -- as ct_linearize_ingest.  Reads only selected elements of the frames, touches nothing
 * outside F*C*ho*wo elements of the outputs.
 */
int ct_linearize_ingest_strided(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom, int32_t step,
                                const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                                float std_value, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev,
                                const float *consts_dev /* may be NULL */, void *stream);

/*
 * ct_linearize_std_flat / ct_linearize_ingest_flat / ct_linearize_ingest_strided_flat -- ct_linearize_std, ct_linearize_ingest
 * (consts_dev NULL) or ct_linearize_ingest_data, and ct_linearize_ingest_strided with the flat-field correction of
 * linearize_dataset_generator (linearization.py:48-57,118-130; the mean a constant) applied to every (lin, std) before it is
 * stored: bit for bit the parent followed by ct_flatfield_apply(value float32, std in, through_mean NULL) with the same
 * flat_mean_dev, without the second trip of both outputs through memory.  Per element, float32, every operation rounded on
 * its own:  den = flat + 1e-6;  lin' = (lin / den) * M;  grad = -(M * lin) / (den * den);  var = sd * sd
 * (+ (grad * flat_std)^2 with a flat_std);  sd' = sqrt(var).
 *   flat_dev       planar (C, plane) float32 of the OUTPUT's shape: (C, H_tile, W) -- the rows of the band for a row band --
 *                  and (C, ho, wo) behind a step; dense, aligned to 4 bytes
 *   flat_std_dev   its uncertainty, same shape, or NULL (no flat-field term in sd')
 *   flat_mean_dev  M: C floats in device memory, read when the kernel runs
 * Every other argument, and every refusal in its order, as the parent.  Behind them: flat_dev or flat_mean_dev NULL, or one of
 * the three misaligned, is CT_ERR_INVALID_ARGUMENT, and so is std_out_dev NULL -- the correction writes a std.
 */
int ct_linearize_std_flat(const void *frames_dev, int32_t dtype, float max_code, int64_t n_frames, const ct_geometry *geom,
                          const float *std_dev, int32_t std_mode, float std_value, const ct_icrf *icrf, float *lin_out_dev,
                          float *std_out_dev, const float *flat_dev, const float *flat_std_dev /* may be NULL */,
                          const float *flat_mean_dev, void *stream);
int ct_linearize_ingest_flat(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                             const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                             float std_value, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev,
                             const float *consts_dev /* may be NULL */, const float *flat_dev,
                             const float *flat_std_dev /* may be NULL */, const float *flat_mean_dev, void *stream);
int ct_linearize_ingest_strided_flat(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom, int32_t step,
                                     const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                                     float std_value, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev,
                                     const float *consts_dev /* may be NULL */, const float *flat_dev,
                                     const float *flat_std_dev /* may be NULL */, const float *flat_mean_dev, void *stream);

/*
 * ct_linearize_dark_ingest -- ct_linearize_dark on RAW frames behind a recognised gpu_transforms chain (the stage list of
 * ct_ingest_transform, declared above): for every frame lin_out and std_out are bit for bit those of
 * ct_ingest_transform on it into a planar float32 image x, ct_dark_field_blur on x (batch = 1, dark_batch = 1) into xb and
 * sigma_eff, and ct_linearize_std on (xb, CT_DTYPE_F32, std = sigma_eff, CT_STD_EXPLICIT) -- in one pass and without the three
 * float32 stacks: sizeof(element) + 8 bytes read per sample (+ 4 with explicit image uncertainties) and 8 written, 18 (22) for
 * uint16 where the three launches move 42 (46).
 *   frames_dev   CT_DTYPE_U8 / U16 / F32; geom->layout CT_LAYOUT_NCHW (any C) or, with C == 3, CT_LAYOUT_NHWC / NHWC_BGR: raw
 *                (F, H, W, 3) frames as ct_linearize_ingest reads them (BGR: memory channel cm feeds plane 2 - cm);
 *                geom->image_stride elements between frames; the whole image (no row band)
 *   stages       0 to CT_INGEST_MAX_STAGES of CT_INGEST_AFFINE / CT_INGEST_CLAMP; a CT_INGEST_AFFINE_DATA stage is
 *                CT_ERR_INVALID_ARGUMENT.  Every tap of the 3 x 3 window goes through the chain with its PLANE channel
 *   std_dev / std_mode / std_value   sigma of the image BEHIND the chain, as ct_dark_field_blur takes it on x (EXPLICIT: planar
 *                (F, C, H, W) float32, dense, like the outputs whatever the layout of the frames; CT_STD_MULTIPLIER multiplies
 *                x, not xb)
 *   dark_devs, dark_std_devs   HOST arrays of n_frames device pointers as ct_linearize_dark takes them: planar (C, H, W)
 *                float32 in plane (RGB) order
 *   lin_out_dev, std_out_dev   planar (F, C, H, W) float32, dense; both required
 * Status, in this order: what ct_linearize_dark refuses first (a missing pointer, n_frames <= 0, a NULL entry of either
 * array); the dark geometry (width < 2 or h_global < 2, a bad std mode: CT_ERR_INVALID_ARGUMENT; a row band:
 * CT_ERR_UNSUPPORTED; a short image_stride); the stack and the stage list as ct_linearize_ingest (an unknown dtype, layout or
 * kind, more than CT_INGEST_MAX_STAGES: CT_ERR_INVALID_ARGUMENT; an interleaved layout with C != 3, per-channel clamp pairs
 * with C > CT_INGEST_MAX_CHANNELS: CT_ERR_UNSUPPORTED); the model, CT_ERR_NO_GRADIENT_PATH for LOOKUP, CT_ERR_TOO_LARGE for a
 * LUT beyond 160 KiB of LDS or 2^31 elements per frame; last, CT_ERR_INVALID_ARGUMENT for a pointer not aligned to its
 * element.  Every argument is validated before anything touches the device.  Allocates nothing, synchronises nothing, reads
 * nothing back, never writes the frames, the dark fields or the uncertainties.
 */
int ct_linearize_dark_ingest(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                             const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                             float std_value, const float *const *dark_devs, const float *const *dark_std_devs,
                             float threshold, float alpha, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev,
                             void *stream);

/*
 * ct_linearize_dark_ingest_data -- ct_linearize_dark_ingest whose chain may hold at most one CT_INGEST_AFFINE_DATA stage with
 * PER-FRAME constants, as ct_linearize_ingest_data reads them: sub and div of frame f are consts_dev[4 f] and
 * consts_dev[4 f + 1] (consts_dev: (n_frames, 4) floats as ct_ingest_extrema_frames leaves them, 4-byte aligned, read when the
 * kernel runs).  For every frame the outputs are bit for bit those of ct_ingest_transform_data on that frame with its four
 * constants, ct_dark_field_blur on the result and ct_linearize_std on (xb, sigma_eff).  All nine taps of a sample's window take
 * the frame's own pair (the reflected border taps belong to the same frame).  No zero-range check happens here
 * (consts_dev[4 f + 1] == 0 divides by zero, as ct_ingest_transform_data does).
 * consts_dev NULL: ct_linearize_dark_ingest, which refuses that kind.  With constants, a second CT_INGEST_AFFINE_DATA stage and a
 * consts_dev not aligned to 4 bytes are CT_ERR_INVALID_ARGUMENT, checked with the stage list (in front of the model); constants
 * beside a chain without such a stage are not read.  Everything else, and every other refusal in its order, as
 * ct_linearize_dark_ingest: no row band (CT_ERR_UNSUPPORTED), no LOOKUP (CT_ERR_NO_GRADIENT_PATH).
 */
int ct_linearize_dark_ingest_data(const void *frames_dev, int32_t dtype, int64_t n_frames, const ct_geometry *geom,
                                  const ct_ingest_stage *stages, int32_t n_stages, const float *std_dev, int32_t std_mode,
                                  float std_value, const float *const *dark_devs, const float *const *dark_std_devs,
                                  float threshold, float alpha, const ct_icrf *icrf, float *lin_out_dev, float *std_out_dev,
                                  const float *consts_dev, void *stream);

/*
 * ct_hdr_merge_ingest_batch -- such a chain and one batch of compute_hdr_image's loop body in ONE pass over B raw frames:
 * state and outputs are bit for bit those of ct_ingest_transform (with consts_dev: ct_ingest_transform_data) into a dense
 * planar float32 (B, C, H_tile, W) stack followed by ct_hdr_merge_batch on that stack with CT_DTYPE_F32, the same geometry
 * with layout CT_LAYOUT_NCHW and the same flags,
 *   x = the stage list applied to (float)code (CT_INGEST_AFFINE / CT_INGEST_CLAMP, at most CT_INGEST_MAX_STAGES; n_stages = 0
 *       is the cast alone; with consts_dev non-NULL at most one CT_INGEST_AFFINE_DATA stage, whose sub and div are
 *       consts_dev[0..1] as ct_ingest_extrema left them, read when the kernel runs; without it that kind is
 *       CT_ERR_INVALID_ARGUMENT)
 *   then the closed-form merge of a float32 pixel x: LUT coordinate clamped with its gradient mask (x may lie below 0 or
 *       above 1 behind a chain), float32 moments about a per-pixel pivot, sigma = std_value (CONSTANT), std_value * x
 *       (MULTIPLIER, x behind the chain) or std_dev[...] (EXPLICIT)
 * without the float32 stack in between: B * sizeof(code) bytes read and 12 written per output element, where the two
 * launches move 8 B per sample more (4 written, 4 read again), and no (B, C, H_tile, W) float32 buffer exists.
 *   frames_dev   CT_DTYPE_U8 / U16 codes, aligned to their element (CT_DTYPE_F32 is CT_ERR_UNSUPPORTED: such a stack has no
 *                copy to save); geom->layout CT_LAYOUT_NCHW (any C) or, with C == 3, CT_LAYOUT_NHWC / NHWC_BGR: the order of
 *                the SOURCE (a folded CvToTorch); frames image_stride elements apart, exposures sorted as for ct_hdr_merge_batch
 *   geom         h_global / row_offset as for ct_hdr_merge_batch: a row band gives the same rows of the whole image
 *   std_dev      EXPLICIT: planar (B, C, H_tile, W) float32, dense, like the state -- not like the frames: gpu_transforms
 *                never touch the uncertainty images (as ct_linearize_ingest takes it)
 *   exposure_dev, icrf, weight_mode, state, outputs   as ct_hdr_merge_batch; state and outputs are planar (C, H_tile, W)
 *   flags        CT_MERGE_FIRST_BATCH, CT_MERGE_FINALIZE, CT_MERGE_MEAN_OUT_F32, CT_MERGE_CLOSED_FORM
 * CT_ERR_UNSUPPORTED: CT_MERGE_F64_MOMENTS, CT_MERGE_REFERENCE_ORDER, CT_MERGE_OUT_AS_INPUT, and every call that
 * ct_hdr_merge_batch would send to the reference-order kernel (LOOKUP / CATMULL with uncertainties and no
 * CT_MERGE_CLOSED_FORM: that kernel waits for its float64 arithmetic, not for its bytes); an interleaved layout with C != 3;
 * clamp pairs that differ between channels with C > CT_INGEST_MAX_CHANNELS.  CT_ERR_NO_GRADIENT_PATH and CT_ERR_TOO_LARGE as
 * ct_hdr_merge_batch.  Every argument is validated before anything touches the device; batch == 0 or an empty image is
 * CT_OK without a launch.  Allocates nothing, synchronises nothing, reads nothing back, never writes the frames, touches
 * nothing outside C*H_tile*W elements of the state and the outputs.
 */
int ct_hdr_merge_ingest_batch(const void *frames_dev, int32_t dtype, int32_t batch, const ct_geometry *geom,
                              const ct_ingest_stage *stages, int32_t n_stages, const float *consts_dev, const float *std_dev,
                              int32_t std_mode, float std_value, const double *exposure_dev, const ct_icrf *icrf,
                              int32_t weight_mode, double *mean_state_dev, float *sumw_state_dev, float *var_state_dev,
                              void *mean_out_dev, float *std_out_dev, uint32_t flags, void *stream);

/*
 * ct_hdr_merge_ingest_batches -- n_batches consecutive batches of one merge behind one chain in one call: exactly
 * ct_hdr_merge_ingest_batch applied to batch 0 .. n_batches - 1 in turn with the state carried along, bit for bit -- but where
 * it can, ONE launch walks all of them with (mean, sum of weights, variance) in registers in between: the state arrays are
 * read at most once (not at all with CT_MERGE_FIRST_BATCH) and written at most once, where a launch per batch reads 16 B and
 * writes 16 B per element and batch beside B * sizeof(code) bytes of samples.
 *   frames_devs, batch_sizes   HOST arrays of n_batches (1 .. 16) device pointers / batch sizes: batch b is batch_sizes[b]
 *                frames at frames_devs[b], each as ct_hdr_merge_ingest_batch takes it; one dtype, one geometry (image_stride
 *                included), one stage list for all of them.  A batch of size 0 is skipped.
 *   consts_devs  HOST array of n_batches device pointers, each the 4 floats ct_ingest_extrema left for that batch (read when
 *                the kernel runs), or NULL as a whole without a CT_INGEST_AFFINE_DATA stage
 *   std_devs     CT_STD_EXPLICIT: HOST array of n_batches device pointers, each planar (B_b, C, H_tile, W) float32; else
 *                NULL as a whole
 *   exposure_dev the exposure times of all batches, concatenated (sum of batch_sizes doubles)
 *   flags        as ct_hdr_merge_ingest_batch; CT_MERGE_FIRST_BATCH applies to the first and CT_MERGE_FINALIZE to the last
 *                batch that is not empty.  With more than one batch a state is required unless both are set.
 *                CT_MERGE_REQUIRE_ONE_LAUNCH: CT_ERR_UNSUPPORTED instead of one launch per batch.
 * n_batches outside 1 .. 16 is CT_ERR_INVALID_ARGUMENT; n_batches == 1 is ct_hdr_merge_ingest_batch.  Every batch is judged
 * as ct_hdr_merge_ingest_batch judges it (the same status codes, the first refusal wins) before anything touches the device.
 * One launch needs every batch, or none, to have constants, and the LUT with 8 B per exposure of ALL batches to fit 160 KiB
 * of LDS; otherwise the batches are launched one by one with the state in memory, which then must be given
 * (CT_ERR_INVALID_ARGUMENT without).  Allocates nothing, synchronises nothing, reads nothing back, never writes the frames,
 * touches nothing outside C*H_tile*W elements of the state and the outputs.
 */
int ct_hdr_merge_ingest_batches(const void *const *frames_devs, const int32_t *batch_sizes, int32_t n_batches, int32_t dtype,
                                const ct_geometry *geom, const ct_ingest_stage *stages, int32_t n_stages,
                                const float *const *consts_devs, const float *const *std_devs, int32_t std_mode, float std_value,
                                const double *exposure_dev, const ct_icrf *icrf, int32_t weight_mode, double *mean_state_dev,
                                float *sumw_state_dev, float *var_state_dev, void *mean_out_dev, float *std_out_dev,
                                uint32_t flags, void *stream);

/*
 * ct_hdr_merge_ingest_strided_batches -- StridedDownscale(step), such a chain and n_batches consecutive batches of one merge in
 * ONE pass over the RAW full-size frames: state and outputs are bit for bit those of ct_strided_downscale on every batch
 * followed by ct_hdr_merge_ingest_batches on the compacted frames, without the compacted copies.  With ho = ceil(H / step) and
 * wo = ceil(W / step), output element (c, i, j) reads row i * step, column j * step of plane c of every frame.
 *   geom         of the SOURCE frames (layout, H, W, image_stride) as ct_hdr_merge_ingest_batch takes it.  With step > 1 a row
 *                band (row_offset != 0 or h_tile != h_global) is CT_ERR_INVALID_ARGUMENT: which rows of a band a downscale
 *                selects depends on row_offset % step, a phase that is not carried
 *   step         >= 1, else CT_ERR_INVALID_ARGUMENT (tested first).  step == 1 is ct_hdr_merge_ingest_batches itself, row band
 *                included
 *   std_devs     CT_STD_EXPLICIT: each planar (B_b, C, ho, wo) float32, dense -- already of the OUTPUT shape: gpu_transforms are
 *                applied to the value images only
 *   consts_devs  as ct_hdr_merge_ingest_batches: per batch, computed by the caller on the frames as given (ct_ingest_extrema on
 *                the FULL batch: a Normalize in front of the downscale)
 *   state, outputs   planar (C, ho, wo)
 * The LINEAR / CATMULL LUT row is the flat NCHW index of the DOWNSCALED frame modulo C, (c * ho * wo + i * wo + j) % C.
 * With step > 1: the list is checked (n_batches outside 1 .. 16: CT_ERR_INVALID_ARGUMENT), then every batch is judged as
 * ct_hdr_merge_ingest_batch judges it ON THE SOURCE GEOMETRY, in its order (image_stride must hold a source frame), then for
 * the row band, before anything touches the device.  CT_DTYPE_F32, CT_MERGE_REFERENCE_ORDER, CT_MERGE_F64_MOMENTS,
 * CT_MERGE_OUT_AS_INPUT and the reference-order modes are CT_ERR_UNSUPPORTED as there.  One launch takes 1 .. 16 batches; the
 * conditions of one launch, the walk batch by batch with the state in memory otherwise and CT_MERGE_REQUIRE_ONE_LAUNCH are
 * those of ct_hdr_merge_ingest_batches.  Reads only selected elements of the frames, never writes them, touches nothing
 * outside C*ho*wo elements of the state and the outputs.
 */
int ct_hdr_merge_ingest_strided_batches(const void *const *frames_devs, const int32_t *batch_sizes, int32_t n_batches, int32_t dtype,
                                        const ct_geometry *geom, int32_t step, const ct_ingest_stage *stages, int32_t n_stages,
                                        const float *const *consts_devs, const float *const *std_devs, int32_t std_mode,
                                        float std_value, const double *exposure_dev, const ct_icrf *icrf, int32_t weight_mode,
                                        double *mean_state_dev, float *sumw_state_dev, float *var_state_dev, void *mean_out_dev,
                                        float *std_out_dev, uint32_t flags, void *stream);

/*
 * ct_hdr_merge_dark_ingest_batches -- n_batches consecutive dark-field batches of one merge behind one chain in one call, on
 * the RAW frames: for every batch the state and the outputs are bit for bit those of ct_ingest_transform (with constants:
 * ct_ingest_transform_data) into a dense planar float32 (B_b, C, H_tile, W) stack followed by ct_hdr_merge_dark_batch on that
 * stack with CT_DTYPE_F32, the same dark fields, uncertainties, halo, geometry (layout CT_LAYOUT_NCHW) and flags, batch 0 ..
 * n_batches - 1 in turn on the same state -- without the float32 stack: sizeof(element) + 8 bytes read per sample (+ 4 with
 * explicit image uncertainties), 10 for uint16 where the two launches move 18; with one shared dark field per batch about 2
 * against about 10.  Where it can, ONE launch walks all batches with (mean, sum of weights, variance) in registers in between:
 * the state arrays are read at most once (not at all with CT_MERGE_FIRST_BATCH) and written at most once.  n_batches == 1 is
 * the same kernel with a list of one.
 *   frames_devs, batch_sizes   HOST arrays of n_batches (1 .. 16) entries: batch b is batch_sizes[b] >= 1 raw frames at
 *                frames_devs[b], CT_DTYPE_U8 / U16 / F32, aligned to their element; geom->layout CT_LAYOUT_NCHW (any C) or,
 *                with C == 3, CT_LAYOUT_NHWC / NHWC_BGR: raw (B, H, W, 3) frames (BGR: memory channel cm feeds plane 2 - cm);
 *                geom->image_stride elements between frames; one dtype, geometry and stage list for all batches
 *   geom         a row band (h_tile < h_global) with CT_LAYOUT_NCHW only; CT_ERR_UNSUPPORTED on interleaved frames
 *   stages       0 to CT_INGEST_MAX_STAGES of CT_INGEST_AFFINE / CT_INGEST_CLAMP and, with consts_devs, at most one
 *                CT_INGEST_AFFINE_DATA.  Every tap of the 3 x 3 window goes through the chain with its PLANE channel.  No
 *                StridedDownscale: the caller compacts first
 *   consts_devs  HOST array of n_batches device pointers, each the 4 floats ct_ingest_extrema left for that batch (sub and div
 *                are read when the kernel runs), or NULL as a whole; its entries are all NULL or all non-NULL
 *   halo_devs    HOST array of n_batches device pointers, each the (B_b, C, 2, W) RAW rows of the frames' dtype just above and
 *                below the band (they go through the chain like any other tap), or NULL as a whole; all NULL or all non-NULL
 *   std_devs / std_mode / std_value   sigma of the image BEHIND the chain, as ct_dark_field_blur takes it on the float32 stack
 *                (EXPLICIT: HOST array of n_batches device pointers, each planar (B_b, C, H_tile, W) float32, dense, whatever
 *                the layout of the frames; else NULL as a whole; CT_STD_MULTIPLIER multiplies x behind the chain, not xb)
 *   dark_devs, dark_std_devs, dark_batches   as ct_hdr_merge_dark_batches takes them: planar (1 | B_b, C, H_tile, W) float32 in
 *                plane (RGB) order; shared and per-frame dark fields may alternate between the batches of one call;
 *                dark_std_devs NULL as a whole, or all entries NULL: no uncertainty is propagated
 *   exposure_dev the exposure times of all batches, concatenated (sum of batch_sizes doubles)
 *   icrf, weight_mode, state, outputs   as ct_hdr_merge_dark_batch; state and outputs are planar (C, H_tile, W)
 *   flags        CT_MERGE_FIRST_BATCH (of batch 0), CT_MERGE_FINALIZE (of the last batch), CT_MERGE_MEAN_OUT_F32,
 *                CT_MERGE_CLOSED_FORM; CT_MERGE_REQUIRE_ONE_LAUNCH: CT_ERR_TOO_LARGE instead of one launch per batch
 * Status, in this order: n_batches outside 1 .. 16 or a missing array / geometry: CT_ERR_INVALID_ARGUMENT; a mixture of NULL
 * and non-NULL entries in dark_std_devs, halo_devs or consts_devs: CT_ERR_INVALID_ARGUMENT; the stage list as
 * ct_ingest_transform judges it (an unknown dtype, layout or kind, more than CT_INGEST_MAX_STAGES, a CT_INGEST_AFFINE_DATA
 * stage without consts_devs, more than one of them: CT_ERR_INVALID_ARGUMENT; an interleaved layout with C != 3, per-channel
 * clamp pairs with C > CT_INGEST_MAX_CHANNELS: CT_ERR_UNSUPPORTED); a row band on interleaved frames: CT_ERR_UNSUPPORTED; then
 * every batch as ct_hdr_merge_dark_batch judges the float32 stack (its checks in its order, the same status codes, the first
 * refusal wins -- width < 2, h_global < 2, a one-row band at the image's edge, a band without its halo, CT_MERGE_REFERENCE_ORDER,
 * LOOKUP / CATMULL with a dark std and no CT_MERGE_CLOSED_FORM, ... -- the flags being those of the whole call, so a state is
 * needed unless both FIRST_BATCH and FINALIZE are set) and its constants' alignment.  One launch needs the LUT with 8 B per
 * exposure of ALL batches to fit 160 KiB of LDS; where only each batch alone fits, the batches are launched one by one on the
 * state in memory, which then must be given (CT_ERR_UNSUPPORTED without; CT_ERR_TOO_LARGE with CT_MERGE_REQUIRE_ONE_LAUNCH).
 * Every argument is validated before anything touches the device.  Allocates nothing, synchronises nothing, reads nothing
 * back, never writes the frames, the dark fields or the uncertainties, touches nothing outside C*H_tile*W elements of the
 * state and the outputs.
 */
int ct_hdr_merge_dark_ingest_batches(const void *const *frames_devs, const int32_t *batch_sizes, int32_t n_batches, int32_t dtype,
                                     const ct_geometry *geom, const ct_ingest_stage *stages, int32_t n_stages,
                                     const float *const *consts_devs, const void *const *halo_devs, const float *const *std_devs,
                                     int32_t std_mode, float std_value, const float *const *dark_devs,
                                     const float *const *dark_std_devs, const int32_t *dark_batches, float threshold, float alpha,
                                     const double *exposure_dev, const ct_icrf *icrf, int32_t weight_mode, double *mean_state_dev,
                                     float *sumw_state_dev, float *var_state_dev, void *mean_out_dev, float *std_out_dev,
                                     uint32_t flags, void *stream);

/*
 * ct_video_stats_ingest_batch -- such a chain and one batch of compute_video_mean_and_std's loop body in ONE pass over B raw
 * frames: the state is bit for bit that of ct_ingest_transform (with consts_dev: ct_ingest_transform_data) into a dense
 * planar float32 (B, C, H_tile, W) stack followed by ct_video_stats_batch on that stack with CT_DTYPE_F32 and the same
 * geometry with layout CT_LAYOUT_NCHW,
 *   x = the stage list applied to (float)code (CT_INGEST_AFFINE / CT_INGEST_CLAMP, at most CT_INGEST_MAX_STAGES; n_stages = 0
 *       is the cast alone; with consts_dev non-NULL at most one CT_INGEST_AFFINE_DATA stage, whose sub and div are
 *       consts_dev[0..1] as ct_ingest_extrema left them, read when the kernel runs; without it that kind is
 *       CT_ERR_INVALID_ARGUMENT)
 *   then the optional ICRF of a float32 pixel x (LUT coordinate clamped on both sides: x may lie below 0 or above 1 behind a
 *       chain) and the unweighted WBOMeanVar update in ct_video_stats_batch's order of operations
 * without the float32 stack in between: sizeof(code) bytes read per sample, where the two launches move 8 B per sample more
 * (4 written, 4 read again), and no (B, C, H_tile, W) float32 buffer exists.  The state traffic, 16 B per element and
 * batch, is the same.
 *   frames_dev   CT_DTYPE_U8 / U16 codes, aligned to their element and no further (CT_DTYPE_F32 is CT_ERR_UNSUPPORTED: such a
 *                stack has no copy to save); geom->layout CT_LAYOUT_NCHW (any C) or, with C == 3, CT_LAYOUT_NHWC / NHWC_BGR:
 *                the order of the SOURCE (a folded CvToTorch); frames image_stride elements apart
 *   geom         h_global / row_offset as for ct_video_stats_batch: a row band gives the same rows of the whole image (the
 *                LINEAR / CATMULL LUT row is the global flat NCHW index modulo C, the LOOKUP row the channel)
 *   frames_before, mean_state_dev, m2_state_dev   as ct_video_stats_batch: planar (C, H_tile, W) float32, updated in place,
 *                aligned to 4 bytes (an interior slice of a larger buffer is fine)
 * CT_ERR_UNSUPPORTED: an interleaved layout with C != 3; clamp pairs that differ between channels with
 * C > CT_INGEST_MAX_CHANNELS.  CT_ERR_TOO_LARGE: C * H_global * W >= 2^31, a LUT beyond the 160 KB of LDS, more than 65535
 * planar channels.  Every argument is validated before anything touches the device; batch == 0 or an empty image is CT_OK
 * without a launch.  Allocates nothing, synchronises nothing, reads nothing back, never writes the frames, touches nothing
 * outside C*H_tile*W elements of the state.
 */
int ct_video_stats_ingest_batch(const void *frames_dev, int32_t dtype, int32_t batch, const ct_geometry *geom,
                                const ct_ingest_stage *stages, int32_t n_stages, const float *consts_dev,
                                const ct_icrf *icrf, float frames_before, float *mean_state_dev, float *m2_state_dev,
                                void *stream);

/*
 * ct_video_stats_batches / ct_video_stats_ingest_batches -- n_batches consecutive batches of one video in one call: exactly
 * ct_video_stats_batch / ct_video_stats_ingest_batch applied to batch 0 .. n_batches - 1 in turn, bit for bit in mean_state
 * and m2_state -- but where it can, ONE launch walks all of them with (mean, m2) in registers in between: the state arrays are
 * read at most once (not at all with frames_before == 0) and written once, where a launch per batch reads 8 B and writes 8 B
 * per element and batch beside B * sizeof(code) bytes of samples (at the reference's batch_size of 4: 80 % of the traffic of
 * uint8 frames, 67 % of uint16 frames).
 *   frames_devs, batch_sizes   HOST arrays of n_batches (1 .. CT_STATS_MAX_BATCHES) device pointers / batch sizes, read during
 *                the call: batch b is batch_sizes[b] frames at frames_devs[b], each as the single-batch entry point takes it.
 *                The batches may be separate allocations; they share one dtype, one geometry (image_stride included), one
 *                layout and one stage list.  A batch of size 0 is skipped (a negative size is CT_ERR_INVALID_ARGUMENT).
 *   consts_devs  HOST array of n_batches device pointers, each the 4 floats ct_ingest_extrema left for that batch (its own
 *                data-dependent Normalize constants, read when the kernel runs), or NULL as a whole
 *   frames_before   the frames merged before batch 0.  Batch b is merged into a state of frames_before plus the sizes of the
 *                batches in front of it: the float of that exact integer count, formed on the host -- what a caller of the
 *                single-batch entry point would pass -- and handed to the kernel by value; nothing is summed in float32 on the
 *                device.
 *   flags        CT_STATS_REQUIRE_ONE_LAUNCH: CT_ERR_UNSUPPORTED instead of one launch per batch.
 * n_batches outside 1 .. 16 is CT_ERR_INVALID_ARGUMENT; n_batches == 1 is the single-batch entry point (flags ignored; one
 * batch of size 0 is CT_OK for both).  Every batch is judged as the single-batch entry point judges it (the same status
 * codes, the first refusal wins; an empty batch needs neither its frames nor the state) before anything touches the device.
 * If all batches are empty, or the image of the ingest form is, the call is CT_OK without a launch.
 * One pass: where every non-empty batch has at most 32 frames (the register-cached walks, BMAX 16 / 32 chosen from the
 * largest batch) and, for the ingest form, every batch or none has constants, one launch walks all batches -- plus the scalar
 * launch for heads and tails the single-batch entry points have.  Each thread owns the same elements for every batch, each
 * frame byte is read once.  ct_video_stats_batches reads the frames as 4-element packets only where EVERY batch is aligned
 * to them (and the state to 16 bytes); a misaligned frame pointer in any batch sends all batches down the element-wise form,
 * which gives the same bits.  The ingest form reads codes at any alignment, as ct_video_stats_ingest_batch does.
 * Fallback: a batch of more than 32 frames, or batches with and without constants mixed, run one launch per batch through the
 * single-batch kernels; with CT_STATS_REQUIRE_ONE_LAUNCH that is CT_ERR_UNSUPPORTED and nothing is launched.
 * Allocates nothing, synchronises nothing, reads nothing back, never writes the frames, touches nothing outside C*H_tile*W
 * elements of the two state arrays.
 */
int ct_video_stats_batches(const void *const *frames_devs, const int32_t *batch_sizes, int32_t n_batches, int32_t dtype,
                           float max_code, const ct_geometry *geom, const ct_icrf *icrf, float frames_before,
                           float *mean_state_dev, float *m2_state_dev, uint32_t flags, void *stream);
int ct_video_stats_ingest_batches(const void *const *frames_devs, const int32_t *batch_sizes, int32_t n_batches, int32_t dtype,
                                  const ct_geometry *geom, const ct_ingest_stage *stages, int32_t n_stages,
                                  const float *const *consts_devs, const ct_icrf *icrf, float frames_before,
                                  float *mean_state_dev, float *m2_state_dev, uint32_t flags, void *stream);

/*
 * ct_pair_residual_ingest_fwd / ct_pair_residual_ingest_bwd -- such a chain and ct_pair_residual_fwd / _bwd in ONE pass over
 * N raw frames: the sums (the LUT gradient) are those of ct_ingest_transform (with consts_dev: ct_ingest_transform_data) into
 * a dense planar float32 (N, C, H_tile, W) stack followed by ct_pair_residual_fwd (_bwd) on that stack with CT_DTYPE_F32 and
 * the same geometry with layout CT_LAYOUT_NCHW.  Every staged sample has the bits of that route -- x = the stage list applied
 * to (float)code, then the ICRF of a float32 pixel (LUT coordinate clamped on both sides), the Gaussian weight, the validity
 * mask lower <= x <= upper and sigma (CT_STD_CONSTANT / MULTIPLIER on x) -- and for contiguous allocations of one shape the
 * tiles are walked alike, so the results differ by the order of the float64 atomic additions alone.  No float32 stack exists:
 * sizeof(code) bytes are read per sample and launch where the float32 stack costs 4, and the ct_ingest_transform pass
 * (sizeof(code) read, 4 written per sample) is gone.
 *   frames_dev   CT_DTYPE_U8 / U16 codes aligned to their element (CT_DTYPE_F32 is CT_ERR_UNSUPPORTED: such a stack has no
 *                copy to save); geom->layout CT_LAYOUT_NCHW (any C) or, with C == 3, CT_LAYOUT_NHWC / NHWC_BGR: the order of
 *                the SOURCE (a folded CvToTorch); frames image_stride elements apart
 *   stages, n_stages, consts_dev   as ct_video_stats_ingest_batch takes them (at most one CT_INGEST_AFFINE_DATA stage, and
 *                only with consts_dev, whose first two floats are read when the kernel runs)
 *   std_dev      CT_STD_EXPLICIT: PLANAR float32 (N, C, H_tile, W), dense, whatever the layout of the frames (gpu_transforms
 *                never touch the uncertainty images); else NULL
 *   every other argument as ct_pair_residual_fwd / ct_pair_residual_bwd take it; the backward's workspace is that of
 *   ct_pair_residual_bwd_workspace.
 * Validation needs no device memory and comes first: the geometry, the stack and the stage list, the dtype, the constants'
 * alignment and the model as ct_video_stats_ingest_batch judges them, then everything ct_pair_residual_fwd / _bwd refuse
 * (n_images < 2, an empty plane, CT_INTERP_LOOKUP with a std mode: CT_ERR_NO_GRADIENT_PATH, ...).  Allocates nothing,
 * synchronises nothing, reads nothing back, never writes the frames.
 */
int ct_pair_residual_ingest_fwd(const void *frames_dev, int32_t dtype, const ct_ingest_stage *stages, int32_t n_stages,
                                const float *consts_dev, int32_t n_images, const ct_geometry *geom, const float *std_dev,
                                const ct_icrf *icrf, const int32_t *i_idx_dev, const int32_t *j_idx_dev, const double *ratio_dev,
                                int32_t n_pairs, const ct_pair_params *params, int32_t level, const double *center_dev,
                                double *sums_dev, void *stream);
int ct_pair_residual_ingest_bwd(const void *frames_dev, int32_t dtype, const ct_ingest_stage *stages, int32_t n_stages,
                                const float *consts_dev, int32_t n_images, const ct_geometry *geom, const float *std_dev,
                                const ct_icrf *icrf, const double *ratio_dev, int32_t n_pairs,
                                const int32_t *partner_offsets_dev, const int32_t *partner_sample_dev,
                                const int32_t *partner_pair_dev, const ct_pair_params *params, const double *coef_dev,
                                const double *smean_dev, double *lut_grad_dev, void *workspace_dev, int64_t workspace_bytes,
                                void *stream);

/*
 * ct_export_cv -- the array save_image hands to cv.imwrite (clair_torch/common/data_io.py:228-234: astype, transpose to
 * (H, W, C), channel reversal of a 3-channel image), made on the device from planar results:
 *   dst[f][p][c'] = (dst type) src[f][c][p],  p < plane = H*W,  c' = channels-1-c when reverse_channels, else c
 *   src_dev (n_images, channels, plane), dst_dev (n_images, plane, channels), float32 or float64 each (*_is_f64), dense,
 *   aligned to their element only (an interior slice of a larger buffer is fine).
 * Casts round to nearest even and keep subnormals (float64 -> float32 as numpy's astype); the same type is a bit copy.
 * Touches nothing outside n_images*channels*plane elements of either side; an empty input is CT_OK without a launch.
 */
int ct_export_cv(const void *src_dev, int32_t src_is_f64, void *dst_dev, int32_t dst_is_f64, int64_t n_images,
                 int32_t channels, int64_t plane, int32_t reverse_channels, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CLAIR_HIP_H */
