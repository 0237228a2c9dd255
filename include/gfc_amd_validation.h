/* Validation pass (ground-truth matches, NLL loss, matcher metrics): the C entries of csrc/gt_matches.hip and
 * csrc/lg_validation.hip, exported by libgfc_amd.so like those of gfc_amd.h and written in the same grammar
 * (glue-factory-colon_amd/_native.py parses both).  They are in a header of their own for one reason: the suite pins
 * the number of functions gfc_amd.h declares (tests/test_native_binding_host.py), and existing tests are not edited. */
#ifndef GFC_AMD_VALIDATION_H
#define GFC_AMD_VALIDATION_H

#include "gfc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ground-truth matches from a homography for the validation pass: gt_matches_from_homography (gluefactory/geometry/
 * gt_generation.py:730-801) in full.  kp0 [B,M,2], kp1 [B,N,2], H / Hinv [B,3,3] as gfc_eval_matches_homography takes them; valid0 [B,M], valid1 [B,N]
 * (nullable: all valid) mask the distance to +inf outside valid0 x valid1; pos_th and neg_th are independent.
 * matches0 [B,M], matches1 [B,N] int64 (-1 unmatched, -2 ignore), proj_0to1 [B,M,2], proj_1to0 [B,N,2].  The
 * reference's order of decisions: arg-min of the MASKED distance (ties to the first index, a row of +inf has arg-min 0
 * and is not positive), `negative` from the UNMASKED one-way minimum ANDed with valid, negative overrides positive.
 * positive0 (nullable) [B,M] int32: the column of the row's positive assignment BEFORE that override, -1 for none --
 * the sparse form of `assignment`.  assignment [B,M,N] uint8 and reward [B,M,N] float32 (each nullable; assignment
 * needs positive0) are written by a second launch gridded over rows and column blocks.
 * One workgroup per pair with all its key points in LDS, no M x N matrix for the sparse outputs:
 * gfc_gt_matches_homography_lds_bytes(M, N) = 21 (M + N), no static LDS; GFC_ERR_UNSUPPORTED (nothing launched) exactly
 * when that exceeds 160 KB (163840 bytes): M + N <= 7801 is admitted, 3901 x 3901 is the first square shape refused.
 * B, M <= 65535 (GFC_ERR_INVALID otherwise).  M == 0 or N == 0 is the reference's early return: no kernel is launched,
 * the matches (and positive0) of the other side are set to -1, nothing else is written (the pointers of an empty side
 * may be NULL). */
size_t gfc_gt_matches_homography_lds_bytes(int M, int N);
int gfc_gt_matches_homography(const float* kp0, const float* kp1, const float* H, const float* Hinv,
                              const uint8_t* valid0, const uint8_t* valid1, int B, int M, int N, double pos_th,
                              double neg_th, int64_t* matches0, int64_t* matches1, float* proj_0to1, float* proj_1to0,
                              int32_t* positive0, uint8_t* assignment, float* reward, void* stream);

/* The matching part of gt_matches_from_pose_depth (geometry/gt_generation.py:666-727) from projections that exist:
 * proj_0to1 [B,M,2], proj_1to0 [B,N,2], visible0/1 (the mask of the distance) and valid0/1 (valid depth: who may be
 * `negative`), all from gfc_eval_pose_project (depth sampled from the maps) or gfc_gt_project_depth (depth given).
 * Same kernel, same order of decisions, same LDS account (gfc_gt_matches_homography_lds_bytes) and the same
 * positive0 / assignment / reward outputs as gfc_gt_matches_homography.  epi_th >= 0 adds the reference's th_epi rule
 * (gt_generation.py:705-712): a point without valid depth becomes unmatched when its smallest symmetric epipolar
 * distance (sym_epipolar_distance_all, geometry/epipolar.py:59-72) to the `ignore` points of the other image exceeds
 * epi_th -- a row / column minimum over ignore x ignore that is never stored; epi_th < 0: no such rule.
 * F [B,3,3] (needed with epi_th >= 0 or reward) = K1^-T [t]x R K0^-1 from the pinhole calibration matrices.
 * reward = (dist < pos_th^2) - (epi > epi_th), epi +inf outside ignore x ignore (the matches BEFORE the rule), or
 * without epi_th (dist < pos_th^2) - (epi > neg_th) on the unmasked epi, as the reference writes it. */
int gfc_gt_matches_depth(const float* kp0, const float* kp1, const float* proj_0to1, const float* proj_1to0,
                         const uint8_t* visible0, const uint8_t* visible1, const uint8_t* valid0, const uint8_t* valid1,
                         const float* F, int B, int M, int N, double pos_th, double neg_th, double epi_th,
                         int64_t* matches0, int64_t* matches1, int32_t* positive0, uint8_t* assignment, float* reward,
                         void* stream);

/* project() of the reference (geometry/depth.py, ccth = None) for key points whose depth is given -- the cached
 * depth_keypoints input of the depth matcher: kp [B,K,2], depth_kp [B,K], valid [B,K]; cameras float[10] and pose
 * float[12] per pair as gfc_eval_pose_project takes them -> proj [B,K,2], visible [B,K]. */
int gfc_gt_project_depth(const float* kp, const float* depth_kp, const uint8_t* valid, const float* cam_i, int model_i,
                         const float* cam_j, int model_j, const float* T_itoj, int B, int K, float* proj,
                         uint8_t* visible, void* stream);

/* Validation loss and matcher metrics of B equal-sized pairs in one launch (one workgroup per pair): NLLLoss.forward
 * (gluefactory/models/utils/losses.py:6-73), row_norm (models/matchers/lightglue.py:606) and matcher_metrics
 * (models/utils/metrics.py:4-50).  log_assignment [B,M+1,N+1]; gt_matches0 [B,M], gt_matches1 [B,N] int64;
 * gt_assignment (nullable) [B,M,N] uint8: without it the positives are la[i, gt_matches0[i]] where that is > -1;
 * matches0 [B,M] int64 and matching_scores0 [B,M]: the prediction.  out [B,10] = nll_pos, nll_neg, num_matchable,
 * num_unmatchable, assignment_nll, row_norm, match_recall, match_precision, accuracy, average_precision.
 * The weight matrix of nll_loss is never built; sums are fp64, every output is rounded to fp32 once; exp is fp32 (1 ulp).
 * average_precision = p_last (r_last - r_first), what ranking_ap sums to; r_first belongs to the top score, the lowest
 * index among equal maxima. */
int gfc_lg_validation_metrics(const float* log_assignment, const int64_t* gt_matches0, const int64_t* gt_matches1,
                              const uint8_t* gt_assignment, const int64_t* matches0, const float* matching_scores0, int B,
                              int M, int N, float nll_balancing, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GFC_AMD_VALIDATION_H */
