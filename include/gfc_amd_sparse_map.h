/* Ground-truth labels from Endomapper sparse maps: the C entries of csrc/gt_sparse_map.hip, exported by libgfc_amd.so
 * and written in the grammar of gfc_amd.h (glue-factory-colon_amd/_native.py parses all three headers).  A header of
 * its own because the suite pins the function lists of gfc_amd.h and gfc_amd_validation.h; it declares functions only
 * and takes its types from gfc_amd.h. */
#ifndef GFC_AMD_SPARSE_MAP_H
#define GFC_AMD_SPARSE_MAP_H

#include "gfc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The matching part of gt_matches_from_pose_sparse_map and gt_matches_from_pose_sparse_dense_map (gluefactory/geometry/
 * gt_generation.py:441-591 and 271-438) from projections that exist (gfc_gt_project_depth).
 * kp0 [B,M,2], kp1 [B,N,2], proj_0to1 [B,M,2], proj_1to0 [B,N,2]; visible0/1 mask the distance, valid0/1 (valid depth)
 * say who may be `negative`; ids0 [B,M], ids1 [B,N] int64 (both NULL: no id seeding, use_gt_pos false or the
 * sparse-dense function) with valid3d0/1 (each NULL: all valid); F [B,3,3] as gfc_gt_matches_depth takes it.
 * pos_th, neg_th, epi_th: a value < 0 means None.  The reference's order of decisions is the contract:
 *  1. m0 = m1 = -2 (:467-468).
 *  2. ids given (:488-500): positive_gt[i,j] = ids0[i] == ids1[j] && valid3d0[i] && valid3d1[j]; m0[i] = the LOWEST such
 *     j, m1[j] the lowest such i (argmax of a 0/1 row); mask_pos_3d_map = positive_gt.any.  Duplicate ids are legal.
 *  3. dist = max(dist0, dist1), +inf outside visible0 x visible1 (:511-518); arg-min as torch.min: the first index wins
 *     a tie and a row of +inf has arg-min 0 -- however the columns of a row are split over lanes, tiles, workgroups.
 *  4. pos_th set (:520-530): positive_dist = mutual arg-min and dist < pos_th^2; mask_pos_reproj = positive_dist.any;
 *     m0[i] = min0[i] only where m0[i] is still -2: a seed wins.
 *  5. neg_th set (:532-538): negative0 = (min_j dist0 > neg_th^2) & valid0 on the UNMASKED one-way distance;
 *     mask_neg_reproj = negative0; m0[i] = -1 only where it is still -2: a positive is NOT overridden (unlike
 *     gfc_gt_matches_depth).
 *  6. epi_th set (:549-557): exclude0 = (min over (m0 == -2) x (m1 == -2) of the symmetric epipolar distance, never
 *     stored) > epi_th; mask_neg_epi = exclude0 for EVERY point; m0[i] = -1 where exclude0 & !valid0 & m0 == -2.
 *     Without epi_th mask_neg_epi is zero.
 *  7. dense (:559-568): assignment = positive_gt | positive_dist; reward = max(dist < pos_th^2, assignment) - penalty,
 *     penalty = (epi > epi_val), epi_val = epi_th, else neg_th, else no penalty; with epi_th set epi is +inf outside
 *     ignore x ignore of the state BEFORE step 6.
 * F is required with epi_th set, and with reward when epi_th or neg_th is set (GFC_ERR_INVALID otherwise).
 * Outputs: matches0 [B,M], matches1 [B,N] int64; masks0 [B,4,M], masks1 [B,4,N] uint8 (nullable), rows pos_3d_map,
 * pos_reproj, neg_reproj, neg_epi; positive0 [B,M] int32 (nullable): the column of the row's distance positive, -1 for
 * none; extra_positives [B] int32 (nullable): the number of (i, j) with assignment true and matches0[i] != j -- the
 * positives a loss that sees only matches0 loses -- computed without the dense matrix: per row |S_i u {p_i}| - 1 when
 * that set is not empty, S_i the id-equal valid columns counted in the id sweep, p_i the distance positive;
 * assignment [B,M,N] uint8 and reward [B,M,N] float (each nullable).
 * M == 0 or N == 0: no kernel; matches and positive0 of the other side are -1, masks and extra_positives 0 (the dict of
 * the sparse-dense function, :282-314; the early return of the sparse-map function, :453-461, returns a tuple its
 * caller cannot use).
 * Launch plan.  A pair is split over workgroups of 256 threads; nothing waits for another workgroup.
 *  sweep   grid (ceil(M/16) + ceil(N/16), B): a workgroup owns 16 key points of one side, 16 lanes each, and streams the
 *          other side through LDS in tiles of 256 elements (float4 of coordinates, flag byte, 8-byte id).  Lane l takes
 *          elements l, l + 16, ... of every tile in ascending order; the 16 lanes are reduced on (distance, index), the
 *          lower index winning equal distances.  Per key point into the workspace: masked minimum and arg-min, unmasked
 *          one-way minimum, first id partner and their count.  One 2048 + 2048 pair: 128 + 128 = 256 workgroups.
 *  finish  grid (ceil((M+N)/256), B): steps 2-5 per key point, positive0, extra_positives, the `ignore` state.
 *  epi     (epi_th set) gridded as the sweep: step 6.
 *  dense   (assignment or reward) grid (ceil(N/256), M, B), one thread per element.
 * No LDS-derived size limit: B, M, N <= 65535 (GFC_ERR_INVALID otherwise) and GFC_ERR_WORKSPACE (nothing launched)
 * when workspace_bytes < gfc_gt_matches_sparse_map_workspace_bytes(B, M, N) = about 24 B (M + N) bytes, 0 for an empty
 * side or invalid sizes. */
size_t gfc_gt_matches_sparse_map_workspace_bytes(int B, int M, int N);
int gfc_gt_matches_sparse_map(const float* kp0, const float* kp1, const float* proj_0to1, const float* proj_1to0,
                              const uint8_t* visible0, const uint8_t* visible1, const uint8_t* valid0,
                              const uint8_t* valid1, const int64_t* ids0, const int64_t* ids1, const uint8_t* valid3d0,
                              const uint8_t* valid3d1, const float* F, int B, int M, int N, double pos_th, double neg_th,
                              double epi_th, int64_t* matches0, int64_t* matches1, uint8_t* masks0, uint8_t* masks1,
                              int32_t* positive0, int32_t* extra_positives, uint8_t* assignment, float* reward,
                              void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GFC_AMD_SPARSE_MAP_H */
