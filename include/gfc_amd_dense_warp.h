/* Ground-truth labels from dense warps (RoMa): the C entries of csrc/gt_dense_warp.hip, exported by libgfc_amd.so and
 * written in the grammar of gfc_amd.h (glue-factory-colon_amd/_native.py parses all four headers).  A header of its own
 * because the suite pins the function lists of the other three; it declares functions only and takes its types from
 * gfc_amd.h.  The network that produces the warps is not part of this library: everything here starts from its output,
 * channel-last float32 fields of NORMALISED coordinates (warp [B,H,W,2]) and a certainty [B,H,W] per direction. */
#ifndef GFC_AMD_DENSE_WARP_H
#define GFC_AMD_DENSE_WARP_H

#include "gfc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The sampling rule of all three entries is F.grid_sample(mode bilinear, padding zeros, align_corners False) on a field
 * of size h x w at a normalised position (cx, cy): ix = ((cx + 1) * w - 1) / 2, iy alike with h; taps at x0 = floor(ix),
 * x0 + 1, y0 = floor(iy), y0 + 1 with weights (x1 - ix)(y1 - iy), (ix - x0)(y1 - iy), (x1 - ix)(iy - y0),
 * (ix - x0)(iy - y0), summed in that order from 0.  Every tap INSIDE the field is multiplied through, a zero weight
 * included, so a NaN or inf tap makes the sample NaN as in torch; a tap outside adds nothing.  A position that is not
 * finite gives NaN.  A warp is read as one float2 per pixel: its pointer must be 8-byte aligned (GFC_ERR_INVALID otherwise).
 *
 * gfc_dense_cycle_error: cycle_dist(q_to_ref, ref_to_q, normalized=False) (gluefactory/utils/image.py:260-270) on
 * channel-last fields, without the transposed copy of :264.  q_to_ref [B,H,W,2], ref_to_q [B,Hr,Wr,2], out [B,H,W].
 * Per pixel (x, y):
 *  1. sample ref_to_q at q_to_ref[y, x] by the rule above on Hr x Wr (:264);
 *  2. denormalize_coords with hw = None (:240-247), which reads the size off the SAMPLED tensor -- that has the shape of
 *     q_to_ref, not of ref_to_q: (c + 1) / 2 * (W - 1), (H - 1);
 *  3. subtract it from the pixel grid (x + 0.5, y + 0.5) of get_pixel_grid (:187-227), Euclidean norm (:266).
 * The grid has the half pixel and the de-normalisation has not: that is the reference's and is restated, not repaired.
 * One thread per pixel, grid (ceil(H W / 256), B).  B <= 65535, H, W, Hr, Wr in 1..32768 (GFC_ERR_INVALID otherwise).
 *
 * gfc_gt_sample_dense_warp: sample_dense of gluefactory/geometry/gt_generation.py:127-134 for one direction.  kp [B,M,2]
 * in pixels of the query image (q_h, q_w); warp [B,H,W,2], certainty [B,H,W], cycle_error [B,H,W] (nullable), other_warp
 * [B,Hr,Wr,2] (nullable; Hr, Wr ignored when it is NULL); the target image is (t_h, t_w).  Per key point:
 *  1. normalize_coords with the IMAGE size (:250-257): x / (q_w - 1) * 2 - 1, in that order of operations;
 *  2. the rule above on the FIELD's size H x W, for the two channels of the warp, the certainty and the cycle error;
 *  3. proj = denormalize_coords of the sampled warp with the target image's size: (c + 1) / 2 * (t_w - 1), (t_h - 1).
 * cycle_kp: with cycle_error given it is sampled like the certainty; with cycle_error NULL and other_warp given the
 * cycle error of each inside tap pixel is computed by the device function of gfc_dense_cycle_error (q_to_ref = warp,
 * ref_to_q = other_warp) and combined by the same code, bit-equal to calling that entry and sampling its output (the
 * library is built without contraction); with both NULL it is 0.
 * Outputs proj [B,M,2], certainty_kp [B,M], cycle_kp [B,M].  One thread per key point, grid (ceil(M / 256), B).
 * M == 0: nothing is launched.  B, M <= 65535, field sides as above, image sides >= 1 (GFC_ERR_INVALID otherwise).
 *
 * gfc_gt_matches_roma: the label part of gt_matches_from_roma (gt_generation.py:149-269).  kp0 [B,M,2], kp1 [B,N,2],
 * proj_0to1 [B,M,2], proj_1to0 [B,N,2], certainty_kp0/1 and cycle_kp0/1 [B,M] / [B,N], valid0/1 uint8.  pos_th and
 * neg_th are required (>= 0); pos_cert_th, pos_cycle_error_th, neg_cert_th, neg_cycle_error_th: a value < 0 means None.
 * A threshold is compared as the reference compares a float32 tensor with a Python double: rounded once to float32,
 * the squares of pos_th and neg_th squared in double first.  Inequalities are strict as written there.
 *  1. valid_pos = valid & finite proj (both coordinates) & finite certainty (:149-157); pos_cert_th set: & certainty >
 *     pos_cert_th (:158-160); pos_cycle_error_th set: & finite cycle & cycle < pos_cycle_error_th (:161-163).
 *  2. dist = max(dist0, dist1), +inf outside valid_pos0 x valid_pos1 (:165-170); arg-min as torch.min (:178-179): the
 *     first index wins a tie and a row of +inf has arg-min 0 -- however a row is split over lanes, tiles, workgroups.
 *  3. positive = mutual arg-min & dist < pos_th^2 (:180-187); m0/m1 take the arg-min there, -2 elsewhere.
 *  4. neg_far0 = valid_pos0 & (min over the valid_pos1 columns of the ONE-WAY dist0) > neg_th^2 (:195-198); a row with
 *     no valid column is +inf, hence far.  neg_far1 alike with dist1 over the valid_pos0 rows.
 *  5. neg_unreliable, only when BOTH neg_cert_th and neg_cycle_error_th are set (:202-216): valid (not valid_pos) &
 *     finite certainty & finite cycle & certainty < neg_cert_th & cycle > neg_cycle_error_th; otherwise zero.
 *  6. neg = (neg_far | neg_unreliable) & ~positive, m = -1 there (:218-221): a positive is never overridden.
 *  7. scores = positive ? certainty_kp : 0 (:223-228) -- not 0 / 1.
 *  8. masks0 [B,4,M], masks1 [B,4,N] uint8 (nullable), rows: mask_pos = valid_pos (NOT "is positive", the reference
 *     names it so), mask_neg_far and mask_neg_unreliable (both raw, not reduced by the positives), mask_ign = valid &
 *     ~positive & ~neg (:243-244).
 *  9. dense, each nullable (:230-242): assignment [B,M,N] uint8 = positive; reward [B,M,N] float =
 *     max(valid_pair & dist < pos_th^2, assignment) - (valid_pair & dist > neg_th^2).
 * 10. M == 0 or N == 0 (:62-94): no kernel; matches of the other side are -1, its scores and masks 0.  The reference
 *     returns kp[:, :, 0] as certainty_kp and cycle_error_kp and an uninitialised proj there; those belong to the
 *     caller (dense_warp.py returns exactly that), this entry neither reads nor writes them.
 * Known difference: the running minima use '<' and fminf, which skip a NaN distance where torch.min would propagate
 * it; it needs a key point that is valid with a NaN coordinate (a NaN projection is excluded by step 1).  The same
 * difference as in gfc_gt_matches_sparse_map.
 * Launch plan.  A pair is split over workgroups of 256 threads; nothing waits for another workgroup.
 *  sweep   grid (ceil(M/16) + ceil(N/16), B): a workgroup owns 16 key points of one side, 16 lanes each, and streams the
 *          other side through LDS in tiles of 256 elements (float4 of coordinates, one flag byte = valid_pos).  Lane l
 *          takes elements l, l + 16, ... of every tile in ascending order; the 16 lanes are reduced on (distance,
 *          index), the lower index winning equal distances.  Per key point into the workspace: the masked symmetric
 *          minimum with its arg-min, and the one-way minimum masked by the tile element's flag.
 *  finish  grid (ceil((M+N)/256), B): steps 3-8 per key point.
 *  dense   (assignment or reward) grid (ceil(N/256), M, B), one thread per element.
 * No LDS-derived size limit: B, M, N <= 65535 (GFC_ERR_INVALID otherwise) and GFC_ERR_WORKSPACE (nothing launched,
 * no output written) when workspace_bytes < gfc_gt_matches_roma_workspace_bytes(B, M, N) = about 13 B (M + N) + 4 B M
 * bytes, 0 for an empty side or invalid sizes.  Status: GFC_OK, GFC_ERR_INVALID (sizes, a required pointer NULL, pos_th
 * or neg_th < 0), GFC_ERR_WORKSPACE, GFC_ERR_LAUNCH. */
int gfc_dense_cycle_error(const float* q_to_ref, const float* ref_to_q, float* out, int B, int H, int W, int Hr, int Wr,
                          void* stream);
int gfc_gt_sample_dense_warp(const float* kp, const float* warp, const float* certainty, const float* cycle_error,
                             const float* other_warp, int B, int M, int H, int W, int Hr, int Wr, int q_h, int q_w,
                             int t_h, int t_w, float* proj, float* certainty_kp, float* cycle_kp, void* stream);
size_t gfc_gt_matches_roma_workspace_bytes(int B, int M, int N);
int gfc_gt_matches_roma(const float* kp0, const float* kp1, const float* proj_0to1, const float* proj_1to0,
                        const float* certainty_kp0, const float* certainty_kp1, const float* cycle_kp0,
                        const float* cycle_kp1, const uint8_t* valid0, const uint8_t* valid1, int B, int M, int N,
                        double pos_th, double neg_th, double pos_cert_th, double pos_cycle_error_th, double neg_cert_th,
                        double neg_cycle_error_th, int64_t* matches0, int64_t* matches1, float* scores0, float* scores1,
                        uint8_t* masks0, uint8_t* masks1, uint8_t* assignment, float* reward, void* workspace,
                        size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GFC_AMD_DENSE_WARP_H */
