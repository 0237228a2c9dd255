/* Gradients of the deep-supervision loss with respect to the assignment head and the exit token of one layer, and the
 * direct gradient at that layer's descriptors: the C entries of csrc/lg_head_backward.hip, exported by libgfc_amd.so and
 * written in the grammar of gfc_amd.h (glue-factory-colon_amd/_native.py parses all seven headers).  A header of its own
 * because the suite pins the function lists of the other six; it declares functions only and takes its types from
 * gfc_amd.h. */
#ifndef GFC_AMD_HEAD_BACKWARD_H
#define GFC_AMD_HEAD_BACKWARD_H

#include "gfc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The assignment head of layer `layer` (MatchAssignment, gluefactory/models/matchers/lightglue.py:271-288, with
 * sigmoid_log_double_softmax, lightglue.py:257-269) under NLLLoss (gluefactory/models/utils/losses.py:6-73), for B
 * equal-sized pairs; d = 256, s = d^-1/4:
 *   md0 = s (x0 Wf^T + bf), md1 likewise (lightglue.py:281-284); S = md0 md1^T (lightglue.py:285);
 *   z0 = x0 . wm + bm, z1 likewise (lightglue.py:286-287);
 *   la_ij = 2 S_ij - lse_row_i - lse_col_j + logsigmoid(z0_i) + logsigmoid(z1_j); the dustbins are logsigmoid(-z0_i) and
 *   logsigmoid(-z1_j).
 * Labels: W = (gt_assignment != 0) [B,M,N] when it is given, else W[i, gt_matches0[i]] = 1 where -1 < gt_matches0[i] < N;
 * n0 = (gt_matches0 == -1), n1 = (gt_matches1 == -1) (-2 is ignored); P = max(sum W, 1), Q = max(sum n0, 1) +
 * max(sum n1, 1) (losses.py:13-23); r_i = sum_j W_ij, c_j = sum_i W_ij, which may exceed 1.
 * g [B]: the weight of this layer's nll in the differentiated scalar, per pair: grad_total[b] w_l / sum_w with the layer
 * weights of lightglue.py:611-626.  With lambda = nll_balancing, a = g lambda / P and c = g (1 - lambda) / Q:
 *   G_ij  = a (r_i softmax_row(S)_ij + c_j softmax_col(S)_ij - 2 W_ij)
 *   dz0_i = -a r_i sigmoid(-z0_i) + c n0_i sigmoid(z0_i), dz1_j with c_j and n1_j
 *   dmd0 = G md1, dmd1 = G^T md0
 *   dWf [256,256] = s (dmd0^T x0 + dmd1^T x1), dbf [256] = s (column sums of dmd0 and dmd1)
 *   dwm [256] = sum_i dz0_i x0_i + sum_j dz1_j x1_j, dbm [1] = sum dz0 + sum dz1
 *   dx [B*M + B*N, 256] (nullable, side 0 first) = s dmd Wf + dz (x) wm: the DIRECT gradient at the layer's descriptors.
 * Every output is summed over the pairs and OVERWRITTEN.  p: the packed fp32 parameters (GFC_LG_FP32; GFC_ERR_INVALID
 * otherwise); x0 [B*M,256], x1 [B*N,256]; gt_matches0 [B,M], gt_matches1 [B,N]; gt_assignment nullable.
 * S is evaluated once and kept [B,M,N] in the workspace; md, S and z come from gfc_linear, gfc_batched_nt and
 * gfc_lg_rowdot, the forward's entry points.  The products G md1, G^T md0, dmd^T x and dmd Wf run on
 * v_mfma_f32_32x32x2_f32 (exact fp32), 128 x 128 output tiles, a pair per grid z, so a pair is split over workgroups and
 * there is no LDS-derived limit on M or N.  exp is taken of S - lse clamped to <= 0 only; the sigmoids come from
 * exp(-|z|), so z = +-1e4 gives exactly 0 and 1; a pair with W = 0, n0 = 0 and n1 = 0 contributes exact zeros.
 * Reductions: dmd^T x is split over rows into parts of at most 1024 rows (at most 128 parts per side) and the column
 * sums into chunks of 128 rows; both go through the workspace and a finishing launch adds them in ascending order in
 * fp64, rounded once.  No atomics: two calls on the same inputs give the same bits.
 * Workspace, each slot rounded up to 256 bytes, R = B (M + N), floats:
 *   md R*256 | z R | S B*M*N | lse_row B*M | lse_col B*N | r B*M | c B*N | (a, c) 2B | dz R | dmd R*256 |
 *   dWf parts (parts(B*M) + parts(B*N)) * 65536 | column-sum chunks ceil(R / 128) * 520,
 *   parts(rows) = ceil(rows / k), k = ceil(ceil(rows / min(ceil(rows / 1024), 128)) / 16) * 16.
 * M, N >= 1; B, M, N <= 65535 and B (M + N) <= 8388607 (GFC_ERR_INVALID otherwise); GFC_ERR_WORKSPACE when ws_bytes <
 * gfc_lg_head_backward_workspace_bytes(B, M, N) (0 for a refused shape) or ws is not 16-byte aligned; all of it before
 * any launch.  The workspace may hold anything on entry. */
size_t gfc_lg_head_backward_workspace_bytes(int B, int M, int N);
int gfc_lg_head_backward(const gfc_lg_params* p, int layer, const float* x0, const float* x1, const int64_t* gt_matches0,
                         const int64_t* gt_matches1, const uint8_t* gt_assignment, const float* g, float nll_balancing,
                         int B, int M, int N, float* dWf, float* dbf, float* dwm, float* dbm, float* dx, void* ws,
                         size_t ws_bytes, void* stream);

/* The exit token of one layer l < L - 1 under TokenConfidence.loss (lightglue.py:82-95; BCEWithLogitsLoss,
 * lightglue.py:73), whose descriptors are detached (lightglue.py:83-85), so no dx:
 *   dlogit0_i = g[b] (sigmoid(logit0_i) - correct0_i) / (2 M (L - 1)), dlogit1_j with N (lightglue.py:93-95,618-623);
 *   dtoken_w [256] = sum dlogit x, dtoken_b [1] = sum dlogit, over both sides and all pairs, OVERWRITTEN.
 * x0 [B*M,256], x1 [B*N,256]; logit0 [B,M], logit1 [B,N]: token[0] before the sigmoid (gfc_lg_rowdot with apply_sigmoid
 * = 0); correct0 [B,M], correct1 [B,N]: the targets gfc_lg_layer_scores writes; g [B] = grad_total; n_layers = L >= 2.
 * Chunks of 128 rows through the workspace, added in ascending order in fp64: no atomics.  Workspace, floats, each
 * slot rounded up to 256 bytes: dlogit R | chunks ceil(R / 128) * 520.  Shapes and refusals as above. */
size_t gfc_lg_token_backward_workspace_bytes(int B, int M, int N);
int gfc_lg_token_backward(const float* x0, const float* x1, const float* logit0, const float* logit1,
                          const uint8_t* correct0, const uint8_t* correct1, const float* g, int n_layers, int B, int M,
                          int N, float* dtoken_w, float* dtoken_b, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GFC_AMD_HEAD_BACKWARD_H */
