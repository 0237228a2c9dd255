/* Per-layer scores of the deep-supervision loss and the exit report: the C entry of csrc/lg_layer_scores.hip and the
 * layer entry of csrc/api.hip that keeps a host-driven full-depth pass on the whole matcher's bits, exported
 * by libgfc_amd.so and written in the grammar of gfc_amd.h (glue-factory-colon_amd/_native.py parses all six headers).
 * A header of its own because the suite pins the function lists of the other five; it declares functions only and takes
 * its types from gfc_amd.h. */
#ifndef GFC_AMD_LAYER_SCORES_H
#define GFC_AMD_LAYER_SCORES_H

#include "gfc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One layer's agreement with the final assignment, its token-confidence loss and its share of confident points, for B
 * equal-sized pairs: TokenConfidence.loss (gluefactory/models/matchers/lightglue.py:82-95) and the predicate of
 * check_if_stop (lightglue.py:577-580).  la_layer and la_final [B,M+1,N+1]: the log assignment of the layer's own head
 * and of the last head; logit0 [B,M], logit1 [B,N]: token[0] of the layer BEFORE the sigmoid (gfc_lg_rowdot with
 * apply_sigmoid = 0); threshold: the layer's confidence threshold.
 *   correct0[i] = (arg-max over j in 0..N of la_layer[i,j]) == (arg-max over j in 0..N of la_final[i,j]), i < M: the
 *     dustbin column N takes part, as in la[:, :-1, :].max(-1) (lightglue.py:86-88);
 *   correct1[j] likewise down the columns, over i in 0..M, j < N (lightglue.py:89-91).
 * Ties go to the LOWER index; the reference leaves that to torch.max.  Known difference: a NaN entry is skipped by the
 * running maximum (torch.max returns the NaN's index); a row or column with no entry above -inf has arg-max 0.
 * out [B,6] = agree0, agree1, bce0, bce1, conf0, conf1:
 *   agree0 / agree1 = the number of set correct0 / correct1;
 *   bce0 = mean over i of max(x,0) - x y + log1p(exp(-|x|)), x = logit0[i], y = correct0[i] (BCEWithLogitsLoss,
 *     lightglue.py:73,93-94; each term in fp32, the sum and the mean in fp64, rounded to fp32 once); bce1 over j;
 *   conf0 = #{ i : !(sigmoid(logit0[i]) < threshold) }, the sigmoid that of gfc_lg_rowdot; conf1 over j.
 * correct0 [B,M], correct1 [B,N] (each nullable) receive the 0 / 1 targets.
 * Two launches on `stream`.  The first splits every pair over workgroups: a wave per row of both matrices (16 rows per
 * workgroup), and 256-column tiles of 128-row chunks that keep a running (max, index) per column in registers; sums
 * and per-chunk column maxima go to the workspace.  The second (one workgroup per pair) combines the chunks with the
 * lower index winning and adds the partial sums in a fixed order: no float atomics, nothing depends on the order in
 * which workgroups run.  No LDS-derived size limit.  M, N >= 1; B, M, N <= 65535 (GFC_ERR_INVALID otherwise);
 * GFC_ERR_WORKSPACE when ws_bytes < gfc_lg_layer_scores_workspace_bytes(B, M, N) (0 for a refused shape); all of it
 * before any launch.  The workspace may hold anything on entry. */
size_t gfc_lg_layer_scores_workspace_bytes(int B, int M, int N);
int gfc_lg_layer_scores(const float* la_layer, const float* la_final, const float* logit0, const float* logit1,
                        float threshold, int B, int M, int N, float* out, uint8_t* correct0, uint8_t* correct1,
                        void* ws, size_t ws_bytes, void* stream);

/* gfc_lg_layer (csrc/api.hip) for a uniform batch of B equal pairs of M and N key points, with the cross attention
 * gfc_lg_forward_packed chooses for that batch: from 8 pairs with min(M, N) >= 128 on (fp32), sim is evaluated once
 * (gfc_attention_cross_stored, in that function's chunks of pairs); below that, or in fp16, this is gfc_lg_layer.  So a
 * host that drives the layers one by one to keep every layer's rows (LightGlue.forward_layers, the reference's
 * training-mode forward, lightglue.py:483-498) gets the bits of the whole-matcher entry at every batch size.
 * x [B*M + B*N, 256] (side 0 first, updated in place), cos_tab / sin_tab [rows,64]; self_problems / cross_problems
 * [2B][4] as gfc_lg_layer takes them, problem b = side 0 of pair b and B + b = side 1 (the first B cross problems are
 * the pairs' first directions).  ws needs gfc_lg_layer_pairs_workspace_bytes(B, M, N) bytes (0: shape refused, as the
 * whole-matcher entries refuse it): GFC_ERR_WORKSPACE if smaller. */
size_t gfc_lg_layer_pairs_workspace_bytes(int B, int M, int N);
int gfc_lg_layer_pairs(const gfc_lg_params* p, int layer, float* x, const float* cos_tab, const float* sin_tab, int B,
                       int M, int N, const int32_t* self_problems, const int32_t* cross_problems, void* ws,
                       size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GFC_AMD_LAYER_SCORES_H */
