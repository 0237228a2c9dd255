/* The backward of LightGlue's bidirectional cross attention, and of the cross block's to_qk / to_v around it: the C
 * entries of csrc/lg_cross_attn_backward.hip, exported by libgfc_amd.so and written in the grammar of gfc_amd.h
 * (glue-factory-colon_amd/_native.py parses all nine headers).  A header of its own because the suite pins the function
 * lists of the other eight; it declares functions only and takes its types from gfc_amd.h. */
#ifndef GFC_AMD_CROSS_ATTN_BACKWARD_H
#define GFC_AMD_CROSS_ATTN_BACKWARD_H

#include "gfc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The cross attention of one CrossBlock (gluefactory/models/matchers/lightglue.py:196-218, the non-flash branch without
 * a mask) per pair and head, head dim 64, q_a = qk rows of side a, v_a likewise:
 *   S = scale q0 q1^T                        (:208-209; scale = 64^-0.5 there)
 *   P01 = softmax_j S, P10^T = softmax_i S   (:212-213, the column soft-max of the same S)
 *   ctx0 = P01 v1, ctx1 = P10 v0             (:214-215)
 * Given dctx0, dctx1, the gradients at ctx:
 *   D0[i] = dctx0[i] . ctx0[i], D1[j] = dctx1[j] . ctx1[j]         (per head)
 *   dS[i,j] = P01[i,j] (dctx0[i] . v1[j] - D0[i]) + P10^T[i,j] (v0[i] . dctx1[j] - D1[j])
 *   dq0 = scale dS q1, dq1 = scale dS^T q0
 *   dv1 = P01^T dctx0, dv0 = P10^T dctx1     (dv0[i] = sum_j P10^T[i,j] dctx1[j])
 * The whole of it is symmetric under swapping the sides, so one kernel serves both directions as two problems per pair.
 *
 * Packed rows, the layout of forward_layers: [B*M + B*N, 256], side 0 of every pair (M rows each), then side 1 (N rows
 * each); columns head-major, 64 per head.  qk, v, ctx, dctx are read and dqk, dv written (every element, overwritten)
 * with their own leading dimensions in floats.
 * Launches: D per row and head (a wave per row); the log-sum-exp of every row over the other side (running maximum and
 * sum over ascending tiles of 32 keys); the main kernel: a workgroup owns 128 rows of one side and head, a wave 32 of
 * them, and streams the other side in ascending tiles of 32 keys through LDS; per tile S, dctx_a v_b^T, v_a dctx_b^T,
 * then dS q_b and P_ba^T dctx_b, ten products of depth 64 per score element, all on v_mfma_f32_32x32x2_f32 (exact fp32).
 * No M x N matrix is stored.  exp is taken of (scale S - lse) clamped to <= 0 only.  Every output row has one owner: no
 * atomics, the keys are not split over workgroups, two calls on the same inputs give the same bits; dctx = 0 gives exact
 * zeros.  There is no LDS-derived limit on M, N.
 * Workspace, each slot rounded up to 256 bytes, floats, R = B (M + N):
 *   lse R*4 | D R*4.
 * GFC_ERR_INVALID: heads * 64 != 256; B, M or N < 1; B (M + N) > 8388607; a NULL pointer, one that is not 16-byte
 * aligned, or a leading dimension below 256 or not a multiple of 4.  GFC_ERR_WORKSPACE: ws_bytes <
 * gfc_attention_cross_backward_workspace_bytes(B, M, N, heads) (0 for a refused shape) or ws not 16-byte aligned.  All of
 * it before any launch.  The workspace may hold anything on entry. */
size_t gfc_attention_cross_backward_workspace_bytes(int B, int M, int N, int heads);
int gfc_attention_cross_backward(const float* qk, int ld_qk, const float* v, int ld_v, const float* ctx, int ld_ctx,
                                 const float* dctx, int ld_dctx, int B, int M, int N, int heads, float scale, float* dqk,
                                 int ld_dqk, float* dv, int ld_dv, void* ws, size_t ws_bytes, void* stream);

/* The attention part of one CrossBlock's backward (lightglue.py:196-218) on packed rows, 4 heads, scale 64^-0.5:
 *   qk = x Wqk^T + bqk, v = x Wv^T + bv      (:196-197; recomputed here by gfc_linear, the forward's entry point)
 *   dqk, dv = gfc_attention_cross_backward(qk, v, ctx, dctx)
 *   dWqk [256,256] = dqk^T x, dbqk [256] = sum dqk, dWv [256,256] = dv^T x, dbv [256] = sum dv   (rows of both sides)
 *   dx [R,256] (nullable) = dx_in + (dqk Wqk + dv Wv); with dx_in = NULL the attention part alone.
 * x: the rows the cross block reads; ctx: its attention context before to_out; dctx: the gradient there (the dctx of
 * gfc_lg_ffn_backward); dx_in (nullable, not dx itself): the gradient at x by every other path (the dx_in of
 * gfc_lg_ffn_backward), so that dx is the complete gradient at x.  All [R,256] contiguous, R = B (M + N).  The weights
 * are the state-dict fp32 to_qk / to_v tensors.  Every parameter output is OVERWRITTEN.
 * The two weight gradients are split over rows into parts of at most 1024 rows (at most 128 parts, then longer ones) and
 * the two bias gradients into chunks of 128 rows, as in gfc_lg_ffn_backward: a finishing launch adds them in ascending
 * order in fp64, rounded once.  No atomics.
 * Workspace, each slot rounded up to 256 bytes, floats:
 *   qk R*256 | v R*256 | dqk R*256 | dv R*256 | dv Wv R*256 | split-K parts parts(R) * 65536 |
 *   column-sum chunks ceil(R / 128) * 520 | the workspace of gfc_attention_cross_backward,
 *   parts(R) as in gfc_amd_ffn_backward.h.
 * GFC_ERR_INVALID: B, M or N < 1; R > 8388607; a NULL required pointer; x, ctx, dctx or dx not 16-byte aligned; dx_in
 * without dx or equal to it.  GFC_ERR_WORKSPACE: ws_bytes < gfc_lg_cross_attn_backward_workspace_bytes(B, M, N) (0 for a
 * refused shape) or ws not 16-byte aligned.  All of it before any launch. */
size_t gfc_lg_cross_attn_backward_workspace_bytes(int B, int M, int N);
int gfc_lg_cross_attn_backward(const float* x, const float* ctx, const float* dctx, const float* dx_in, const float* Wqk,
                               const float* bqk, const float* Wv, const float* bv, int B, int M, int N, float* dWqk,
                               float* dbqk, float* dWv, float* dbv, float* dx, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GFC_AMD_CROSS_ATTN_BACKWARD_H */
