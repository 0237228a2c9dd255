/* The backward of LightGlue's rotary self attention, of the self block's Wqkv around it, and the layer entry that keeps
 * the self attention's context: the C entries of csrc/lg_self_attn_backward.hip (and, for the layer, csrc/api.hip),
 * exported by libgfc_amd.so and written in the grammar of gfc_amd.h (glue-factory-colon_amd/_native.py parses all ten
 * headers).  A header of its own because the suite pins the function lists of the other nine; it declares functions
 * only and takes its types from gfc_amd.h. */
#ifndef GFC_AMD_SELF_ATTN_BACKWARD_H
#define GFC_AMD_SELF_ATTN_BACKWARD_H

#include "gfc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The self attention of one SelfBlock (gluefactory/models/matchers/lightglue.py:43-50, 124-129, 157-162, the non-flash
 * branch without a mask) per side of a pair and per head, head dim 64, on the rows of that side alone:
 *   q' = Rot(q), k' = Rot(k)                 (:43-50, 157-159) adjacent columns paired, per-column tables c, s [rows,64]:
 *       o[2i] = t[2i] c[2i] - t[2i+1] s[2i],  o[2i+1] = t[2i+1] c[2i+1] + t[2i] s[2i+1]
 *     (what gfc_linear's rotary epilogue evaluates; the same table for all four heads)
 *   S = scale q' k'^T, P = softmax_j S       (:124-129; scale = 64^-0.5 there)
 *   ctx = P v                                (:129)
 * Given dctx, the gradient at ctx:
 *   D[i] = dctx[i] . ctx[i]                  (per head)
 *   dS = P o (dctx v^T - D)
 *   dq' = scale dS k', dk' = scale dS^T q', dv = P^T dctx
 *   dq = Rot^T(dq'), dk = Rot^T(dk'), the gradients at the GEMM's output BEFORE the rotation:
 *       dt[2i] = do[2i] c[2i] + do[2i+1] s[2i+1],  dt[2i+1] = do[2i+1] c[2i+1] - do[2i] s[2i]
 *     evaluated on do = scale * (the accumulated sum), each product rounded, then one addition.
 * No gradient reaches the tables: c and s get gradient from every layer (posenc.Wr is shared), so a share through one
 * layer would be partial; it is not produced.
 *
 * Packed rows, the layout of forward_layers: [B*M + B*N, .], side 0 of every pair (M rows each), then side 1 (N rows
 * each).  qkv [R,768] holds q' | k' | v, 256 columns each, head-major, 64 per head, ALREADY rotated, as the forward's qkv
 * buffer does; ctx, dctx [R,256]; cos, sin [R,64] contiguous, NULL together: no rotation (dq = dq', dk = dk').  dqkv
 * [R,768] = dq | dk | dv is written, every element overwritten.  qkv, ctx, dctx, dqkv have their own leading dimensions
 * in floats.
 * Launches: D per row and head (a wave per row); the log-sum-exp of every row over its own side (running maximum and sum
 * over ascending tiles of 32 keys); dq: a workgroup owns 128 rows of one side and head as queries, a wave 32 of them,
 * and streams the side as keys in ascending tiles of 32 through LDS; dk, dv: the same ownership with the rows as keys and
 * the side streamed as queries.  S_ij and S_ji are different matrices, so the two roles share no product: two kernels.
 * Per score element eight products of depth 64 (S twice, dctx v^T twice, dS k', dS^T q', P^T dctx and the log-sum-exp's
 * S), all on v_mfma_f32_32x32x2_f32 (exact fp32).  No n x n matrix is stored.  exp is taken of (scale S - lse) clamped to
 * <= 0 only.  Every output element has one owner: no atomics, the streamed rows are not split over workgroups, two calls
 * on the same inputs give the same bits; dctx = 0 gives exact zeros.  There is no LDS-derived limit on M, N.
 * Workspace, each slot rounded up to 256 bytes, floats, R = B (M + N):
 *   lse R*4 | D R*4.
 * GFC_ERR_INVALID: heads * 64 != 256; B, M or N < 1; B (M + N) > 2796202 (R * 768 stays inside an int); a NULL qkv,
 * ctx, dctx or dqkv, a pointer that is not 16-byte aligned, a leading dimension below 768 (qkv, dqkv) / 256 (ctx, dctx)
 * or not a multiple of 4; one of cos, sin NULL and the other not.  GFC_ERR_WORKSPACE: ws_bytes <
 * gfc_attention_self_backward_workspace_bytes(B, M, N, heads) (0 for a refused shape) or ws not 16-byte aligned.  All of
 * it before any launch.  The workspace may hold anything on entry. */
size_t gfc_attention_self_backward_workspace_bytes(int B, int M, int N, int heads);
int gfc_attention_self_backward(const float* qkv, int ld_qkv, const float* ctx, int ld_ctx, const float* dctx, int ld_dctx,
                                const float* cos, const float* sin, int B, int M, int N, int heads, float scale,
                                float* dqkv, int ld_dqkv, void* ws, size_t ws_bytes, void* stream);

/* The attention part of one SelfBlock's backward (lightglue.py:151-162) on packed rows, 4 heads, scale 64^-0.5:
 *   qkv = x Wqkv^T + bqkv, rotated on the columns < 512   (recomputed here by gfc_linear, the forward's own call)
 *   dqkv = gfc_attention_self_backward(qkv, ctx, dctx, cos, sin)
 *   dWqkv [768,256] = dqkv^T x, dbqkv [768] = sum dqkv    (rows of both sides)
 *   dx [R,256] (nullable) = dx_in + dqkv Wqkv; with dx_in = NULL the attention's share alone.
 * x: the rows the self block reads; cos, sin [R,64]: the rotary tables of those rows (required); ctx: the self
 * attention's context before out_proj; dctx: the gradient there (the dctx of gfc_lg_ffn_backward on the self block);
 * dx_in (nullable, not dx itself): the gradient at x by every other path (the dx_in of that call), so that dx is the
 * complete gradient at x through the block.  All [R,256] contiguous, R = B (M + N).
 * Wqkv [768,256], bqkv [768] are in the library's PACKED row order s*256 + head*64 + dd (s = 0 q, 1 k, 2 v), the order
 * gfc_lg_params.wqkv holds; dWqkv and dbqkv come out in the same order (the state-dict row is head*192 + dd*3 + s).
 * Every parameter output is OVERWRITTEN.  No gradient for posenc.Wr is produced (see above).
 * The weight gradient is split over rows into parts of at most 1024 rows (at most 128 parts, then longer ones) and the
 * bias gradient into chunks of 128 rows, as in gfc_lg_ffn_backward: a finishing launch adds them in ascending order in
 * fp64, rounded once.  No atomics.
 * Workspace, each slot rounded up to 256 bytes, floats:
 *   qkv R*768 | dqkv R*768 | split-K parts parts(R) * 196608 | column-sum chunks ceil(R / 128) * 768 |
 *   the workspace of gfc_attention_self_backward,
 *   parts(R) as in gfc_amd_ffn_backward.h.
 * GFC_ERR_INVALID: B, M or N < 1; R > 2796202; a NULL required pointer; x, cos, sin, ctx, dctx, Wqkv or dx not 16-byte
 * aligned; dx_in without dx or equal to it.  GFC_ERR_WORKSPACE: ws_bytes <
 * gfc_lg_self_attn_backward_workspace_bytes(B, M, N) (0 for a refused shape) or ws not 16-byte aligned.  All of it before
 * any launch. */
size_t gfc_lg_self_attn_backward_workspace_bytes(int B, int M, int N);
int gfc_lg_self_attn_backward(const float* x, const float* cos, const float* sin, const float* ctx, const float* dctx,
                              const float* dx_in, const float* Wqkv, const float* bqkv, int B, int M, int N, float* dWqkv,
                              float* dbqkv, float* dx, void* ws, size_t ws_bytes, void* stream);

/* gfc_lg_layer_pairs_keep (gfc_amd_ffn_backward.h) with one more device-to-device copy-out: ctx_self [R,256], the SELF
 * attention's context before out_proj (or before the folded ffn[0]) of layer l.  fp32 matcher only.  The launches are
 * those of gfc_lg_layer_pairs, so x, x_mid and ctx keep its bits at every batch size.  The workspace is that of
 * gfc_lg_layer_pairs.  GFC_ERR_INVALID: what gfc_lg_layer_pairs_keep refuses, or a NULL ctx_self. */
int gfc_lg_layer_pairs_keep_self(const gfc_lg_params* p, int l, float* x, const float* cosb, const float* sinb, int B, int M,
                                 int N, const int32_t* self_p, const int32_t* cross_p, float* x_mid, float* ctx,
                                 float* ctx_self, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GFC_AMD_SELF_ATTN_BACKWARD_H */
