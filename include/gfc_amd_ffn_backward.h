/* The backward of one LightGlue FFN block with the projection in front of it, and the last layer's forward with the two
 * tensors that backward starts from kept: the C entries of csrc/lg_ffn_backward.hip (and, for gfc_lg_layer_pairs_keep,
 * csrc/api.hip), exported by libgfc_amd.so and written in the grammar of gfc_amd.h (glue-factory-colon_amd/_native.py
 * parses all eight headers).  A header of its own because the suite pins the function lists of the other seven; it
 * declares functions only and takes its types from gfc_amd.h. */
#ifndef GFC_AMD_FFN_BACKWARD_H
#define GFC_AMD_FFN_BACKWARD_H

#include "gfc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One transformer block's output stage (gluefactory/models/matchers/lightglue.py:143-148 the FFN, :160-164 the self
 * block, :219-222 the cross block) for R packed rows, d = 256:
 *   m = ctx Wout^T + bout                      (to_out / out_proj; Wout = NULL: m = ctx)
 *   h = [x | m] W0^T + b0                      (ffn.0, Linear(512, 512))
 *   mu = mean(h), var = mean((h - mu)^2) (biased, two passes), rstd = 1 / sqrt(var + 1e-5)
 *   n = (h - mu) rstd, u = n gamma + beta      (ffn.1, LayerNorm(512))
 *   a = GELU(u) = u Phi(u)                     (ffn.2, erf form)
 *   y = x + a W3^T + b3                        (ffn.3, Linear(512, 256), and the residual)
 * Given dy [R,256], the gradient at y:
 *   da = dy W3; dW3 [256,512] = dy^T a; db3 [256] = sum dy
 *   du = da o (Phi(u) + u phi(u)); dgamma [512] = sum du o n; dbeta [512] = sum du
 *   dn = du o gamma; dh = rstd (dn - mean(dn) - n mean(dn o n))
 *   dW0 [512,512] = dh^T [x | m]; db0 [512] = sum dh; dcat = dh W0
 *   dm = dcat[:, 256:]; dWout [256,256] = dm^T ctx; dbout [256] = sum dm
 *   dx_in [R,256] (nullable) = dy + dcat[:, :256]: the gradient at the block's input rows through the residual and the
 *     first half of the concatenation ONLY (not through the attention that made ctx)
 *   dctx [R,256] (nullable) = dm Wout (dm itself without Wout): the gradient at the attention context.
 * The sums run over the R rows; every parameter output is OVERWRITTEN.  The weights are the reference's own (state-dict,
 * unfolded) fp32 tensors, not gfc_lg_params, whose ffn.0 may hold to_out folded in: x, ctx, dy [R,256]; Wout [256,256]
 * and bout [256], both or neither; W0 [512,512], b0, gamma, beta [512], W3 [256,512].  dWout and dbout are required with
 * Wout and must be NULL without it.  The forward quantities are recomputed here (m and h by gfc_linear, the forward's
 * entry point), never taken from the caller.
 * Every product (dy W3, dy^T a, dh^T [x | m], dh W0, dm^T ctx, dm Wout) runs on v_mfma_f32_32x32x2_f32 (exact fp32), 128
 * x 128 output tiles.  The LayerNorm / GELU backward is one row kernel, a wave per 512-wide row read with 16-byte loads,
 * which turns (h, da) into (dh, a) in place; Phi comes from the erf of this build's GELU (Abramowitz & Stegun 7.1.26 in
 * the default library, the exact chain in the exact-erf library), phi from one exp of -u^2 / 2 <= 0, so u = +-1e4 gives a
 * derivative of exactly 1 or 0; dy = 0 gives exact zeros in every output.
 * Reductions: dy^T a, dh^T [x | m] and dm^T ctx are split over rows into parts of at most 1024 rows (at most 128 parts,
 * then longer ones); db3 and dbout (column sums) and dgamma, dbeta, db0 (the row kernel) into chunks of 128 rows.  All
 * go through the workspace and a finishing launch adds them in ascending order in fp64, rounded once.  No atomics: two
 * calls on the same inputs give the same bits.
 * Workspace, each slot rounded up to 256 bytes, floats:
 *   m R*256 | h, then dh R*512 | da, then a R*512 | dm R*256 (m and dm unused without Wout) |
 *   split-K parts parts(R) * 262144 (used by dW3, dW0, dWout in turn) | column-sum chunks ceil(R / 128) * 520 |
 *   row-kernel chunks ceil(R / 128) * 1536 (dgamma | dbeta | db0),
 *   parts(R) = ceil(R / k), k = ceil(ceil(R / min(ceil(R / 1024), 128)) / 16) * 16.
 * 1 <= R <= 8388607 and the pointer rules above (GFC_ERR_INVALID otherwise); GFC_ERR_WORKSPACE when ws_bytes <
 * gfc_lg_ffn_backward_workspace_bytes(R) (0 for a refused R) or ws is not 16-byte aligned; all of it before any
 * launch.  There is no LDS-derived limit.  The workspace may hold anything on entry. */
size_t gfc_lg_ffn_backward_workspace_bytes(int R);
int gfc_lg_ffn_backward(const float* x, const float* ctx, const float* dy, const float* Wout, const float* bout,
                        const float* W0, const float* b0, const float* gamma, const float* beta, const float* W3, int R,
                        float* dWout, float* dbout, float* dW0, float* db0, float* dgamma, float* dbeta, float* dW3,
                        float* db3, float* dx_in, float* dctx, void* ws, size_t ws_bytes, void* stream);

/* gfc_lg_layer_pairs (gfc_amd_layer_scores.h) with two more outputs, fp32 only (GFC_ERR_INVALID for GFC_LG_FP16): x_mid
 * [B*M + B*N, 256], the rows after the self block, which the cross block reads, and ctx [B*M + B*N, 256], the cross
 * attention's context before to_out: with them, (x_mid, ctx) is the (x, ctx) of gfc_lg_ffn_backward for the cross block
 * of this layer.  The same launches as gfc_lg_layer_pairs plus two device-to-device copies, so x holds the same bits at
 * every batch size; arguments, workspace (gfc_lg_layer_pairs_workspace_bytes) and refusals as there. */
int gfc_lg_layer_pairs_keep(const gfc_lg_params* p, int layer, float* x, const float* cos_tab, const float* sin_tab,
                            int B, int M, int N, const int32_t* self_problems, const int32_t* cross_problems,
                            float* x_mid, float* ctx, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GFC_AMD_FFN_BACKWARD_H */
