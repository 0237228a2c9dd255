/* gfc_amd.h -- C ABI of libgfc_amd.so: SuperPoint + LightGlue hot path on MI355X (gfx950).
 *
 * The reference (ipastore/glue-factory-colon) is pure Python on PyTorch: it has no FFI
 * for this path.  The boundary it offers is the model registry
 * (gluefactory/models/__init__.py:7-30 `get_model`) and the module contract
 * `BaseModel.forward(data: dict) -> dict` (gluefactory/models/base_model.py:101-113).
 * Each entry point below replaces the ATen op sequence of one reference function; the
 * reference file:line it replaces is cited on every declaration.  The Python binding a
 * maintainer adds is shown in INTEGRATION.md (ctypes, no torch types cross this line).
 *
 * Conventions
 *   - all pointers are DEVICE pointers (hipMalloc'ed or torch-allocated) unless marked
 *     "host"; fp32 everywhere, int32 for counts/tables, int64 for match indices
 *     (the reference returns torch.long, lightglue.py:294-319);
 *   - no allocation and no synchronisation inside: the caller passes a workspace of at
 *     least gfc_*_workspace_bytes() and a hipStream_t (as void*); every kernel is
 *     enqueued on that stream and the call returns immediately;
 *   - no MUTABLE global state: calls are re-entrant per stream and from any host thread.
 *     What the library keeps process-wide is read-only after its first use and never
 *     changes a result: the tuning knobs (GFC_GEMM_TILE, GFC_ATTN_CFG, ... read ONCE from
 *     the environment by the first call, csrc/runtime.h -- set them before that call;
 *     they select between kernel variants held to the same parity tests) and per-device
 *     facts (CU count, the dynamic-LDS attribute of each kernel instantiation);
 *   - return value: 0 = ok, otherwise a gfc_status.  Nothing is written on error.
 *   - activations inside the extractor are NHWC ("channels last").
 */
#ifndef GFC_AMD_H
#define GFC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GFC_OK = 0,
  GFC_ERR_INVALID = 1,     /* bad shape / null pointer / unsupported combination of arguments */
  GFC_ERR_WORKSPACE = 2,   /* workspace smaller than gfc_*_workspace_bytes() */
  GFC_ERR_UNSUPPORTED = 3, /* valid for the reference, not built here (e.g. nms_radius > 4) */
  GFC_ERR_LAUNCH = 4       /* hipGetLastError() != hipSuccess after a launch */
} gfc_status;

/* Library / device identification ("gfx950" builds only). */
const char* gfc_version(void);

/* ------------------------------------------------------------------------------------
 * Primitives (also exported so that parity tests can pin each kernel in isolation)
 * ---------------------------------------------------------------------------------- */

/* Re-pack a conv weight from the state-dict layout [Cout][Cin][3][3] to the kernel
 * layout [tap=ky*3+kx][Cout][Cin].  (nn.Conv2d weights, superpoint_open.py:64-66) */
int gfc_pack_conv3x3(const float* w_oihw, float* w_packed, int cout, int cin, void* stream);

/* 3x3 convolution, stride 1, zero padding 1, NHWC, fused epilogue
 *   y = conv(x) + bias;  if relu: y = max(y,0);  if scale: y = y*scale + shift;
 *   if pool: 2x2/2 max-pool of y (floor semantics).
 * Replaces VGGBlock (superpoint_open.py:61-77: conv -> ReLU -> BatchNorm(eval)) followed by
 * nn.MaxPool2d(2,2) (superpoint_open.py:104-106), and conv+ReLU(+pool) of
 * gluefactory_nonfree/superpoint.py:214-224.  cin % 32 == 0 (or cin == 1), cout % 64 == 0.
 * x [B,H,W,cin], w packed [9][cout][cin] (cin == 1: [9][cout]), y [B,Ho,Wo,cout]. */
int gfc_conv3x3(const float* x, const float* w_packed, const float* bias, const float* scale,
                const float* shift, float* y, int B, int H, int W, int cin, int cout, int relu,
                int pool, void* stream);

/* The same layer as gfc_conv3x3 (relu / BN affine / pool epilogue, NHWC) as Winograd F(2x2,3x3) on fp32 MFMA:
 * 16 instead of 36 multiplications per 2x2 output block, fp32 products and accumulation, filter transform done
 * once in float64 by gfc_pack_conv3x3_wino (w_packed: 16*cout*cin floats in MFMA-fragment order).
 * cin % 16 == 0, cout % 64 == 0.  gfc_sp_stem_wino = gfc_sp_stem with conv1b in this form. */
int gfc_pack_conv3x3_wino(const float* w_oihw, float* w_packed, int cout, int cin, void* stream);
int gfc_conv3x3_wino(const float* x, const float* w_wino, const float* bias, const float* scale, const float* shift,
                     float* y, int B, int H, int W, int cin, int cout, int relu, int pool, void* stream);
int gfc_sp_stem_wino(const float* image, const float* w1, const float* b1, const float* s1, const float* t1,
                     const float* w2_wino, const float* b2, const float* s2, const float* t2, float* y, int B, int H,
                     int W, void* stream);

/* The stem with conv1b as Winograd F(4x4,3x3) (36 instead of 64 products per 4x4 output block and input channel)
 * and conv1a evaluated on the matrix pipe; same function and arguments as gfc_sp_stem_wino except for the filter
 * packing (gfc_pack_conv3x3_wino43: [64][64][3][3] -> 36*64*64 floats in MFMA-fragment order, transform in float64).
 * superpoint_open.py:61-77,100-108; superpoint.py:214-218. */
int gfc_pack_conv3x3_wino43(const float* w_oihw, float* w_packed, int cout, int cin, void* stream);
int gfc_sp_stem_wino43(const float* image, const float* w1, const float* b1, const float* s1, const float* t1,
                       const float* w2_wino43, const float* b2, const float* s2, const float* t2, float* y, int B, int H,
                       int W, void* stream);

/* Extractor stem: conv1a (1 -> 64) + conv1b (64 -> 64) + 2x2 max-pool in ONE launch.  The first layer is
 * recomputed per workgroup on the 18x18 halo of its 16x16 tile from a 20x20 image patch in LDS, so its
 * [B,H,W,64] output (the largest activation of the network) never exists in HBM.
 * image [B,H,W] (one channel), w1 [9][64], w2 packed [9][64][64], y [B,H/2,W/2,64].
 * Replaces backbone.0 of superpoint_open.py:100-106 / conv1a, conv1b, pool of superpoint.py:214-216. */
int gfc_sp_stem(const float* image, const float* w1, const float* b1, const float* s1, const float* t1,
                const float* w2_packed, const float* b2, const float* s2, const float* t2, float* y, int B, int H,
                int W, void* stream);

/* y[M,N] = epilogue( [A0 | A1][M,K0+K1] * W[N,K0+K1]^T + bias ).  Row-major, leading
 * dimensions in floats.  Replaces nn.Linear / 1x1 conv (F.linear -> addmm) at
 * lightglue.py:139-148,158,163-164,181-189 and superpoint_open.py:112-118.
 *   A1 may be NULL (K1 = 0): the two-source form implements torch.cat([x, msg], -1) of
 *   lightglue.py:164,221-222 without materialising the concatenation.
 *   scale/shift (per column, nullable): y = y*scale + shift  (BatchNorm of the 1x1 heads)
 *   alpha: y *= alpha (final_proj / d^(1/4), lightglue.py:281-284)
 *   residual (nullable, ld = ldy): y += residual (lightglue.py:164)
 *   rot_cos/rot_sin (nullable, [M,64]): rotary embedding applied to columns < rot_cols,
 *     pairing adjacent columns (lightglue.py:43-50,160-161); columns are head-major, 64 wide.
 * K0, K1 multiples of 32. */
int gfc_linear(const float* A0, int lda0, int K0, const float* A1, int lda1, int K1, const float* W,
               int ldw, const float* bias, const float* scale, const float* shift, float alpha,
               const float* residual, const float* rot_cos, const float* rot_sin, int rot_cols,
               float* Y, int ldy, int M, int N, void* stream);

/* Batched similarity: for z < batch: Y_z[M,N] = A_z[M,K] * B_z[N,K]^T (einsum "bmd,bnd->bmn",
 * lightglue.py:285).  Strides between batch entries in floats. */
int gfc_batched_nt(const float* A, int lda, long long strideA, const float* Bm, int ldb,
                   long long strideB, float* Y, int ldy, long long strideY, int M, int N, int K,
                   int batch, void* stream);

/* Multi-head attention over packed rows, head_dim 64, fp32 MFMA, never materialising the
 * score matrix.  problems[p] = {q_row0, n_q, kv_row0, n_kv} (int32 x4, device).  For every
 * problem and head h:  O[q_row0+i, 64h:64h+64] = softmax_j(Q_i . K_j * scale) V_j.
 * Replaces F.scaled_dot_product_attention (lightglue.py:119-122) and, called with the two
 * directions as two problems, the bidirectional cross attention of lightglue.py:207-217. */
int gfc_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O,
                  int ldo, const int32_t* problems, int n_problems, int max_nq, int heads, float scale,
                  void* ws, size_t ws_bytes, void* stream);
/* Optional scratch (ws may be NULL): small problem sets (batch 1..2) share each query block's keys out over
 * several workgroups and merge the partial soft-maxes; 0 when the set is large enough not to need it. */
size_t gfc_attention_workspace_bytes(int n_problems, int max_nq, int heads);

/* In-place LayerNorm(eps 1e-5, affine) + exact (erf) GELU over rows of width 512.
 * Replaces ffn[1], ffn[2] (lightglue.py:143-148). */
int gfc_layernorm_gelu(float* x, int ld, int rows, int width, const float* gamma, const float* beta,
                       void* stream);

/* The WHOLE LightGlue FFN with its residual in one kernel (lightglue.py:143-148, called at :162-164,219-222):
 *   Y[M,256] = residual + ( GELU_erf( LayerNorm_512( [A0 | A1] * W0[512,K0+K1]^T + b0 ; gamma, beta, eps 1e-5 ) )
 *                           * W3[256,512]^T + b3 ).
 * Row-owning 128-row workgroup tiles: the row statistics, the [M,512] pre-activation AND the activated hidden tile stay
 * on chip (the hidden tile goes from the first GEMM's accumulators through LDS into the second GEMM).  residual
 * (nullable) and Y share the row stride ldy and may alias (in-place residual update); b3 nullable.  Bit-identical to
 * gfc_linear_layernorm_gelu followed by gfc_linear(..., residual). */
int gfc_ffn_fused(const float* A0, int lda0, int K0, const float* A1, int lda1, int K1, const float* W0, int ldw0,
                  const float* b0, const float* gamma, const float* beta, const float* W3, int ldw3, const float* b3,
                  const float* residual, float* Y, int ldy, int M, void* stream);

/* The first two stages of the LightGlue FFN in one kernel (lightglue.py:143-148, called at :164,221-222):
 *   Y[M,512] = GELU_erf( LayerNorm_512( [A0 | A1] * W[512,K0+K1]^T + bias ; gamma, beta, eps 1e-5 ) ).
 * Row-owning workgroup tiles (128 rows x all 512 columns): the row statistics stay on chip and the
 * pre-activation never reaches HBM.  N must be 512; same operand conventions as gfc_linear. */
int gfc_linear_layernorm_gelu(const float* A0, int lda0, int K0, const float* A1, int lda1, int K1, const float* W,
                              int ldw, const float* bias, const float* gamma, const float* beta, float* Y, int ldy,
                              int M, int N, void* stream);

/* fp16-operand forms of gfc_linear, gfc_batched_nt and gfc_attention (the GFC_LG_FP16 matcher): fp16 products on
 * v_mfma_f32_32x32x16_f16, fp32 sums; every fp32 -> fp16 rounding is to nearest even.
 * gfc_linear_f16: Y[M,N] = ( [A0 | A1] * W[N,K0+K1]^T + bias ) rotated, * alpha, + residual.  A0 / A1 are fp16
 *   (a*_f16 = 1; ld a multiple of 8) or fp32 (0; ld a multiple of 4, rounded to fp16 on the way in); W fp16 (ldw a
 *   multiple of 8); bias, residual (ld = ldy), rotary tables fp32; Y fp32 (y_f16 = 0) or fp16 (1).  Rotary on the
 *   columns < rot_cols (a multiple of 64) from either the packed table rot_cs [M][32][cos, sin] or rot_cos / rot_sin
 *   [M,64] (gfc_linear's tables).  K0, K1 multiples of 32 (A1 NULL when K1 = 0).
 * gfc_batched_nt_f16: for z < batch: Y_z[M,N] (fp32) = A_z[M,K] * B_z[N,K]^T, A and B fp16; strides in elements.
 * gfc_attention_f16: gfc_attention on fp16 Q, K, V (ld multiples of 8) with fp16 O; soft-max statistics in fp32,
 *   P rounded to fp16 for P.V; the same problem tables, key split and scratch. */
int gfc_linear_f16(const void* A0, int a0_f16, int lda0, int K0, const void* A1, int a1_f16, int lda1, int K1,
                   const void* W, int ldw, const float* bias, float alpha, const float* residual, const float* rot_cs,
                   const float* rot_cos, const float* rot_sin, int rot_cols, void* Y, int y_f16, int ldy, int M, int N,
                   void* stream);
int gfc_batched_nt_f16(const void* A, int lda, long long strideA, const void* Bm, int ldb, long long strideB, float* Y,
                       int ldy, long long strideY, int M, int N, int K, int batch, void* stream);
int gfc_attention_f16(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                      const int32_t* problems, int n_problems, int max_nq, int heads, float scale, void* ws,
                      size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * SuperPoint extractor
 * ---------------------------------------------------------------------------------- */
typedef struct {
  /* encoder conv1a..conv4b.  w[0]: [9][64] (cin = 1); w[1..7]: packed [9][cout][cin].
   * scale/shift: folded eval-mode BatchNorm (alpha = gamma/sqrt(var+eps), beta - mean*alpha),
   * NULL for the official (no-BN) variant. */
  const float* w[8];
  const float* bias[8];
  const float* scale[8];
  const float* shift[8];
  /* both 3x3 heads merged: 128 -> 512 = [detector hidden | descriptor hidden] */
  const float* wh;
  const float* bias_h;
  const float* scale_h;
  const float* shift_h;
  /* 1x1 detector 256 -> 65 ([65][256]) and 1x1 descriptor 256 -> desc_dim ([desc_dim][256]) */
  const float* wp;
  const float* bias_p;
  const float* scale_p;
  const float* shift_p;
  const float* wd;
  const float* bias_d;
  const float* scale_d;
  const float* shift_d;
  int desc_dim;
  /* conv_mode = 0: direct implicit GEMM on fp32 MFMA (gfc_conv3x3 / gfc_sp_stem).  (1 was the round-1 bf16x3-split
   * arithmetic, retired from the library in round 4: gfc_sp_dense rejects it.) */
  int conv_mode;
  /* conv_mode = 2: Winograd F(2x2,3x3) on the fp32 matrix pipe (gfc_conv3x3_wino / gfc_sp_stem_wino): w_wino[1..7] /
   * wh_wino are the filters transformed (in float64) and packed by gfc_pack_conv3x3_wino; w[0] (conv1a, cin = 1)
   * is still used.  Every product and accumulation is fp32; 2.25x fewer multiplications than conv_mode 0. */
  const float* w_wino[8];
  const float* wh_wino;
  /* conv_mode = 2, optional: conv1b's filters transformed for Winograd F(4x4,3x3) and packed by
   * gfc_pack_conv3x3_wino43.  When set, the stem (conv1a + conv1b + pool) runs as gfc_sp_stem_wino43; NULL (or
   * $GFC_STEM_F43=0): gfc_sp_stem_wino (F(2x2,3x3), w_wino[1]).  Only the stem: for deeper layers F(4x4,3x3) does
   * not hold the 1e-5 heat-map bar (tools/micro/winograd_f43_numerics.py). */
  const float* w_stem_wino43;
} gfc_sp_params;

typedef enum { GFC_SAMPLE_OPEN = 0, GFC_SAMPLE_LEGACY = 1, GFC_SAMPLE_FIXED = 2 } gfc_sample_mode;

/* Optional per-launch timing of a hot kernel (host struct owned by the caller, no global state): the entry point
 * that takes a gfc_trace brackets every launch of ITS traced kernel with hipEventRecord(start[count]) /
 * hipEventRecord(stop[count]) on the call's stream and increments count (while count < capacity):
 *   gfc_sp_dense           -> the stem kernel (conv1a + conv1b + pool, 44 % of the extractor's FLOPs),
 *   gfc_lg_forward_packed  -> the attention launches (2 brackets per layer: self, cross; the cross bracket holds one
 *                             launch, or every launch of gfc_attention_cross_stored), the largest share of the step.
 * Events come from gfc_event_create().  Used by bench.py for the live roofline figures; NULL in production. */
typedef struct {
  void** start;
  void** stop;
  int capacity;
  int count;
} gfc_trace;

int gfc_event_create(void** event);
int gfc_event_destroy(void* event);
/* milliseconds between two recorded events (both must have completed) */
int gfc_event_elapsed_ms(void* start, void* stop, float* ms);

/* bench-only: what the matrix pipe of THIS device sustains.  Every SIMD of every CU issues `mfmas_per_wave`
 * back-to-back v_mfma_f32_32x32x2_f32 (registers only, 4 accumulators); returns the fp32-MFMA rate over the whole
 * launch and the shader clock it ran at (s_memtime ticks, = shader cycles, per 100 MHz s_memrealtime tick).  The
 * data-sheet peak (157.3 TFLOP/s) assumes 2.4 GHz; under full matrix load the part clocks lower. */
int gfc_probe_mfma_peak(int mfmas_per_wave, float* tflops, float* shader_clock_ghz, void* stream);

size_t gfc_sp_workspace_bytes(int B, int C, int H, int W);

/* image [B,C,H,W] (C = 1 or 3, RGB -> grey fused) -> heat-map [B, 8*(H/8), 8*(W/8)] (softmax over
 * 65 logits, dustbin dropped, depth-to-space) and raw descriptor map [B,H/8,W/8,desc_dim]
 * (NHWC, before L2 normalisation).  superpoint_open.py:128-144; superpoint.py:208-241. */
int gfc_sp_dense(const gfc_sp_params* p, const float* image, int B, int C, int H, int W, float* heatmap,
                 float* desc_raw, void* ws, size_t ws_bytes, gfc_trace* trace, void* stream);

/* Detector head in one launch: 1x1 convolution 256 -> 65 (+ eval-BN affine when scale / shift are given), softmax over the
 * 65 logits of every cell, dustbin dropped, 8x8 depth-to-space:  heat[b, 8y+i, 8x+j] = softmax_c(W . hidden[b,y,x,:] + b)[8i+j].
 * hidden [B*h8*w8][lda] NHWC rows (the detector's 256 hidden channels first, lda >= 256, a multiple of 4); w [65][256];
 * hidden and w 16-byte aligned (GFC_ERR_INVALID otherwise: both are read with 128-bit loads);
 * bias / scale / shift [65] (scale and shift nullable together); heat [B][8 h8][8 w8].  The logits never reach HBM.
 * superpoint_open.py:111-114,138-144; superpoint.py:193-194,229-235 (part of gfc_sp_dense). */
int gfc_sp_detector_head(const float* hidden, int lda, const float* w, const float* bias, const float* scale,
                         const float* shift, int B, int h8, int w8, float* heat, void* stream);

/* Max-pool NMS with two recovery rounds, then outer `border` rows/cols := -1.
 * valid_wh (nullable, int32 [B,2] = (w,h)): right/bottom border measured from the true image
 * extent.  superpoint_open.py:36-51,148-154; superpoint.py:63-83,249-260.  radius <= 4. */
int gfc_sp_nms(const float* heatmap, int B, int H, int W, int radius, int border, const int32_t* valid_wh,
               float* out, void* stream);

size_t gfc_sp_select_workspace_bytes(int B, int H, int W);

/* Per image: candidates = pixels with score > threshold in row-major order; if more than k
 * (k < 0: unlimited) the k best by descending score (ties: lower linear index first), else all
 * of them in row-major order.  kpts [B,cap,2] (x,y as floats), scores [B,cap], counts [B].
 * cap = row capacity of the output arrays (>= k when k >= 0; H*W when unlimited).
 * superpoint_open.py:156-192,54-58; superpoint.py:262-300,86-90. */
int gfc_sp_select(const float* scores, int B, int H, int W, float threshold, int k, int cap, float* kpts,
                  float* kscores, int32_t* counts, void* ws, size_t ws_bytes, void* stream);

/* gfc_sp_nms + gfc_sp_select in one pass over the heat-map: the NMS kernel appends every pixel above the
 * threshold to the per-image key list (unordered; keys are unique, so the result is still deterministic) and the
 * selection kernel skips its scan.  nms_out (nullable) receives the suppressed map.
 * 1 <= k <= 8192, 1 <= radius <= 4 (radius 0 keeps ~all pixels: use the two separate stages). */
size_t gfc_sp_nms_select_workspace_bytes(int B, int H, int W);
int gfc_sp_nms_select(const float* heatmap, int B, int H, int W, int radius, int border, const int32_t* valid_wh,
                      float threshold, int k, int cap, float* nms_out, float* kpts, float* kscores, int32_t* counts,
                      void* ws, size_t ws_bytes, void* stream);

/* Bilinear sampling of L2-normalised dense descriptors at keypoints + L2 normalisation.
 * desc_raw [B,h,w,D] un-normalised (normalisation over D is applied per corner on the fly),
 * kpts [B,cap,2] integer-valued pixel coordinates, n_kpts [B] (nullable = cap for all),
 * out [B,cap,D].  If kpts_out != NULL it receives kpts + 0.5 (may alias kpts).
 * superpoint_open.py:22-33,133-135,221; superpoint.py:120-152. */
int gfc_sp_sample(const float* desc_raw, int B, int h, int w, int D, const float* kpts, const int32_t* n_kpts,
                  int cap, int mode, float* out, float* kpts_out, void* stream);

/* pad_and_stack(mode="random_c") for key points + zeros for their scores, in place, one launch, no host sync
 * (gluefactory/models/utils/misc.py:19-62,103-113; force_num_keypoints at superpoint_open.py:193-219,
 * superpoint.py:330-365, disk_kornia.py:109-124): slots in [counts[b], k) get per-coordinate uniform samples in
 * [min, max] of the image's own key points ([low, high] when it has none; high = min over `sizes` if given, else
 * high_fallback) from a counter-based generator keyed by (seed, image, slot) -- random padding, as in the reference. */
int gfc_sp_pad_keypoints(float* kpts, float* kscores, const int32_t* counts, int B, int cap, int k, float low,
                         const float* sizes, int n_sizes, float high_fallback, unsigned int seed, void* stream);

/* L2-normalise rows in place (dense_outputs: F.normalize over channels, superpoint_open.py:133-135). */
int gfc_l2norm_rows(float* x, long long rows, int width, void* stream);

/* ------------------------------------------------------------------------------------
 * DISK extractor: the stages behind the network (disk_kornia.py:42-47,129-137; kornia's
 * heatmap_to_keypoints / nms / merge_with_descriptors restated: parity for them is unpinned, kornia is absent)
 * ---------------------------------------------------------------------------------- */
/* heat-map [B,H,W] -> key points.  A pixel survives iff it is the first maximum (row-major window scan, as
 * F.max_pool2d(return_indices=True) reports it) of the window x window neighbourhood centred on it and > cutoff.
 * n >= 0: keep the scores strictly above the (n+1)-th largest survivor (min(n+1, count)-th: with count <= n the
 * minimum is dropped), first n in row-major order; n < 0: all survivors.  kpts [B,cap,2] (x,y as floats, integer
 * valued, NOT sorted by score), kscores [B,cap], counts [B].  cap >= n (n >= 0) or >= H*W.  window odd, <= 9. */
size_t gfc_disk_select_workspace_bytes(int B, int H, int W);
int gfc_disk_nms_select(const float* heatmap, int B, int H, int W, int window, float cutoff, int n, int cap,
                        float* kpts, float* kscores, int32_t* counts, void* ws, size_t ws_bytes, void* stream);
/* dense descriptors [B,D,H,W] (NCHW) read at the integer key-point pixels and L2-normalised over D
 * (F.normalize, eps 1e-12) -> out [B,cap,D]; slots >= counts[b] (counts nullable) are zero-filled. */
int gfc_disk_gather_descriptors(const float* dense_nchw, int B, int D, int H, int W, const float* kpts,
                                const int32_t* counts, int cap, float* out, void* stream);
/* the same from an NHWC array [B,H,W,D] (what gfc_disk_conv5x5 writes: one contiguous row per key point) */
int gfc_disk_gather_descriptors_nhwc(const float* dense_nhwc, int B, int D, int H, int W, const float* kpts,
                                     const int32_t* counts, int cap, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * DISK network (disk_kornia.py:24-47 -> kornia.feature.DISK.heatmap_and_dense_descriptors): the thin U-Net
 * Unet(in_features=3, size=5, down=[16,32,64,64,64], up=[64,64,64,desc_dim+1]) of kornia/feature/disk/_unets,
 * restated from kornia's published source (absent offline: NETWORK PARITY UNPINNED).  Activations are NHWC fp32.
 * One "Conv" of that network = [InstanceNorm2d -> PReLU ->] Conv2d(5x5, padding 2, bias): the statistics come from
 * gfc_disk_instnorm_stats, normalisation and gate are applied while gfc_disk_conv5x5 stages its input.
 * ---------------------------------------------------------------------------------- */
/* Conv2d weights OIHW [cout][cin][5][5] -> the layout gfc_disk_conv5x5 reads (cin padded to 16, cout to 32). */
size_t gfc_disk_conv5x5_packed_floats(int cout, int cin);
int gfc_disk_pack_conv5x5(const float* w_oihw, float* w_packed, int cout, int cin, void* stream);
/* y[b,y,x, 0:co_count] (channel stride ldy >= co_count: a slice of a wider, concatenated tensor) =
 *   conv5x5(gate(norm(x)))[b,y,x, co_first : co_first + co_count] + bias  of a layer with cout_total output channels
 * (co_first % 32 == 0; the whole layer: co_first 0, co_count cout_total -- DISK's last layer is run as descriptors
 * [0,128) and heat-map [128,129) into two arrays);  x [B,H,W,cin] contiguous, cin % 4 == 0 (channels beyond cin of the
 * last 16-chunk count as zero); mean/rstd [B,cin] (both or neither; InstanceNorm2d without affine), prelu [cin] or
 * NULL (PReLU slope per channel); zero padding is applied AFTER normalisation and gate, as Conv2d pads its own input.
 * w_packed / bias are the layer's whole arrays (not offset by the caller). */
int gfc_disk_conv5x5(const float* x, const float* mean, const float* rstd, const float* prelu, const float* w_packed,
                     const float* bias, float* y, int ldy, int B, int H, int W, int cin, int cout_total, int co_first,
                     int co_count, void* stream);
/* per (image, channel) mean and 1 / sqrt(biased variance + eps) over H x W of x [B,H,W,C] contiguous
 * (float64 sums, fixed summation order); C in {16, 32, 64, 80, 96, 128} or any C with 480 % (C/4) == 0. */
size_t gfc_disk_instnorm_workspace_bytes(int B, int C);
int gfc_disk_instnorm_stats(const float* x, int B, int H, int W, int C, float eps, float* mean, float* rstd, void* ws,
                            size_t ws_bytes, void* stream);
/* F.avg_pool2d(x, 2): x [B,H,W,C] with channel stride ldx (H, W even) -> y [B,H/2,W/2,C] contiguous */
int gfc_disk_avgpool2(const float* x, int ldx, int B, int H, int W, int C, float* y, void* stream);
/* F.interpolate(scale_factor=2, mode="bilinear", align_corners=False): x [B,h,w,C] contiguous -> the first C
 * channels of y [B,2h,2w,ldy] */
int gfc_disk_upsample2(const float* x, int B, int h, int w, int C, float* y, int ldy, void* stream);
/* image [B,3,H,W] -> [B,H,W,4] (fourth channel zero): the NHWC input of the first convolution */
int gfc_disk_nchw3_to_nhwc4(const float* image, int B, int H, int W, float* y, void* stream);

/* ------------------------------------------------------------------------------------
 * LightGlue matcher
 * ---------------------------------------------------------------------------------- */
#define GFC_LG_MAX_LAYERS 16
typedef struct {
  int n_layers;    /* 9 */
  int input_dim;   /* 256, or 128 with input_proj */
  const float* input_proj_w; /* [256][input_dim] or NULL */
  const float* input_proj_b;
  const float* posenc_wr;    /* [32][posenc_dim] */
  int posenc_dim;            /* 2, or 4 with add_scale_ori (0 is read as 2) */
  /* self block.  wqkv rows re-ordered to [q(256) | k(256) | v(256)], each head-major:
   * new row s*256 + h*64 + d  <-  state-dict row h*192 + d*3 + s   (lightglue.py:157-159) */
  const float* wqkv[GFC_LG_MAX_LAYERS];
  const float* bqkv[GFC_LG_MAX_LAYERS];
  /* out_proj.  NULL = folded into s_ffn0_w at load time (no GEMM of its own):
   *   ffn0(cat[x, out_proj(ctx)]) = [x | ctx] . [W0a | W0b.Wo]^T + (b0 + W0b.bo)   (lightglue.py:163-164) */
  const float* s_out_w[GFC_LG_MAX_LAYERS];
  const float* s_out_b[GFC_LG_MAX_LAYERS];
  const float* s_ffn0_w[GFC_LG_MAX_LAYERS]; /* [512][512] */
  const float* s_ffn0_b[GFC_LG_MAX_LAYERS];
  const float* s_ln_g[GFC_LG_MAX_LAYERS];
  const float* s_ln_b[GFC_LG_MAX_LAYERS];
  const float* s_ffn3_w[GFC_LG_MAX_LAYERS]; /* [256][512] */
  const float* s_ffn3_b[GFC_LG_MAX_LAYERS];
  /* cross block.  c_qkv_w = [to_qk ; to_v] stacked to [512][256] */
  const float* c_qkv_w[GFC_LG_MAX_LAYERS];
  const float* c_qkv_b[GFC_LG_MAX_LAYERS];
  const float* c_out_w[GFC_LG_MAX_LAYERS]; /* to_out; NULL = folded into c_ffn0_w (lightglue.py:219-222) */
  const float* c_out_b[GFC_LG_MAX_LAYERS];
  const float* c_ffn0_w[GFC_LG_MAX_LAYERS];
  const float* c_ffn0_b[GFC_LG_MAX_LAYERS];
  const float* c_ln_g[GFC_LG_MAX_LAYERS];
  const float* c_ln_b[GFC_LG_MAX_LAYERS];
  const float* c_ffn3_w[GFC_LG_MAX_LAYERS];
  const float* c_ffn3_b[GFC_LG_MAX_LAYERS];
  /* assignment heads log_assignment.{i} (lightglue.py:272-291).  gfc_lg_forward uses layer n_layers-1;
   * the adaptive path (early stop) may read any layer's head, and every layer's matchability for pruning */
  const float* final_proj_w[GFC_LG_MAX_LAYERS]; /* [256][256] */
  const float* final_proj_b[GFC_LG_MAX_LAYERS];
  const float* matchability_w[GFC_LG_MAX_LAYERS]; /* [256] */
  const float* matchability_b[GFC_LG_MAX_LAYERS]; /* [1] */
  /* token_confidence.{i}.token.0 (lightglue.py:69-80), i < n_layers-1 */
  const float* token_w[GFC_LG_MAX_LAYERS]; /* [256] */
  const float* token_b[GFC_LG_MAX_LAYERS]; /* [1] */
  /* Arithmetic of the matrix products.  GFC_LG_FP32 (0, what a zero-initialised struct holds): every contraction in
   * exact fp32.  GFC_LG_FP16 (1): products in fp16, sums in fp32 (v_mfma_f32_32x32x16_f16) for input_proj, the QKV
   * projections, out_proj / to_out (when not folded), ffn[0], ffn[3], Q.K^T and P.V of both attentions, final_proj
   * and the assignment similarity; their operands are rounded to nearest even, and the buffers that are only an
   * operand (qkv, attention output, out_proj output, final_proj output) are held in fp16.  Positional encoding,
   * soft-max statistics, LayerNorm, GELU, residual adds, matchability, token confidence, the log double soft-max and
   * the filter stay fp32, and so does the row buffer.  The fp16 path needs the fp16 copies below (same layouts as the
   * fp32 matrices; a missing one: GFC_ERR_INVALID) and fits in the workspaces the fp32 path is sized for. */
  int precision;
  const void* input_proj_w16;                  /* fp16 [256][input_dim] or NULL (input_dim == 256) */
  const void* wqkv16[GFC_LG_MAX_LAYERS];
  const void* s_out_w16[GFC_LG_MAX_LAYERS];    /* NULL when folded */
  const void* s_ffn0_w16[GFC_LG_MAX_LAYERS];
  const void* s_ffn3_w16[GFC_LG_MAX_LAYERS];
  const void* c_qkv_w16[GFC_LG_MAX_LAYERS];
  const void* c_out_w16[GFC_LG_MAX_LAYERS];    /* NULL when folded */
  const void* c_ffn0_w16[GFC_LG_MAX_LAYERS];
  const void* c_ffn3_w16[GFC_LG_MAX_LAYERS];
  const void* final_proj_w16[GFC_LG_MAX_LAYERS];
} gfc_lg_params;
#define GFC_LG_FP32 0
#define GFC_LG_FP16 1

size_t gfc_lg_workspace_bytes(int B, int M, int N);

/* Rotary tables: kpts [rows,2] pixel coords, per image i: rows [row0[i], row0[i]+n[i]) are
 * normalised with size[i] = (w,h): (k - size/2) / (max(size)/2), projected by Wr [32][dim];
 * cos/sin [rows,64] with each value repeated twice.  lightglue.py:28-40,53-66.
 * dim = 4 (conf.add_scale_ori, lightglue.py:359,436-453): scale_ori [rows,2] = (scale, orientation) is appended to
 * the normalised key point before the projection; dim = 2: scale_ori must be NULL. */
int gfc_lg_posenc(const float* kpts, const float* scale_ori, const float* sizes, const int32_t* row0, const int32_t* n,
                  int n_images, int max_n, const float* wr, int dim, float* cos_out, float* sin_out, void* stream);

/* log assignment [B,M+1,N+1] from sim [B,M,N] (ld = N), z0 [B,M], z1 [B,N]:
 * sigmoid_log_double_softmax, lightglue.py:257-269.  ws: 2*B*(M+N) floats. */
int gfc_lg_log_assignment(const float* sim, const float* z0, const float* z1, int B, int M, int N, float* out,
                          void* ws, size_t ws_bytes, void* stream);

/* Mutual arg-max matches from a log assignment [B,M+1,N+1]: filter_matches, lightglue.py:294-319.
 * m0 [B,M] int64, m1 [B,N] int64, ms0 [B,M], ms1 [B,N].  Ties: first index.
 * ws: B*(M+N)*(4+4) bytes. */
int gfc_lg_filter_matches(const float* scores, int B, int M, int N, float threshold, int64_t* m0, int64_t* m1,
                          float* ms0, float* ms1, void* ws, size_t ws_bytes, void* stream);

/* One transformer layer (self block on every image + bidirectional cross block, lightglue.py:231-245) on the
 * packed descriptor rows x [rows,256] (updated in place), with rotary tables cos/sin [rows,64] and attention
 * problem tables {q_row0, n_q, kv_row0, n_kv} (int32 x4 per entry, n_problems entries each; device).
 * Building block of the whole-matcher entry points; driven layer by layer by the host for adaptive depth / width
 * (early stop and point pruning, lightglue.py:500-521), where rows are re-packed between layers. */
size_t gfc_lg_layer_workspace_bytes(int rows);
int gfc_lg_layer(const gfc_lg_params* p, int layer, float* x, const float* cos_tab, const float* sin_tab, int rows,
                 const int32_t* self_problems, const int32_t* cross_problems, int n_problems, int max_n, void* ws,
                 size_t ws_bytes, void* stream);

/* out[row] = x[row,:256] . w + b, optionally through a sigmoid: TokenConfidence (lightglue.py:69-80) and
 * MatchAssignment.get_matchability (lightglue.py:290-291). */
int gfc_lg_rowdot(const float* x, int ld, int rows, const float* w, const float* b, int apply_sigmoid, float* out,
                  void* stream);

/* MatchAssignment of layer `layer` + filter_matches on x0 [B*M,256], x1 [B*N,256]
 * (lightglue.py:279-288,294-319); outputs as gfc_lg_forward. */
size_t gfc_lg_assign_workspace_bytes(int B, int M, int N);
int gfc_lg_assign(const gfc_lg_params* p, int layer, const float* x0, const float* x1, int B, int M, int N,
                  float threshold, int64_t* m0, int64_t* m1, float* ms0, float* ms1, float* log_assignment, void* ws,
                  size_t ws_bytes, void* stream);

/* Whole matcher: LightGlue.forward (lightglue.py:422-553) with early stop / pruning disabled.  The three whole-matcher
 * entry points (gfc_lg_forward, gfc_lg_forward_packed, gfc_lg_forward_ragged) describe their batch as groups of equal
 * (m, n) pairs -- a uniform batch is one group -- and run the same launch sequence on it: problem tables, rotary tables,
 * input_proj (input_dim != 256), n_layers x gfc_lg_layer, gfc_lg_assign once per group.  Every workspace size comes
 * from the same planner, and every entry point refuses a batch whose total row count B*(M+N) (ragged: sum(m) + sum(n))
 * exceeds INT_MAX / 768 (workspace 0, GFC_ERR_INVALID).
 * kpts0 [B,M,2], kpts1 [B,N,2] (pixel coords), desc0 [B,M,Din], desc1 [B,N,Din],
 * size0/size1 [B,2] = (w,h) floats; scale_ori0 [B,M,2] / scale_ori1 [B,N,2] = (scales, oris) of the key points when
 * p->posenc_dim == 4 (add_scale_ori), NULL otherwise.  Outputs as filter_matches + log_assignment [B,M+1,N+1]
 * + ref_desc0 [B,M,256], ref_desc1 [B,N,256] (last-layer descriptors, lightglue.py:495-498).  The two sides are
 * packed into the front of ws (descriptors read in place when desc1 starts where desc0 ends), then the packed
 * layout below runs on the rest. */
int gfc_lg_forward(const gfc_lg_params* p, const float* kpts0, const float* kpts1, const float* desc0,
                   const float* desc1, const float* size0, const float* size1, const float* scale_ori0,
                   const float* scale_ori1, int B, int M, int N,
                   float threshold, int64_t* m0, int64_t* m1, float* ms0, float* ms1, float* log_assignment,
                   float* ref_desc0, float* ref_desc1, void* ws, size_t ws_bytes, void* stream);

/* The same matcher on PACKED rows, without a single device-to-device copy: kpts [B*M + B*N, 2] and desc
 * [B*M + B*N, Din] hold the rows of side 0 (pair-major) followed by the rows of side 1 -- the layout one extractor
 * call over both views' images produces; scale_ori [B*M + B*N, 2] or NULL likewise.  `rows` [B*M + B*N, 256] is the
 * caller's row buffer: layer 0 reads the descriptors where they are (desc is never written), every later layer
 * works in place on `rows`, which ends up holding the last layer's descriptors = ref_descriptors0 (first B*M rows)
 * and ref_descriptors1.  attention_trace: optional event pairs around the attention launches (see gfc_trace).
 * The uniform batch: one group of B pairs.  Replaces the same reference lines as gfc_lg_forward (lightglue.py:422-553). */
size_t gfc_lg_packed_workspace_bytes(int B, int M, int N);
int gfc_lg_forward_packed(const gfc_lg_params* p, const float* kpts, const float* desc, const float* size0,
                          const float* size1, const float* scale_ori, int B, int M, int N, float threshold, int64_t* m0,
                          int64_t* m1, float* ms0, float* ms1, float* log_assignment, float* rows, void* ws,
                          size_t ws_bytes, gfc_trace* attention_trace, void* stream);

/* The same matcher over B pairs with THEIR OWN key-point counts (m[i], n[i] > 0, host arrays, B <=
 * GFC_LG_MAX_RAGGED_PAIRS): the regime of the reference's evaluation loop, which calls the matcher once per pair only
 * because the IMAGES of an HPatches-style list differ in size (gluefactory/utils/export_predictions.py:36-45,
 * datasets/hpatches.py:60) -- LightGlue itself is image-size independent once the key points exist.  One launch
 * sequence for all pairs: the layers run over all rows at once (the attention kernel takes a per-problem table
 * anyway), the assignment head once per GROUP = maximal run of consecutive pairs with equal (m, n).
 * Row layout of kpts [R,2] / desc [R,Din] / scale_ori [R,2] / rows [R,256], R = sum(m) + sum(n): group after group,
 * inside a group the side-0 rows of its pairs (pair-major) followed by their side-1 rows -- i.e. every group is laid out
 * as gfc_lg_forward_packed lays out a uniform batch (B equal pairs = one group = the same batch, the same launches and
 * the same workspace size as that function's).
 * Outputs are flat, in pair order: m0 / ms0 [sum m], m1 / ms1 [sum n], log_assignment [sum (m+1)(n+1)] (pair i's
 * [m+1, n+1] matrix contiguous).  size0 / size1 [B,2] (device).  No allocation, no synchronisation; the counts travel
 * to the device as kernel arguments.  Same arithmetic per pair as gfc_lg_forward_packed (lightglue.py:422-553). */
#define GFC_LG_MAX_RAGGED_PAIRS 128
size_t gfc_lg_ragged_workspace_bytes(int B, const int32_t* m, const int32_t* n);
int gfc_lg_forward_ragged(const gfc_lg_params* p, const float* kpts, const float* desc, const float* size0,
                          const float* size1, const float* scale_ori, int B, const int32_t* m, const int32_t* n,
                          float threshold, int64_t* m0, int64_t* m1, float* ms0, float* ms1, float* log_assignment,
                          float* rows, void* ws, size_t ws_bytes, gfc_trace* attention_trace, void* stream);

/* Adaptive depth / width for a BATCH of pairs: the step between layer `layer` and the next one
 * (lightglue.py:500-521,555-580) for B <= GFC_LG_MAX_RAGGED_PAIRS live pairs, on the device.
 *
 * In: the live rows x [rows,256] with cos_tab / sin_tab [rows,64] and ind [rows] (each row's index in its image's
 * un-pruned key-point list); seg [2B][2] = {row0, n} of side 0 (entry 2b) and side 1 (entry 2b + 1) of pair b; pairs
 * [B][2] = {un-pruned m + n (the denominator of check_if_stop's ratio), slot}; prune_off [n_slots][2] = where image
 * `side` of slot `slot` starts in the prune counters (static; the slot is the pair's position in the caller's list and
 * travels with the pair through every step).  All tables live on the device, 16-byte aligned, like the row buffers.
 *
 * Decide.  Per row tok = sigmoid(x . token_w[layer] + token_b[layer]) and sc = sigmoid(x . matchability_w[layer] +
 * matchability_b[layer]) from one read of the row, bit for bit what gfc_lg_rowdot(apply_sigmoid = 1) returns.  Per pair
 * cnt = #(tok < thr) and stop = (double)(1.0f - (float)cnt / (float)(m + n)) > depth_confidence (do_stop).  Per row of a
 * pair that goes on: keep = sc > keep_thr || tok <= thr (do_prune; the second term only with do_stop), where keep_thr is
 * (float)(1 - width_confidence).  At least one of do_stop / do_prune must be set.
 *
 * Re-pack (a copy: x_out, cos_out, sin_out, ind_out are a second set of buffers of `rows` rows, never the inputs).  The
 * pairs that stay live come first, in their order, each as its kept side-0 rows followed by its kept side-1 rows
 * (stable); the pairs that finish at this step follow, in their order and in the same form: a pair that stopped with
 * all its rows, a pair one side of which emptied with the rows it kept.  prune [prune_len] (int32) gets + 1 at
 * prune_off[slot][side] + ind for every kept row of a pair that did not stop.  Rows behind the last pair are not written.
 *
 * Tables of the next layer: self_problems / cross_problems [2 * live][4] as gfc_lg_layer takes them, seg_out [2B][2]
 * and pairs_out [B][2] in the output order (never the input tables).
 *
 * report [B][4] = {state, cm, cn, cnt} of input pair b (cm, cn: its rows in the output; cnt 0 without do_stop): all the
 * host needs to know where everything went, and the only thing it has to read.  max_n >= every segment's n sizes the
 * grid (longer segments are still packed completely).  No allocation, no synchronisation. */
#define GFC_LG_ADAPTIVE_LIVE 0
#define GFC_LG_ADAPTIVE_STOPPED 1
#define GFC_LG_ADAPTIVE_EMPTIED 2
size_t gfc_lg_adaptive_step_workspace_bytes(int B, int rows);
int gfc_lg_adaptive_step(const gfc_lg_params* p, int layer, const float* x, const float* cos_tab, const float* sin_tab,
                         const int32_t* ind, int rows, const int32_t* seg, const int32_t* pairs,
                         const int32_t* prune_off, int n_slots, int B, int max_n, float thr, float keep_thr,
                         double depth_confidence, int do_stop, int do_prune, float* x_out, float* cos_out,
                         float* sin_out, int32_t* ind_out, int32_t* prune, int prune_len, int32_t* self_problems,
                         int32_t* cross_problems, int32_t* seg_out, int32_t* pairs_out, int32_t* report, void* ws,
                         size_t ws_bytes, void* stream);

/* Nearest-neighbour matcher ("next" row; the matcher of the reference's superpoint+NN configurations):
 * sim = desc0 . desc1^T, top-2 per row / column, ratio test d1 <= ratio^2 d2 and distance test d1 <= th^2 on
 * d = 2(1 - sim) (thresholds <= 0 disable a test; they are doubles because the reference squares the configured
 * double and rounds the square to fp32 once -- an fp32 threshold squared in fp32 differs by an ulp and flips a test met
 * with equality; a binding that still declares them float passes garbage without any error: re-declare it),
 * ties of the best: lower index wins; optional mutual check; matching scores are 0/1;
 * log_assignment (nullable) [B,M+1,N+1] = log_softmax rows + log_softmax columns, zero border.
 * Replaces NearestNeighborMatcher._forward (gluefactory/models/matchers/nearest_neighbor_matcher.py:15-79). */
size_t gfc_nn_workspace_bytes(int B, int M, int N);
int gfc_nn_match(const float* desc0, const float* desc1, int B, int M, int N, int D, double ratio_thresh,
                 double distance_thresh, int mutual, int64_t* m0, int64_t* m1, float* ms0, float* ms1, float* sim,
                 float* log_assignment, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Evaluation ("next" row: the caller right after the matcher)
 * ---------------------------------------------------------------------------------- */

/* Match metrics against a ground-truth homography, one workgroup per pair, M x N distance matrix never
 * materialised.  kp0 [B,M,2], kp1 [B,N,2] (pixels), m0 [B,M] int64 (-1 = unmatched), H / Hinv [B,3,3]
 * (H_0to1 and its inverse, row-major).  out [B,6] = prec@1px, prec@3px, num_matches, num_keypoints,
 * gt_match_recall@pos_th, gt_match_precision@pos_th;  gt_m0_out (nullable) [B,M] int64 ground-truth
 * matches (-1 unmatched, -2 ignore).  Replaces eval_matches_homography (gluefactory/eval/utils.py:141-185),
 * sym_homography_error (geometry/homography.py:314-323), gt_matches_from_homography
 * (geometry/gt_generation.py:730-801; the evaluation calls it with pos_th = neg_th = 3).
 * A match index >= N names no key point of image 1: it is never read, it counts in num_matches (and, with a ground
 * truth other than ignore, in the precision denominator), its transfer error is infinite (in neither prec@), and it
 * equals no ground-truth index.  (gfc_eval_homography_dlt skips such a match.)
 * Every key point of a pair lives in LDS: GFC_ERR_UNSUPPORTED (nothing launched) exactly when
 * gfc_eval_matches_homography_lds_bytes(M, N) = 16 M + 20 N + the kernel's static LDS exceeds 160 KB (163840 bytes);
 * about 4500 x 4500 key points.  GFC_ERR_LAUNCH when the runtime refuses more than 64 KB of dynamic LDS. */
size_t gfc_eval_matches_homography_lds_bytes(int M, int N);
int gfc_eval_matches_homography(const float* kp0, const float* kp1, const int64_t* m0, const float* H,
                                const float* Hinv, int B, int M, int N, float pos_th, float neg_th, float* out,
                                int64_t* gt_m0_out, void* stream);

/* Soft-argmax refinement of selected key points (official variant, `refinement_radius` > 0): kpts [B,cap,2] (x, y,
 * integer valued, the first counts[b] rows of image b; counts nullable = all cap) move by the score-weighted mean
 * offset inside the (2*radius+1)^2 window of the dense heat-map [B,H,W] (zero outside).  Replaces
 * soft_argmax_refinement (gluefactory_nonfree/superpoint.py:100-116, called at :302-305). */
int gfc_sp_refine_keypoints(const float* heatmap, int B, int H, int W, float* kpts, const int32_t* counts, int cap,
                            int radius, void* stream);

/* Specular-mask filtering of key points (reference gluefactory/models/extractors/utils.py:4-42; mask [B,Hm,Wm] bytes,
 * non-zero = keep; image_wh nullable [B,2] int32 = (w, h): the mask is cropped to it, key points beyond are dropped).
 * gfc_sp_mask_scores: the open variant's order (superpoint_open.py:177-188, filter BEFORE top-k): every pixel of the
 * suppressed score map [B,H,W] outside the mask becomes -inf, then gfc_sp_select runs on it.
 * gfc_sp_filter_keypoints: the official variant's order (gluefactory_nonfree/superpoint.py:310-328, filter AFTER
 * top-k): stable in-place compaction of kpts [B,cap,2] (x, y before the +0.5 offset) / kscores [B,cap]; counts [B]
 * is read and updated.  A key point survives when floor/ceil(kp - keypoint_offset) are inside and the mask is set on
 * all four pixels (the reference's callers pass keypoint_offset = 0). */
int gfc_sp_mask_scores(float* scores, int B, int H, int W, const uint8_t* mask, int Hm, int Wm, const int32_t* image_wh,
                       void* stream);
int gfc_sp_filter_keypoints(float* kpts, float* kscores, int32_t* counts, int B, int cap, const uint8_t* mask, int Hm,
                            int Wm, const int32_t* image_wh, float keypoint_offset, void* stream);

/* Weighted DLT homography from the predicted matches and its corner error ("next" row rank 3).  kp0 [B,M,2],
 * kp1 [B,N,2], m0 [B,M] int64 (-1 = unmatched), scores0 [B,M] (the weights), H_gt [B,9] row-major, image_size0 [B,2]
 * = (w, h) of view 0.  H_out [B,9]: normalised-DLT estimate divided by (H[2][2] + 1e-8), all +inf when a pair has
 * fewer than 4 matches or the estimate is not finite; err_out [B]: mean distance of the 4 warped image corners to
 * their ground-truth positions (+inf likewise).  Replaces eval_homography_dlt (gluefactory/eval/utils.py:276-302):
 * kornia's find_homography_dlt (third-party, unpinned) + homography_corner_error (geometry/homography.py:336-342). */
int gfc_eval_homography_dlt(const float* kp0, const float* kp1, const int64_t* m0, const float* scores0,
                            const float* H_gt, const float* image_size0, int B, int M, int N, float* H_out,
                            float* err_out, void* stream);

/* Robust homography from the predicted matches: RANSAC, MSAC-scored at T thresholds in one pass, locally optimised by
 * the normalised DLT above (DESIGN.md "Robust homography"; the estimator behind eval_homography_robust,
 * gluefactory/eval/utils.py:225-273 -- there OpenCV / PoseLib: parity with either is unpinned).  kp0 [B,M,2],
 * kp1 [B,N,2], m0 [B,M] int64 (a match is 0 <= m0[i] < N), stream_id [B] int64 (nullable: 0..B-1) names the random
 * stream of a pair: with (seed, stream_id) fixed a pair's result does not depend on the batch it is in.  H_gt [B,9] and
 * image_size0 [B,2] are given together with err_out or all three are NULL.  thresholds: T values in pixels in HOST
 * memory, 1 <= T <= 8, each positive and finite.  Outputs per (pair, threshold): H_out [B,T,9] fp64 (the model as computed) divided by H[2][2];
 * inliers [B,T,M] uint8 over key points 0; num_inliers [B,T] int32; success [B,T] uint8; best_hypothesis [B,T] int32
 * (the winning sample, -1 on failure); H_minimal [B,T,9] fp64 (its model before the local optimisation); err_out [B,T]
 * the corner error of H_out rounded to fp32, as gfc_eval_homography_dlt.  Fewer than 4 matches or no non-degenerate sample: success 0, H identity,
 * no inliers, error +inf.  GFC_ERR_INVALID (nothing launched): B <= 0, M < 0, N < 0, T outside 1..8,
 * num_hypotheses <= 0, lo_iters < 0, a threshold that is not positive and finite, a NULL required pointer. */
size_t gfc_eval_homography_ransac_workspace_bytes(int B, int M, int T, int num_hypotheses);
int gfc_eval_homography_ransac(const float* kp0, const float* kp1, const int64_t* m0, const int64_t* stream_id,
                               const float* H_gt, const float* image_size0, int B, int M, int N,
                               const float* thresholds, int T, int num_hypotheses, int lo_iters, uint64_t seed,
                               double* H_out, uint8_t* inliers, int32_t* num_inliers, uint8_t* success,
                               int32_t* best_hypothesis, double* H_minimal, float* err_out, void* ws, size_t ws_bytes,
                               void* stream);

/* Robust relative pose from the predicted matches: five-point RANSAC, MSAC-scored with the squared Sampson distance at
 * T thresholds in one pass, cheirality vote, Gauss-Newton local optimisation (DESIGN.md "Robust relative pose"; the
 * estimator behind eval_relative_pose_robust, gluefactory/eval/utils.py:188-222 -- there OpenCV / PoseLib / pycolmap:
 * parity with them is unpinned).  kp0 [B,M,2], kp1 [B,N,2] in pixels, m0 [B,M] int64 (a match is 0 <= m0[i] < N),
 * stream_id [B] int64 (nullable: 0..B-1) the random stream of a pair, cam0 / cam1 [B,10] and model0 / model1 as in the
 * pose / depth evaluation below (points go through image2cam: only OPENCV_FISHEYE removes its distortion).  T_gt
 * [B,12] (R row-major, t; X1 = R X0 + t) is given together with r_err and t_err or all three are NULL.  thresholds: T
 * values in pixels in HOST memory, 1 <= T <= 8, each positive and finite; a pair uses threshold / mean(fx0, fy0, fx1,
 * fy1).  Outputs per (pair, threshold): R_out [B,T,9], t_out [B,T,3] (unit), E_out [B,T,9] = [t]x R, E_minimal [B,T,9]
 * (the winning minimal model, unit Frobenius norm, its largest-magnitude entry positive), all fp64; inliers [B,T,M]
 * uint8 over key points 0; num_inliers, best_hypothesis (the winning sample), best_solution (which of its <= 10
 * models) [B,T] int32; success [B,T] uint8; r_err, t_err [B,T] fp64 degrees (t up to sign; t_err 0 when |t_gt| <
 * ignore_gt_t_thr).  Fewer than 5 matches or no usable sample: success 0, R identity, t, E, E_minimal zero, no
 * inliers, best_hypothesis and best_solution -1, errors +inf.  GFC_ERR_INVALID (nothing launched): B <= 0 or > 65535,
 * M < 0, N < 0, T outside 1..8, num_hypotheses <= 0 or >= 2^27, lo_iters < 0, a model outside GFC_CAM_*, a threshold
 * that is not positive and finite, a negative or NaN ignore_gt_t_thr, a NULL required pointer. */
size_t gfc_eval_relative_pose_ransac_workspace_bytes(int B, int M, int T, int num_hypotheses);
/* Camera.image2cam of kp [B,K,2] (pixels) with cam [B,10] and one model: out [B,K,2], the point on the z = 1 plane --
 * the device function the estimator's records go through (only OPENCV_FISHEYE removes its distortion). */
int gfc_eval_pose_image2cam(const float* kp, const float* cam, int model, int B, int K, float* out, void* stream);
int gfc_eval_relative_pose_ransac(const float* kp0, const float* kp1, const int64_t* m0, const int64_t* stream_id,
                                  const float* cam0, int model0, const float* cam1, int model1, const float* T_gt, int B,
                                  int M, int N, const float* thresholds, int T, int num_hypotheses, int lo_iters,
                                  uint64_t seed, double ignore_gt_t_thr, double* R_out, double* t_out, double* E_out,
                                  double* E_minimal, uint8_t* inliers, int32_t* num_inliers, uint8_t* success,
                                  int32_t* best_hypothesis, int32_t* best_solution, double* r_err, double* t_err,
                                  void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Pose / depth evaluation (csrc/eval_pose.hip): what the reference's pose benchmarks score matches with.
 * One workgroup per pair, no workspace, no allocation, no synchronisation; everything per pair lives in LDS.
 *
 * A camera is float[10] per pair = w, h, fx, fy, cx, cy, d0..d3 (unused coefficients are ignored); `model` is one of
 * the GFC_CAM_* values below and is shared by all pairs of a call, as a stacked reference Camera shares its model.
 * PINHOLE: no coefficient; RADIAL: k1 k2; OPENCV: k1 k2 p1 p2; OPENCV_FISHEYE: k1..k4 of the Kannala-Brandt model.
 * A pose is float[12] per pair = R row-major, then t (x_j = R x_i + t).  Pixel centres are at +0.5.  The arrays of an
 * empty side (K, M or N of 0) may be NULL; any other NULL required pointer is GFC_ERR_INVALID.  The arithmetic is
 * fp32 in the reference's operation order (Camera.image2cam / cam2image, gluefactory/geometry/wrappers.py:407-481 with
 * geometry/utils.py:92-248; sample_depth / project, geometry/depth.py:8-59).
 * ---------------------------------------------------------------------------------- */
enum { GFC_CAM_PINHOLE = 0, GFC_CAM_RADIAL = 1, GFC_CAM_OPENCV = 2, GFC_CAM_OPENCV_FISHEYE = 3 };

/* sample_depth + project(ccth=None) for the key points of view i: kp [B,K,2], depth_i [B,Hi,Wi] (<= 0 = hole) ->
 * depth_kp [B,K] (NaN where the bilinear and the nearest sample are holes, 0 where the nearest falls outside),
 * valid [B,K] uint8 (finite and > 0), proj [B,K,2] the pixels in view j, visible [B,K] uint8 (valid, in front of
 * camera j, inside its distortion model's range and inside its image: 0 <= p <= size - 1).  What
 * gt_matches_from_pose_depth returns as depth_keypoints*, proj_*, visible*. */
int gfc_eval_pose_project(const float* kp, const float* depth_i, const float* cam_i, int model_i, const float* cam_j,
                          int model_j, const float* T_itoj, int B, int K, int Hi, int Wi, float* depth_kp,
                          uint8_t* valid, float* proj, uint8_t* visible, void* stream);

/* eval_matches_depth (gluefactory/eval/utils.py:77-138): kp0 [B,M,2], kp1 [B,N,2], matches0 [B,M] int64 (-1 =
 * unmatched), depth0 [B,H0,W0], depth1 [B,H1,W1], T_1to0 the inverse of T_0to1 (computed by the caller, as Hinv of
 * gfc_eval_matches_homography).  out [B,7] = reproj_prec@1px, @3px, @5px (symmetric reprojection error
 * 0.5 (|p01 - p1| + |p10 - p0|) over the matches whose two points have valid depth, NaN counted as +inf), covisible
 * (their number), covisible_percent (of all matches), gt_match_recall, gt_match_precision against the ground-truth
 * matches of gt_matches_from_pose_depth (geometry/gt_generation.py:594-727, epi_th = cc_th = None; the evaluation
 * calls it with pos_th 3, neg_th 5): dist = max(d0, d1), +inf outside visible0 x visible1; mutual argmin (first index
 * on ties) and dist < pos_th^2 is a match; -1 where the UNMASKED min of d0 (d1 for view 1) exceeds neg_th^2 and the
 * point's depth is valid; -2 otherwise.  Means over an empty set are 0.  gt_matches0 [B,M] / gt_matches1 [B,N] int64,
 * each nullable.  M == 0 or N == 0: all -1.  The M x N matrix is never materialised.  A match index >= N counts as
 * a match (covisible_percent, precision denominator), is never covisible and equals no ground-truth index.
 * GFC_ERR_UNSUPPORTED (nothing launched) exactly when the pair does not fit in 160 KB (163840 bytes) of LDS:
 * gfc_eval_matches_depth_lds_bytes(M, N) = 24 M + 28 N + the kernel's static LDS; about 3100 x 3100 key points.
 * GFC_ERR_LAUNCH when the runtime refuses more than 64 KB of dynamic LDS. */
size_t gfc_eval_matches_depth_lds_bytes(int M, int N);
int gfc_eval_matches_depth(const float* kp0, const float* kp1, const int64_t* matches0, const float* depth0,
                           const float* depth1, const float* cam0, int model0, const float* cam1, int model1,
                           const float* T_0to1, const float* T_1to0, int B, int M, int N, int H0, int W0, int H1, int W1,
                           float pos_th, float neg_th, float* out, int64_t* gt_matches0, int64_t* gt_matches1,
                           void* stream);

/* eval_matches_epipolar (gluefactory/eval/utils.py:45-74): out [B,5] = epi_prec@1e-4, @5e-4, @1e-3, num_matches,
 * num_keypoints = (M + N) / 2.  The error of a match is sym_epipolar_distance(squared=False) (geometry/epipolar.py:32-56,
 * both squared norms clamped at 1e-6) of its image2cam points under E = [t]x R. */
int gfc_eval_matches_epipolar(const float* kp0, const float* kp1, const int64_t* matches0, const float* cam0, int model0,
                              const float* cam1, int model1, const float* T_0to1, int B, int M, int N, float* out,
                              void* stream);

/* Image preprocessing ("next" row rank 1): [uint8 -> float /255 ->] antialiased bilinear resize, fused.
 * src: src_is_u8_hwc != 0: B interleaved HxWxC byte images (bgr != 0 reverses the channel order, as read_image does
 * after cv2.imread, utils/image.py:135-145), converted like numpy_image_to_torch (image.py:148-156); else B planar
 * CxHxW fp32 images.  dst [B,C,OH,OW] fp32.  antialias != 0 and a down-scaling axis: Gaussian blur with
 * sigma = max((in/out - 1)/2, 0.001) per axis, kernel size int(max(4 sigma, 3)) made odd, reflect border, then
 * bilinear interpolation with torch's align_corners=False/True source-index rule.  Replaces the
 * kornia.geometry.transform.resize call of ImagePreprocessor.__call__ (gluefactory/utils/image.py:33-47; kornia is
 * third-party and unpinned).  GFC_ERR_UNSUPPORTED for blur kernels wider than 63 taps (down-scaling > ~30x). */
int gfc_preprocess_resize(const void* src, int src_is_u8_hwc, int bgr, int B, int C, int H, int W, float* dst, int OH,
                          int OW, int align_corners, int antialias, void* stream);

/* Crop + nearest / area resample in one launch: what the posed_images reader does to depth maps, specular masks and
 * images (gluefactory/datasets/posed_images.py:219-269: crop, then ImagePreprocessor with "nearest" / "area").
 * src_kind: GFC_RS_F32_CHW B planar CxHxW fp32 images; GFC_RS_U8_HWC B interleaved HxWxC byte images converted like
 * numpy_image_to_torch; GFC_RS_U8_PLANE B byte planes HxW, non-zero = 1; GFC_RS_BITS B bit planes as numpy.packbits
 * makes them of the flattened HxW mask (bit k = y W + x is (byte[k >> 3] >> (7 - (k & 7))) & 1, ceil(H W / 8) bytes per
 * plane; posed_images.py:75-82).  The two mask kinds need C = 1.  (left, top, cw, ch): the crop window inside HxW;
 * everything else sees only the window (GFC_ERR_INVALID when it leaves the plane).  value_scale multiplies every
 * source value at load (the per-image depth scale, posed_images.py:235-236).
 * mode GFC_RS_NEAREST: torch's legacy "nearest", source index min((int)floorf(dst * ((float)in / (float)out)), in - 1);
 * with antialias != 0 and a down-scaling axis the window is blurred first as gfc_preprocess_resize blurs (same sigma,
 * kernel size, weights and reflect border -- at the WINDOW's edges -- same GFC_ERR_UNSUPPORTED / GFC_ERR_INVALID).
 * mode GFC_RS_AREA: adaptive average pooling, box [floor(i in / out), ceil((i + 1) in / out)) per axis, fp32 sum / count;
 * GFC_ERR_UNSUPPORTED together with a blur.
 * dst: fp32 [B,C,OH,OW] for the two image kinds, and valid (optional, same shape) = dst > 0 ? 1.f : 0.f
 * (posed_images.py:249); uint8 [B,1,OH,OW] holding value > 0.5 for the two mask kinds (valid must be NULL). */
#define GFC_RS_F32_CHW 0
#define GFC_RS_U8_HWC 1
#define GFC_RS_U8_PLANE 2
#define GFC_RS_BITS 3
#define GFC_RS_NEAREST 0
#define GFC_RS_AREA 1
int gfc_preprocess_resample(const void* src, int src_kind, int B, int C, int H, int W, int left, int top, int cw, int ch,
                            int mode, int antialias, float value_scale, void* dst, float* valid, int OH, int OW,
                            void* stream);

/* Perspective warp of a batch of items in one launch: the pair generator of the `homographies` dataset
 * (gluefactory/datasets/homographies.py:37-44: cv2.warpPerspective(img, H, size) per view; :714-718 the vignette crop;
 * :517-519 the grey sum after the warp).  UNPINNED: the rule restates OpenCV's warpPerspective with INTER_LINEAR and
 * BORDER_CONSTANT 0 -- OpenCV is absent here, the pin is the float64 restatement of tests/warp_reference.py.
 * src: S sources of HxW, GFC_RS_U8_HWC (interleaved HxWxC bytes converted like numpy_image_to_torch: value / 255) or
 * GFC_RS_F32_CHW (planar CxHxW fp32); C is 1 or 3.  (left, top, cw, ch): the crop window shared by the launch; the
 * window IS the image -- a tap outside it counts as 0 even where the plane goes on (GFC_ERR_INVALID when the window
 * leaves the plane).  Per item b < B, on the device: src_index[b] (int32; an index outside [0, S) reads nothing and
 * gives a zero image) and M + 9 b, nine doubles row-major, the DESTINATION -> SOURCE matrix (the inverse of the sampler's
 * H_; the caller inverts in float64).
 * Per destination pixel (x, y), in fp64: X = M0 x + (M1 y + M2), Y and W alike; W <- 32 / W when W != 0, else 0;
 * fX = X W, fY = Y W saturated to the int32 range and rounded half to even -> qx, qy; source cell (qx >> 5, qy >> 5)
 * (arithmetic shift), fractions (qx & 31) / 32, (qy & 31) / 32; the weights w00 = (1 - fx)(1 - fy), w01 = fx (1 - fy),
 * w10 = (1 - fx) fy, w11 = fx fy are exact in fp32; out = t00 w00 + t01 w01 + t10 w10 + t11 w11 summed left to right in
 * fp32 (t01 the tap at x + 1, t10 at y + 1).
 * dst: fp32 [B,C,OH,OW]; with gray != 0 (needs C = 3) [B,1,OH,OW] = 0.299 r + 0.587 g + 0.114 b in fp32, left to right.
 * No workspace, no LDS. */
int gfc_warp_perspective(const void* src, int src_kind, int S, int C, int H, int W, int left, int top, int cw, int ch,
                         const int* src_index, const double* M, int B, int gray, float* dst, int OH, int OW,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * SIFT: scale space, detection, orientation, descriptor (csrc/sift.hip).  The algorithm is the one stated in
 * tests/sift_reference.py: Lowe's detector and descriptor with pycolmap's meaning of the reference's conf keys
 * (gluefactory/models/extractors/sift.py:139-144).  UNPINNED: OpenCV, pycolmap and CudaSift are absent here; these
 * are NOT their key points, the pin is the float64 restatement.
 * Shared arguments: image fp32 [B,H,W], clipped to [0, 1] where it is read (the reference's np.clip, sift.py:208); valid_wh int32 [B,2] (w, h) on the device or NULL (every image is
 * W x H): each image's pyramid is that of ITS OWN top-left valid region (own octave sizes, own replicate border, own
 * number of octaves).  first_octave is -1 (2x bilinear up-sample first) or 0; num_octaves 1..8; an octave exists
 * while its shorter side is >= 16; 3 layers per octave, 6 Gaussian and 5 DoG levels.
 * GFC_ERR_UNSUPPORTED (nothing launched): another first_octave, num_octaves outside 1..8, a base level (H, W; doubled
 * for first_octave -1) with a side above 16384 or a shorter side below 16.  (No level is ever narrower than a tap
 * radius: the widest incremental blur has radius 13 and the narrowest level 16 samples; a 16-sample side under 27 taps,
 * where both replicate borders fall inside one window, is the extreme.)
 * Layout: per image one array of gauss_floats and one of dog_floats; octave o holds 6 (5) planes of h_o x w_o floats,
 * row stride w_o, sized from the PADDED (H, W); an image writes and reads only its own region of each plane.  The
 * layout call fills out[35] (int64, host): n_octaves, gauss_floats, dog_floats, then (h_o, w_o, gauss offset, dog
 * offset) per octave. */
int gfc_sift_pyramid_layout(int H, int W, int first_octave, int num_octaves, int64_t* out);
/* image fp32 [B,3,H,W] -> out [B,H,W] = 0.299 r + 0.587 g + 0.114 b, summed left to right in fp32 (the package's
 * rgb-to-grey kernel; the reference's kornia rgb_to_grayscale has the same weights). */
int gfc_sift_gray(const float* image, float* out, int B, int H, int W, void* stream);
/* gauss [B,gauss_floats], dog [B,dog_floats].  One launch per level: the input tile and its halo pass through LDS once,
 * rows then columns (taps: radius ceil(4 sigma), float64 on the host, normalised, rounded to fp32), and the same launch
 * writes the DoG level and, for level 3, every second pixel into level 0 of the next octave.  No workspace. */
int gfc_sift_pyramid(const float* image, int B, int H, int W, const int32_t* valid_wh, int first_octave,
                     int num_octaves, float* gauss, float* dog, void* stream);
/* Extrema of the DoG levels (strictly above or below all 26 neighbours, |v| > 0.8 detection_threshold), refined in fp64
 * (quadratic fit, at most 5 moves while an offset exceeds 0.6), accepted when |D| >= detection_threshold and
 * tr^2 / det < (r + 1)^2 / r, det > 0, r = edge_threshold.  Per image at most `cap` candidates are kept: the ones
 * beyond are counted, not stored.  Output, ordered by (octave, layer, y, x) of the integer extremum whatever the order
 * of arrival: raw_f fp32 [B,cap,8] = (x, y, sigma, |D|, x_oct, y_oct, sigma_oct, 0) -- x, y in input pixels, corner
 * convention (+ 0.5), sigma in input pixels, the _oct values in the octave's own pixels; raw_i int32 [B,cap,8] =
 * (octave, layer, y, x of the extremum, layer, y, x after the moves, 0); counts int32 [B,4] = (key points, candidates
 * found, candidates beyond cap, 0).  B <= 21845.
 * COST LIMIT: the order is made by counting, every candidate of an image against every other -- n^2 / 2 key reads for
 * n candidates, sized for the few thousand of a VGA image (8 700 candidates: 3.4 ms for 32 images); the top-k of the
 * filter call below ranks its kept list the same way.  cap bounds n; a cap far above 2^16 buys quadratic time, not a
 * faster sort (the radix select of the SuperPoint selection is not reused here). */
size_t gfc_sift_detect_workspace_bytes(int B, int cap);
int gfc_sift_detect(const float* dog, int B, int H, int W, const int32_t* valid_wh, int first_octave,
                    int num_octaves, double detection_threshold, double edge_threshold, int cap, float* raw_f,
                    int32_t* raw_i, int32_t* counts, void* ws, size_t ws_bytes, void* stream);
/* 36-bin gradient histogram on the key point's Gaussian level (radius round(4.5 sigma_oct), weight magnitude x Gaussian
 * of 1.5 sigma_oct, linear in the bin), smoothed six times, peaks >= 0.8 max refined parabolically: one output per peak,
 * at most 4 per key point, in the order (key point, bin).  ori_f fp32 [B,ocap,8] = the raw record with the angle in
 * (-pi, pi] in slot 7; ori_i int32 [B,ocap,4] = (raw index, octave, level, peak); ocounts int32 [B,2] = (written,
 * beyond ocap).  One wave per key point; the bins are 64-bit fixed-point integers, so the sums do not depend on order. */
size_t gfc_sift_orient_workspace_bytes(int B, int cap);
int gfc_sift_orient(const float* gauss, int B, int H, int W, const int32_t* valid_wh, int first_octave,
                    int num_octaves, const float* raw_f, const int32_t* raw_i, const int32_t* counts, int cap,
                    int ocap, float* ori_f, int32_t* ori_i, int32_t* ocounts, void* ws, size_t ws_bytes,
                    void* stream);
/* 4 x 4 cells x 8 bins, cell width 3 sigma_oct, window rotated by the angle, trilinear, Gaussian weight of 2 cells,
 * samples outside the level skipped; L2, clamp at 0.2, L2 (pycolmap's Normalization.L2).  desc fp32 [B,ocap,128], index
 * (cell_y * 4 + cell_x) * 8 + bin; rows at and beyond ocounts[b][0] are not written.  One wave per key point. */
int gfc_sift_describe(const float* gauss, int B, int H, int W, const int32_t* valid_wh, int first_octave,
                      int num_octaves, const float* ori_f, const int32_t* ori_i, const int32_t* ocounts, int ocap,
                      float* desc, void* stream);
/* The reference's post-processing of a SIFT list on the device (sift.py:288-380), per image, on the oriented list of
 * the calls above (x, y in slots 0-1, sigma 2, score 3, angle 7): the specular-mask rule (extractors/utils.py:4-42,
 * offset 0.5; specular uint8 [B,H,W], nonzero = keep, NULL = none; cropped to the image's valid size), then
 * filter_dog_point (sift.py:29-62; nms_radius < 0 skips it, as conf nms_radius None does; GFC_ERR_UNSUPPORTED above
 * 16): per pixel round(p - 0.5) the largest score, among equals the smallest |angle|, then the (2 r + 1)^2 max-pool
 * test -- planes of order-preserving integer keys built with vector atomic max / min, so the result does not depend on
 * order -- then the k largest by score (score x sigma with scale_weighting; k <= 0: all) in torch.topk's descending
 * order, the list order when nothing is cut.  Outputs [B,out_cap,...], out_cap >= min(k, ocap): kpts (rows at and
 * beyond counts_out[b] are left as they are, for the padding), scales, oris, scores (0 there), desc_out (rootsift != 0:
 * sift_to_rootsift of every row, sift.py:65-68, the padded rows included as in the reference), index int32 (row of the
 * oriented list, -1 beyond the count), counts_out int32 [B]. */
size_t gfc_sift_filter_workspace_bytes(int B, int H, int W, int ocap);
int gfc_sift_filter(const float* ori_f, const float* desc, const int32_t* ocounts, int B, int ocap, int H, int W,
                    const int32_t* valid_wh, const unsigned char* specular, int nms_radius, int scale_weighting, int k,
                    int rootsift, int out_cap, float* kpts, float* scales, float* oris, float* scores, float* desc_out,
                    int32_t* index, int32_t* counts_out, void* ws, size_t ws_bytes, void* stream);
/* The stages above in sequence on one stream -- pyramid, detect, orient, describe, filter -- with every intermediate in
 * ONE workspace and no host read in between: the same launches as the separate calls with the same cap and ocap, hence
 * the same bits.  counts [B,4] and ocounts [B,2] are those of detect and orient (the candidates beyond cap and the
 * orientations beyond ocap are counted there, never dropped silently); the other outputs are the filter's.  The
 * workspace holds both pyramids, the raw and the oriented list, B x ocap descriptors and the largest stage scratch. */
size_t gfc_sift_extract_workspace_bytes(int B, int H, int W, int first_octave, int num_octaves, int cap, int ocap);
int gfc_sift_extract(const float* image, int B, int H, int W, const int32_t* valid_wh, const unsigned char* specular,
                     int first_octave, int num_octaves, double detection_threshold, double edge_threshold, int cap,
                     int ocap, int nms_radius, int scale_weighting, int k, int rootsift, int out_cap, float* kpts,
                     float* scales, float* oris, float* scores, float* desc_out, int32_t* index, int32_t* counts_out,
                     int32_t* counts, int32_t* ocounts, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * SuperGlue matcher (gluefactory_nonfree/superglue.py:268-322, inference path).  All fp32; rows are row-major
 * [rows,256] where the reference is channel-first Conv1d on [B,256,N]; a batch is packed as LightGlue's: the side-0
 * rows of every pair, then the side-1 rows.
 * Head order: the reference splits heads with view(b, dim, h, -1) (superglue.py:133), so channel c belongs to head
 * c % 4 at position c / 4 -- interleaved, not head-major.  The caller permutes the rows of the three proj weights
 * (packed row h*64 + d <- state-dict row d*4 + h) and the columns of merge the same way, so that the kernels see
 * head-major 64-wide columns.
 * ---------------------------------------------------------------------------------- */
#define GFC_SG_MAX_LAYERS 32
typedef struct {
  int n_layers;                  /* len(GNN_layers), 18 */
  int use_scores;                /* 1: the encoder reads [x, y, score]; 0: [x, y] */
  int cross[GFC_SG_MAX_LAYERS];  /* per layer: 0 = "self", 1 = "cross" (superglue.py:179-185) */
  /* kenc.encoder (superglue.py:98-111): layers 0..3 TRANSPOSED to [cin][cout] (cin = 3 or 2, 32, 64, 128) with their
   * eval-mode BatchNorm1d (eps 1e-5) folded to y * scale + shift; layer 4 as stored, [256][256], no BatchNorm. */
  const float* kenc_w[5];
  const float* kenc_b[5];
  const float* kenc_scale[4];
  const float* kenc_shift[4];
  /* gnn.layers.{l}: attn.proj.{0,1,2} stacked to [768][256] = [q | k | v], each head-major; attn.merge [256][256] with
   * head-major columns; mlp.0 [512][512] with mlp.1 (BatchNorm1d) folded to scale / shift [512]; mlp.3 [256][512]. */
  const float* wqkv[GFC_SG_MAX_LAYERS];
  const float* bqkv[GFC_SG_MAX_LAYERS];
  const float* merge_w[GFC_SG_MAX_LAYERS];
  const float* merge_b[GFC_SG_MAX_LAYERS];
  const float* mlp0_w[GFC_SG_MAX_LAYERS];
  const float* mlp0_b[GFC_SG_MAX_LAYERS];
  const float* mlp_scale[GFC_SG_MAX_LAYERS];
  const float* mlp_shift[GFC_SG_MAX_LAYERS];
  const float* mlp1_w[GFC_SG_MAX_LAYERS];
  const float* mlp1_b[GFC_SG_MAX_LAYERS];
  const float* final_proj_w; /* [256][256] */
  const float* final_proj_b;
  float bin_score;
} gfc_sg_params;

/* desc [B*n,256] += kenc([x, y, score]) in place (superglue.py:85-111,289-290).  kpts [B,n,2] pixel coordinates are
 * normalised per image with sizes [B,2] = (w, h): (k - size/2) / (0.7 max(w, h)); scores [B,n], NULL exactly when
 * p->use_scores == 0.  Layers 3 -> 32 -> 64 -> 128 -> 256 run in one kernel with the activations in LDS, the last
 * 256 -> 256 layer and the addition on the matrix pipe.  ws: [B*n,256] hidden rows.  Only the kenc_* fields of p are read. */
size_t gfc_sg_keypoint_encoder_workspace_bytes(int rows);
int gfc_sg_keypoint_encoder(const gfc_sg_params* p, const float* kpts, const float* scores, const float* sizes, int B,
                            int n, float* desc, void* ws, size_t ws_bytes, void* stream);

/* The propagation MLP with its residual in one kernel (superglue.py:140-149, the desc + delta of :175):
 *   Y[M,256] = residual + ( ReLU( ([A0 | A1] * W0[512,512]^T + b0) * scale + shift ) * W1[256,512]^T + b1 ),
 * A0, A1 [M,256] (row strides lda0, lda1, multiples of 4), scale / shift [512] = the folded BatchNorm1d.  The 512-wide
 * hidden tile stays on chip (the tiles of the fused LightGlue FFN kernel).  residual (nullable) and Y share ldy and may
 * alias; b0, b1 nullable. */
int gfc_sg_mlp(const float* A0, int lda0, const float* A1, int lda1, const float* W0, const float* b0,
               const float* scale, const float* shift, const float* W1, const float* b1, const float* residual, float* Y,
               int ldy, int M, void* stream);

/* log_optimal_transport + log_sinkhorn_iterations (superglue.py:188-216): from cost [B,M,N] and bin_score, `iters`
 * iterations of u = log_mu - LSE_j(Z + v), v = log_nu - LSE_i(Z + u) on the augmented [M+1,N+1] matrix in the log
 * domain (maximum subtracted), out [B,M+1,N+1] = Z + u + v - norm.  A workgroup holds a block of whole rows in LDS:
 * the matrix is read once per iteration; the two half-steps are separate launches in stream order (no workgroup waits
 * for another).  GFC_ERR_UNSUPPORTED when one row of N + 1 floats and v do not fit in 160 KB of LDS. */
size_t gfc_sg_sinkhorn_workspace_bytes(int B, int M, int N);
int gfc_sg_sinkhorn(const float* cost, float bin_score, int B, int M, int N, int iters, float* out, void* ws,
                    size_t ws_bytes, void* stream);

/* The whole matcher for B pairs of (M, N) key points: encoder, n_layers x (256 -> 768 projection, attention with
 * scale 1/8 -- self: problems (i, i); cross: (0 <- 1) and (1 <- 0) --, merge, MLP), final_proj, cost = mdesc0 .
 * mdesc1^T / 16, Sinkhorn, the mutual-argmax filter LightGlue uses (superglue.py:303-313 is the same rule).
 * kpts0 [B,M,2], kpts1 [B,N,2] pixels; scores0 [B,M], scores1 [B,N] (NULL when !use_scores); desc0 [B,M,256], desc1
 * [B,N,256] (read-only); size0 / size1 [B,2] = (w, h).  Outputs: sinkhorn_cost [B,M,N], log_assignment [B,M+1,N+1],
 * m0 [B,M] / m1 [B,N] int64, ms0 / ms1; desc_taps (nullable) [4][B*M + B*N, 256]: the rows after the encoder, layer 0,
 * layer 1 (slots 1, 2 only when those layers exist) and the last layer. */
size_t gfc_sg_workspace_bytes(int B, int M, int N);
int gfc_sg_forward(const gfc_sg_params* p, const float* kpts0, const float* kpts1, const float* scores0,
                   const float* scores1, const float* desc0, const float* desc1, const float* size0, const float* size1,
                   int B, int M, int N, int iters, float threshold, float* sinkhorn_cost, float* log_assignment,
                   int64_t* m0, int64_t* m1, float* ms0, float* ms1, float* desc_taps, void* ws, size_t ws_bytes,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GFC_AMD_H */
