// Host-side orchestration behind the C ABI: which kernels run, in which order, on which slices of
// the caller's workspace.  No allocation, no synchronisation: everything is enqueued on the
// caller's stream (graph-capturable).
#include <algorithm>
#include <climits>

#include "../../include/gfc_amd_cross_attention.h"
#include "../../include/gfc_amd_layer_scores.h"
#include "../../include/gfc_amd_ffn_backward.h"
#include "common.h"
#include "lg_rowdot.h"

// from the other translation units
int gfc_rgb_to_gray(const float* img, float* out, int B, int H, int W, hipStream_t stream);
int gfc_det_head_softmax_d2s(const float* hidden, int lda, const float* wp, const float* bias, const float* scale,
                             const float* shift, int B, int h8, int w8, float* heat, hipStream_t st);
int gfc_rowdot256(const float* x, int ld, int rows, const float* w, const float* bias, float* z, hipStream_t st);
size_t gfc_assign_tail_bytes(int B, int M, int N);
int gfc_assign_filter_fused(float* scores, const float* z0, const float* z1, int B, int M, int N, float threshold,
                            int64_t* m0, int64_t* m1, float* ms0, float* ms1, void* tail, hipStream_t st);

// GFC_SOURCE_HASH: content hash of the whole source set, passed by csrc/build.py when it compiles this unit
#ifndef GFC_SOURCE_HASH
#define GFC_SOURCE_HASH "unknown"
#endif
extern "C" const char* gfc_version(void) { return "gfc_amd 0.6.0 (gfx950, fp32 MFMA) src " GFC_SOURCE_HASH; }

#define GFC_TRY(expr)            \
  do {                           \
    int _s = (expr);             \
    if (_s != GFC_OK) return _s; \
  } while (0)

// ---------------------------------------------------------------------------------------------
// SuperPoint dense forward
// ---------------------------------------------------------------------------------------------
struct SpPlan {
  int H[5], W[5];  // resolution of stage 1..4 (index 1..4)
  size_t gray, bufA, bufB, total;  // workspace slots (gray: empty unless C == 3)
};

static SpPlan sp_plan(int B, int C, int H, int W) {
  SpPlan p;
  p.H[1] = H; p.W[1] = W;
  for (int i = 2; i <= 4; ++i) { p.H[i] = p.H[i - 1] / 2; p.W[i] = p.W[i - 1] / 2; }
  // conv1a never touches HBM (fused into the stem kernel): the largest activation is conv2a's
  auto px = [&](int i) { return (size_t)B * p.H[i] * p.W[i]; };  // pixels of stage i
  gfc_slots s;
  p.gray = s.take(C == 3 ? (size_t)B * H * W * sizeof(float) : 0);
  p.bufA = s.take(std::max({px(2) * 64, px(3) * 128, px(4) * 512}) * sizeof(float));
  p.bufB = s.take(std::max({px(2) * 64, px(3) * 64, px(4) * 128}) * sizeof(float));
  p.total = s.off;
  return p;
}

extern "C" size_t gfc_sp_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || H < 8 || W < 8) return 0;
  return sp_plan(B, C, H, W).total;
}

extern "C" int gfc_event_create(void** event) {
  if (!event) return GFC_ERR_INVALID;
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return GFC_ERR_LAUNCH;
  *event = (void*)e;
  return GFC_OK;
}
extern "C" int gfc_event_destroy(void* event) {
  return hipEventDestroy((hipEvent_t)event) == hipSuccess ? GFC_OK : GFC_ERR_LAUNCH;
}
extern "C" int gfc_event_elapsed_ms(void* start, void* stop, float* ms) {
  if (!start || !stop || !ms) return GFC_ERR_INVALID;
  return hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop) == hipSuccess ? GFC_OK : GFC_ERR_LAUNCH;
}

// ---- bench-only probe: sustained fp32-MFMA rate and shader clock of this device (gfc_amd.h) ----
__global__ __launch_bounds__(256) void mfma_peak_probe_kernel(unsigned long long* out, int n, float seed) {
  f32x16 a0, a1, a2, a3;
#pragma unroll
  for (int r = 0; r < 16; ++r) { a0[r] = seed * r; a1[r] = seed + r; a2[r] = seed - r; a3[r] = seed * 0.5f * r; }
  // full-entropy operands (switching activity like real data), bounded accumulators
  const float x = __sinf(seed * (threadIdx.x + 1) * 0.37f), y = __cosf(seed * (threadIdx.x + 3) * 0.21f) * 1e-3f;
  const unsigned long long t0 = __builtin_readcyclecounter(), w0 = wall_clock64();
  for (int i = 0; i < n; i += 4) {
    a0 = mfma32(x, y, a0);
    a1 = mfma32(y, x, a1);
    a2 = mfma32(x, x * 1e-3f, a2);
    a3 = mfma32(y, y, a3);
  }
  const unsigned long long t1 = __builtin_readcyclecounter(), w1 = wall_clock64();
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += a0[r] + a1[r] + a2[r] + a3[r];
  if (s == 12345.678f) out[0] = 1;  // keeps the accumulators alive
  if (blockIdx.x == 0 && threadIdx.x == 0) { out[1] = t1 - t0; out[2] = w1 - w0; }
}

extern "C" int gfc_probe_mfma_peak(int mfmas_per_wave, float* tflops, float* shader_clock_ghz, void* stream) {
  if (mfmas_per_wave < 4 || !tflops || !shader_clock_ghz) return GFC_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* d = nullptr;
  if (hipMalloc(&d, 4 * sizeof(unsigned long long)) != hipSuccess) return GFC_ERR_LAUNCH;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { (void)hipFree(d); return GFC_ERR_LAUNCH; }
  const int n = mfmas_per_wave & ~3, cus = gfc_device_cus();
  (void)hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), st);
  hipLaunchKernelGGL(mfma_peak_probe_kernel, dim3(cus), dim3(256), 0, st, d, n, 0.5f);  // clock ramp
  (void)hipEventRecord(e0, st);
  hipLaunchKernelGGL(mfma_peak_probe_kernel, dim3(cus), dim3(256), 0, st, d, n, 0.37f);
  (void)hipEventRecord(e1, st);
  unsigned long long h[4] = {0, 0, 0, 0};
  float ms = 0.f;
  const bool ok = hipStreamSynchronize(st) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess &&
                  hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess && ms > 0.f && h[2] > 0;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(d);
  if (!ok) return GFC_ERR_LAUNCH;
  *tflops = (float)((double)cus * 4 * n * 4096.0 / (ms * 1e-3) / 1e12);
  *shader_clock_ghz = (float)((double)h[1] / ((double)h[2] * 10.0));  // ticks per (10 ns tick) = GHz
  return GFC_OK;
}

// optional event bracket around one launch (gfc_trace, include/gfc_amd.h)
static inline bool trace_begin(gfc_trace* tr, hipStream_t st) {
  const bool rec = tr && tr->start && tr->stop && tr->count < tr->capacity;
  if (rec) (void)hipEventRecord((hipEvent_t)tr->start[tr->count], st);
  return rec;
}
static inline void trace_end(gfc_trace* tr, hipStream_t st, bool rec) {
  if (!rec) return;
  (void)hipEventRecord((hipEvent_t)tr->stop[tr->count], st);
  tr->count++;
}

// stem (conv1a + conv1b + pool) with optional event bracket
static int traced_stem(gfc_trace* tr, hipStream_t st, const gfc_sp_params* p, const float* x, float* y, int B, int H,
                       int W) {
  const bool rec = tr && tr->start && tr->stop && tr->count < tr->capacity;
  if (rec && hipEventRecord((hipEvent_t)tr->start[tr->count], st) != hipSuccess) return GFC_ERR_LAUNCH;
  int s = (p->conv_mode == 2 && p->w_stem_wino43 && gfc_knobs().stem_f43 != 0)
              ? gfc_sp_stem_wino43(x, p->w[0], p->bias[0], p->scale[0], p->shift[0], p->w_stem_wino43, p->bias[1],
                                   p->scale[1], p->shift[1], y, B, H, W, st)
          : p->conv_mode == 2
              ? gfc_sp_stem_wino(x, p->w[0], p->bias[0], p->scale[0], p->shift[0], p->w_wino[1], p->bias[1],
                                 p->scale[1], p->shift[1], y, B, H, W, st)
              : gfc_sp_stem(x, p->w[0], p->bias[0], p->scale[0], p->shift[0], p->w[1], p->bias[1], p->scale[1],
                            p->shift[1], y, B, H, W, st);
  if (s != GFC_OK) return s;
  if (rec) {
    if (hipEventRecord((hipEvent_t)tr->stop[tr->count], st) != hipSuccess) return GFC_ERR_LAUNCH;
    tr->count++;
  }
  return GFC_OK;
}

extern "C" int gfc_sp_dense(const gfc_sp_params* p, const float* image, int B, int C, int H, int W, float* heatmap,
                            float* desc_raw, void* ws, size_t ws_bytes, gfc_trace* trace, void* stream) {
  if (!p || !image || !heatmap || !desc_raw || !ws || B <= 0 || (C != 1 && C != 3) || H < 8 || W < 8)
    return GFC_ERR_INVALID;
  if (p->desc_dim <= 0) return GFC_ERR_INVALID;
  if (p->conv_mode != 0 && p->conv_mode != 2) return GFC_ERR_INVALID;  // 1 (split arithmetic) was retired in round 4
  if (p->conv_mode == 2) {
    if (!p->wh_wino) return GFC_ERR_INVALID;
    for (int i = 1; i < 8; ++i)
      if (!p->w_wino[i]) return GFC_ERR_INVALID;
  }
  const SpPlan pl = sp_plan(B, C, H, W);
  if (ws_bytes < pl.total) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* gray = (float*)((char*)ws + pl.gray);
  float* A = (float*)((char*)ws + pl.bufA);
  float* Bf = (float*)((char*)ws + pl.bufB);
  const float* x = image;
  if (C == 3) {
    GFC_TRY(gfc_rgb_to_gray(image, gray, B, H, W, st));
    x = gray;
  }
  const int* Hs = pl.H;
  const int* Ws = pl.W;
  // conv1a + conv1b + pool in one launch (conv1a is recomputed on the halo tile, never written to HBM)
  GFC_TRY(traced_stem(trace, st, p, x, Bf, B, Hs[1], Ws[1]));
  // 3x3 layers after the stem: Winograd F(2x2,3x3) (default) or the direct implicit GEMM, both on fp32 MFMA
  auto conv = [&](int li, const float* in, float* out, int hh, int ww, int ci, int co, int pool) -> int {
    if (p->conv_mode == 2)
      return gfc_conv3x3_wino(in, p->w_wino[li], p->bias[li], p->scale[li], p->shift[li], out, B, hh, ww, ci, co, 1,
                              pool, st);
    return gfc_conv3x3(in, p->w[li], p->bias[li], p->scale[li], p->shift[li], out, B, hh, ww, ci, co, 1, pool, st);
  };
  // conv2a, conv2b+pool
  GFC_TRY(conv(2, Bf, A, Hs[2], Ws[2], 64, 64, 0));
  GFC_TRY(conv(3, A, Bf, Hs[2], Ws[2], 64, 64, 1));
  // conv3a, conv3b+pool
  GFC_TRY(conv(4, Bf, A, Hs[3], Ws[3], 64, 128, 0));
  GFC_TRY(conv(5, A, Bf, Hs[3], Ws[3], 128, 128, 1));
  // conv4a, conv4b
  GFC_TRY(conv(6, Bf, A, Hs[4], Ws[4], 128, 128, 0));
  GFC_TRY(conv(7, A, Bf, Hs[4], Ws[4], 128, 128, 0));
  // merged 3x3 heads: [detector hidden | descriptor hidden]
  if (p->conv_mode == 2)
    GFC_TRY(gfc_conv3x3_wino(Bf, p->wh_wino, p->bias_h, p->scale_h, p->shift_h, A, B, Hs[4], Ws[4], 128, 512, 1, 0, st));
  else
    GFC_TRY(gfc_conv3x3(Bf, p->wh, p->bias_h, p->scale_h, p->shift_h, A, B, Hs[4], Ws[4], 128, 512, 1, 0, st));
  const int rows = B * Hs[4] * Ws[4];
  // detector: 1x1 -> 65 logits -> softmax -> depth-to-space in ONE launch (sp_heads.hip; the logits never reach HBM);
  // descriptor: 1x1 -> desc_raw (normalised by the sampler at the four corners it reads)
  GFC_TRY(gfc_det_head_softmax_d2s(A, 512, p->wp, p->bias_p, p->scale_p, p->shift_p, B, Hs[4], Ws[4], heatmap, st));
  GFC_TRY(gfc_linear(A + 256, 512, 256, nullptr, 0, 0, p->wd, 256, p->bias_d, p->scale_d, p->shift_d, 1.f, nullptr,
                     nullptr, nullptr, 0, desc_raw, p->desc_dim, rows, p->desc_dim, st));
  return GFC_OK;
}

// ---------------------------------------------------------------------------------------------
// LightGlue forward
// ---------------------------------------------------------------------------------------------
// workspace of one layer: qkv [R,768] | ctx [R,256] | msg [R,256] | hbuf [R,512] | attention key-split scratch, every
// slot sized for fp32.  The scratch is only needed for small row counts and is sized for the full split of the worst
// case, n_problems * maxn = R query slots (uniform packed rows); gfc_attention lowers the split where that is exceeded.
struct LgLayerWs { size_t qkv, ctx, msg, hbuf, att, total, att_bytes; };
static LgLayerWs lg_layer_ws(int rows) {
  const size_t r = rows, att_bytes = rows <= 8192 ? gfc_att_scratch_bytes(r, 4, GFC_ATT_MAX_SPLIT) : 0;
  gfc_slots s;
  return {s.take(r * 768 * 4), s.take(r * 256 * 4), s.take(r * 256 * 4), s.take(r * 512 * 4), s.take(att_bytes), s.off,
          att_bytes};
}

// workspace of the assignment head: md [R,256] | z [R] | statistics + two-pass tail scratch (lg_misc.hip)
struct LgAssignWs { size_t md, z, tail, total; };
static LgAssignWs lg_assign_ws(int B, int M, int N) {
  const size_t R = (size_t)B * (M + N);
  gfc_slots s;
  return {s.take(R * 256 * 4), s.take(R * 4), s.take(gfc_assign_tail_bytes(B, M, N)), s.off};
}

// A batch of B pairs in GROUPS = maximal runs of consecutive pairs with equal (m, n).  Rows: group after group, inside
// a group the side-0 rows of its pairs (pair-major) followed by their side-1 rows.  A uniform batch is one group.
struct LgGroup {
  int first, count, m, n, row0;  // first pair, pairs, key points per side, first row
};
struct LgGroups {  // by value to the tables kernel: 2.5 KB of kernel arguments
  LgGroup g[GFC_LG_MAX_RAGGED_PAIRS];
};
struct LgBatch {
  int B, groups, R, maxn;
  LgGroups tab;
  size_t stage_bytes;  // one layer's workspace, re-used by every group's assignment head afterwards
  size_t stage, cosb, sinb, csb, tables, total;  // workspace slots
  int cross_chunk;       // pairs per gfc_attention_cross_stored call (lg_cross_chunk), 0: the cross block is one launch
  size_t sim, sim_bytes;  // its score array: one chunk's, re-used by every chunk and layer (behind the tables)
  size_t x, kp;  // gfc_lg_forward only, in front: the rows x [R,256] | its separate arrays packed, kp [R,2] + so [R,2]
};

// The cross block of a batch that is one group of equal pairs evaluates sim once (gfc_attention_cross_stored: one launch
// per direction and a [pairs, 4, N, M] score array between them) from 8 pairs with min(M, N) >= 128 on.
//  * Pairs go through in chunks of the smallest count with which each direction's launch alone fills the chip, pairs x
//    heads x ceil(min(M, N) / 256) >= 2 workgroups on each of 256 CUs (32 pairs at 1024 x 1024: 537 MB of scores; 16 at
//    2048 x 2048), or all at once when the batch is smaller than that.  The CU count is a constant of the library, not
//    a device query: the workspace sizes below must come out the same on a host without a GPU.
//  * Why 8 pairs and not where it starts to pay (1024 x 1024: -0.55 % at 8 pairs, +1.8 % at 16, +2.2 % at 32,
//    profiles/cross_stored_sim.md): the second direction of the stored path is one rounding per product away from the
//    one-launch cross block, and the matcher's outputs are bit-identical across batch sizes from 8 pairs up (32 pairs
//    against the same pairs 8 at a time, tests/test_gpu_batch32.py).  So the arithmetic changes below that range, where
//    floats already differ in the last bits between batch sizes (key split of 1-3 pairs), and depends on the pair shape
//    only from there on.
//  * min(M, N) >= 128: with less than one full 128-query workgroup per (pair, head) the launches are mostly padding
//    (not measured).  Smaller batches and smaller pairs keep the workspace sizes they have always had.
// Returns the chunk; 0: the two directions stay in one launch.
constexpr int GFC_LG_FILL_CUS = 256;
static int lg_cross_chunk(int B, int M, int N) {
  if ((M < N ? M : N) < 128) return 0;
  const long long per_pair = 4LL * (((M < N ? M : N) + 255) / 256);
  if (B < 8) return 0;
  long long chunk = (2 * GFC_LG_FILL_CUS + per_pair - 1) / per_pair;
  if (chunk > B) chunk = B;
  if (gfc_attention_cross_stored_workspace_bytes((int)chunk, M, N, 4) == 0) return 0;
  return (int)chunk;
}

// rows and workspace of the groups in b.tab; false for a non-positive count, or when row offsets x 768 columns would
// leave the int arithmetic of the kernels
static bool lg_layout(LgBatch& b, bool staged) {
  long long R = 0;
  size_t asg = 0;
  b.maxn = 0;
  for (int i = 0; i < b.groups; ++i) {
    LgGroup& g = b.tab.g[i];
    if (g.count <= 0 || g.m <= 0 || g.n <= 0) return false;
    g.row0 = (int)R;
    R += (long long)g.count * ((long long)g.m + g.n);
    if (R > INT_MAX / 768) return false;
    if (g.m > b.maxn) b.maxn = g.m;
    if (g.n > b.maxn) b.maxn = g.n;
    const size_t a = lg_assign_ws(g.count, g.m, g.n).total;
    if (a > asg) asg = a;
  }
  b.R = (int)R;
  b.stage_bytes = lg_layer_ws(b.R).total;
  if (asg > b.stage_bytes) b.stage_bytes = asg;
  gfc_slots s;
  if (staged) {
    b.x = s.take(R * 256 * 4);
    b.kp = s.take(R * 4 * 4);
  }
  b.stage = s.take(b.stage_bytes);
  b.cosb = s.take(R * 64 * 4);
  b.sinb = s.take(R * 64 * 4);
  b.csb = s.take(R * 64 * 4);  // the same values packed (cos, sin) per frequency: what the QKV epilogue reads
  b.tables = s.take((size_t)b.B * (2 * 4 * 2 + 2 + 2 + 4) * 4 + 256);
  b.cross_chunk = b.groups == 1 ? lg_cross_chunk(b.B, b.tab.g[0].m, b.tab.g[0].n) : 0;
  b.sim_bytes = b.cross_chunk ? gfc_attention_cross_stored_workspace_bytes(b.cross_chunk, b.tab.g[0].m, b.tab.g[0].n, 4) : 0;
  b.sim = s.take(b.sim_bytes);
  b.total = s.off;
  return true;
}

// B equal pairs: one group, any B
static bool lg_uniform(int B, int M, int N, LgBatch& b, bool staged = false) {
  b = LgBatch{};
  b.B = B; b.groups = 1;
  b.tab.g[0] = {0, B, M, N, 0};
  return lg_layout(b, staged);
}

// B <= GFC_LG_MAX_RAGGED_PAIRS pairs with their own (m[i], n[i])
static bool lg_ragged(int B, const int32_t* m, const int32_t* n, LgBatch& b) {
  if (B <= 0 || B > GFC_LG_MAX_RAGGED_PAIRS || !m || !n) return false;
  b = LgBatch{};
  b.B = B;
  for (int i = 0; i < B;) {
    int j = i + 1;
    while (j < B && m[j] == m[i] && n[j] == n[i]) ++j;
    b.tab.g[b.groups++] = {i, j - i, m[i], n[i], 0};
    i = j;
  }
  return lg_layout(b, false);
}

extern "C" size_t gfc_lg_workspace_bytes(int B, int M, int N) {
  LgBatch b;
  return lg_uniform(B, M, N, b, true) ? b.total : 0;
}
extern "C" size_t gfc_lg_packed_workspace_bytes(int B, int M, int N) {
  LgBatch b;
  return lg_uniform(B, M, N, b) ? b.total : 0;
}
extern "C" size_t gfc_lg_ragged_workspace_bytes(int B, const int32_t* m, const int32_t* n) {
  LgBatch b;
  return lg_ragged(B, m, n, b) ? b.total : 0;
}

// tables: self problems [2B][4], cross problems [2B][4], row0 [2B], n [2B], sizes [2B][2]; problem b = side 0 of
// pair b, B + b = side 1
__global__ void lg_tables_kernel(LgGroups t, int groups, int B, const float* size0, const float* size1, int* self_p,
                                 int* cross_p, int* row0, int* nrow, float* sizes) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int gi = 0;
  while (gi + 1 < groups && b >= t.g[gi + 1].first) ++gi;
  const LgGroup g = t.g[gi];
  const int M = g.m, N = g.n, k = b - g.first;
  const int r0 = g.row0 + k * M, r1 = g.row0 + g.count * M + k * N;
  int* s = self_p + 4 * b;
  s[0] = r0; s[1] = M; s[2] = r0; s[3] = M;
  s = self_p + 4 * (B + b);
  s[0] = r1; s[1] = N; s[2] = r1; s[3] = N;
  int* c = cross_p + 4 * b;
  c[0] = r0; c[1] = M; c[2] = r1; c[3] = N;
  c = cross_p + 4 * (B + b);
  c[0] = r1; c[1] = N; c[2] = r0; c[3] = M;
  row0[b] = r0; nrow[b] = M;
  row0[B + b] = r1; nrow[B + b] = N;
  sizes[2 * b] = size0[2 * b]; sizes[2 * b + 1] = size0[2 * b + 1];
  sizes[2 * (B + b)] = size1[2 * b]; sizes[2 * (B + b) + 1] = size1[2 * b + 1];
}

// ---- stage entry points (gfc_lg_forward is built from them; the adaptive depth / width path of
// lightglue.py:500-521 drives them layer by layer from the host) ----

extern "C" size_t gfc_lg_layer_workspace_bytes(int rows) { return rows <= 0 ? 0 : lg_layer_ws(rows).total; }

// the cross block with sim evaluated once: B pairs of (M, N) in chunks of `chunk`, score array sim (lg_cross_chunk)
struct LgCrossStored { int B, M, N, chunk; void* sim; size_t sim_bytes; };

static int lg_layer_impl(const gfc_lg_params* p, int l, float* x, const float* cosb, const float* sinb, const float* csb,
                         int R, const int32_t* self_p, const int32_t* cross_p, int n_problems, int maxn, void* ws,
                         size_t ws_bytes, void* stream, const float* x_in = nullptr, gfc_trace* tr = nullptr,
                         const LgCrossStored* xst = nullptr, float* keep_mid = nullptr, float* keep_ctx = nullptr,
                         float* keep_self = nullptr);

extern "C" int gfc_lg_layer(const gfc_lg_params* p, int l, float* x, const float* cosb, const float* sinb, int R,
                            const int32_t* self_p, const int32_t* cross_p, int n_problems, int maxn, void* ws,
                            size_t ws_bytes, void* stream) {
  return lg_layer_impl(p, l, x, cosb, sinb, nullptr, R, self_p, cross_p, n_problems, maxn, ws, ws_bytes, stream);
}

// ---- the two precisions of the matcher (gfc_lg_params.precision).  What a stage needs to know about one: the element
// type T of its matrix-product operands between two kernels (qkv, ctx, msg, mdesc; the rows x, hbuf and every output
// stay fp32), which matrix of a pair (w, w16) is read, and the GEMM / attention entry points in ONE argument order.
// linear(): a0 / y are T where a0_t / y_t say so and fp32 otherwise (to fp32 both are the same thing), a1 is always T.
struct LgF32 {  // GFC_LG_FP32: every contraction on the fp32 MFMA (gemm.hip, attention.hip)
  using T = float;
  static constexpr bool fp32 = true;
  static const void* w(const float* w32, const void*) { return w32; }
  static int linear(const void* a0, bool, int lda0, int k0, const T* a1, int lda1, int k1, const void* w, int ldw,
                    const float* bias, float alpha, const float* resid, const float*, const float* rot_cos,
                    const float* rot_sin, int rot_cols, void* y, bool, int ldy, int M, int N, hipStream_t st) {
    return gfc_linear((const float*)a0, lda0, k0, a1, lda1, k1, (const float*)w, ldw, bias, nullptr, nullptr, alpha,
                      resid, rot_cos, rot_sin, rot_cols, (float*)y, ldy, M, N, st);
  }
  static constexpr auto attention = gfc_attention;
  static constexpr auto batched_nt = gfc_batched_nt;
};
struct LgF16 {  // GFC_LG_FP16: fp16 operands (half of their fp32 slot in the workspace), fp32 sums (lg_fp16.hip)
  using T = _Float16;
  static constexpr bool fp32 = false;
  static const void* w(const float*, const void* w16) { return w16; }
  static int linear(const void* a0, bool a0_t, int lda0, int k0, const T* a1, int lda1, int k1, const void* w, int ldw,
                    const float* bias, float alpha, const float* resid, const float* rot_cs, const float* rot_cos,
                    const float* rot_sin, int rot_cols, void* y, bool y_t, int ldy, int M, int N, hipStream_t st) {
    return gfc_linear_f16(a0, a0_t, lda0, k0, a1, a1 != nullptr, lda1, k1, w, ldw, bias, alpha, resid, rot_cs, rot_cos,
                          rot_sin, rot_cols, y, y_t, ldy, M, N, st);
  }
  static constexpr auto attention = gfc_attention_f16;
  static constexpr auto batched_nt = gfc_batched_nt_f16;
};

static bool lg_f16_layer_ok(const gfc_lg_params* p, int l) {
  if (!p->wqkv16[l] || !p->s_ffn0_w16[l] || !p->s_ffn3_w16[l] || !p->c_qkv_w16[l] || !p->c_ffn0_w16[l] ||
      !p->c_ffn3_w16[l])
    return false;
  return (!p->s_out_w[l] || p->s_out_w16[l]) && (!p->c_out_w[l] || p->c_out_w16[l]);
}

// csb (optional): the rotary table packed for the QKV epilogue (one float4 per four channels instead of two)
// x_in (optional): the rows the SELF block reads (QKV operand, first half of the ffn[0] operand, residual); its result
// and everything after it live in x.  gfc_lg_forward_packed passes the caller's descriptors for layer 0, so that they
// are never copied into the row buffer.  tr (optional): event pairs around the two attention launches.  xst (optional,
// fp32 only): the cross block evaluates sim once; still one event pair around all of its launches.  keep_mid / keep_ctx
// (optional, fp32 only, [R,256]): copies of the rows the cross block reads and of the cross attention's context;
// keep_self (likewise): a copy of the SELF attention's context.
static int lg_layer_impl(const gfc_lg_params* p, int l, float* x, const float* cosb, const float* sinb, const float* csb,
                         int R, const int32_t* self_p, const int32_t* cross_p, int n_problems, int maxn, void* ws,
                         size_t ws_bytes, void* stream, const float* x_in, gfc_trace* tr, const LgCrossStored* xst,
                         float* keep_mid, float* keep_ctx, float* keep_self) {
  if ((keep_mid || keep_ctx || keep_self) && (!p || p->precision != GFC_LG_FP32)) return GFC_ERR_INVALID;
  if (!p || !x || !cosb || !sinb || !self_p || !cross_p || !ws || R <= 0 || n_problems <= 0 || maxn <= 0)
    return GFC_ERR_INVALID;
  if (l < 0 || l >= p->n_layers) return GFC_ERR_INVALID;
  if (p->precision != GFC_LG_FP32 && p->precision != GFC_LG_FP16) return GFC_ERR_INVALID;
  if (p->precision == GFC_LG_FP16 && !lg_f16_layer_ok(p, l)) return GFC_ERR_INVALID;
  const LgLayerWs L = lg_layer_ws(R);
  if (ws_bytes < L.total) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int D = 256;
  char* base = (char*)ws;
  float* hbuf = (float*)(base + L.hbuf);
  const float* xs = x_in ? x_in : x;  // what the self block reads

  auto layer = [&](auto prec) -> int {
    using P = decltype(prec);
    using T = typename P::T;
    T* qkv = (T*)(base + L.qkv);
    T* ctx = (T*)(base + L.ctx);
    T* msg = (T*)(base + L.msg);
    // attention (with its key split for small problem sets)
    auto attn = [&](const T* q, int ldq, const T* k, int ldk, const T* v, int ldv, const int32_t* probs) -> int {
      const bool rec = trace_begin(tr, st);
      const int s = P::attention(q, ldq, k, ldk, v, ldv, ctx, D, probs, n_problems, maxn, 4, 0.125f, base + L.att,
                                 L.att_bytes, st);
      trace_end(tr, st, rec);
      return s;
    };
    // y[R,n] (T) = a[R,256] . W^T + bias, rotated on the columns < rot_cols
    auto proj = [&](const void* a, bool a_t, const void* w, const float* bias, const float* rot_cs, const float* rot_cos,
                    const float* rot_sin, int rot_cols, T* y, int n) -> int {
      return P::linear(a, a_t, D, D, nullptr, 0, 0, w, D, bias, 1.f, nullptr, rot_cs, rot_cos, rot_sin, rot_cols, y, true, n,
                       R, n, st);
    };
    // the FFN (lightglue.py:143-148): [a0 | a1] . W0^T + b0 -> LayerNorm -> GELU (in place in the fp32 hbuf) ->
    // . W3^T + b3 + resid -> x.  fp32 only: the whole of it in one row-owning kernel once there are enough 128-row tiles
    // to cover the chip (>= 128: batch >= 8 pairs of 1024 points)
    auto ffn = [&](const float* a0, const T* a1, const void* w0, const float* b0, const float* ln_g, const float* ln_b,
                   const void* w3, const float* b3, const float* resid) -> int {
      if constexpr (P::fp32)
        if (R >= 128 * 128)
          return gfc_ffn_fused(a0, D, D, a1, D, D, (const float*)w0, 512, b0, ln_g, ln_b, (const float*)w3, 512, b3,
                               resid, x, D, R, st);
      GFC_TRY(P::linear(a0, false, D, D, a1, D, D, w0, 512, b0, 1.f, nullptr, nullptr, nullptr, nullptr, 0, hbuf, false,
                        512, R, 512, st));
      GFC_TRY(gfc_layernorm_gelu(hbuf, 512, R, 512, ln_g, ln_b, st));
      return P::linear(hbuf, false, 512, 512, nullptr, 0, 0, w3, 512, b3, 1.f, resid, nullptr, nullptr, nullptr, 0, x,
                       false, D, R, D, st);
    };
    // ---- self block (lightglue.py:151-164) ----
    if (P::fp32 && csb)  // fp32 only: a GEMM of its own whose epilogue reads the packed rotary table
      GFC_TRY(gfc_linear_rot_packed(xs, D, D, p->wqkv[l], D, p->bqkv[l], csb, 512, (float*)qkv, 768, R, 768, st));
    else
      GFC_TRY(proj(xs, false, P::w(p->wqkv[l], p->wqkv16[l]), p->bqkv[l], csb, csb ? nullptr : cosb,
                   csb ? nullptr : sinb, 512, qkv, 768));
    GFC_TRY(attn(qkv, 768, qkv + 256, 768, qkv + 512, 768, self_p));
    if (keep_self &&
        hipMemcpyAsync(keep_self, ctx, (size_t)R * D * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return GFC_ERR_LAUNCH;
    // out_proj is either a GEMM of its own, or (s_out_w == NULL) already folded into ffn0's second
    // K block at load time: [x | ctx] . [W0a | W0b.Wo]^T + (b0 + W0b.bo)
    const T* a1s = ctx;
    if (p->s_out_w[l]) {
      GFC_TRY(proj(ctx, true, P::w(p->s_out_w[l], p->s_out_w16[l]), p->s_out_b[l], nullptr, nullptr, nullptr, 0, msg, D));
      a1s = msg;
    }
    GFC_TRY(ffn(xs, a1s, P::w(p->s_ffn0_w[l], p->s_ffn0_w16[l]), p->s_ffn0_b[l], p->s_ln_g[l], p->s_ln_b[l],
                P::w(p->s_ffn3_w[l], p->s_ffn3_w16[l]), p->s_ffn3_b[l], xs));
    if (keep_mid && hipMemcpyAsync(keep_mid, x, (size_t)R * D * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return GFC_ERR_LAUNCH;
    // ---- cross block (lightglue.py:193-222) ----
    GFC_TRY(proj(x, false, P::w(p->c_qkv_w[l], p->c_qkv_w16[l]), p->c_qkv_b[l], nullptr, nullptr, nullptr, 0, qkv, 512));
    bool stored = false;
    if constexpr (P::fp32) {
      if (xst) {
        // the first xst->B problems of cross_p are the pairs' first directions: a chunk of them is a pair table
        stored = true;
        const bool rec = trace_begin(tr, st);
        int s = GFC_OK;
        for (int b0 = 0; b0 < xst->B && s == GFC_OK; b0 += xst->chunk)
          s = gfc_attention_cross_stored(qkv, 512, qkv + 256, 512, ctx, D, cross_p + 4 * b0,
                                         xst->B - b0 < xst->chunk ? xst->B - b0 : xst->chunk, xst->M, xst->N, 4, 0.125f,
                                         xst->sim, xst->sim_bytes, st);
        trace_end(tr, st, rec);
        GFC_TRY(s);
      }
    }
    if (!stored) GFC_TRY(attn(qkv, 512, qkv, 512, qkv + 256, 512, cross_p));
    if (keep_ctx && hipMemcpyAsync(keep_ctx, ctx, (size_t)R * D * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return GFC_ERR_LAUNCH;
    const T* a1c = ctx;
    if (p->c_out_w[l]) {
      GFC_TRY(proj(ctx, true, P::w(p->c_out_w[l], p->c_out_w16[l]), p->c_out_b[l], nullptr, nullptr, nullptr, 0, msg, D));
      a1c = msg;
    }
    return ffn(x, a1c, P::w(p->c_ffn0_w[l], p->c_ffn0_w16[l]), p->c_ffn0_b[l], p->c_ln_g[l], p->c_ln_b[l],
               P::w(p->c_ffn3_w[l], p->c_ffn3_w16[l]), p->c_ffn3_b[l], x);
  };
  return p->precision == GFC_LG_FP16 ? layer(LgF16{}) : layer(LgF32{});
}

// One layer of a uniform batch driven from the host, with the cross attention lg_forward_core takes for that batch
// (include/gfc_amd_layer_scores.h).  Workspace: one layer's | the score array of one chunk of pairs (lg_cross_chunk).
struct LgLayerPairsWs { size_t layer, sim, total, layer_bytes, sim_bytes; int chunk; };
static bool lg_layer_pairs_ws(int B, int M, int N, LgLayerPairsWs& L) {
  if (B <= 0 || M <= 0 || N <= 0 || (long long)B * ((long long)M + N) > INT_MAX / 768) return false;
  const int R = B * (M + N);
  L.chunk = lg_cross_chunk(B, M, N);
  L.layer_bytes = lg_layer_ws(R).total;
  L.sim_bytes = L.chunk ? gfc_attention_cross_stored_workspace_bytes(L.chunk, M, N, 4) : 0;
  gfc_slots s;
  L.layer = s.take(L.layer_bytes);
  L.sim = s.take(L.sim_bytes);
  L.total = s.off;
  return true;
}

extern "C" size_t gfc_lg_layer_pairs_workspace_bytes(int B, int M, int N) {
  LgLayerPairsWs L;
  return lg_layer_pairs_ws(B, M, N, L) ? L.total : 0;
}

static int lg_layer_pairs_impl(const gfc_lg_params* p, int l, float* x, const float* cosb, const float* sinb, int B, int M,
                               int N, const int32_t* self_p, const int32_t* cross_p, float* keep_mid, float* keep_ctx,
                               float* keep_self, void* ws, size_t ws_bytes, void* stream) {
  LgLayerPairsWs L;
  if (!p || !ws || !lg_layer_pairs_ws(B, M, N, L)) return GFC_ERR_INVALID;
  if (ws_bytes < L.total) return GFC_ERR_WORKSPACE;
  char* base = (char*)ws;
  const LgCrossStored xst = {B, M, N, L.chunk, base + L.sim, L.sim_bytes};
  const bool stored = L.chunk > 0 && p->precision == GFC_LG_FP32 && gfc_knobs().cross_stored != 0;
  return lg_layer_impl(p, l, x, cosb, sinb, nullptr, B * (M + N), self_p, cross_p, 2 * B, M > N ? M : N, base + L.layer,
                       L.layer_bytes, stream, nullptr, nullptr, stored ? &xst : nullptr, keep_mid, keep_ctx, keep_self);
}

extern "C" int gfc_lg_layer_pairs(const gfc_lg_params* p, int l, float* x, const float* cosb, const float* sinb, int B,
                                  int M, int N, const int32_t* self_p, const int32_t* cross_p, void* ws, size_t ws_bytes,
                                  void* stream) {
  return lg_layer_pairs_impl(p, l, x, cosb, sinb, B, M, N, self_p, cross_p, nullptr, nullptr, nullptr, ws, ws_bytes,
                             stream);
}

// ... with the rows the cross block reads and the cross attention's context kept (include/gfc_amd_ffn_backward.h)
extern "C" int gfc_lg_layer_pairs_keep(const gfc_lg_params* p, int l, float* x, const float* cosb, const float* sinb,
                                       int B, int M, int N, const int32_t* self_p, const int32_t* cross_p, float* x_mid,
                                       float* ctx, void* ws, size_t ws_bytes, void* stream) {
  if (!x_mid || !ctx) return GFC_ERR_INVALID;
  return lg_layer_pairs_impl(p, l, x, cosb, sinb, B, M, N, self_p, cross_p, x_mid, ctx, nullptr, ws, ws_bytes, stream);
}

// ... and the self attention's context too (include/gfc_amd_self_attn_backward.h)
extern "C" int gfc_lg_layer_pairs_keep_self(const gfc_lg_params* p, int l, float* x, const float* cosb, const float* sinb,
                                            int B, int M, int N, const int32_t* self_p, const int32_t* cross_p,
                                            float* x_mid, float* ctx, float* ctx_self, void* ws, size_t ws_bytes,
                                            void* stream) {
  if (!x_mid || !ctx || !ctx_self) return GFC_ERR_INVALID;
  return lg_layer_pairs_impl(p, l, x, cosb, sinb, B, M, N, self_p, cross_p, x_mid, ctx, ctx_self, ws, ws_bytes, stream);
}

// token confidence / matchability logits: out[row] = (sigmoid?)(x[row,:256] . w + b)   (lightglue.py:69-80,290-291)
__global__ void sigmoid_inplace_kernel(float* v, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = gfc_sigmoid(v[i]);
}
extern "C" int gfc_lg_rowdot(const float* x, int ld, int rows, const float* w, const float* b, int apply_sigmoid,
                             float* out, void* stream) {
  if (!x || !w || !b || !out || rows <= 0 || ld % 4) return GFC_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  GFC_TRY(gfc_rowdot256(x, ld, rows, w, b, out, st));
  if (apply_sigmoid) {
    hipLaunchKernelGGL(sigmoid_inplace_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, out, rows);
    GFC_LAUNCH_CHECK();
  }
  return GFC_OK;
}

extern "C" size_t gfc_lg_assign_workspace_bytes(int B, int M, int N) {
  return B <= 0 || M <= 0 || N <= 0 ? 0 : lg_assign_ws(B, M, N).total;
}

// MatchAssignment of layer l + filter_matches (lightglue.py:279-288,294-319).  x0 [B*M,256], x1 [B*N,256].
extern "C" int gfc_lg_assign(const gfc_lg_params* p, int l, const float* x0, const float* x1, int B, int M, int N,
                             float threshold, int64_t* m0, int64_t* m1, float* ms0, float* ms1, float* log_assignment,
                             void* ws, size_t ws_bytes, void* stream) {
  if (!p || !x0 || !x1 || !m0 || !m1 || !ms0 || !ms1 || !log_assignment || !ws || B <= 0 || M <= 0 || N <= 0)
    return GFC_ERR_INVALID;
  if (l < 0 || l >= p->n_layers || !p->final_proj_w[l] || !p->matchability_w[l]) return GFC_ERR_INVALID;
  if (p->precision != GFC_LG_FP32 && p->precision != GFC_LG_FP16) return GFC_ERR_INVALID;
  if (p->precision == GFC_LG_FP16 && !p->final_proj_w16[l]) return GFC_ERR_INVALID;
  const LgAssignWs L = lg_assign_ws(B, M, N);
  if (ws_bytes < L.total) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int D = 256, R0 = B * M, R1 = B * N;
  float* md = (float*)((char*)ws + L.md);
  float* z = (float*)((char*)ws + L.z);
  void* tail = (char*)ws + L.tail;
  auto head = [&](auto prec) -> int {
    using P = decltype(prec);
    // mdesc (T: fp16 fills the front half of the fp32 slot) and the similarity on this precision's MFMA; sim is fp32
    typename P::T* md0 = (typename P::T*)md;
    typename P::T* md1 = md0 + (size_t)R0 * D;
    const void* w = P::w(p->final_proj_w[l], p->final_proj_w16[l]);
    GFC_TRY(P::linear(x0, false, D, D, nullptr, 0, 0, w, D, p->final_proj_b[l], 0.25f, nullptr, nullptr, nullptr, nullptr,
                      0, md0, true, D, R0, D, st));
    GFC_TRY(P::linear(x1, false, D, D, nullptr, 0, 0, w, D, p->final_proj_b[l], 0.25f, nullptr, nullptr, nullptr, nullptr,
                      0, md1, true, D, R1, D, st));
    GFC_TRY(gfc_rowdot256(x0, D, R0, p->matchability_w[l], p->matchability_b[l], z, st));
    GFC_TRY(gfc_rowdot256(x1, D, R1, p->matchability_w[l], p->matchability_b[l], z + R0, st));
    GFC_TRY(P::batched_nt(md0, D, (long long)M * D, md1, D, (long long)N * D, log_assignment, N + 1,
                          (long long)(M + 1) * (N + 1), M, N, D, B, st));
    // statistics in one sweep, final scores + arg-max in a second one
    return gfc_assign_filter_fused(log_assignment, z, z + R0, B, M, N, threshold, m0, m1, ms0, ms1, tail, st);
  };
  return p->precision == GFC_LG_FP16 ? head(LgF16{}) : head(LgF32{});
}

// descriptors [R, input_dim] -> rows x [R,256] (input_proj, lightglue.py:352-355,464-465)
static int lg_input_proj(const gfc_lg_params* p, const float* desc, float* x, int R, hipStream_t st) {
  const int Din = p->input_dim;
  auto run = [&](auto prec) -> int {
    using P = decltype(prec);
    return P::linear(desc, false, Din, Din, nullptr, 0, 0, P::w(p->input_proj_w, p->input_proj_w16), Din, p->input_proj_b,
                     1.f, nullptr, nullptr, nullptr, nullptr, 0, x, false, 256, R, 256, st);
  };
  return p->precision == GFC_LG_FP16 ? run(LgF16{}) : run(LgF32{});
}

// The matcher over a batch: tables -> rotary tables -> input_proj -> n_layers x layer -> one assignment head + filter
// per group.  kp [R,2] / so [R,2] (nullable) / desc [R,Din] in the batch's row order; desc == NULL: the rows are
// already in x.  x [R,256]: the row buffer every layer updates in place; it ends up holding the last layer's
// descriptors.  Outputs are flat in pair order (one group: exactly the [B,M] / [B,N] / [B,M+1,N+1] arrays).
static int lg_forward_core(const gfc_lg_params* p, const LgBatch& bt, const float* kp, const float* so, const float* desc,
                           const float* size0, const float* size1, float threshold, int64_t* m0, int64_t* m1,
                           float* ms0, float* ms1, float* log_assignment, float* x, char* base, gfc_trace* tr,
                           hipStream_t st) {
  const int B = bt.B, R = bt.R, D = 256;
  float* cosb = (float*)(base + bt.cosb);
  float* sinb = (float*)(base + bt.sinb);
  float* csb = (float*)(base + bt.csb);
  int* self_p = (int*)(base + bt.tables);
  int* cross_p = self_p + 8 * B;
  int* row0 = cross_p + 8 * B;
  int* nrow = row0 + 2 * B;
  float* sizes = (float*)(nrow + 2 * B);
  const int pdim = p->posenc_dim == 0 ? 2 : p->posenc_dim;

  hipLaunchKernelGGL(lg_tables_kernel, dim3((B + 63) / 64), dim3(64), 0, st, bt.tab, bt.groups, B, size0, size1, self_p,
                     cross_p, row0, nrow, sizes);
  GFC_LAUNCH_CHECK();
  GFC_TRY(gfc_lg_posenc_packed(kp, so, sizes, row0, nrow, 2 * B, bt.maxn, p->posenc_wr, pdim, cosb, sinb, csb, st));

  // descriptors -> rows.  input_dim == 256: layer 0's self block reads them where they are (no copy);
  // otherwise input_proj writes the rows (lightglue.py:352-355,464-465)
  const float* x_in = desc;
  if (p->input_dim != D) {
    GFC_TRY(lg_input_proj(p, desc, x, R, st));
    x_in = nullptr;
  }
  // fp32, one group of equal pairs that passes the gate of lg_cross_chunk: the cross block evaluates sim once
  const LgCrossStored xst = {B, bt.tab.g[0].m, bt.tab.g[0].n, bt.cross_chunk, base + bt.sim, bt.sim_bytes};
  const bool stored = bt.cross_chunk > 0 && p->precision == GFC_LG_FP32 && gfc_knobs().cross_stored != 0;
  for (int l = 0; l < p->n_layers; ++l)
    GFC_TRY(lg_layer_impl(p, l, x, cosb, sinb, csb, R, self_p, cross_p, 2 * B, bt.maxn, base + bt.stage, bt.stage_bytes, st,
                          l == 0 ? x_in : nullptr, tr, stored ? &xst : nullptr));

  // ---- assignment (lightglue.py:279-288) + filter (lightglue.py:294-319), one batched call per group ----
  size_t o0 = 0, o1 = 0, os = 0;
  for (int i = 0; i < bt.groups; ++i) {
    const LgGroup& g = bt.tab.g[i];
    const float* x0 = x + (size_t)g.row0 * D;
    const float* x1 = x0 + (size_t)g.count * g.m * D;
    GFC_TRY(gfc_lg_assign(p, p->n_layers - 1, x0, x1, g.count, g.m, g.n, threshold, m0 + o0, m1 + o1, ms0 + o0,
                          ms1 + o1, log_assignment + os, base + bt.stage, bt.stage_bytes, st));
    o0 += (size_t)g.count * g.m; o1 += (size_t)g.count * g.n; os += (size_t)g.count * (g.m + 1) * (g.n + 1);
  }
  return GFC_OK;
}

static bool lg_params_ok(const gfc_lg_params* p, bool has_so) {
  if (p->n_layers <= 0 || p->n_layers > GFC_LG_MAX_LAYERS) return false;
  if (p->input_dim != 256 && (!p->input_proj_w || !p->input_proj_b || p->input_dim % 32)) return false;
  const int pdim = p->posenc_dim == 0 ? 2 : p->posenc_dim;
  if (!((pdim == 2 || pdim == 4) && (pdim == 4) == has_so)) return false;
  if (p->precision == GFC_LG_FP32) return true;
  if (p->precision != GFC_LG_FP16 || (p->input_dim != 256 && !p->input_proj_w16)) return false;
  for (int l = 0; l < p->n_layers; ++l)
    if (!lg_f16_layer_ok(p, l)) return false;
  return p->final_proj_w16[p->n_layers - 1] != nullptr;
}

// gfc_lg_forward_packed / gfc_lg_forward_ragged behind their pointer checks, on the batch either of them laid out
static int lg_forward_rows(const gfc_lg_params* p, const LgBatch& bt, const float* kpts, const float* desc,
                           const float* size0, const float* size1, const float* scale_ori, float threshold, int64_t* m0,
                           int64_t* m1, float* ms0, float* ms1, float* log_assignment, float* rows, void* ws,
                           size_t ws_bytes, gfc_trace* attention_trace, void* stream) {
  if (!lg_params_ok(p, scale_ori != nullptr)) return GFC_ERR_INVALID;
  if (rows == desc) return GFC_ERR_INVALID;  // the caller's descriptors are read-only
  if (ws_bytes < bt.total) return GFC_ERR_WORKSPACE;
  return lg_forward_core(p, bt, kpts, scale_ori, desc, size0, size1, threshold, m0, m1, ms0, ms1, log_assignment, rows,
                         (char*)ws, attention_trace, (hipStream_t)stream);
}

extern "C" int gfc_lg_forward_packed(const gfc_lg_params* p, const float* kpts, const float* desc, const float* size0,
                                     const float* size1, const float* scale_ori, int B, int M, int N, float threshold,
                                     int64_t* m0, int64_t* m1, float* ms0, float* ms1, float* log_assignment, float* rows,
                                     void* ws, size_t ws_bytes, gfc_trace* attention_trace, void* stream) {
  if (!p || !kpts || !desc || !size0 || !size1 || !m0 || !m1 || !ms0 || !ms1 || !log_assignment || !rows || !ws)
    return GFC_ERR_INVALID;
  LgBatch bt;
  if (!lg_uniform(B, M, N, bt)) return GFC_ERR_INVALID;
  return lg_forward_rows(p, bt, kpts, desc, size0, size1, scale_ori, threshold, m0, m1, ms0, ms1, log_assignment, rows, ws,
                         ws_bytes, attention_trace, stream);
}

extern "C" int gfc_lg_forward_ragged(const gfc_lg_params* p, const float* kpts, const float* desc, const float* size0,
                                     const float* size1, const float* scale_ori, int B, const int32_t* m,
                                     const int32_t* n, float threshold, int64_t* m0, int64_t* m1, float* ms0, float* ms1,
                                     float* log_assignment, float* rows, void* ws, size_t ws_bytes,
                                     gfc_trace* attention_trace, void* stream) {
  if (!p || !kpts || !desc || !size0 || !size1 || !m0 || !m1 || !ms0 || !ms1 || !log_assignment || !rows || !ws)
    return GFC_ERR_INVALID;
  LgBatch bt;
  if (!lg_ragged(B, m, n, bt)) return GFC_ERR_INVALID;
  return lg_forward_rows(p, bt, kpts, desc, size0, size1, scale_ori, threshold, m0, m1, ms0, ms1, log_assignment, rows, ws,
                         ws_bytes, attention_trace, stream);
}

extern "C" int gfc_lg_forward(const gfc_lg_params* p, const float* kpts0, const float* kpts1, const float* desc0,
                              const float* desc1, const float* size0, const float* size1,
                              const float* scale_ori0, const float* scale_ori1, int B, int M, int N,
                              float threshold, int64_t* m0, int64_t* m1, float* ms0, float* ms1,
                              float* log_assignment, float* ref_desc0, float* ref_desc1, void* ws, size_t ws_bytes,
                              void* stream) {
  if (!p || !kpts0 || !kpts1 || !desc0 || !desc1 || !size0 || !size1 || !m0 || !m1 || !ms0 || !ms1 ||
      !log_assignment || !ws)
    return GFC_ERR_INVALID;
  LgBatch bt;
  if (!lg_params_ok(p, scale_ori0 != nullptr && scale_ori1 != nullptr) || !lg_uniform(B, M, N, bt, true))
    return GFC_ERR_INVALID;
  if ((scale_ori0 != nullptr) != (scale_ori1 != nullptr)) return GFC_ERR_INVALID;
  const int R0 = B * M, R1 = B * N;
  const int Din = p->input_dim;
  const bool adjacent = desc1 == desc0 + (size_t)R0 * Din;
  // descriptors of an input_dim != 256 model that are not adjacent are packed into the layer scratch: they must fit
  if (!adjacent && Din != 256 && (size_t)bt.R * Din * 4 > bt.stage_bytes) return GFC_ERR_INVALID;
  if (ws_bytes < bt.total) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  float* x = (float*)(base + bt.x);
  float* kp = (float*)(base + bt.kp);
  auto d2d = [&](void* dst, const void* src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
  };
  // the two sides arrive as separate arrays: pack key points (and scales / orientations) behind each other
  if (!d2d(kp, kpts0, (size_t)R0 * 2 * 4) || !d2d(kp + (size_t)R0 * 2, kpts1, (size_t)R1 * 2 * 4)) return GFC_ERR_LAUNCH;
  float* so = nullptr;
  if (scale_ori0) {
    so = kp + (size_t)bt.R * 2;
    if (!d2d(so, scale_ori0, (size_t)R0 * 2 * 4) || !d2d(so + (size_t)R0 * 2, scale_ori1, (size_t)R1 * 2 * 4))
      return GFC_ERR_LAUNCH;
  }
  // descriptors: packed into the row buffer (input_dim == 256), or -- when the two arrays happen to be adjacent in
  // memory -- read in place; with an input projection the packed copy lives in the (not yet used) layer scratch
  const float* desc = desc0;
  if (!adjacent) {
    float* stage = Din == 256 ? x : (float*)(base + bt.stage);
    if (!d2d(stage, desc0, (size_t)R0 * Din * 4) || !d2d(stage + (size_t)R0 * Din, desc1, (size_t)R1 * Din * 4))
      return GFC_ERR_LAUNCH;
    desc = stage;
  }
  // (desc == x is fine here: layer 0 then simply works in place)
  GFC_TRY(lg_forward_core(p, bt, kp, so, desc == x ? nullptr : desc, size0, size1, threshold, m0, m1, ms0, ms1,
                          log_assignment, x, base, nullptr, st));
  if (ref_desc0 && !d2d(ref_desc0, x, (size_t)R0 * 256 * 4)) return GFC_ERR_LAUNCH;
  if (ref_desc1 && !d2d(ref_desc1, x + (size_t)R0 * 256, (size_t)R1 * 256 * 4)) return GFC_ERR_LAUNCH;
  return GFC_OK;
}
