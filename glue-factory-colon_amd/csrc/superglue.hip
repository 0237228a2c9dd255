// SuperGlue matcher (gluefactory_nonfree/superglue.py:268-322, inference path): the key-point encoder, the Sinkhorn
// optimal-transport solver and the host sequence of the whole matcher.  The attention, the GEMMs, the batched
// similarity and the match filter are the kernels LightGlue runs on (attention.hip, gemm.hip, lg_misc.hip); the
// propagation MLP is the BatchNorm + ReLU instantiation of the fused FFN kernel (gemm.hip).  All fp32; rows are
// row-major [rows,256] where the reference is channel-first Conv1d on [B,256,N].
#include <climits>
#include <cmath>

#include "common.h"

#define GFC_TRY(expr)            \
  do {                           \
    int s_ = (expr);             \
    if (s_ != GFC_OK) return s_; \
  } while (0)

// ------------------------------------------------------------------------------------------
// Key-point encoder (superglue.py:85-111): [x, y, score] -> 32 -> 64 -> 128 -> 256 (-> 256 by the GEMM behind it).
// One workgroup owns KE_ROWS rows; the activations of every layer stay in LDS.  In a layer with COUT outputs thread t
// owns output column t % COUT of KE_ROWS * COUT / 256 rows, so a weight is loaded once for all of them (the weights are
// packed [cin][cout]: consecutive lanes read consecutive floats) and the activations are LDS broadcasts.
// ------------------------------------------------------------------------------------------
#define KE_ROWS 32
#define KE_LDA 260  // row strides of the two LDS activation buffers in floats (16-byte aligned rows):
#define KE_LDB 132  // A holds the input and the 64- and 256-wide layers, B the 32- and 128-wide ones

template <int CIN, int COUT, int LDI, int LDO>
__device__ __forceinline__ void kenc_layer(const float* __restrict__ in, float* __restrict__ out,
                                           const float* __restrict__ wt, const float* __restrict__ bias,
                                           const float* __restrict__ scale, const float* __restrict__ shift, int tid) {
  constexpr int GROUPS = 256 / COUT, RPT = KE_ROWS / GROUPS;
  const int c = tid % COUT, r0 = (tid / COUT) * RPT;
  float acc[RPT];
#pragma unroll
  for (int j = 0; j < RPT; ++j) acc[j] = 0.f;
  if constexpr (CIN % 4 == 0) {
    for (int k = 0; k < CIN; k += 4) {
      const float w0 = wt[(k + 0) * COUT + c], w1 = wt[(k + 1) * COUT + c];
      const float w2 = wt[(k + 2) * COUT + c], w3 = wt[(k + 3) * COUT + c];
#pragma unroll
      for (int j = 0; j < RPT; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(in + (r0 + j) * LDI + k);
        acc[j] = fmaf(a.x, w0, acc[j]);
        acc[j] = fmaf(a.y, w1, acc[j]);
        acc[j] = fmaf(a.z, w2, acc[j]);
        acc[j] = fmaf(a.w, w3, acc[j]);
      }
    }
  } else {
    for (int k = 0; k < CIN; ++k) {
      const float w = wt[k * COUT + c];
#pragma unroll
      for (int j = 0; j < RPT; ++j) acc[j] = fmaf(in[(r0 + j) * LDI + k], w, acc[j]);
    }
  }
  const float b = bias[c], sc = scale[c], sh = shift[c];
#pragma unroll
  for (int j = 0; j < RPT; ++j) out[(r0 + j) * LDO + c] = fmaxf((acc[j] + b) * sc + sh, 0.f);
}

struct KencArgs {
  const float* w[4];      // [cin][cout]
  const float* b[4];
  const float* scale[4];  // eval-mode BatchNorm folded: y * scale + shift
  const float* shift[4];
};

template <int CIN>
__global__ __launch_bounds__(256) void sg_kenc_kernel(KencArgs a, const float* __restrict__ kpts,
                                                      const float* __restrict__ scores,
                                                      const float* __restrict__ sizes, int n, int rows,
                                                      float* __restrict__ hidden) {
  __shared__ __attribute__((aligned(16))) float bufA[KE_ROWS * KE_LDA];
  __shared__ __attribute__((aligned(16))) float bufB[KE_ROWS * KE_LDB];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * KE_ROWS;
  if (tid < KE_ROWS) {  // normalize_keypoints (superglue.py:92-94): (k - size / 2) / (0.7 max(w, h))
    const int row = min(row0 + tid, rows - 1);
    const int img = row / n;
    const float w = sizes[2 * img], h = sizes[2 * img + 1];
    const float sc = fmaxf(w, h) * 0.7f;
    bufA[tid * KE_LDA + 0] = (kpts[2 * (size_t)row] - w / 2.f) / sc;
    bufA[tid * KE_LDA + 1] = (kpts[2 * (size_t)row + 1] - h / 2.f) / sc;
    if (CIN == 3) bufA[tid * KE_LDA + 2] = scores[row];
  }
  __syncthreads();
  kenc_layer<CIN, 32, KE_LDA, KE_LDB>(bufA, bufB, a.w[0], a.b[0], a.scale[0], a.shift[0], tid);
  __syncthreads();
  kenc_layer<32, 64, KE_LDB, KE_LDA>(bufB, bufA, a.w[1], a.b[1], a.scale[1], a.shift[1], tid);
  __syncthreads();
  kenc_layer<64, 128, KE_LDA, KE_LDB>(bufA, bufB, a.w[2], a.b[2], a.scale[2], a.shift[2], tid);
  __syncthreads();
  kenc_layer<128, 256, KE_LDB, KE_LDA>(bufB, bufA, a.w[3], a.b[3], a.scale[3], a.shift[3], tid);
  __syncthreads();
  for (int r = 0; r < KE_ROWS; ++r)
    if (row0 + r < rows) hidden[(size_t)(row0 + r) * 256 + tid] = bufA[r * KE_LDA + tid];
}

struct KencWs { size_t hidden, total; };
static KencWs kenc_ws(long long rows) {
  gfc_slots s;
  return {s.take((size_t)rows * 256 * 4), s.off};
}

extern "C" size_t gfc_sg_keypoint_encoder_workspace_bytes(int rows) { return rows <= 0 ? 0 : kenc_ws(rows).total; }

static bool sg_kenc_ok(const gfc_sg_params* p) {
  for (int i = 0; i < 4; ++i)
    if (!p->kenc_w[i] || !p->kenc_b[i] || !p->kenc_scale[i] || !p->kenc_shift[i]) return false;
  return p->kenc_w[4] && p->kenc_b[4];
}

extern "C" int gfc_sg_keypoint_encoder(const gfc_sg_params* p, const float* kpts, const float* scores,
                                       const float* sizes, int B, int n, float* desc, void* ws, size_t ws_bytes,
                                       void* stream) {
  if (!p || !kpts || !sizes || !desc || !ws || B <= 0 || n <= 0 || !sg_kenc_ok(p)) return GFC_ERR_INVALID;
  if ((p->use_scores != 0) != (scores != nullptr)) return GFC_ERR_INVALID;
  const long long rows = (long long)B * n;
  if (rows > INT_MAX / 768) return GFC_ERR_INVALID;
  const KencWs L = kenc_ws(rows);
  if (ws_bytes < L.total) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* hidden = (float*)((char*)ws + L.hidden);
  KencArgs a;
  for (int i = 0; i < 4; ++i) {
    a.w[i] = p->kenc_w[i]; a.b[i] = p->kenc_b[i]; a.scale[i] = p->kenc_scale[i]; a.shift[i] = p->kenc_shift[i];
  }
  const dim3 grid((unsigned)((rows + KE_ROWS - 1) / KE_ROWS));
  if (scores)
    hipLaunchKernelGGL(sg_kenc_kernel<3>, grid, dim3(256), 0, st, a, kpts, scores, sizes, n, (int)rows, hidden);
  else
    hipLaunchKernelGGL(sg_kenc_kernel<2>, grid, dim3(256), 0, st, a, kpts, scores, sizes, n, (int)rows, hidden);
  GFC_LAUNCH_CHECK();
  // the last layer has no BatchNorm / ReLU: desc += hidden . W4^T + b4 on the matrix pipe
  return gfc_linear(hidden, 256, 256, nullptr, 0, 0, p->kenc_w[4], 256, p->kenc_b[4], nullptr, nullptr, 1.f, desc, nullptr,
                    nullptr, 0, desc, 256, (int)rows, 256, st);
}

// ------------------------------------------------------------------------------------------
// Sinkhorn (superglue.py:188-216) in the log domain.  The augmented matrix Z [M+1,N+1] (scores, a last row and a last
// column of bin_score) is never stored: it is read from `cost`, the border synthesised.  One iteration is
//   rows kernel : a workgroup owns `rb` whole rows, holds them in LDS (one read of the matrix per iteration), computes
//                 u_i = log_mu_i - LSE_j(Z_ij + v_j) for them and, with u known, the partial (max, sum) over ITS rows
//                 of Z_ij + u_i for every column j;
//   merge kernel: v_j = log_nu_j - LSE_i(..) from the partials of all row blocks.
// Each half-step needs the whole of the other vector, so the two are separate launches in stream order: no workgroup
// ever waits for another one inside a kernel.  LSE as torch.logsumexp: maximum subtracted, log(sum(exp)) + maximum.
// ------------------------------------------------------------------------------------------
#define SK_THREADS 512
#define SK_LDS_MAX (160 * 1024)

struct SkPlan {
  int rb, nblk;       // rows per workgroup, row blocks per matrix
  size_t lds;         // dynamic LDS of the rows kernel
  size_t u, v, part, total;  // workspace slots: u [B,M+1] | v [B,N+1] | part [B,nblk,N+1][max, sum]
};
// false: a single row of N + 1 columns (plus v) does not fit in LDS
static bool sk_plan(int B, int M, int N, SkPlan& k) {
  const size_t row = (size_t)(N + 1) * 4;
  const size_t fit = (SK_LDS_MAX - 32 * 4) / row;  // rows + the v vector, beside at most 32 values of u
  if (fit < 2) return false;
  // a function of (M, N) alone, so that a pair's result does not depend on the batch it runs in: about 64 row blocks
  // per matrix (a single pair still spreads over the chip, and the partials stay near an eighth of the matrix), at
  // least 8 and at most 32 rows each
  int rb = (M + 64) / 64;
  if (rb < 8) rb = 8;
  if (rb > 32) rb = 32;
  if (rb > (int)(fit - 1)) rb = (int)(fit - 1);
  if (rb > M + 1) rb = M + 1;
  k.rb = rb;
  k.nblk = (M + rb) / rb;  // ceil((M + 1) / rb)
  k.lds = (size_t)(rb + 1) * row + (size_t)rb * 4;
  gfc_slots s;
  k.u = s.take((size_t)B * (M + 1) * 4);
  k.v = s.take((size_t)B * (N + 1) * 4);
  k.part = s.take((size_t)B * k.nblk * (N + 1) * 8);
  k.total = s.off;
  return true;
}

__global__ __launch_bounds__(SK_THREADS) void sg_sinkhorn_rows_kernel(const float* __restrict__ cost, float alpha,
                                                                      const float* __restrict__ v,
                                                                      float* __restrict__ u,
                                                                      float2* __restrict__ part, int M, int N, int rb,
                                                                      int nblk, float log_mu, float log_mu_bin) {
  extern __shared__ __attribute__((aligned(16))) float sk_smem[];
  const int C = N + 1;
  float* tile = sk_smem;               // [rb][C]
  float* vs = sk_smem + (size_t)rb * C;  // [C]
  float* us = vs + C;                  // [rb]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int row0 = blk * rb;
  const int nr = min(rb, M + 1 - row0);  // >= 1
  const float* cb = cost + (size_t)b * M * N;
  const float* vb = v + (size_t)b * C;
  for (int j = tid; j < C; j += SK_THREADS) vs[j] = vb[j];
  for (int r = 0; r < nr; ++r) {
    const int i = row0 + r;
    float* t = tile + (size_t)r * C;
    if (i < M) {
      const float* c = cb + (size_t)i * N;
      for (int j = tid; j < N; j += SK_THREADS) t[j] = c[j];
      if (tid == 0) t[N] = alpha;
    } else {
      for (int j = tid; j < C; j += SK_THREADS) t[j] = alpha;
    }
  }
  __syncthreads();
  // u of my rows: one wave per row
  for (int r = wave; r < nr; r += SK_THREADS / 64) {
    const float* t = tile + (size_t)r * C;
    float mx = -INFINITY;
    for (int j = lane; j < C; j += 64) mx = fmaxf(mx, t[j] + vs[j]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int j = lane; j < C; j += 64) s += expf((t[j] + vs[j]) - mx);
    s = wave_sum(s);
    const float ui = (row0 + r < M ? log_mu : log_mu_bin) - (logf(s) + mx);
    if (lane == 0) {
      us[r] = ui;
      u[(size_t)b * (M + 1) + row0 + r] = ui;
    }
  }
  __syncthreads();
  // per column: (max, sum of exp) of Z + u over my rows
  float2* pb = part + ((size_t)b * nblk + blk) * C;
  for (int j = tid; j < C; j += SK_THREADS) {
    float mx = -INFINITY;
    for (int r = 0; r < nr; ++r) mx = fmaxf(mx, tile[(size_t)r * C + j] + us[r]);
    float s = 0.f;
    for (int r = 0; r < nr; ++r) s += expf((tile[(size_t)r * C + j] + us[r]) - mx);
    pb[j] = make_float2(mx, s);
  }
}

__global__ __launch_bounds__(256) void sg_sinkhorn_merge_kernel(const float2* __restrict__ part, int N, int nblk,
                                                                float log_nu, float log_nu_bin,
                                                                float* __restrict__ v) {
  const int C = N + 1;
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= C) return;
  const float2* p = part + (size_t)b * nblk * C + j;
  float mx = -INFINITY;
  for (int k = 0; k < nblk; ++k) mx = fmaxf(mx, p[(size_t)k * C].x);
  float s = 0.f;
  for (int k = 0; k < nblk; ++k) {
    const float2 q = p[(size_t)k * C];
    s += q.y * expf(q.x - mx);
  }
  v[(size_t)b * C + j] = (j < N ? log_nu : log_nu_bin) - (logf(s) + mx);
}

__global__ __launch_bounds__(256) void sg_sinkhorn_finalize_kernel(const float* __restrict__ cost, float alpha,
                                                                   const float* __restrict__ u,
                                                                   const float* __restrict__ v, int M, int N,
                                                                   float norm, float* __restrict__ out) {
  const int C = N + 1;
  const int i = blockIdx.y, b = blockIdx.z;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= C) return;
  const float z = (i < M && j < N) ? cost[((size_t)b * M + i) * N + j] : alpha;
  out[((size_t)b * (M + 1) + i) * C + j] = ((z + u[(size_t)b * (M + 1) + i]) + v[(size_t)b * C + j]) - norm;
}

extern "C" size_t gfc_sg_sinkhorn_workspace_bytes(int B, int M, int N) {
  SkPlan k;
  return B <= 0 || M <= 0 || N <= 0 || !sk_plan(B, M, N, k) ? 0 : k.total;
}

extern "C" int gfc_sg_sinkhorn(const float* cost, float bin_score, int B, int M, int N, int iters, float* out, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!cost || !out || !ws || B <= 0 || M <= 0 || N <= 0 || iters < 0) return GFC_ERR_INVALID;
  if (B > 65535 || M + 1 > 65535 || (long long)B * (M + 1) > INT_MAX / 32) return GFC_ERR_INVALID;  // grid limits
  SkPlan k;
  if (!sk_plan(B, M, N, k)) return GFC_ERR_UNSUPPORTED;
  if (ws_bytes < k.total) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* u = (float*)((char*)ws + k.u);
  float* v = (float*)((char*)ws + k.v);
  float2* part = (float2*)((char*)ws + k.part);
  // log_mu / log_nu of superglue.py:209-211, in fp32 like the reference's tensors
  const float ms = (float)M, ns = (float)N;
  const float norm = -logf(ms + ns);
  const float log_mu_bin = logf(ns) + norm, log_nu_bin = logf(ms) + norm;
  if (hipMemsetAsync(u, 0, (size_t)B * (M + 1) * 4, st) != hipSuccess) return GFC_ERR_LAUNCH;
  if (hipMemsetAsync(v, 0, (size_t)B * (N + 1) * 4, st) != hipSuccess) return GFC_ERR_LAUNCH;
  static std::atomic<unsigned long long> lds_ok{0};
  gfc_allow_dynamic_lds((const void*)sg_sinkhorn_rows_kernel, SK_LDS_MAX, lds_ok);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(sg_sinkhorn_rows_kernel, dim3((unsigned)(B * k.nblk)), dim3(SK_THREADS), k.lds, st, cost, bin_score,
                       v, u, part, M, N, k.rb, k.nblk, norm, log_mu_bin);
    hipLaunchKernelGGL(sg_sinkhorn_merge_kernel, dim3((N + 256) / 256, B), dim3(256), 0, st, part, N, k.nblk, norm,
                       log_nu_bin, v);
  }
  hipLaunchKernelGGL(sg_sinkhorn_finalize_kernel, dim3((N + 256) / 256, M + 1, B), dim3(256), 0, st, cost, bin_score, u, v,
                     M, N, norm, out);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

// ------------------------------------------------------------------------------------------
// The whole matcher for a uniform batch (superglue.py:268-322)
// ------------------------------------------------------------------------------------------
// x [R,256] rows (side 0 of every pair, then side 1) | qkv [R,768] (first the encoder's hidden rows, last the
// final_proj output) | ctx [R,256] attention output | msg [R,256] merged message | attention key-split scratch |
// problem tables | Sinkhorn | filter
struct SgWs { size_t x, qkv, ctx, msg, att, tables, sink, filt, total, att_bytes, sink_bytes, filt_bytes; };
static bool sg_ws(int B, int M, int N, SgWs& L) {
  if (B <= 0 || M <= 0 || N <= 0) return false;
  const long long R = (long long)B * ((long long)M + N);
  if (R > INT_MAX / 768) return false;
  SkPlan k;
  if (!sk_plan(B, M, N, k)) return false;
  const size_t r = (size_t)R;
  L.att_bytes = R <= 8192 ? gfc_att_scratch_bytes(r, 4, GFC_ATT_MAX_SPLIT) : 0;
  L.sink_bytes = k.total;
  L.filt_bytes = (size_t)B * (M + N) * 8;
  gfc_slots s;
  L.x = s.take(r * 256 * 4);
  L.qkv = s.take(r * 768 * 4);
  L.ctx = s.take(r * 256 * 4);
  L.msg = s.take(r * 256 * 4);
  L.att = s.take(L.att_bytes);
  L.tables = s.take((size_t)B * 16 * 4);
  L.sink = s.take(L.sink_bytes);
  L.filt = s.take(L.filt_bytes);
  L.total = s.off;
  return true;
}

extern "C" size_t gfc_sg_workspace_bytes(int B, int M, int N) {
  SgWs L;
  return sg_ws(B, M, N, L) ? L.total : 0;
}

// attention problems {q_row0, n_q, kv_row0, n_kv}: entry b = side 0 of pair b, B + b = side 1
__global__ void sg_tables_kernel(int B, int M, int N, int* __restrict__ self_p, int* __restrict__ cross_p) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int r0 = b * M, r1 = B * M + b * N;
  int* s = self_p + 4 * b;
  s[0] = r0; s[1] = M; s[2] = r0; s[3] = M;
  s = self_p + 4 * (B + b);
  s[0] = r1; s[1] = N; s[2] = r1; s[3] = N;
  int* c = cross_p + 4 * b;
  c[0] = r0; c[1] = M; c[2] = r1; c[3] = N;
  c = cross_p + 4 * (B + b);
  c[0] = r1; c[1] = N; c[2] = r0; c[3] = M;
}

extern "C" int gfc_sg_forward(const gfc_sg_params* p, const float* kpts0, const float* kpts1, const float* scores0,
                              const float* scores1, const float* desc0, const float* desc1, const float* size0,
                              const float* size1, int B, int M, int N, int iters, float threshold,
                              float* sinkhorn_cost, float* log_assignment, int64_t* m0, int64_t* m1, float* ms0,
                              float* ms1, float* desc_taps, void* ws, size_t ws_bytes, void* stream) {
  if (!p || !kpts0 || !kpts1 || !desc0 || !desc1 || !size0 || !size1 || !sinkhorn_cost || !log_assignment || !m0 ||
      !m1 || !ms0 || !ms1 || !ws || iters < 0)
    return GFC_ERR_INVALID;
  if (p->n_layers < 0 || p->n_layers > GFC_SG_MAX_LAYERS || !sg_kenc_ok(p) || !p->final_proj_w || !p->final_proj_b)
    return GFC_ERR_INVALID;
  if ((p->use_scores != 0) != (scores0 != nullptr) || (scores0 != nullptr) != (scores1 != nullptr))
    return GFC_ERR_INVALID;
  for (int l = 0; l < p->n_layers; ++l)
    if (!p->wqkv[l] || !p->bqkv[l] || !p->merge_w[l] || !p->merge_b[l] || !p->mlp0_w[l] || !p->mlp0_b[l] ||
        !p->mlp_scale[l] || !p->mlp_shift[l] || !p->mlp1_w[l] || !p->mlp1_b[l])
      return GFC_ERR_INVALID;
  SgWs L;
  if (!sg_ws(B, M, N, L)) return GFC_ERR_INVALID;
  if (ws_bytes < L.total) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  const int D = 256, R0 = B * M, R1 = B * N, R = R0 + R1;
  float* x = (float*)(base + L.x);
  float* qkv = (float*)(base + L.qkv);
  float* ctx = (float*)(base + L.ctx);
  float* msg = (float*)(base + L.msg);
  int* self_p = (int*)(base + L.tables);
  int* cross_p = self_p + 8 * B;
  auto d2d = [&](void* dst, const void* src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess;
  };
  auto tap = [&](int slot) {  // desc_taps [4][R,256]: the rows after the encoder, layer 0, layer 1, the last layer
    return !desc_taps || d2d(desc_taps + (size_t)slot * R * D, x, (size_t)R * D * 4);
  };
  if (!d2d(x, desc0, (size_t)R0 * D * 4) || !d2d(x + (size_t)R0 * D, desc1, (size_t)R1 * D * 4)) return GFC_ERR_LAUNCH;
  hipLaunchKernelGGL(sg_tables_kernel, dim3((B + 63) / 64), dim3(64), 0, st, B, M, N, self_p, cross_p);
  GFC_LAUNCH_CHECK();
  // desc + kenc(normalised key points, scores) (superglue.py:281-290); the hidden rows live in the qkv slot
  GFC_TRY(gfc_sg_keypoint_encoder(p, kpts0, scores0, size0, B, M, x, qkv, kenc_ws(R0).total, st));
  GFC_TRY(gfc_sg_keypoint_encoder(p, kpts1, scores1, size1, B, N, x + (size_t)R0 * D, qkv, kenc_ws(R1).total, st));
  if (!tap(0)) return GFC_ERR_LAUNCH;
  const int maxn = M > N ? M : N;
  for (int l = 0; l < p->n_layers; ++l) {  // AttentionalPropagation (superglue.py:130-149,175-185)
    GFC_TRY(gfc_linear(x, D, D, nullptr, 0, 0, p->wqkv[l], D, p->bqkv[l], nullptr, nullptr, 1.f, nullptr, nullptr,
                       nullptr, 0, qkv, 768, R, 768, st));
    GFC_TRY(gfc_attention(qkv, 768, qkv + 256, 768, qkv + 512, 768, ctx, D, p->cross[l] ? cross_p : self_p, 2 * B, maxn,
                          4, 0.125f, base + L.att, L.att_bytes, st));
    GFC_TRY(gfc_linear(ctx, D, D, nullptr, 0, 0, p->merge_w[l], D, p->merge_b[l], nullptr, nullptr, 1.f, nullptr,
                       nullptr, nullptr, 0, msg, D, R, D, st));
    GFC_TRY(gfc_sg_mlp(x, D, msg, D, p->mlp0_w[l], p->mlp0_b[l], p->mlp_scale[l], p->mlp_shift[l], p->mlp1_w[l],
                       p->mlp1_b[l], x, x, D, R, st));
    if (l < 2 && !tap(1 + l)) return GFC_ERR_LAUNCH;
  }
  if (!tap(3)) return GFC_ERR_LAUNCH;
  // final_proj on both sides, each scaled by 256^(-1/4) = 1/4: their product is scores / sqrt(256), exactly
  float* md = qkv;
  GFC_TRY(gfc_linear(x, D, D, nullptr, 0, 0, p->final_proj_w, D, p->final_proj_b, nullptr, nullptr, 0.25f, nullptr,
                     nullptr, nullptr, 0, md, D, R, D, st));
  GFC_TRY(gfc_batched_nt(md, D, (long long)M * D, md + (size_t)R0 * D, D, (long long)N * D, sinkhorn_cost, N,
                         (long long)M * N, M, N, D, B, st));
  GFC_TRY(gfc_sg_sinkhorn(sinkhorn_cost, p->bin_score, B, M, N, iters, log_assignment, base + L.sink, L.sink_bytes, st));
  return gfc_lg_filter_matches(log_assignment, B, M, N, threshold, m0, m1, ms0, ms1, base + L.filt, L.filt_bytes, st);
}
