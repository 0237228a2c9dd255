// Gradients of the deep-supervision loss with respect to one layer's assignment head and exit token, and the direct
// gradient at that layer's descriptors, for a batch of equal-sized pairs.  The closed form, the label rules and the
// reference lines are stated in include/gfc_amd_head_backward.h.
//
// The head of one layer, in launch order:
//   md = s (x Wf^T + bf), z = x.wm + bm, S = md0 md1^T   the forward's own entry points (gfc_linear, gfc_lg_rowdot,
//                                                        gfc_batched_nt): S is evaluated ONCE and stored [B,M,N]
//   row / column log-sum-exp of S, label counts r_i, c_j, the pair's a = g lambda / P and c = g (1 - lambda) / Q
//   G (in place over S) and dz
//   dmd0 = G md1, dmd1 = G^T md0, dWf parts = dmd^T x (split over rows), dx = s dmd Wf + dz (x) wm:
//                                                        hb_gemm_kernel, v_mfma_f32_32x32x2_f32, exact fp32
//   column sums (dbf, dwm, dbm) per chunk of rows, then the finishing launches add the chunks and the split-K parts in
//   ascending order.
// Nothing is accumulated by atomics and no sum depends on the order in which workgroups run.
#include <climits>

#include "lg_backward_common.h"  // the split-K GEMM, hb_split, the column sums
#include "../../include/gfc_amd_head_backward.h"

#define HB_S 0.25f        // d^-1/4

// ---- workspace: one description, used by the *_workspace_bytes exports and by the launchers --------------------------
static inline bool hb_sizes_ok(int B, int M, int N) {
  return B >= 1 && M >= 1 && N >= 1 && B <= 65535 && M <= 65535 && N <= 65535 &&
         (size_t)B * ((size_t)M + N) <= HB_MAX_ROWS;
}
struct HbLayout { size_t md, z, sim, rlse, clse, rcnt, ccnt, coef, dz, dmd, wpart, cpart, total; };
static inline HbLayout hb_layout(int B, int M, int N) {
  const size_t R = (size_t)B * ((size_t)M + N), f = sizeof(float);
  const int parts = hb_split(B * M).parts + hb_split(B * N).parts;
  gfc_slots s;
  return {s.take(R * HB_D * f), s.take(R * f), s.take((size_t)B * M * N * f), s.take((size_t)B * M * f),
          s.take((size_t)B * N * f), s.take((size_t)B * M * f), s.take((size_t)B * N * f), s.take((size_t)B * 2 * f),
          s.take(R * f), s.take(R * HB_D * f), s.take((size_t)parts * HB_D * HB_D * f),
          s.take((size_t)hb_chunks(R) * HB_CS_STRIDE * f), s.off};
}
struct HbTokenLayout { size_t dl, cpart, total; };
static inline HbTokenLayout hb_token_layout(int B, int M, int N) {
  const size_t R = (size_t)B * ((size_t)M + N);
  gfc_slots s;
  return {s.take(R * sizeof(float)), s.take((size_t)hb_chunks(R) * HB_CS_STRIDE * sizeof(float)), s.off};
}

// sigmoid(z) and sigmoid(-z) from one exp of a non-positive argument: z = +-1e4 gives exactly 1 and 0
__device__ __forceinline__ void hb_sigmoids(float z, float& sp, float& sn) {
  const float e = expf(-fabsf(z));
  const float big = 1.f / (1.f + e), small = e / (1.f + e);
  sp = z >= 0.f ? big : small;
  sn = z >= 0.f ? small : big;
}

// ---- log-sum-exp of S along rows (a wave per row) and down columns (32 columns x 8 row groups) ---------------------
__global__ __launch_bounds__(256) void hb_lse_rows_kernel(const float* __restrict__ S, int M, int N,
                                                          float* __restrict__ rlse) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;
  const float* p = S + ((size_t)b * M + i) * N;
  float m = -INFINITY;
  for (int j = lane; j < N; j += 64) m = fmaxf(m, p[j]);
  m = wave_max(m);
  float s = 0.f;
  for (int j = lane; j < N; j += 64) s += expf(p[j] - m);
  s = wave_sum(s);
  if (lane == 0) rlse[(size_t)b * M + i] = m + logf(s);
}

__global__ __launch_bounds__(256) void hb_lse_cols_kernel(const float* __restrict__ S, int M, int N,
                                                          float* __restrict__ clse) {
  __shared__ float sm[8][32], ss[8][32];
  const int cx = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int j = blockIdx.x * 32 + cx, b = blockIdx.y;
  const float* p = S + (size_t)b * M * N;
  float m = -INFINITY, s = 0.f;
  if (j < N)
    for (int i = rg; i < M; i += 8) {
      const float v = p[(size_t)i * N + j];
      if (v > m) { s = s * expf(m - v) + 1.f; m = v; } else { s += expf(v - m); }
    }
  sm[rg][cx] = m;
  ss[rg][cx] = s;
  __syncthreads();
  if (rg == 0 && j < N) {
    float mm = -INFINITY;
    for (int q = 0; q < 8; ++q) mm = fmaxf(mm, sm[q][cx]);
    float t = 0.f;
    for (int q = 0; q < 8; ++q) t += (ss[q][cx] > 0.f) ? ss[q][cx] * expf(sm[q][cx] - mm) : 0.f;
    clse[(size_t)b * N + j] = mm + logf(t);
  }
}

// ---- labels: r_i = sum_j W_ij (a wave per row), c_j = sum_i W_ij (a thread per column), the pair's a and c ---------
__global__ __launch_bounds__(256) void hb_label_rows_kernel(const long long* __restrict__ gt0,
                                                            const unsigned char* __restrict__ gta, int M, int N,
                                                            float* __restrict__ rcnt) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;
  int r = 0;
  if (gta) {
    const unsigned char* p = gta + ((size_t)b * M + i) * N;
    for (int j = lane; j < N; j += 64) r += p[j] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o, 64);
  } else {
    const long long t = gt0[(size_t)b * M + i];
    r = t > -1 && t < N;
  }
  if (lane == 0) rcnt[(size_t)b * M + i] = (float)r;
}

__global__ __launch_bounds__(256) void hb_label_cols_kernel(const long long* __restrict__ gt0,
                                                            const unsigned char* __restrict__ gta, int M, int N,
                                                            float* __restrict__ ccnt) {
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= N) return;
  int c = 0;
  if (gta) {
    const unsigned char* p = gta + (size_t)b * M * N + j;
    for (int i = 0; i < M; ++i) c += p[(size_t)i * N] != 0;
  } else {
    const long long* t = gt0 + (size_t)b * M;
    for (int i = 0; i < M; ++i) c += t[i] == (long long)j;
  }
  ccnt[(size_t)b * N + j] = (float)c;
}

// coef[b] = { a = g lambda / max(sum W, 1), c = g (1 - lambda) / (max(#n0, 1) + max(#n1, 1)) }; counts are integers
__global__ __launch_bounds__(256) void hb_coef_kernel(const float* __restrict__ rcnt, const long long* __restrict__ gt0,
                                                      const long long* __restrict__ gt1, const float* __restrict__ g,
                                                      float lambda, int M, int N, float* __restrict__ coef) {
  __shared__ long long red[3][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  long long s[3] = {0, 0, 0};
  for (int i = tid; i < M; i += 256) {
    s[0] += (long long)rcnt[(size_t)b * M + i];
    s[1] += gt0[(size_t)b * M + i] == -1;
  }
  for (int j = tid; j < N; j += 256) s[2] += gt1[(size_t)b * N + j] == -1;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    long long v = s[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((tid & 63) == 0) red[q][tid >> 6] = v;
  }
  __syncthreads();
  if (tid == 0) {
    long long t[3];
    for (int q = 0; q < 3; ++q) t[q] = red[q][0] + red[q][1] + red[q][2] + red[q][3];
    const double P = (double)(t[0] > 1 ? t[0] : 1);
    const double Q = (double)(t[1] > 1 ? t[1] : 1) + (double)(t[2] > 1 ? t[2] : 1);
    coef[2 * b] = (float)((double)g[b] * (double)lambda / P);
    coef[2 * b + 1] = (float)((double)g[b] * (1.0 - (double)lambda) / Q);
  }
}

// G_ij = a (r_i exp(S_ij - lse_row_i) + c_j exp(S_ij - lse_col_j) - 2 W_ij), in place over S; exp of arguments <= 0
__global__ __launch_bounds__(256) void hb_g_kernel(float* __restrict__ S, const float* __restrict__ rlse,
                                                   const float* __restrict__ clse, const float* __restrict__ rcnt,
                                                   const float* __restrict__ ccnt, const float* __restrict__ coef,
                                                   const long long* __restrict__ gt0,
                                                   const unsigned char* __restrict__ gta, int M, int N) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
  if (j >= N) return;
  const size_t row = (size_t)b * M + i, e = row * N + j;
  const float v = S[e], a = coef[2 * b];
  const float pr = expf(fminf(v - rlse[row], 0.f)), pc = expf(fminf(v - clse[(size_t)b * N + j], 0.f));
  const float w = gta ? (float)(gta[e] != 0) : (float)(gt0[row] == (long long)j);
  S[e] = a * ((rcnt[row] * pr + ccnt[(size_t)b * N + j] * pc) - 2.f * w);
}

// dz0_i = -a r_i sigmoid(-z0_i) + c n0_i sigmoid(z0_i), dz1_j with c_j and n1_j; rows of side 0 first
__global__ __launch_bounds__(256) void hb_dz_kernel(const float* __restrict__ z, const float* __restrict__ rcnt,
                                                    const float* __restrict__ ccnt, const float* __restrict__ coef,
                                                    const long long* __restrict__ gt0, const long long* __restrict__ gt1,
                                                    int B, int M, int N, float* __restrict__ dz) {
  const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x, R0 = (size_t)B * M, R = R0 + (size_t)B * N;
  if (row >= R) return;
  const bool side1 = row >= R0;
  const size_t k = side1 ? row - R0 : row;
  const int b = (int)(k / (side1 ? N : M));
  const float cnt = side1 ? ccnt[k] : rcnt[k];
  const float neg = (float)((side1 ? gt1[k] : gt0[k]) == -1);
  float sp, sn;
  hb_sigmoids(z[row], sp, sn);
  dz[row] = coef[2 * b + 1] * neg * sp - coef[2 * b] * cnt * sn;
}

// dlogit of the exit token: g (sigmoid(logit) - correct) / (2 points (L - 1))
__global__ __launch_bounds__(256) void hb_token_dl_kernel(const float* __restrict__ logit0,
                                                          const float* __restrict__ logit1,
                                                          const unsigned char* __restrict__ correct0,
                                                          const unsigned char* __restrict__ correct1,
                                                          const float* __restrict__ g, int B, int M, int N, float inv0,
                                                          float inv1, float* __restrict__ dl) {
  const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x, R0 = (size_t)B * M, R = R0 + (size_t)B * N;
  if (row >= R) return;
  const bool side1 = row >= R0;
  const size_t k = side1 ? row - R0 : row;
  const int b = (int)(k / (side1 ? N : M));
  float sp, sn;
  hb_sigmoids(side1 ? logit1[k] : logit0[k], sp, sn);
  const float y = (float)((side1 ? correct1[k] : correct0[k]) != 0);
  dl[row] = g[b] * ((sp - y) * (side1 ? inv1 : inv0));
}

// dWf = s * (the split-K parts in ascending order), in fp64, rounded once
__global__ __launch_bounds__(256) void hb_wf_finish_kernel(const float* __restrict__ part, int parts,
                                                           float* __restrict__ dWf) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  double s = 0.0;
  for (int p = 0; p < parts; ++p) s += (double)part[(size_t)p * HB_D * HB_D + e];
  dWf[e] = (float)((double)HB_S * s);
}

extern "C" size_t gfc_lg_head_backward_workspace_bytes(int B, int M, int N) {
  return hb_sizes_ok(B, M, N) ? hb_layout(B, M, N).total : 0;
}

extern "C" int gfc_lg_head_backward(const gfc_lg_params* p, int layer, const float* x0, const float* x1,
                                    const int64_t* gt_matches0, const int64_t* gt_matches1, const uint8_t* gt_assignment,
                                    const float* g, float nll_balancing, int B, int M, int N, float* dWf, float* dbf,
                                    float* dwm, float* dbm, float* dx, void* ws, size_t ws_bytes, void* stream) {
  if (!hb_sizes_ok(B, M, N)) return GFC_ERR_INVALID;
  if (!p || !x0 || !x1 || !gt_matches0 || !gt_matches1 || !g || !dWf || !dbf || !dwm || !dbm) return GFC_ERR_INVALID;
  if (layer < 0 || layer >= p->n_layers || layer >= GFC_LG_MAX_LAYERS || p->precision != GFC_LG_FP32)
    return GFC_ERR_INVALID;
  const float* Wf = p->final_proj_w[layer];
  const float* bf = p->final_proj_b[layer];
  const float* wm = p->matchability_w[layer];
  const float* bm = p->matchability_b[layer];
  if (!Wf || !bf || !wm || !bm) return GFC_ERR_INVALID;
  const HbLayout L = hb_layout(B, M, N);
  if (!ws || ws_bytes < L.total || ((uintptr_t)ws & 15)) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  const int R0 = B * M, R1 = B * N, R = R0 + R1;
  float* md = (float*)(base + L.md);
  float* z = (float*)(base + L.z);
  float* S = (float*)(base + L.sim);
  float* rlse = (float*)(base + L.rlse);
  float* clse = (float*)(base + L.clse);
  float* rcnt = (float*)(base + L.rcnt);
  float* ccnt = (float*)(base + L.ccnt);
  float* coef = (float*)(base + L.coef);
  float* dz = (float*)(base + L.dz);
  float* dmd = (float*)(base + L.dmd);
  float* wpart = (float*)(base + L.wpart);
  float* cpart = (float*)(base + L.cpart);
  float* md1 = md + (size_t)R0 * HB_D;
  float* dmd1 = dmd + (size_t)R0 * HB_D;
  const long long* gt0 = (const long long*)gt_matches0;
  const long long* gt1 = (const long long*)gt_matches1;

  // the head's forward, with the forward's entry points
  HB_TRY(gfc_linear(x0, HB_D, HB_D, nullptr, 0, 0, Wf, HB_D, bf, nullptr, nullptr, HB_S, nullptr, nullptr, nullptr, 0, md,
                    HB_D, R0, HB_D, stream));
  HB_TRY(gfc_linear(x1, HB_D, HB_D, nullptr, 0, 0, Wf, HB_D, bf, nullptr, nullptr, HB_S, nullptr, nullptr, nullptr, 0, md1,
                    HB_D, R1, HB_D, stream));
  HB_TRY(gfc_lg_rowdot(x0, HB_D, R0, wm, bm, 0, z, stream));
  HB_TRY(gfc_lg_rowdot(x1, HB_D, R1, wm, bm, 0, z + R0, stream));
  HB_TRY(gfc_batched_nt(md, HB_D, (long long)M * HB_D, md1, HB_D, (long long)N * HB_D, S, N, (long long)M * N, M, N,
                        HB_D, B, stream));
  hipLaunchKernelGGL(hb_lse_rows_kernel, dim3((M + 3) / 4, B), dim3(256), 0, st, S, M, N, rlse);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(hb_lse_cols_kernel, dim3((N + 31) / 32, B), dim3(256), 0, st, S, M, N, clse);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(hb_label_rows_kernel, dim3((M + 3) / 4, B), dim3(256), 0, st, gt0, gt_assignment, M, N, rcnt);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(hb_label_cols_kernel, dim3((N + 255) / 256, B), dim3(256), 0, st, gt0, gt_assignment, M, N, ccnt);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(hb_coef_kernel, dim3(B), dim3(256), 0, st, rcnt, gt0, gt1, g, nll_balancing, M, N, coef);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(hb_g_kernel, dim3((N + 255) / 256, M, B), dim3(256), 0, st, S, rlse, clse, rcnt, ccnt, coef, gt0,
                     gt_assignment, M, N);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(hb_dz_kernel, dim3((R + 255) / 256), dim3(256), 0, st, z, rcnt, ccnt, coef, gt0, gt1, B, M, N, dz);
  GFC_LAUNCH_CHECK();

  // dmd0 = G md1 and dmd1 = G^T md0, a pair per grid z
  HbGemm q{};
  q.alpha = 1.f;
  q.A = S; q.a_m = N; q.a_k = 1; q.a_z = (long long)M * N;
  q.B = md1; q.b_k = HB_D; q.b_z = (long long)N * HB_D;
  q.C = dmd; q.c_m = HB_D; q.c_z = (long long)M * HB_D; q.c_p = 0;
  q.M = M; q.N = HB_D; q.K = N; q.kchunk = N;
  HB_TRY(hb_gemm(q, true, 1, B, st));
  q.a_m = 1; q.a_k = N;
  q.B = md; q.b_z = (long long)M * HB_D;
  q.C = dmd1; q.c_z = (long long)N * HB_D;
  q.M = N; q.K = M; q.kchunk = M;
  HB_TRY(hb_gemm(q, false, 1, B, st));

  // dWf parts: dmd^T x over the rows of each side, split over rows
  const HbSplit s0 = hb_split(R0), s1 = hb_split(R1);
  HbGemm w{};
  w.alpha = 1.f;
  w.a_m = 1; w.a_k = HB_D; w.a_z = 0;
  w.b_k = HB_D; w.b_z = 0;
  w.c_m = HB_D; w.c_z = 0; w.c_p = (long long)HB_D * HB_D;
  w.M = HB_D; w.N = HB_D;
  w.A = dmd; w.B = x0; w.C = wpart; w.K = R0; w.kchunk = s0.kchunk;
  HB_TRY(hb_gemm(w, false, s0.parts, 1, st));
  w.A = dmd1; w.B = x1; w.C = wpart + (size_t)s0.parts * HB_D * HB_D; w.K = R1; w.kchunk = s1.kchunk;
  HB_TRY(hb_gemm(w, false, s1.parts, 1, st));
  hipLaunchKernelGGL(hb_wf_finish_kernel, dim3(HB_D * HB_D / 256), dim3(256), 0, st, wpart, s0.parts + s1.parts, dWf);
  GFC_LAUNCH_CHECK();

  HB_TRY(hb_colsums(dmd, dz, x0, x1, (size_t)R0, (size_t)R, cpart, HB_S, dbf, dwm, dbm, st));

  if (dx) {  // dx = s dmd Wf + dz (x) wm, all rows of both sides at once
    HbGemm d{};
    d.alpha = HB_S;
    d.A = dmd; d.a_m = HB_D; d.a_k = 1; d.a_z = 0;
    d.B = Wf; d.b_k = HB_D; d.b_z = 0;
    d.C = dx; d.c_m = HB_D; d.c_z = 0; d.c_p = 0;
    d.M = R; d.N = HB_D; d.K = HB_D; d.kchunk = HB_D;
    d.rv = dz; d.cv = wm;
    HB_TRY(hb_gemm(d, true, 1, 1, st));
  }
  return GFC_OK;
}

extern "C" size_t gfc_lg_token_backward_workspace_bytes(int B, int M, int N) {
  return hb_sizes_ok(B, M, N) ? hb_token_layout(B, M, N).total : 0;
}

extern "C" int gfc_lg_token_backward(const float* x0, const float* x1, const float* logit0, const float* logit1,
                                     const uint8_t* correct0, const uint8_t* correct1, const float* g, int n_layers,
                                     int B, int M, int N, float* dtoken_w, float* dtoken_b, void* ws, size_t ws_bytes,
                                     void* stream) {
  if (!hb_sizes_ok(B, M, N) || n_layers < 2) return GFC_ERR_INVALID;
  if (!x0 || !x1 || !logit0 || !logit1 || !correct0 || !correct1 || !g || !dtoken_w || !dtoken_b)
    return GFC_ERR_INVALID;
  const HbTokenLayout L = hb_token_layout(B, M, N);
  if (!ws || ws_bytes < L.total || ((uintptr_t)ws & 15)) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* dl = (float*)((char*)ws + L.dl);
  float* cpart = (float*)((char*)ws + L.cpart);
  const size_t R0 = (size_t)B * M, R = R0 + (size_t)B * N;
  const float inv0 = (float)(1.0 / (2.0 * M * (n_layers - 1))), inv1 = (float)(1.0 / (2.0 * N * (n_layers - 1)));
  hipLaunchKernelGGL(hb_token_dl_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, logit0, logit1, correct0,
                     correct1, g, B, M, N, inv0, inv1, dl);
  GFC_LAUNCH_CHECK();
  return hb_colsums(nullptr, dl, x0, x1, R0, R, cpart, 1.f, nullptr, dtoken_w, dtoken_b, st);
}
