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

#include "common.h"
#include "../../include/gfc_amd_head_backward.h"

#define HB_D 256          // descriptor_dim
#define HB_S 0.25f        // d^-1/4
#define HB_TM 128         // output tile of a GEMM workgroup: 4 waves of 64x64
#define HB_TN 128
#define HB_TK 16          // k per LDS tile
#define HB_LD (HB_TM + 2) // LDS row stride: the 16 k x 2 m that a 32-lane half stores from a k-fast operand hit 32 banks
#define HB_KSPLIT 1024    // rows per split-K part of dWf (at most HB_MAX_PARTS parts per side)
#define HB_MAX_PARTS 128
#define HB_CS_ROWS 128    // rows per column-sum chunk
#define HB_CS_STRIDE 520  // floats of one chunk's record: 256 sums of dmd | 256 sums of v x | the sum of v
#define HB_MAX_ROWS 8388607  // B (M + N): row * 256 stays inside an int, as the forward's planner asks

#define HB_TRY(expr)                 \
  do {                               \
    const int hb_status = (expr);    \
    if (hb_status != GFC_OK) return hb_status; \
  } while (0)

// ---- workspace: one description, used by the *_workspace_bytes exports and by the launchers --------------------------
struct HbSplit { int parts, kchunk; };
static inline HbSplit hb_split(int rows) {
  int parts = (rows + HB_KSPLIT - 1) / HB_KSPLIT;
  if (parts > HB_MAX_PARTS) parts = HB_MAX_PARTS;
  int kchunk = (rows + parts - 1) / parts;
  kchunk = (kchunk + HB_TK - 1) / HB_TK * HB_TK;
  return {(rows + kchunk - 1) / kchunk, kchunk};
}
static inline int hb_chunks(size_t rows) { return (int)((rows + HB_CS_ROWS - 1) / HB_CS_ROWS); }
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

// ---- C[z][p] (M x N, n contiguous) = alpha * A_z[:, k in part p] B_z[k in part p, :] (+ rv[m] cv[n]) -----------------
// Element (m, k) of A at A[z a_z + m a_m + k a_k], one of a_m, a_k is 1 (A_KFAST: a_k); (k, n) of B at
// B[z b_z + k b_k + n].  K tiles through LDS as [k][m] / [k][n]; the next tile is read into registers while the current
// one is multiplied.  Rows, columns and k outside the problem are read as 0 and never stored.
struct HbGemm {
  const float* A; long long a_m, a_k, a_z;
  const float* B; long long b_k, b_z;
  float* C; long long c_m, c_z, c_p;
  int M, N, K, kchunk;
  float alpha;
  const float* rv; const float* cv;  // nullable pair; rv is indexed by z * M + m
};

template <bool A_KFAST>
__global__ __launch_bounds__(256) void hb_gemm_kernel(const HbGemm g) {
  __shared__ float As[HB_TK][HB_LD];
  __shared__ float Bs[HB_TK][HB_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
  const int tiles_n = (g.N + HB_TN - 1) / HB_TN;
  const int m0 = (int)(blockIdx.x / tiles_n) * HB_TM, n0 = (int)(blockIdx.x % tiles_n) * HB_TN;
  const int part = blockIdx.y, zb = blockIdx.z;
  const int k_begin = part * g.kchunk, k_end = min(g.K, k_begin + g.kchunk);
  const float* __restrict__ A = g.A + (long long)zb * g.a_z;
  const float* __restrict__ B = g.B + (long long)zb * g.b_z;
  // this thread's eight elements of each tile
  const int ak = A_KFAST ? (tid & 15) : (tid >> 7), am = A_KFAST ? (tid >> 4) : (tid & 127);
  const int bk = tid >> 7, bn = tid & 127;
  float ra[8], rb[8];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = k0 + (A_KFAST ? ak : ak + 2 * q), m = m0 + (A_KFAST ? am + 16 * q : am);
      ra[q] = (k < k_end && m < g.M) ? A[(long long)m * g.a_m + (long long)k * g.a_k] : 0.f;
      const int kb = k0 + bk + 2 * q, n = n0 + bn;
      rb[q] = (kb < k_end && n < g.N) ? B[(long long)kb * g.b_k + n] : 0.f;
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  if (k_begin < k_end) fetch(k_begin);
  for (int k0 = k_begin; k0 < k_end; k0 += HB_TK) {
    __syncthreads();  // the previous tile has been read
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (A_KFAST) As[ak][am + 16 * q] = ra[q]; else As[ak + 2 * q][am] = ra[q];
      Bs[bk + 2 * q][bn] = rb[q];
    }
    __syncthreads();
    if (k0 + HB_TK < k_end) fetch(k0 + HB_TK);
#pragma unroll
    for (int kk = 0; kk < HB_TK; kk += 2) {
      const float a0 = As[kk + h][wm + l31], a1 = As[kk + h][wm + 32 + l31];
      const float b0 = Bs[kk + h][wn + l31], b1 = Bs[kk + h][wn + 32 + l31];
      acc[0][0] = mfma32(a0, b0, acc[0][0]);
      acc[0][1] = mfma32(a0, b1, acc[0][1]);
      acc[1][0] = mfma32(a1, b0, acc[1][0]);
      acc[1][1] = mfma32(a1, b1, acc[1][1]);
    }
  }
  float* __restrict__ C = g.C + (long long)zb * g.c_z + (long long)part * g.c_p;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn + 32 * j + l31;
      if (n >= g.N) continue;
      const float cvn = g.cv ? g.cv[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + 32 * i + acc_row(r, h);
        if (m >= g.M) continue;
        float v = g.alpha * acc[i][j][r];
        if (g.rv) v += g.rv[(long long)zb * g.M + m] * cvn;
        C[(long long)m * g.c_m + n] = v;
      }
    }
}

static int hb_gemm(const HbGemm& g, bool a_kfast, int parts, int batch, hipStream_t st) {
  const dim3 grid(((g.M + HB_TM - 1) / HB_TM) * ((g.N + HB_TN - 1) / HB_TN), parts, batch);
  if (a_kfast) hipLaunchKernelGGL(hb_gemm_kernel<true>, grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL(hb_gemm_kernel<false>, grid, dim3(256), 0, st, g);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
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

// One chunk of HB_CS_ROWS rows, a thread per column: sums of dmd[row, :] (dmd nullable), of v[row] x[row, :] and of v
__global__ __launch_bounds__(256) void hb_colsum_kernel(const float* __restrict__ dmd, const float* __restrict__ v,
                                                        const float* __restrict__ x0, const float* __restrict__ x1,
                                                        size_t R0, size_t R, float* __restrict__ part) {
  const int t = threadIdx.x;
  const size_t r_begin = (size_t)blockIdx.x * HB_CS_ROWS, r_end = min(R, r_begin + HB_CS_ROWS);
  float sd = 0.f, sx = 0.f, sv = 0.f;
  for (size_t row = r_begin; row < r_end; ++row) {
    const float vr = v[row];
    const float* x = row < R0 ? x0 + row * HB_D : x1 + (row - R0) * HB_D;
    if (dmd) sd += dmd[row * HB_D + t];
    sx += vr * x[t];
    sv += vr;
  }
  float* out = part + (size_t)blockIdx.x * HB_CS_STRIDE;
  out[t] = sd;
  out[HB_D + t] = sx;
  if (t == 0) out[2 * HB_D] = sv;
}

// chunks added in ascending order, in fp64, rounded once: o_d[256] = scale * sums of dmd (nullable), o_w[256], o_b[1]
__global__ __launch_bounds__(256) void hb_colsum_finish_kernel(const float* __restrict__ part, int chunks, float scale,
                                                               float* __restrict__ o_d, float* __restrict__ o_w,
                                                               float* __restrict__ o_b) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e > 2 * HB_D) return;
  if (e < HB_D && !o_d) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += (double)part[(size_t)c * HB_CS_STRIDE + e];
  if (e < HB_D) o_d[e] = (float)((double)scale * s);
  else if (e < 2 * HB_D) o_w[e - HB_D] = (float)s;
  else o_b[0] = (float)s;
}

// dWf = s * (the split-K parts in ascending order), in fp64, rounded once
__global__ __launch_bounds__(256) void hb_wf_finish_kernel(const float* __restrict__ part, int parts,
                                                           float* __restrict__ dWf) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  double s = 0.0;
  for (int p = 0; p < parts; ++p) s += (double)part[(size_t)p * HB_D * HB_D + e];
  dWf[e] = (float)((double)HB_S * s);
}

static int hb_colsums(const float* dmd, const float* v, const float* x0, const float* x1, size_t R0, size_t R,
                      float* part, float scale, float* o_d, float* o_w, float* o_b, hipStream_t st) {
  const int chunks = hb_chunks(R);
  hipLaunchKernelGGL(hb_colsum_kernel, dim3(chunks), dim3(256), 0, st, dmd, v, x0, x1, R0, R, part);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(hb_colsum_finish_kernel, dim3(3), dim3(256), 0, st, part, chunks, scale, o_d, o_w, o_b);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
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
