// What the backward units share (lg_head_backward.hip, lg_ffn_backward.hip, lg_cross_attn_backward.hip): the strided
// split-K GEMM on v_mfma_f32_32x32x2_f32, the split of a row count into parts, the column sums per chunk of rows with
// their finishing launch, and the finishing launch of the split-K parts.  Nothing here is accumulated by atomics and no sum depends on the order in which workgroups run.
#pragma once
#include "common.h"

#define HB_D 256          // descriptor_dim
#define HB_TM 128         // output tile of a GEMM workgroup: 4 waves of 64x64
#define HB_TN 128
#define HB_TK 16          // k per LDS tile
#define HB_LD (HB_TM + 2) // LDS row stride: the 16 k x 2 m that a 32-lane half stores from a k-fast operand hit 32 banks
#define HB_KSPLIT 1024    // rows per split-K part of a weight gradient (at most HB_MAX_PARTS parts)
#define HB_MAX_PARTS 128
#define HB_CS_ROWS 128    // rows per column-sum chunk
#define HB_CS_STRIDE 520  // floats of one chunk's record: 256 sums of dmd | 256 sums of v x | the sum of v
#define HB_MAX_ROWS 8388607  // B (M + N): row * 256 stays inside an int, as the forward's planner asks

#define HB_TRY(expr)                 \
  do {                               \
    const int hb_status = (expr);    \
    if (hb_status != GFC_OK) return hb_status; \
  } while (0)

struct HbSplit { int parts, kchunk; };
static inline HbSplit hb_split(int rows) {
  int parts = (rows + HB_KSPLIT - 1) / HB_KSPLIT;
  if (parts > HB_MAX_PARTS) parts = HB_MAX_PARTS;
  int kchunk = (rows + parts - 1) / parts;
  kchunk = (kchunk + HB_TK - 1) / HB_TK * HB_TK;
  return {(rows + kchunk - 1) / kchunk, kchunk};
}
static inline int hb_chunks(size_t rows) { return (int)((rows + HB_CS_ROWS - 1) / HB_CS_ROWS); }

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

// One chunk of HB_CS_ROWS rows, a thread per column: sums of dmd[row, :] (dmd nullable), and, with v (nullable, then
// x0 and x1 are not read), of v[row] x[row, :] and of v
static __global__ __launch_bounds__(256) void hb_colsum_kernel(const float* __restrict__ dmd, const float* __restrict__ v,
                                                        const float* __restrict__ x0, const float* __restrict__ x1,
                                                        size_t R0, size_t R, float* __restrict__ part) {
  const int t = threadIdx.x;
  const size_t r_begin = (size_t)blockIdx.x * HB_CS_ROWS, r_end = min(R, r_begin + HB_CS_ROWS);
  float sd = 0.f, sx = 0.f, sv = 0.f;
  for (size_t row = r_begin; row < r_end; ++row) {
    if (dmd) sd += dmd[row * HB_D + t];
    if (v) {
      const float vr = v[row];
      const float* x = row < R0 ? x0 + row * HB_D : x1 + (row - R0) * HB_D;
      sx += vr * x[t];
      sv += vr;
    }
  }
  float* out = part + (size_t)blockIdx.x * HB_CS_STRIDE;
  out[t] = sd;
  out[HB_D + t] = sx;
  if (t == 0) out[2 * HB_D] = sv;
}

// chunks added in ascending order, in fp64, rounded once: o_d[256] = scale * sums of dmd, o_w[256], o_b[1]; each
// output nullable
static __global__ __launch_bounds__(256) void hb_colsum_finish_kernel(const float* __restrict__ part, int chunks, float scale,
                                                               float* __restrict__ o_d, float* __restrict__ o_w,
                                                               float* __restrict__ o_b) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e > 2 * HB_D) return;
  if (e < HB_D ? !o_d : e < 2 * HB_D ? !o_w : !o_b) return;
  double s = 0.0;
#pragma unroll 8  // eight loads in flight; the additions stay in ascending order
  for (int c = 0; c < chunks; ++c) s += (double)part[(size_t)c * HB_CS_STRIDE + e];
  if (e < HB_D) o_d[e] = (float)((double)scale * s);
  else if (e < 2 * HB_D) o_w[e - HB_D] = (float)s;
  else o_b[0] = (float)s;
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

// out[e] = the sum over `n` records of `stride` floats of rec[e], in ascending order, in fp64, rounded once
static __global__ __launch_bounds__(256) void hb_finish_kernel(const float* __restrict__ rec, int n, size_t stride, int count,
                                                        float* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  double s = 0.0;
#pragma unroll 8  // eight loads in flight; the additions stay in ascending order
  for (int p = 0; p < n; ++p) s += (double)rec[(size_t)p * stride + e];
  out[e] = (float)s;
}

static int hb_finish(const float* rec, int n, size_t stride, int count, float* out, hipStream_t st) {
  hipLaunchKernelGGL(hb_finish_kernel, dim3((count + 255) / 256), dim3(256), 0, st, rec, n, stride, count, out);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
