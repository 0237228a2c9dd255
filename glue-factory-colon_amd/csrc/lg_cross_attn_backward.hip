// The backward of LightGlue's bidirectional cross attention on packed rows, and of the cross block's to_qk / to_v
// around it.  The closed form, the workspace and the refusals are stated in include/gfc_amd_cross_attn_backward.h.
//
// gfc_attention_cross_backward, in launch order:
//   D = dctx . ctx per row and 64-wide head segment                        ca_rowdot_kernel, a wave per row
//   lse = log sum exp(scale q_a q_b^T) over the other side                 ca_lse_kernel
//   dq_a, dv_a                                                             ca_backward_kernel
// One kernel serves both directions as two problems per pair: (own side a, other side b) = (0, 1) and (1, 0).  A
// workgroup owns CA_BR rows of a for one head, a wave 32 of them, and streams b in tiles of CA_BK keys through LDS, in
// ascending order.  Every output row has one owner: no atomics, no sum depends on the order in which workgroups run.
//
// Plan edges (tests/test_gpu_cross_attn_backward.py lists a shape at each): 32 rows per wave, CA_BR = 128 rows per
// workgroup, CA_BK = 32 keys per tile.  The keys are not split over workgroups.
#include "lg_backward_common.h"
#include "../../include/gfc_amd_cross_attn_backward.h"

#define CA_HD 64     // head dim
#define CA_HEADS 4   // HB_D / CA_HD
#define CA_BR 128    // own rows per workgroup: 4 waves of 32
#define CA_BK 32     // keys per tile
#define CA_LDT 65    // LDS row stride of a [CA_BK][64] tile: a column read by 32 lanes hits 32 banks
#define CA_LDP 33    // LDS row stride of a wave's [32][CA_BK] tile

struct CaArgs {
  const float *qk, *v, *ctx, *dctx;
  long long ld_qk, ld_v, ld_ctx, ld_dctx, ld_dqk, ld_dv;
  float *dqk, *dv;
  float *lse, *dd;  // [rows][CA_HEADS]
  int B, M, N, blocks0, blocks1;
  float scale;
};

// workgroup id -> (pair, head, side, row block): first packed row of the own and of the other side, their counts
struct CaWork { long long own0, oth0; int na, nb, head, row0; };
__device__ __forceinline__ CaWork ca_work(const CaArgs& a, unsigned id) {
  const unsigned blocks = a.blocks0 + a.blocks1, per_pair = CA_HEADS * blocks;
  const unsigned pair = id / per_pair, rem = id % per_pair, blk = rem % blocks;
  const long long s0 = (long long)pair * a.M, s1 = (long long)a.B * a.M + (long long)pair * a.N;
  CaWork w;
  w.head = (int)(rem / blocks);
  if (blk < (unsigned)a.blocks0) {
    w.own0 = s0; w.oth0 = s1; w.na = a.M; w.nb = a.N; w.row0 = (int)blk * CA_BR;
  } else {
    w.own0 = s1; w.oth0 = s0; w.na = a.N; w.nb = a.M; w.row0 = (int)(blk - a.blocks0) * CA_BR;
  }
  return w;
}

// rows [0, valid) of a [CA_BK][64] tile from src (row stride ld) into LDS, the others as zeros
__device__ __forceinline__ void ca_load_tile(float (*T)[CA_LDT], const float* __restrict__ src, long long ld, int valid,
                                             int tid) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int row = (tid >> 4) + 16 * q, c = (tid & 15) * 4;
    const float4 x = row < valid ? *reinterpret_cast<const float4*>(src + row * ld + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    T[row][c] = x.x; T[row][c + 1] = x.y; T[row][c + 2] = x.z; T[row][c + 3] = x.w;
  }
}

// the lane's MFMA operand of its own row: elements 2 kk + h of the 64 of `row` (zeros for a row outside the side)
__device__ __forceinline__ void ca_own_row(float (&r)[32], const float* __restrict__ row, bool valid, int h) {
#pragma unroll
  for (int kk = 0; kk < 32; ++kk) r[kk] = valid ? row[2 * kk + h] : 0.f;
}

// ---- D[row][head] = dctx[row, head] . ctx[row, head]: a wave per row, 16 lanes per head -----------------------------
__global__ __launch_bounds__(256) void ca_rowdot_kernel(const CaArgs a, size_t rows) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float4 c = *reinterpret_cast<const float4*>(a.ctx + row * a.ld_ctx + 4 * lane);
  const float4 g = *reinterpret_cast<const float4*>(a.dctx + row * a.ld_dctx + 4 * lane);
  float p = ((g.x * c.x + g.y * c.y) + g.z * c.z) + g.w * c.w;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) p += __shfl_xor(p, o);
  if ((lane & 15) == 0) a.dd[row * CA_HEADS + (lane >> 4)] = p;
}

// ---- lse[i] = log sum_j exp(scale q_a[i] . q_b[j]) ------------------------------------------------------------------
// The tile is formed transposed (keys on the accumulator's rows, the own row on the lane), so that a lane's 16 registers
// are 16 keys of ITS row: the running maximum and sum stay in the lane, one per half, and the halves meet once at the end.
__global__ __launch_bounds__(256) void ca_lse_kernel(const CaArgs a) {
  __shared__ float Qb[CA_BK][CA_LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
  const CaWork w = ca_work(a, blockIdx.x);
  const int i = w.row0 + wave * 32 + l31;
  const int col = w.head * CA_HD;
  float qa[32];
  ca_own_row(qa, a.qk + (w.own0 + i) * a.ld_qk + col, i < w.na, h);
  float m = -INFINITY, s = 0.f;
  for (int j0 = 0; j0 < w.nb; j0 += CA_BK) {
    __syncthreads();  // the previous tile has been read
    ca_load_tile(Qb, a.qk + (w.oth0 + j0) * a.ld_qk + col, a.ld_qk, w.nb - j0, tid);
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) acc = mfma32(Qb[l31][2 * kk + h], qa[kk], acc);
    float x[16], tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      x[r] = j0 + acc_row(r, h) < w.nb ? a.scale * acc[r] : -INFINITY;
      tmax = fmaxf(tmax, x[r]);
    }
    const float mn = fmaxf(m, tmax);
    if (mn > -INFINITY) {  // (half 1 of a side of fewer than five keys sees none)
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) t += expf(x[r] - mn);
      s = s * expf(m - mn) + t;
      m = mn;
    }
  }
  const float mo = __shfl_xor(m, 32), so = __shfl_xor(s, 32);
  const float m_lo = h ? mo : m, s_lo = h ? so : s, m_hi = h ? m : mo, s_hi = h ? s : so;  // half 0 holds key 0
  const float mm = fmaxf(m_lo, m_hi);
  const float ss = s_lo * expf(m_lo - mm) + s_hi * expf(m_hi - mm);
  if (h == 0 && i < w.na) a.lse[(w.own0 + i) * CA_HEADS + w.head] = mm + logf(ss);
}

// ---- dq_a and dv_a of CA_BR rows of one head ------------------------------------------------------------------------
// Per tile of CA_BK keys j and per wave (rows i on the accumulator's rows, the key on the lane):
//   S = q_a q_b^T, T1 = dctx_a v_b^T, T2 = v_a dctx_b^T                        3 x 32 MFMAs, b's operands from LDS
//   P1 = exp(min(scale S - lse_a[i], 0)), P2 = exp(min(scale S - lse_b[j], 0)), 0 for a key outside the side
//   dS = P1 (T1 - D_a[i]) + P2 (T2 - D_b[j])
//   dS and P2 cross LDS once (the next products sum over the key, which is the lane here)
//   dq += dS q_b, dv += P2 dctx_b                                               2 x 32 MFMAs
// and dq is scaled once at the end.
__global__ __launch_bounds__(256) void ca_backward_kernel(const CaArgs a) {
  __shared__ float Qb[CA_BK][CA_LDT];
  __shared__ float Vb[CA_BK][CA_LDT];
  __shared__ float Gb[CA_BK][CA_LDT];
  __shared__ float dSs[4][32][CA_LDP];
  __shared__ float Ps[4][32][CA_LDP];
  __shared__ float stat_a[CA_BR][2];  // lse | D of the own rows
  __shared__ float stat_b[CA_BK][2];  // of the tile's keys
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
  const CaWork w = ca_work(a, blockIdx.x);
  const int i = w.row0 + wave * 32 + l31;
  const int col = w.head * CA_HD;
  const bool own = i < w.na;
  float qa[32], va[32], ga[32];
  ca_own_row(qa, a.qk + (w.own0 + i) * a.ld_qk + col, own, h);
  ca_own_row(va, a.v + (w.own0 + i) * a.ld_v + col, own, h);
  ca_own_row(ga, a.dctx + (w.own0 + i) * a.ld_dctx + col, own, h);
  if (tid < CA_BR) {
    const bool in = w.row0 + tid < w.na;
    const long long e = (w.own0 + w.row0 + tid) * CA_HEADS + w.head;
    stat_a[tid][0] = in ? a.lse[e] : 0.f;
    stat_a[tid][1] = in ? a.dd[e] : 0.f;
  }
  f32x16 dq[2], dv[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[c][r] = dv[c][r] = 0.f;
  for (int j0 = 0; j0 < w.nb; j0 += CA_BK) {
    const int valid = w.nb - j0;
    __syncthreads();  // the previous tile has been read
    ca_load_tile(Qb, a.qk + (w.oth0 + j0) * a.ld_qk + col, a.ld_qk, valid, tid);
    ca_load_tile(Vb, a.v + (w.oth0 + j0) * a.ld_v + col, a.ld_v, valid, tid);
    ca_load_tile(Gb, a.dctx + (w.oth0 + j0) * a.ld_dctx + col, a.ld_dctx, valid, tid);
    if (tid < CA_BK) {
      const long long e = (w.oth0 + j0 + tid) * CA_HEADS + w.head;
      stat_b[tid][0] = tid < valid ? a.lse[e] : 0.f;
      stat_b[tid][1] = tid < valid ? a.dd[e] : 0.f;
    }
    __syncthreads();
    f32x16 S, T1, T2;
#pragma unroll
    for (int r = 0; r < 16; ++r) S[r] = T1[r] = T2[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
      const int k = 2 * kk + h;
      S = mfma32(qa[kk], Qb[l31][k], S);
      T1 = mfma32(ga[kk], Vb[l31][k], T1);
      T2 = mfma32(va[kk], Gb[l31][k], T2);
    }
    const bool key = l31 < valid;
    const float lse_b = stat_b[l31][0], d_b = stat_b[l31][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, h);
      const float s = a.scale * S[r];
      const float p1 = key ? expf(fminf(s - stat_a[wave * 32 + row][0], 0.f)) : 0.f;
      const float p2 = key ? expf(fminf(s - lse_b, 0.f)) : 0.f;
      dSs[wave][row][l31] = p1 * (T1[r] - stat_a[wave * 32 + row][1]) + p2 * (T2[r] - d_b);
      Ps[wave][row][l31] = p2;
    }
    __syncthreads();  // a wave reads back its own tiles only; the barrier orders its stores before its loads
#pragma unroll
    for (int kk = 0; kk < CA_BK / 2; ++kk) {
      const int j = 2 * kk + h;
      const float ds = dSs[wave][l31][j], p = Ps[wave][l31][j];
      dq[0] = mfma32(ds, Qb[j][l31], dq[0]);
      dq[1] = mfma32(ds, Qb[j][32 + l31], dq[1]);
      dv[0] = mfma32(p, Gb[j][l31], dv[0]);
      dv[1] = mfma32(p, Gb[j][32 + l31], dv[1]);
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = w.row0 + wave * 32 + acc_row(r, h);
      if (row >= w.na) continue;
      a.dqk[(w.own0 + row) * a.ld_dqk + col + 32 * c + l31] = a.scale * dq[c][r];
      a.dv[(w.own0 + row) * a.ld_dv + col + 32 * c + l31] = dv[c][r];
    }
}

// ---- workspace: one description, used by the *_workspace_bytes exports and by the launchers ---------------------------
static inline long long ca_rows(int B, int M, int N) {
  if (B < 1 || M < 1 || N < 1) return 0;
  const long long rows = (long long)B * ((long long)M + N);
  return rows <= HB_MAX_ROWS ? rows : 0;
}
struct CaLayout { size_t lse, dd, total; };
static inline CaLayout ca_layout(size_t rows) {
  gfc_slots s;
  return {s.take(rows * CA_HEADS * sizeof(float)), s.take(rows * CA_HEADS * sizeof(float)), s.off};
}
struct CbLayout { size_t qk, v, dqk, dv, t, wpart, cpart, core, total; };
static inline CbLayout cb_layout(size_t rows) {
  const size_t f = sizeof(float), rd = rows * HB_D * f;
  gfc_slots s;
  return {s.take(rd), s.take(rd), s.take(rd), s.take(rd), s.take(rd),
          s.take((size_t)hb_split((int)rows).parts * HB_D * HB_D * f), s.take((size_t)hb_chunks(rows) * HB_CS_STRIDE * f),
          s.take(ca_layout(rows).total), s.off};
}

static inline bool ca_ptr_ok(const void* p, int ld) { return p && !((uintptr_t)p & 15) && ld >= HB_D && !(ld & 3); }

extern "C" size_t gfc_attention_cross_backward_workspace_bytes(int B, int M, int N, int heads) {
  const long long rows = ca_rows(B, M, N);
  return rows && heads == CA_HEADS ? ca_layout((size_t)rows).total : 0;
}

extern "C" int gfc_attention_cross_backward(const float* qk, int ld_qk, const float* v, int ld_v, const float* ctx,
                                            int ld_ctx, const float* dctx, int ld_dctx, int B, int M, int N, int heads,
                                            float scale, float* dqk, int ld_dqk, float* dv, int ld_dv, void* ws,
                                            size_t ws_bytes, void* stream) {
  const long long rows = ca_rows(B, M, N);
  if (!rows || heads * CA_HD != HB_D) return GFC_ERR_INVALID;
  if (!ca_ptr_ok(qk, ld_qk) || !ca_ptr_ok(v, ld_v) || !ca_ptr_ok(ctx, ld_ctx) || !ca_ptr_ok(dctx, ld_dctx) ||
      !ca_ptr_ok(dqk, ld_dqk) || !ca_ptr_ok(dv, ld_dv))
    return GFC_ERR_INVALID;
  const CaLayout L = ca_layout((size_t)rows);
  if (!ws || ws_bytes < L.total || ((uintptr_t)ws & 15)) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CaArgs a{};
  a.qk = qk; a.v = v; a.ctx = ctx; a.dctx = dctx;
  a.ld_qk = ld_qk; a.ld_v = ld_v; a.ld_ctx = ld_ctx; a.ld_dctx = ld_dctx; a.ld_dqk = ld_dqk; a.ld_dv = ld_dv;
  a.dqk = dqk; a.dv = dv;
  a.lse = (float*)((char*)ws + L.lse);
  a.dd = (float*)((char*)ws + L.dd);
  a.B = B; a.M = M; a.N = N;
  a.blocks0 = (M + CA_BR - 1) / CA_BR;
  a.blocks1 = (N + CA_BR - 1) / CA_BR;
  a.scale = scale;
  // rows <= HB_MAX_ROWS: at most 4 (rows / 128 + 2 B) workgroups, inside an unsigned
  const unsigned grid = (unsigned)B * CA_HEADS * (unsigned)(a.blocks0 + a.blocks1);
  hipLaunchKernelGGL(ca_rowdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a, (size_t)rows);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(ca_lse_kernel, dim3(grid), dim3(256), 0, st, a);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(ca_backward_kernel, dim3(grid), dim3(256), 0, st, a);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

// dx = (dx_in +) t1 + t2, t1 already in dx
__global__ __launch_bounds__(256) void cb_sum_kernel(float* __restrict__ dx, const float* __restrict__ dx_in,
                                                     const float* __restrict__ t2, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float att = dx[i] + t2[i];
  dx[i] = dx_in ? dx_in[i] + att : att;
}

extern "C" size_t gfc_lg_cross_attn_backward_workspace_bytes(int B, int M, int N) {
  const long long rows = ca_rows(B, M, N);
  return rows ? cb_layout((size_t)rows).total : 0;
}

extern "C" int gfc_lg_cross_attn_backward(const float* x, const float* ctx, const float* dctx, const float* dx_in,
                                          const float* Wqk, const float* bqk, const float* Wv, const float* bv, int B,
                                          int M, int N, float* dWqk, float* dbqk, float* dWv, float* dbv, float* dx,
                                          void* ws, size_t ws_bytes, void* stream) {
  const long long rows = ca_rows(B, M, N);
  if (!rows) return GFC_ERR_INVALID;
  if (!ca_ptr_ok(x, HB_D) || !ca_ptr_ok(ctx, HB_D) || !ca_ptr_ok(dctx, HB_D) || !Wqk || !bqk || !Wv || !bv || !dWqk ||
      !dbqk || !dWv || !dbv || (dx_in && (!dx || dx == dx_in)) || (dx && ((uintptr_t)dx & 15)))
    return GFC_ERR_INVALID;
  const CbLayout L = cb_layout((size_t)rows);
  if (!ws || ws_bytes < L.total || ((uintptr_t)ws & 15)) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  float* qk = (float*)(base + L.qk);
  float* v = (float*)(base + L.v);
  float* dqk = (float*)(base + L.dqk);
  float* dv = (float*)(base + L.dv);
  float* t = (float*)(base + L.t);
  float* wpart = (float*)(base + L.wpart);
  float* cpart = (float*)(base + L.cpart);
  const int R = (int)rows;
  const HbSplit sp = hb_split(R);

  // the forward, with the forward's entry point
  HB_TRY(gfc_linear(x, HB_D, HB_D, nullptr, 0, 0, Wqk, HB_D, bqk, nullptr, nullptr, 1.f, nullptr, nullptr, nullptr, 0, qk,
                    HB_D, R, HB_D, stream));
  HB_TRY(gfc_linear(x, HB_D, HB_D, nullptr, 0, 0, Wv, HB_D, bv, nullptr, nullptr, 1.f, nullptr, nullptr, nullptr, 0, v,
                    HB_D, R, HB_D, stream));
  HB_TRY(gfc_attention_cross_backward(qk, HB_D, v, HB_D, ctx, HB_D, dctx, HB_D, B, M, N, CA_HEADS, 0.125f, dqk, HB_D, dv,
                                      HB_D, base + L.core, ca_layout((size_t)rows).total, stream));

  // dWqk = dqk^T x, dWv = dv^T x, split over rows; the parts buffer is used by one of them at a time
  HbGemm g{};
  g.alpha = 1.f;
  g.a_m = 1; g.a_k = HB_D; g.K = R; g.kchunk = sp.kchunk;
  g.B = x; g.b_k = HB_D; g.C = wpart; g.c_m = HB_D; g.c_p = (long long)HB_D * HB_D;
  g.M = HB_D; g.N = HB_D;
  g.A = dqk;
  HB_TRY(hb_gemm(g, false, sp.parts, 1, st));
  HB_TRY(hb_finish(wpart, sp.parts, (size_t)HB_D * HB_D, HB_D * HB_D, dWqk, st));
  HB_TRY(hb_colsums(dqk, nullptr, nullptr, nullptr, 0, (size_t)rows, cpart, 1.f, dbqk, nullptr, nullptr, st));
  g.A = dv;
  HB_TRY(hb_gemm(g, false, sp.parts, 1, st));
  HB_TRY(hb_finish(wpart, sp.parts, (size_t)HB_D * HB_D, HB_D * HB_D, dWv, st));
  HB_TRY(hb_colsums(dv, nullptr, nullptr, nullptr, 0, (size_t)rows, cpart, 1.f, dbv, nullptr, nullptr, st));

  if (dx) {
    // dx = (dx_in +) dqk Wqk + dv Wv
    HbGemm d{};
    d.alpha = 1.f;
    d.a_m = HB_D; d.a_k = 1; d.b_k = HB_D; d.c_m = HB_D;
    d.M = R; d.N = HB_D; d.K = HB_D; d.kchunk = HB_D;
    d.A = dqk; d.B = Wqk; d.C = dx;
    HB_TRY(hb_gemm(d, true, 1, 1, st));
    d.A = dv; d.B = Wv; d.C = t;
    HB_TRY(hb_gemm(d, true, 1, 1, st));
    const size_t n = (size_t)rows * HB_D;
    hipLaunchKernelGGL(cb_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dx, dx_in, t, n);
    GFC_LAUNCH_CHECK();
  }
  return GFC_OK;
}
