// The backward of LightGlue's rotary self attention on packed rows, and of the self block's Wqkv around it.  The closed
// form, the workspace and the refusals are stated in include/gfc_amd_self_attn_backward.h.
//
// gfc_attention_self_backward, in launch order:
//   D = dctx . ctx per row and 64-wide head segment                        sa_rowdot_kernel, a wave per row
//   lse = log sum exp(scale q' k'^T) over the row's own side               sa_lse_kernel
//   dq                                                                     sa_dq_kernel   (the rows as queries)
//   dk, dv                                                                 sa_dkv_kernel  (the rows as keys)
// S_ij and S_ji are different matrices here (q' k'^T is not symmetric), so the two roles of a row share nothing but
// their inputs: they are two kernels, each lighter than the cross core (two own operands and two or four accumulator
// tiles instead of three and four with three score tiles).  In both a workgroup owns SA_BR rows of one side and head, a
// wave 32 of them, and streams the SAME side in tiles of SA_BK rows through LDS, in ascending order.  Every output row
// has one owner per role: no atomics, no sum depends on the order in which workgroups run.
//
// Plan edges (tests/test_gpu_self_attn_backward.py lists a shape at each): 32 rows per wave, SA_BR = 128 rows per
// workgroup, SA_BK = 32 streamed rows per tile; the second lane half of the log-sum-exp sees no key of a side of fewer
// than five rows.  The streamed rows are not split over workgroups.
//
// The helpers below repeat those of lg_cross_attn_backward.hip instead of sharing a header with it: that unit's outputs
// are pinned to their bits, and nothing here needs it rebuilt.
#include "lg_backward_common.h"
#include "../../include/gfc_amd_self_attn_backward.h"

#define SA_HD 64     // head dim
#define SA_HEADS 4   // HB_D / SA_HD
#define SA_QKV 768   // q' | k' | v, 256 columns each, head-major
#define SA_BR 128    // own rows per workgroup: 4 waves of 32
#define SA_BK 32     // streamed rows per tile
#define SA_LDT 65    // LDS row stride of a [SA_BK][64] tile: a column read by 32 lanes hits 32 banks
#define SA_LDP 33    // LDS row stride of a wave's [32][SA_BK] tile

struct SaArgs {
  const float *qkv, *ctx, *dctx, *cos, *sin;  // cos, sin [rows][64], NULL together
  long long ld_qkv, ld_ctx, ld_dctx, ld_dqkv;
  float* dqkv;
  float *lse, *dd;  // [rows][SA_HEADS]
  int B, M, N, blocks0, blocks1;
  float scale;
};

// workgroup id -> (pair, head, side, row block): first packed row of the side, its row count
struct SaWork { long long own0; int na, head, row0; };
__device__ __forceinline__ SaWork sa_work(const SaArgs& a, unsigned id) {
  const unsigned blocks = a.blocks0 + a.blocks1, per_pair = SA_HEADS * blocks;
  const unsigned pair = id / per_pair, rem = id % per_pair, blk = rem % blocks;
  SaWork w;
  w.head = (int)(rem / blocks);
  if (blk < (unsigned)a.blocks0) {
    w.own0 = (long long)pair * a.M; w.na = a.M; w.row0 = (int)blk * SA_BR;
  } else {
    w.own0 = (long long)a.B * a.M + (long long)pair * a.N; w.na = a.N; w.row0 = (int)(blk - a.blocks0) * SA_BR;
  }
  return w;
}

// rows [0, valid) of a [SA_BK][64] tile from src (row stride ld) into LDS, the others as zeros
__device__ __forceinline__ void sa_load_tile(float (*T)[SA_LDT], const float* __restrict__ src, long long ld, int valid,
                                             int tid) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int row = (tid >> 4) + 16 * q, c = (tid & 15) * 4;
    const float4 x = row < valid ? *reinterpret_cast<const float4*>(src + row * ld + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    T[row][c] = x.x; T[row][c + 1] = x.y; T[row][c + 2] = x.z; T[row][c + 3] = x.w;
  }
}

// the lane's MFMA operand of its own row: elements 2 kk + h of the 64 of `row` (zeros for a row outside the side)
__device__ __forceinline__ void sa_own_row(float (&r)[32], const float* __restrict__ row, bool valid, int h) {
#pragma unroll
  for (int kk = 0; kk < 32; ++kk) r[kk] = valid ? row[2 * kk + h] : 0.f;
}

// One 32x32 accumulator tile of the gradient at a rotated operand (row acc_row(r, h), column 32 c + l31 of the head) ->
// the gradient before the rotation, scaled: g = scale acc, out[2i] = g[2i] c[2i] + g[2i+1] s[2i+1],
// out[2i+1] = g[2i+1] c[2i+1] - g[2i] s[2i].  The partner column is the neighbouring lane's.  Without tables: g itself.
__device__ __forceinline__ void sa_store_unrotated(const SaArgs& a, const SaWork& w, const f32x16& acc, int c, int wave,
                                                   int h, int l31, int col_out) {
  const int cc = 32 * c + l31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float g = a.scale * acc[r];
    const float o = __shfl_xor(g, 1);
    const int row = w.row0 + wave * 32 + acc_row(r, h);
    if (row >= w.na) continue;
    float out = g;
    if (a.cos) {
      const long long t = (w.own0 + row) * SA_HD;
      const float x = g * a.cos[t + cc], y = o * a.sin[t + (cc ^ 1)];
      out = (cc & 1) ? x - y : x + y;
    }
    a.dqkv[(w.own0 + row) * a.ld_dqkv + col_out + cc] = out;
  }
}

// ---- D[row][head] = dctx[row, head] . ctx[row, head]: a wave per row, 16 lanes per head -----------------------------
__global__ __launch_bounds__(256) void sa_rowdot_kernel(const SaArgs a, size_t rows) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float4 c = *reinterpret_cast<const float4*>(a.ctx + row * a.ld_ctx + 4 * lane);
  const float4 g = *reinterpret_cast<const float4*>(a.dctx + row * a.ld_dctx + 4 * lane);
  float p = ((g.x * c.x + g.y * c.y) + g.z * c.z) + g.w * c.w;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) p += __shfl_xor(p, o);
  if ((lane & 15) == 0) a.dd[row * SA_HEADS + (lane >> 4)] = p;
}

// ---- lse[i] = log sum_j exp(scale q'[i] . k'[j]) over the rows j of i's side ----------------------------------------
// The tile is formed transposed (keys on the accumulator's rows, the own row on the lane), so that a lane's 16 registers
// are 16 keys of ITS row: the running maximum and sum stay in the lane, one per half, and the halves meet once at the end.
__global__ __launch_bounds__(256) void sa_lse_kernel(const SaArgs a) {
  __shared__ float Kb[SA_BK][SA_LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
  const SaWork w = sa_work(a, blockIdx.x);
  const int i = w.row0 + wave * 32 + l31;
  const int col = w.head * SA_HD;
  float qa[32];
  sa_own_row(qa, a.qkv + (w.own0 + i) * a.ld_qkv + col, i < w.na, h);
  float m = -INFINITY, s = 0.f;
  for (int j0 = 0; j0 < w.na; j0 += SA_BK) {
    __syncthreads();  // the previous tile has been read
    sa_load_tile(Kb, a.qkv + (w.own0 + j0) * a.ld_qkv + HB_D + col, a.ld_qkv, w.na - j0, tid);
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) acc = mfma32(Kb[l31][2 * kk + h], qa[kk], acc);
    float x[16], tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      x[r] = j0 + acc_row(r, h) < w.na ? a.scale * acc[r] : -INFINITY;
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
  if (h == 0 && i < w.na) a.lse[(w.own0 + i) * SA_HEADS + w.head] = mm + logf(ss);
}

// ---- dq of SA_BR rows of one head: the rows as queries, the side streamed as keys -----------------------------------
// Per tile of SA_BK keys j and per wave (rows i on the accumulator's rows, the key on the lane):
//   S = q'_i k'_j^T, T = dctx_i v_j^T                                          2 x 32 MFMAs, the keys' operands from LDS
//   P = exp(min(scale S - lse[i], 0)), 0 for a key outside the side;  dS = P (T - D[i])
//   dS crosses LDS once (the next product sums over the key, which is the lane here)
//   dq' += dS k'_j                                                              32 MFMAs
// and dq = Rot^T(scale dq') at the end.
__global__ __launch_bounds__(256) void sa_dq_kernel(const SaArgs a) {
  __shared__ float Kb[SA_BK][SA_LDT];
  __shared__ float Vb[SA_BK][SA_LDT];
  __shared__ float dSs[4][32][SA_LDP];
  __shared__ float stat_a[SA_BR][2];  // lse | D of the own rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
  const SaWork w = sa_work(a, blockIdx.x);
  const int i = w.row0 + wave * 32 + l31;
  const int col = w.head * SA_HD;
  const bool own = i < w.na;
  float qa[32], ga[32];
  sa_own_row(qa, a.qkv + (w.own0 + i) * a.ld_qkv + col, own, h);
  sa_own_row(ga, a.dctx + (w.own0 + i) * a.ld_dctx + col, own, h);
  if (tid < SA_BR) {
    const bool in = w.row0 + tid < w.na;
    const long long e = (w.own0 + w.row0 + tid) * SA_HEADS + w.head;
    stat_a[tid][0] = in ? a.lse[e] : 0.f;
    stat_a[tid][1] = in ? a.dd[e] : 0.f;
  }
  f32x16 dq[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[c][r] = 0.f;
  for (int j0 = 0; j0 < w.na; j0 += SA_BK) {
    const int valid = w.na - j0;
    __syncthreads();  // the previous tile has been read
    sa_load_tile(Kb, a.qkv + (w.own0 + j0) * a.ld_qkv + HB_D + col, a.ld_qkv, valid, tid);
    sa_load_tile(Vb, a.qkv + (w.own0 + j0) * a.ld_qkv + 2 * HB_D + col, a.ld_qkv, valid, tid);
    __syncthreads();
    f32x16 S, T;
#pragma unroll
    for (int r = 0; r < 16; ++r) S[r] = T[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
      const int k = 2 * kk + h;
      S = mfma32(qa[kk], Kb[l31][k], S);
      T = mfma32(ga[kk], Vb[l31][k], T);
    }
    const bool key = l31 < valid;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, h);
      const float p = key ? expf(fminf(a.scale * S[r] - stat_a[wave * 32 + row][0], 0.f)) : 0.f;
      dSs[wave][row][l31] = p * (T[r] - stat_a[wave * 32 + row][1]);
    }
    __syncthreads();  // a wave reads back its own tile only; the barrier orders its stores before its loads
#pragma unroll
    for (int kk = 0; kk < SA_BK / 2; ++kk) {
      const int j = 2 * kk + h;
      const float ds = dSs[wave][l31][j];
      dq[0] = mfma32(ds, Kb[j][l31], dq[0]);
      dq[1] = mfma32(ds, Kb[j][32 + l31], dq[1]);
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) sa_store_unrotated(a, w, dq[c], c, wave, h, l31, col);
}

// ---- dk and dv of SA_BR rows of one head: the rows as keys, the side streamed as queries ----------------------------
// Per tile of SA_BK queries i and per wave (own keys j on the accumulator's rows, the query on the lane):
//   S^T = k'_j q'_i^T, T^T = v_j dctx_i^T                                      2 x 32 MFMAs, the queries' operands from LDS
//   P^T = exp(min(scale S^T - lse[i], 0)), 0 for a query outside the side;  dS^T = P^T (T^T - D[i])
//   dS^T and P^T cross LDS once
//   dk' += dS^T q'_i, dv += P^T dctx_i                                          2 x 32 MFMAs
// and dk = Rot^T(scale dk') at the end; dv is stored as it is.
__global__ __launch_bounds__(256) void sa_dkv_kernel(const SaArgs a) {
  __shared__ float Qb[SA_BK][SA_LDT];
  __shared__ float Gb[SA_BK][SA_LDT];
  __shared__ float dSs[4][32][SA_LDP];
  __shared__ float Ps[4][32][SA_LDP];
  __shared__ float stat_b[SA_BK][2];  // lse | D of the tile's queries
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
  const SaWork w = sa_work(a, blockIdx.x);
  const int jrow = w.row0 + wave * 32 + l31;
  const int col = w.head * SA_HD;
  const bool own = jrow < w.na;
  float ka[32], va[32];
  sa_own_row(ka, a.qkv + (w.own0 + jrow) * a.ld_qkv + HB_D + col, own, h);
  sa_own_row(va, a.qkv + (w.own0 + jrow) * a.ld_qkv + 2 * HB_D + col, own, h);
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[c][r] = dv[c][r] = 0.f;
  for (int i0 = 0; i0 < w.na; i0 += SA_BK) {
    const int valid = w.na - i0;
    __syncthreads();  // the previous tile has been read
    sa_load_tile(Qb, a.qkv + (w.own0 + i0) * a.ld_qkv + col, a.ld_qkv, valid, tid);
    sa_load_tile(Gb, a.dctx + (w.own0 + i0) * a.ld_dctx + col, a.ld_dctx, valid, tid);
    if (tid < SA_BK) {
      const long long e = (w.own0 + i0 + tid) * SA_HEADS + w.head;
      stat_b[tid][0] = tid < valid ? a.lse[e] : 0.f;
      stat_b[tid][1] = tid < valid ? a.dd[e] : 0.f;
    }
    __syncthreads();
    f32x16 S, T;
#pragma unroll
    for (int r = 0; r < 16; ++r) S[r] = T[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
      const int k = 2 * kk + h;
      S = mfma32(ka[kk], Qb[l31][k], S);
      T = mfma32(va[kk], Gb[l31][k], T);
    }
    const bool qry = l31 < valid;
    const float lse_i = stat_b[l31][0], d_i = stat_b[l31][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, h);
      const float p = qry ? expf(fminf(a.scale * S[r] - lse_i, 0.f)) : 0.f;
      dSs[wave][row][l31] = p * (T[r] - d_i);
      Ps[wave][row][l31] = p;
    }
    __syncthreads();  // a wave reads back its own tiles only; the barrier orders its stores before its loads
#pragma unroll
    for (int kk = 0; kk < SA_BK / 2; ++kk) {
      const int i = 2 * kk + h;
      const float ds = dSs[wave][l31][i], p = Ps[wave][l31][i];
      dk[0] = mfma32(ds, Qb[i][l31], dk[0]);
      dk[1] = mfma32(ds, Qb[i][32 + l31], dk[1]);
      dv[0] = mfma32(p, Gb[i][l31], dv[0]);
      dv[1] = mfma32(p, Gb[i][32 + l31], dv[1]);
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    sa_store_unrotated(a, w, dk[c], c, wave, h, l31, HB_D + col);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = w.row0 + wave * 32 + acc_row(r, h);
      if (row >= w.na) continue;
      a.dqkv[(w.own0 + row) * a.ld_dqkv + 2 * HB_D + col + 32 * c + l31] = dv[c][r];
    }
  }
}

// ---- workspace: one description, used by the *_workspace_bytes exports and by the launchers ---------------------------
static inline long long sa_rows(int B, int M, int N) {
  if (B < 1 || M < 1 || N < 1) return 0;
  const long long rows = (long long)B * ((long long)M + N);
  return rows <= HB_MAX_ROWS / 3 ? rows : 0;  // row * 768 stays inside an int, as the forward's planner asks
}
struct SaLayout { size_t lse, dd, total; };
static inline SaLayout sa_layout(size_t rows) {
  gfc_slots s;
  return {s.take(rows * SA_HEADS * sizeof(float)), s.take(rows * SA_HEADS * sizeof(float)), s.off};
}
struct SbLayout { size_t qkv, dqkv, wpart, cpart, core, total; };
static inline SbLayout sb_layout(size_t rows) {
  const size_t f = sizeof(float), rq = rows * SA_QKV * f;
  gfc_slots s;
  return {s.take(rq), s.take(rq), s.take((size_t)hb_split((int)rows).parts * SA_QKV * HB_D * f),
          s.take((size_t)hb_chunks(rows) * SA_QKV * f), s.take(sa_layout(rows).total), s.off};
}

static inline bool sa_ptr_ok(const void* p, int ld, int cols) {
  return p && !((uintptr_t)p & 15) && ld >= cols && !(ld & 3);
}

extern "C" size_t gfc_attention_self_backward_workspace_bytes(int B, int M, int N, int heads) {
  const long long rows = sa_rows(B, M, N);
  return rows && heads == SA_HEADS ? sa_layout((size_t)rows).total : 0;
}

extern "C" int gfc_attention_self_backward(const float* qkv, int ld_qkv, const float* ctx, int ld_ctx, const float* dctx,
                                           int ld_dctx, const float* cos, const float* sin, int B, int M, int N, int heads,
                                           float scale, float* dqkv, int ld_dqkv, void* ws, size_t ws_bytes,
                                           void* stream) {
  const long long rows = sa_rows(B, M, N);
  if (!rows || heads * SA_HD != HB_D) return GFC_ERR_INVALID;
  if (!sa_ptr_ok(qkv, ld_qkv, SA_QKV) || !sa_ptr_ok(ctx, ld_ctx, HB_D) || !sa_ptr_ok(dctx, ld_dctx, HB_D) ||
      !sa_ptr_ok(dqkv, ld_dqkv, SA_QKV) || (cos == nullptr) != (sin == nullptr) || ((uintptr_t)cos & 15) ||
      ((uintptr_t)sin & 15))
    return GFC_ERR_INVALID;
  const SaLayout L = sa_layout((size_t)rows);
  if (!ws || ws_bytes < L.total || ((uintptr_t)ws & 15)) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  SaArgs a{};
  a.qkv = qkv; a.ctx = ctx; a.dctx = dctx; a.cos = cos; a.sin = sin;
  a.ld_qkv = ld_qkv; a.ld_ctx = ld_ctx; a.ld_dctx = ld_dctx; a.ld_dqkv = ld_dqkv;
  a.dqkv = dqkv;
  a.lse = (float*)((char*)ws + L.lse);
  a.dd = (float*)((char*)ws + L.dd);
  a.B = B; a.M = M; a.N = N;
  a.blocks0 = (M + SA_BR - 1) / SA_BR;
  a.blocks1 = (N + SA_BR - 1) / SA_BR;
  a.scale = scale;
  // rows <= HB_MAX_ROWS / 3: at most 4 (rows / 128 + 2 B) workgroups, inside an unsigned
  const unsigned grid = (unsigned)B * SA_HEADS * (unsigned)(a.blocks0 + a.blocks1);
  hipLaunchKernelGGL(sa_rowdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a, (size_t)rows);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sa_lse_kernel, dim3(grid), dim3(256), 0, st, a);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sa_dq_kernel, dim3(grid), dim3(256), 0, st, a);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sa_dkv_kernel, dim3(grid), dim3(256), 0, st, a);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

// One chunk of HB_CS_ROWS rows of dqkv [rows][768], a thread per column: part[chunk][768]
__global__ __launch_bounds__(256) void sb_colsum_kernel(const float* __restrict__ dqkv, size_t R, float* __restrict__ part) {
  const int col = blockIdx.y * 256 + threadIdx.x;
  const size_t r_begin = (size_t)blockIdx.x * HB_CS_ROWS, r_end = min(R, r_begin + HB_CS_ROWS);
  float s = 0.f;
  for (size_t row = r_begin; row < r_end; ++row) s += dqkv[row * SA_QKV + col];
  part[(size_t)blockIdx.x * SA_QKV + col] = s;
}

// dx = dx_in + dx
__global__ __launch_bounds__(256) void sb_sum_kernel(float* __restrict__ dx, const float* __restrict__ dx_in, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dx[i] = dx_in[i] + dx[i];
}

extern "C" size_t gfc_lg_self_attn_backward_workspace_bytes(int B, int M, int N) {
  const long long rows = sa_rows(B, M, N);
  return rows ? sb_layout((size_t)rows).total : 0;
}

extern "C" int gfc_lg_self_attn_backward(const float* x, const float* cos, const float* sin, const float* ctx,
                                         const float* dctx, const float* dx_in, const float* Wqkv, const float* bqkv, int B,
                                         int M, int N, float* dWqkv, float* dbqkv, float* dx, void* ws, size_t ws_bytes,
                                         void* stream) {
  const long long rows = sa_rows(B, M, N);
  if (!rows) return GFC_ERR_INVALID;
  if (!sa_ptr_ok(x, HB_D, HB_D) || !sa_ptr_ok(ctx, HB_D, HB_D) || !sa_ptr_ok(dctx, HB_D, HB_D) ||
      !sa_ptr_ok(cos, SA_HD, SA_HD) || !sa_ptr_ok(sin, SA_HD, SA_HD) || !Wqkv || ((uintptr_t)Wqkv & 15) || !bqkv ||
      !dWqkv || !dbqkv || (dx_in && (!dx || dx == dx_in)) || (dx && ((uintptr_t)dx & 15)))
    return GFC_ERR_INVALID;
  const SbLayout L = sb_layout((size_t)rows);
  if (!ws || ws_bytes < L.total || ((uintptr_t)ws & 15)) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  float* qkv = (float*)(base + L.qkv);
  float* dqkv = (float*)(base + L.dqkv);
  float* wpart = (float*)(base + L.wpart);
  float* cpart = (float*)(base + L.cpart);
  const int R = (int)rows;
  const HbSplit sp = hb_split(R);

  // the forward, with the forward's entry point: q and k rotated in the GEMM's epilogue
  HB_TRY(gfc_linear(x, HB_D, HB_D, nullptr, 0, 0, Wqkv, HB_D, bqkv, nullptr, nullptr, 1.f, nullptr, cos, sin, 2 * HB_D, qkv,
                    SA_QKV, R, SA_QKV, stream));
  HB_TRY(gfc_attention_self_backward(qkv, SA_QKV, ctx, HB_D, dctx, HB_D, cos, sin, B, M, N, SA_HEADS, 0.125f, dqkv, SA_QKV,
                                     base + L.core, sa_layout((size_t)rows).total, stream));

  // dWqkv = dqkv^T x, split over rows
  HbGemm g{};
  g.alpha = 1.f;
  g.A = dqkv; g.a_m = 1; g.a_k = SA_QKV; g.K = R; g.kchunk = sp.kchunk;
  g.B = x; g.b_k = HB_D; g.C = wpart; g.c_m = HB_D; g.c_p = (long long)SA_QKV * HB_D;
  g.M = SA_QKV; g.N = HB_D;
  HB_TRY(hb_gemm(g, false, sp.parts, 1, st));
  HB_TRY(hb_finish(wpart, sp.parts, (size_t)SA_QKV * HB_D, SA_QKV * HB_D, dWqkv, st));
  const int chunks = hb_chunks((size_t)rows);
  hipLaunchKernelGGL(sb_colsum_kernel, dim3(chunks, SA_QKV / 256), dim3(256), 0, st, dqkv, (size_t)rows, cpart);
  GFC_LAUNCH_CHECK();
  HB_TRY(hb_finish(cpart, chunks, SA_QKV, SA_QKV, dbqkv, st));

  if (dx) {
    // dx = (dx_in +) dqkv Wqkv
    HbGemm d{};
    d.alpha = 1.f;
    d.A = dqkv; d.a_m = SA_QKV; d.a_k = 1; d.B = Wqkv; d.b_k = HB_D; d.C = dx; d.c_m = HB_D;
    d.M = R; d.N = HB_D; d.K = SA_QKV; d.kchunk = SA_QKV;
    HB_TRY(hb_gemm(d, true, 1, 1, st));
    if (dx_in) {
      const size_t n = (size_t)rows * HB_D;
      hipLaunchKernelGGL(sb_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dx, dx_in, n);
      GFC_LAUNCH_CHECK();
    }
  }
  return GFC_OK;
}
