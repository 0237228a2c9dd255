// One layer's agreement with the final assignment, its token-confidence loss and its share of confident points, for a
// batch of equal-sized pairs.  The definitions, the tie and NaN rules and the reference lines are stated in
// include/gfc_amd_layer_scores.h.
//
// Both log assignments [B, M+1, N+1] are read twice, once along the rows and once down the columns, by ONE launch whose
// grid holds both kinds of workgroup for every pair (a pair is split over workgroups: at B = 32 one workgroup per pair
// would use 32 of 256 CUs):
//   row workgroups     LS_ROWS rows each, a wave per row of both matrices: 16-byte loads from the first 16-byte boundary
//                      of the row on (N + 1 is odd at the sizes used, so rows start at any 4-byte phase), the elements
//                      before it and behind the last whole vector by scalar loads; the wave's (max, index) by shuffles.
//                      The row's target, its BCE term and its confident bit are taken there; the workgroup's sums go to
//                      the workspace.
//   column workgroups  a tile of LS_COLS columns x a chunk of LS_CHUNK rows: every wave walks its quarter of the chunk
//                      row by row (64 consecutive floats per load instruction) with a running (max, index) per column in
//                      registers, the four waves are combined in LDS, the chunk's (max, index) goes to the workspace.
// The finishing launch (one workgroup per pair) combines the chunks of every column in ascending row order, takes the
// column targets and terms, and adds all partial sums in a fixed order.  Every comparison keeps the lower index among
// equals; nothing is accumulated by atomics, so the result does not depend on the order in which workgroups run.
#include "eval_common.h"
#include "lg_rowdot.h"
#include "../../include/gfc_amd_layer_scores.h"

#define LS_THREADS 256
#define LS_WAVES (LS_THREADS / 64)
#define LS_ROWS 16     // rows of a row workgroup: four per wave
#define LS_COLS 256    // columns of a column tile: four per lane, 64 apart
#define LS_CHUNK 128   // rows of a column chunk: 32 per wave
#define LS_FIN_THREADS 1024
#define LS_FIN_WAVES (LS_FIN_THREADS / 64)
#define LS_NONE 0x7fffffff  // index of a running maximum that has not met an entry above -inf

struct alignas(16) LsRowPart { double bce; int agree; int conf; };                       // sums of one row workgroup
struct alignas(16) LsColBest { float v_layer; int i_layer; float v_final; int i_final; };  // one column of one chunk

// Workspace: one description, used by gfc_lg_layer_scores_workspace_bytes and by the launcher.
struct LsLayout { size_t row_part, col_best, total; };
static inline int ls_row_blocks(int M) { return (M + LS_ROWS - 1) / LS_ROWS; }
static inline int ls_col_tiles(int N) { return (N + LS_COLS - 1) / LS_COLS; }
static inline int ls_chunks(int M) { return (M + 1 + LS_CHUNK - 1) / LS_CHUNK; }
static inline bool ls_sizes_ok(int B, int M, int N) {
  return B >= 1 && M >= 1 && N >= 1 && B <= 65535 && M <= 65535 && N <= 65535;
}
static inline LsLayout ls_layout(int B, int M, int N) {
  gfc_slots s;
  return {s.take((size_t)B * ls_row_blocks(M) * sizeof(LsRowPart)),
          s.take((size_t)B * ls_chunks(M) * N * sizeof(LsColBest)), s.off};
}

// entries arrive in ascending index order: the first of equal maxima stays, a NaN never enters
__device__ __forceinline__ void ls_take(float v, int j, float& best, int& bi) {
  if (v > best) { best = v; bi = j; }
}
// two running maxima of disjoint index sets: the lower index among equals
__device__ __forceinline__ void ls_merge(float ov, int oi, float& best, int& bi) {
  if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
}

// arg-max of row[0 .. n) on one wave (every lane returns it)
__device__ __forceinline__ int ls_row_argmax(const float* __restrict__ row, int n, int lane) {
  float best = -INFINITY;
  int bi = LS_NONE;
  int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);  // elements before the 16-byte boundary
  if (head > n) head = n;
  if (lane < head) ls_take(row[lane], lane, best, bi);
  const float4* __restrict__ p = reinterpret_cast<const float4*>(row + head);
  const int nv = (n - head) >> 2;
#pragma unroll 2
  for (int k = lane; k < nv; k += 64) {
    const float4 v = p[k];
    const int j = head + 4 * k;
    ls_take(v.x, j, best, bi);
    ls_take(v.y, j + 1, best, bi);
    ls_take(v.z, j + 2, best, bi);
    ls_take(v.w, j + 3, best, bi);
  }
  const int t = head + 4 * nv + lane;  // at most three elements behind the last whole vector
  if (t < n) ls_take(row[t], t, best, bi);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    ls_merge(ov, oi, best, bi);
  }
  return bi == LS_NONE ? 0 : bi;
}

// BCEWithLogits(x, y), y = 0 / 1, in fp32
__device__ __forceinline__ float ls_bce(float x, int y) {
  return (fmaxf(x, 0.f) - x * (float)y) + log1pf(expf(-fabsf(x)));
}

__global__ __launch_bounds__(LS_THREADS) void ls_sweep_kernel(
    const float* __restrict__ la, const float* __restrict__ lf, const float* __restrict__ logit0, float threshold, int M,
    int N, int row_blocks, int col_tiles, int chunks, unsigned char* __restrict__ correct0,
    LsRowPart* __restrict__ row_part, LsColBest* __restrict__ col_best) {
  __shared__ float sv[2][LS_WAVES][LS_COLS];
  __shared__ int si[2][LS_WAVES][LS_COLS];
  __shared__ LsRowPart sp[LS_WAVES];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t ld = (size_t)N + 1;
  const size_t pair = (size_t)b * ((size_t)M + 1) * ld;
  if ((int)blockIdx.x < row_blocks) {
    double bce = 0.0;
    int agree = 0, conf = 0;
    for (int r = 0; r < LS_ROWS / LS_WAVES; ++r) {
      const int i = (int)blockIdx.x * LS_ROWS + r * LS_WAVES + wave;  // the same in every lane of the wave
      if (i >= M) break;
      const int a = ls_row_argmax(la + pair + (size_t)i * ld, N + 1, lane);
      const int f = ls_row_argmax(lf + pair + (size_t)i * ld, N + 1, lane);
      const int c = a == f;
      const float x = logit0[(size_t)b * M + i];
      bce += (double)ls_bce(x, c);
      agree += c;
      conf += !(gfc_sigmoid(x) < threshold);
      if (correct0 && lane == 0) correct0[(size_t)b * M + i] = (unsigned char)c;
    }
    if (lane == 0) sp[wave] = LsRowPart{bce, agree, conf};
    __syncthreads();
    if (tid == 0) {
      LsRowPart t = sp[0];
      for (int w = 1; w < LS_WAVES; ++w) { t.bce += sp[w].bce; t.agree += sp[w].agree; t.conf += sp[w].conf; }
      row_part[(size_t)b * row_blocks + blockIdx.x] = t;
    }
    return;
  }
  const int t = (int)blockIdx.x - row_blocks;
  const int tile = t % col_tiles, chunk = t / col_tiles;
  const int c0 = tile * LS_COLS;
  const int r0 = chunk * LS_CHUNK + wave * (LS_CHUNK / LS_WAVES);
  const int r1 = min(r0 + LS_CHUNK / LS_WAVES, M + 1);
  float va[4], vf[4];
  int ia[4], jf[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { va[q] = vf[q] = -INFINITY; ia[q] = jf[q] = LS_NONE; }
  const float* __restrict__ A = la + pair + c0 + lane;
  const float* __restrict__ F = lf + pair + c0 + lane;
#pragma unroll 2
  for (int i = r0; i < r1; ++i) {
    const size_t o = (size_t)i * ld;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c0 + lane + 64 * q < N) {  // columns j < N only: the dustbin column has no target
        ls_take(A[o + 64 * q], i, va[q], ia[q]);
        ls_take(F[o + 64 * q], i, vf[q], jf[q]);
      }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    sv[0][wave][lane + 64 * q] = va[q];
    si[0][wave][lane + 64 * q] = ia[q];
    sv[1][wave][lane + 64 * q] = vf[q];
    si[1][wave][lane + 64 * q] = jf[q];
  }
  __syncthreads();
  if (c0 + tid < N) {  // LS_THREADS == LS_COLS: a thread per column of the tile
    LsColBest e{sv[0][0][tid], si[0][0][tid], sv[1][0][tid], si[1][0][tid]};
    for (int w = 1; w < LS_WAVES; ++w) {
      ls_merge(sv[0][w][tid], si[0][w][tid], e.v_layer, e.i_layer);
      ls_merge(sv[1][w][tid], si[1][w][tid], e.v_final, e.i_final);
    }
    col_best[((size_t)b * chunks + chunk) * N + c0 + tid] = e;
  }
}

__global__ __launch_bounds__(LS_FIN_THREADS) void ls_finish_kernel(
    const float* __restrict__ logit1, float threshold, int M, int N, int row_blocks, int chunks,
    const LsRowPart* __restrict__ row_part, const LsColBest* __restrict__ col_best,
    unsigned char* __restrict__ correct1, float* __restrict__ out) {
  __shared__ double red[LS_FIN_WAVES * 6];
  const int b = blockIdx.x, tid = threadIdx.x;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // agree0, agree1, bce0, bce1, conf0, conf1 (counts are exact in fp64)
  for (int k = tid; k < row_blocks; k += LS_FIN_THREADS) {
    const LsRowPart p = row_part[(size_t)b * row_blocks + k];
    s[0] += (double)p.agree;
    s[2] += p.bce;
    s[4] += (double)p.conf;
  }
  for (int j = tid; j < N; j += LS_FIN_THREADS) {
    LsColBest e{-INFINITY, LS_NONE, -INFINITY, LS_NONE};
    for (int ch = 0; ch < chunks; ++ch) {
      const LsColBest o = col_best[((size_t)b * chunks + ch) * N + j];
      ls_merge(o.v_layer, o.i_layer, e.v_layer, e.i_layer);
      ls_merge(o.v_final, o.i_final, e.v_final, e.i_final);
    }
    const int c = (e.i_layer == LS_NONE ? 0 : e.i_layer) == (e.i_final == LS_NONE ? 0 : e.i_final);
    const float x = logit1[(size_t)b * N + j];
    s[1] += (double)c;
    s[3] += (double)ls_bce(x, c);
    s[5] += (double)!(gfc_sigmoid(x) < threshold);
    if (correct1) correct1[(size_t)b * N + j] = (unsigned char)c;
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const double t = wave_sum_f64(s[q]);
    if ((tid & 63) == 0) red[(tid >> 6) * 6 + q] = t;
  }
  __syncthreads();
  if (tid < 6) {
    double t = 0.0;
    for (int w = 0; w < LS_FIN_WAVES; ++w) t += red[w * 6 + tid];
    if (tid == 2) t /= (double)M;
    if (tid == 3) t /= (double)N;
    out[(size_t)b * 6 + tid] = (float)t;
  }
}

extern "C" size_t gfc_lg_layer_scores_workspace_bytes(int B, int M, int N) {
  return ls_sizes_ok(B, M, N) ? ls_layout(B, M, N).total : 0;
}

extern "C" int gfc_lg_layer_scores(const float* la_layer, const float* la_final, const float* logit0,
                                   const float* logit1, float threshold, int B, int M, int N, float* out,
                                   uint8_t* correct0, uint8_t* correct1, void* ws, size_t ws_bytes, void* stream) {
  if (!ls_sizes_ok(B, M, N)) return GFC_ERR_INVALID;
  if (!la_layer || !la_final || !logit0 || !logit1 || !out) return GFC_ERR_INVALID;
  const LsLayout L = ls_layout(B, M, N);
  if (!ws || ws_bytes < L.total || ((uintptr_t)ws & 15)) return GFC_ERR_WORKSPACE;
  LsRowPart* row_part = (LsRowPart*)((char*)ws + L.row_part);
  LsColBest* col_best = (LsColBest*)((char*)ws + L.col_best);
  const int row_blocks = ls_row_blocks(M), col_tiles = ls_col_tiles(N), chunks = ls_chunks(M);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ls_sweep_kernel, dim3(row_blocks + col_tiles * chunks, B), dim3(LS_THREADS), 0, s, la_layer,
                     la_final, logit0, threshold, M, N, row_blocks, col_tiles, chunks, correct0, row_part, col_best);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(ls_finish_kernel, dim3(B), dim3(LS_FIN_THREADS), 0, s, logit1, threshold, M, N, row_blocks, chunks,
                     row_part, col_best, correct1, out);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
