// The RANSAC frame of the robust estimators (ransac.hip: homography; relpose.hip: relative pose), written once: the
// counter-based sampler, the compaction of the matches, the hypothesis ranges and the workspace layout, the scoring
// kernel, the merge of the ranges, the block-wide MSAC score, the acceptance test of the local optimisation, the
// inlier epilogue, the launch of the scoring kernel and the argument checks of the two entry points.  An estimator
// supplies a MODEL type with what truly differs:
//
//   static constexpr int K, MAX_SOL            minimal sample size; most models one hypothesis yields
//   struct args                                the estimator's kernel arguments, passed by value
//   struct work                                per-lane scratch of the solver (empty when it needs none)
//   static int pack(h, k)                      (hypothesis, solution) as the one ordered int that is reduced
//   static double t2(args, b, t)               squared threshold t of pair b
//   static int solve(corr, key, h, n, work, m, ok)   the sample of hypothesis h -> ns models m[k * 9 .. + 9) (3x3,
//                                              row-major) and whether each is valid, ok[k]
//   static double residual2(m, x0, y0, x1, y1) squared residual of one record
//
// A model's score is one lane's serial sum in correspondence order and every winner is chosen by (score, packed index),
// ties to the lower index: the result does not depend on the number of ranges, the batch or the launch shape.
#pragma once
#include "eval_common.h"

#define RS_MAX_T 8
#define RS_LDS_CORR_BYTES (128 * 1024)
#define RS_GOLDEN 0x9E3779B97F4A7C15ull

// T thresholds replicated to RS_MAX_T; the unit (pixels, squared pixels) is the estimator's
struct rs_thresholds { double v[RS_MAX_T]; };

// ---- sampler: splitmix64 finaliser as a counter-based generator ---------------------------------------------
__device__ __host__ __forceinline__ unsigned long long rs_mix64(unsigned long long z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
__device__ __host__ __forceinline__ unsigned long long rs_key(unsigned long long seed, unsigned long long stream) {
  return rs_mix64(rs_mix64(seed + RS_GOLDEN) ^ stream);
}
// the key of pair b: its own stream id, or b
__device__ __forceinline__ unsigned long long rs_pair_key(unsigned long long seed, const long long* stream_id, int b) {
  return rs_key(seed, stream_id ? (unsigned long long)stream_id[b] : (unsigned long long)b);
}

// K distinct indices in [0, n), n >= K: draw j of hypothesis h is u = mix64(key + GOLDEN (K h + j + 1)),
// r_j = ((u >> 32) (n - j)) >> 32, and the r_j index a partial Fisher-Yates over the virtual array a[p] = p ("take
// a[r_j], move the last live element a[n - 1 - j] into the hole"): a hole is looked up latest first.  K = 4 is the
// homography estimator's sampler (ransac.hip), K = 5 the relative-pose one's; eval_utils.ransac_sample_indices is the
// same function in integer numpy, and the GPU tests of both estimators check the kernels against it.
template <int K>
__device__ __host__ __forceinline__ void rs_sample_k(unsigned long long key, int h, int n, int* out) {
  int p[K], v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const unsigned long long u = rs_mix64(key + RS_GOLDEN * ((unsigned long long)K * (unsigned long long)h + (unsigned long long)(j + 1)));
    const int r = (int)(((u >> 32) * (unsigned long long)(n - j)) >> 32);
    const int l = n - 1 - j;
    int idx = r, val = l;
    bool fi = false, fv = false;
#pragma unroll
    for (int q = K - 1; q >= 0; --q) {
      if (q < j) {
        if (!fi && r == p[q]) { idx = v[q]; fi = true; }
        if (!fv && l == p[q]) { val = v[q]; fv = true; }
      }
    }
    out[j] = idx;
    p[j] = r;
    v[j] = val;
  }
}

// the matches (i, m0[i]) with 0 <= m0[i] < N in ascending i -> (x0, y0, x1, y1) records + their key-point-0 index + n
// (defined in ransac.hip)
__global__ __launch_bounds__(EM_THREADS) void ransac_compact_kernel(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                      const long long* __restrict__ m0, int M, int N, float4* __restrict__ corr,
                                      int* __restrict__ cidx, int* __restrict__ cnt);

// ---- scoring --------------------------------------------------------------------------------------------------
// the order every reduction uses: lower score, ties to the lower packed index
__device__ __forceinline__ bool rs_better(double os, int oi, double s, int i) { return os < s || (os == s && oi < i); }

// threshold t of th, t not a compile-time constant (a select chain: no indexed kernel argument)
__device__ __forceinline__ double rs_pick(const rs_thresholds& th, int t) {
  double v = th.v[0];
#pragma unroll
  for (int q = 1; q < RS_MAX_T; ++q) v = (q == t) ? th.v[q] : v;
  return v;
}

// One lane per hypothesis of [h_lo, h_hi): its models in (h, k) order, each with its T MSAC sums over the n records in
// correspondence order (all lanes of a wave read the same record); a lane keeps its best per threshold on strict <.
template <class Model, int T>
__device__ __forceinline__ void rs_score_range(const float4* corr, int n, unsigned long long key, int h_lo, int h_hi,
                                               const double* t2, double* best, int* best_i) {
#pragma unroll
  for (int t = 0; t < T; ++t) { best[t] = INFINITY; best_i[t] = 0x7fffffff; }
  typename Model::work w;
  double ms[Model::MAX_SOL * 9];
  bool ok[Model::MAX_SOL];
  for (int h = h_lo + (int)threadIdx.x; h < h_hi; h += EM_THREADS) {
    const int ns = Model::solve(corr, key, h, n, w, ms, ok);
    for (int k = 0; k < ns; ++k) {
      if (!ok[k]) continue;
      double m[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) m[e] = ms[k * 9 + e];
      double acc[T];
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = 0.0;
      for (int c = 0; c < n; ++c) {
        const float4 q = corr[c];  // the same address in every lane of a wave whose lanes are all here
        const double r2 = Model::residual2(m, q.x, q.y, q.z, q.w);
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] += (r2 < t2[t]) ? r2 : t2[t];
      }
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (acc[t] < best[t]) { best[t] = acc[t]; best_i[t] = Model::pack(h, k); }
    }
  }
}

// One workgroup per (pair, hypothesis range): records staged in LDS (use_lds) or read through L2 -> rs_score_range ->
// argmin over the block per threshold -> part_score / part_idx [pair][range][T], index -1 when nothing scored.
template <class Model, int T>
__global__ __launch_bounds__(EM_THREADS) void ransac_score_kernel(const float4* __restrict__ corr_all,
                                                                  const int* __restrict__ cnt,
                                                                  const long long* __restrict__ stream_id,
                                                                  unsigned long long seed, int M, int S, int NH,
                                                                  int use_lds, typename Model::args a,
                                                                  double* __restrict__ part_score,
                                                                  int* __restrict__ part_idx) {
  extern __shared__ __attribute__((aligned(16))) float4 lds_corr[];
  __shared__ double ws[4 * RS_MAX_T];
  __shared__ int wh[4 * RS_MAX_T];
  const int b = blockIdx.x / S, s = blockIdx.x % S, tid = threadIdx.x;
  const int n = cnt[b];
  const float4* corr = corr_all + (size_t)b * M;
  double* ps = part_score + (size_t)blockIdx.x * T;
  int* ph = part_idx + (size_t)blockIdx.x * T;
  if (n < Model::K) {
    if (tid < T) { ps[tid] = INFINITY; ph[tid] = -1; }
    return;
  }
  const unsigned long long key = rs_pair_key(seed, stream_id, b);
  const int chunk = (NH + S - 1) / S;
  const int h_lo = s * chunk, h_hi = min(NH, h_lo + chunk);
  double t2[T];
#pragma unroll
  for (int t = 0; t < T; ++t) t2[t] = Model::t2(a, b, t);
  double best[T];
  int best_i[T];
  if (use_lds) {
    for (int c = tid; c < n; c += EM_THREADS) lds_corr[c] = corr[c];
    __syncthreads();
    rs_score_range<Model, T>(lds_corr, n, key, h_lo, h_hi, t2, best, best_i);
  } else {
    rs_score_range<Model, T>(corr, n, key, h_lo, h_hi, t2, best, best_i);
  }
  // argmin over the block
#pragma unroll
  for (int t = 0; t < T; ++t) {
    double sc = best[t];
    int hh = best_i[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(sc, o, 64);
      const int oh = __shfl_xor(hh, o, 64);
      if (rs_better(os, oh, sc, hh)) { sc = os; hh = oh; }
    }
    if ((tid & 63) == 0) { ws[(tid >> 6) * RS_MAX_T + t] = sc; wh[(tid >> 6) * RS_MAX_T + t] = hh; }
  }
  __syncthreads();
  if (tid < T) {
    double sc = ws[tid];
    int hh = wh[tid];
    for (int w = 1; w < 4; ++w) {
      const double os = ws[w * RS_MAX_T + tid];
      const int oh = wh[w * RS_MAX_T + tid];
      if (rs_better(os, oh, sc, hh)) { sc = os; hh = oh; }
    }
    ps[tid] = sc;
    ph[tid] = (sc < INFINITY) ? hh : -1;
  }
}

// ---- what the local-optimisation kernels (one workgroup per (pair, threshold)) share -----------------------------
// winner of pair b at threshold t over its S ranges: the packed index, -1 when no range scored
__device__ __forceinline__ int rs_merge_ranges(const double* __restrict__ part_score, const int* __restrict__ part_idx,
                                               int b, int S, int T, int t) {
  double bs = INFINITY;
  int bi = -1;
  for (int s = 0; s < S; ++s) {
    const double os = part_score[((size_t)b * S + s) * T + t];
    const int oi = part_idx[((size_t)b * S + s) * T + t];
    if (oi >= 0 && rs_better(os, oi, bs, bi)) { bs = os; bi = oi; }
  }
  return bi;
}

// MSAC score of model m over the n records, block-wide (thread-strided partial sums, then block_sum_f64)
template <class Model>
__device__ __forceinline__ double rs_block_msac(const double* m, const float4* corr, int n, double t2, double* red,
                                                int tid) {
  double v[1] = {0.0};
  for (int c = tid; c < n; c += EM_THREADS) {
    const float4 q = corr[c];
    const double r2 = Model::residual2(m, q.x, q.y, q.z, q.w);
    v[0] += (r2 < t2) ? r2 : t2;
  }
  block_sum_f64<1>(v, red, tid);
  return v[0];
}

// a candidate of the local optimisation is accepted iff its MSAC score is strictly lower (then cur_score becomes it)
template <class Model>
__device__ __forceinline__ bool rs_lo_accept(const double* cand, double& cur_score, const float4* corr, int n,
                                             double t2, double* red, int tid) {
  const double cand_score = rs_block_msac<Model>(cand, corr, n, t2, red, tid);
  if (!(cand_score < cur_score)) return false;
  cur_score = cand_score;
  return true;
}

// inliers of model m in key-point-0 indexing -- every i is written exactly once: unmatched rows first, matched rows
// through cidx -- and their number
template <class Model>
__device__ __forceinline__ int rs_write_inliers(const double* m, const float4* corr, const int* cidx,
                                                const long long* mm, unsigned char* inl, int n, int M, int N, double t2,
                                                double* red, int tid) {
  for (int i = tid; i < M; i += EM_THREADS) {
    const long long j = mm[i];
    if (!(j > -1 && j < N)) inl[i] = 0;
  }
  double cntv[1] = {0.0};
  for (int c = tid; c < n; c += EM_THREADS) {
    const float4 q = corr[c];
    const bool in = Model::residual2(m, q.x, q.y, q.z, q.w) < t2;
    inl[cidx[c]] = in ? 1 : 0;  // cidx[c] < M by construction (ransac_compact_kernel)
    cntv[0] += in ? 1.0 : 0.0;
  }
  block_sum_f64<1>(cntv, red, tid);
  return (int)cntv[0];
}

// ---- host side ---------------------------------------------------------------------------------------------------
// Hypothesis ranges per pair: ceil(512 / B) of them, so that a small batch still fills the device, but at most
// floor(NH / 256): a range (ceil(NH / S) hypotheses, the last one what is left) then has at least one hypothesis per
// lane whenever NH >= 256.  The winner does not depend on S.
static int rs_splits(int B, int NH) {
  const int want = B >= 512 ? 1 : (511 + B) / B, most = NH / EM_THREADS;  // no overflow for any B > 0
  return (want < most ? want : most) < 1 ? 1 : (want < most ? want : most);
}

// records, their key-point-0 index, counts, the ranges' partial winners; `tail`: tail_bytes per (pair, threshold) of
// the estimator's own (no slot when 0)
struct rs_layout { size_t corr, cidx, cnt, pscore, pidx, tail, total; };
static rs_layout rs_plan(int B, int M, int T, int NH, size_t tail_bytes) {
  const size_t S = (size_t)rs_splits(B, NH);
  gfc_slots s;
  return {s.take((size_t)B * M * sizeof(float4)), s.take((size_t)B * M * sizeof(int)), s.take((size_t)B * sizeof(int)),
          s.take((size_t)B * S * T * sizeof(double)), s.take((size_t)B * S * T * sizeof(int)),
          tail_bytes ? s.take((size_t)B * T * tail_bytes) : s.off, s.off};
}
static size_t rs_workspace_bytes(int B, int M, int T, int NH, size_t tail_bytes) {
  if (B <= 0 || M < 0 || T <= 0 || T > RS_MAX_T || NH <= 0) return 0;
  return rs_plan(B, M, T, NH, tail_bytes).total;
}

// what rs_begin hands to an entry point: the thresholds as given, the carved workspace, the ranges, the stream
struct rs_frame {
  rs_thresholds th;
  float4* corr;
  int* cidx;
  int* cnt;
  double* part_score;
  int* part_idx;
  void* tail;
  int S;
  hipStream_t st;
};

// The checks both entry points share (an empty side has nothing to point at: its arrays may be NULL), the thresholds
// (positive, finite; the last one replicated to RS_MAX_T), the workspace, and the compaction of the matches.  An entry
// point makes its own argument checks first: every one of them is answered before GFC_ERR_WORKSPACE.
static int rs_begin(const float* kp0, const float* kp1, const int64_t* m0, int B, int M, int N, const float* thresholds,
                    int T, int NH, int lo_iters, const uint8_t* inliers, const int32_t* num_inliers,
                    const uint8_t* success, const int32_t* best_hypothesis, size_t tail_bytes, void* ws,
                    size_t ws_bytes, void* stream, rs_frame& f) {
  if (B <= 0 || M < 0 || N < 0 || T <= 0 || T > RS_MAX_T || NH <= 0 || lo_iters < 0) return GFC_ERR_INVALID;
  if ((M > 0 && (!kp0 || !m0 || !inliers)) || (N > 0 && !kp1) || !thresholds || !num_inliers || !success ||
      !best_hypothesis || !ws)
    return GFC_ERR_INVALID;
  f.S = rs_splits(B, NH);
  if ((size_t)B * (size_t)T > 0x7fffffffull || (size_t)B * (size_t)f.S > 0x7fffffffull) return GFC_ERR_INVALID;
  for (int t = 0; t < RS_MAX_T; ++t) {
    const float v = thresholds[t < T ? t : T - 1];
    if (!(v > 0.f) || !(v < INFINITY)) return GFC_ERR_INVALID;
    f.th.v[t] = (double)v;
  }
  const rs_layout L = rs_plan(B, M, T, NH, tail_bytes);
  if (ws_bytes < L.total) return GFC_ERR_WORKSPACE;
  char* w = (char*)ws;
  f.corr = (float4*)(w + L.corr);
  f.cidx = (int*)(w + L.cidx);
  f.cnt = (int*)(w + L.cnt);
  f.part_score = (double*)(w + L.pscore);
  f.part_idx = (int*)(w + L.pidx);
  f.tail = w + L.tail;
  f.st = (hipStream_t)stream;
  hipLaunchKernelGGL(ransac_compact_kernel, dim3(B), dim3(EM_THREADS), 0, f.st, kp0, kp1, (const long long*)m0, M, N,
                     f.corr, f.cidx, f.cnt);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

template <class Model, int T>
static int rs_launch_score(const rs_frame& f, const long long* stream_id, unsigned long long seed, int B, int M, int NH,
                           const typename Model::args& a) {
  const size_t corr_bytes = (size_t)M * sizeof(float4);
  const int use_lds = corr_bytes <= RS_LDS_CORR_BYTES ? 1 : 0;  // beyond: the records are read through L2
  const size_t lds = use_lds ? corr_bytes : 0;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)ransac_score_kernel<Model, T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GFC_ERR_LAUNCH;
  hipLaunchKernelGGL((ransac_score_kernel<Model, T>), dim3(B * f.S), dim3(EM_THREADS), lds, f.st, f.corr, f.cnt, stream_id,
                     seed, M, f.S, NH, use_lds, a, f.part_score, f.part_idx);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

// the scoring kernel of T thresholds
template <class Model>
static int rs_score(int T, const rs_frame& f, const long long* stream_id, unsigned long long seed, int B, int M, int NH,
                    const typename Model::args& a) {
  switch (T) {
    case 1: return rs_launch_score<Model, 1>(f, stream_id, seed, B, M, NH, a);
    case 2: return rs_launch_score<Model, 2>(f, stream_id, seed, B, M, NH, a);
    case 3: return rs_launch_score<Model, 3>(f, stream_id, seed, B, M, NH, a);
    case 4: return rs_launch_score<Model, 4>(f, stream_id, seed, B, M, NH, a);
    case 5: return rs_launch_score<Model, 5>(f, stream_id, seed, B, M, NH, a);
    case 6: return rs_launch_score<Model, 6>(f, stream_id, seed, B, M, NH, a);
    case 7: return rs_launch_score<Model, 7>(f, stream_id, seed, B, M, NH, a);
    default: return rs_launch_score<Model, 8>(f, stream_id, seed, B, M, NH, a);
  }
}
