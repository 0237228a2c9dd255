// Robust relative pose on the GPU: five-point RANSAC with MSAC scoring at T thresholds at once, cheirality vote and a
// Gauss-Newton local optimisation on the Sampson residual.  Counterpart of the estimators behind
// eval_relative_pose_robust (reference gluefactory/eval/utils.py:188-222; there OpenCV / PoseLib / pycolmap on the CPU
// -- randomised third-party code, parity with them is unpinned).  The algorithm is written down in DESIGN.md ("Robust
// relative pose"); a float64 restatement of it is tests/relpose_reference.py; the arithmetic is relpose_solver.h.
//
//   ransac_compact_kernel     (ransac.hip) the matches in ascending i -> (x0, y0, x1, y1) records, their index, n.
//   relpose_bearings_kernel   the records through ep_image2cam of their own camera, in place: (u0, v0, u1, v1).
//   relpose_score_kernel<T>   one workgroup per (pair, hypothesis range): records staged in LDS, ONE LANE PER
//                             HYPOTHESIS: counter-based sample of five -> five-point solve (fp64; the 10x20 matrix and
//                             the Sturm chain are per-lane scratch) -> for each of its <= 10 models the T MSAC sums of
//                             the squared Sampson distance in correspondence order -> (score, h, k) argmin.
//   relpose_lo_kernel         one workgroup per (pair, threshold): merge the ranges, re-solve the winner, decompose,
//                             cheirality vote, up to lo_iters Gauss-Newton rounds, outputs.
// A model's score is one lane's serial sum and the winner is chosen by (score, h, k): the result does not depend on the
// number of ranges, the batch or the launch shape.
#include "ransac_common.h"
#include "relpose_solver.h"

#define RP_WORK_DOUBLES (200 + 121)

struct rp_thresholds { double th[RS_MAX_T]; };

// threshold in normalised units: pixels / mean(fx0, fy0, fx1, fy1), squared
__device__ __forceinline__ double rp_t2(double th_px, const float* cam0, const float* cam1) {
  const double fm = (((double)cam0[2] + (double)cam0[3]) + ((double)cam1[2] + (double)cam1[3])) * 0.25;
  const double t = th_px / fm;
  return t * t;
}

__global__ __launch_bounds__(EM_THREADS) void relpose_bearings_kernel(float4* __restrict__ corr_all,
                                                                      const int* __restrict__ cnt,
                                                                      const float* __restrict__ cam0, int model0,
                                                                      const float* __restrict__ cam1, int model1, int M) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * EM_THREADS + threadIdx.x;
  if (c >= cnt[b] || c >= M) return;
  const EpCam c0 = ep_load_cam(cam0 + (size_t)b * 10), c1 = ep_load_cam(cam1 + (size_t)b * 10);
  float4 q = corr_all[(size_t)b * M + c];
  float u0, v0, u1, v1;
  ep_image2cam(c0, model0, q.x, q.y, u0, v0);
  ep_image2cam(c1, model1, q.z, q.w, u1, v1);
  corr_all[(size_t)b * M + c] = make_float4(u0, v0, u1, v1);
}

// Camera.image2cam of K points per pair, the device function the estimator's records go through
__global__ __launch_bounds__(EM_THREADS) void relpose_image2cam_kernel(const float* __restrict__ kp,
                                                                       const float* __restrict__ cam, int model, int K,
                                                                       float* __restrict__ out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * EM_THREADS + threadIdx.x;
  if (i >= K) return;
  const EpCam c = ep_load_cam(cam + (size_t)b * 10);
  const size_t o = ((size_t)b * K + i) * 2;
  float u, v;
  ep_image2cam(c, model, kp[o], kp[o + 1], u, v);
  out[o] = u;
  out[o + 1] = v;
}

// the five sampled records of hypothesis h -> its models
__device__ __forceinline__ int rp_hypothesis(const float4* corr, unsigned long long key, int h, int n, double* work,
                                             double* Es, bool* ok) {
  int idx[5];
  rs_sample_k<5>(key, h, n, idx);
  double rec[20];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const float4 q = corr[idx[j]];
    rec[4 * j] = q.x; rec[4 * j + 1] = q.y; rec[4 * j + 2] = q.z; rec[4 * j + 3] = q.w;
  }
  return rp_five_point(rec, work, Es, ok);
}

// (h, k) as one ordered integer
__device__ __forceinline__ int rp_pack(int h, int k) { return h * 16 + k; }

template <int T>
__device__ __forceinline__ void rp_score_range(const float4* corr, int n, unsigned long long key, int h_lo, int h_hi,
                                               const double* t2, double* best, int* best_hk) {
#pragma unroll
  for (int t = 0; t < T; ++t) { best[t] = INFINITY; best_hk[t] = 0x7fffffff; }
  double work[RP_WORK_DOUBLES], Es[RP_MAX_SOL * 9];
  bool ok[RP_MAX_SOL];
  for (int h = h_lo + (int)threadIdx.x; h < h_hi; h += EM_THREADS) {
    const int ns = rp_hypothesis(corr, key, h, n, work, Es, ok);
    for (int k = 0; k < ns; ++k) {
      if (!ok[k]) continue;
      double E[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) E[e] = Es[k * 9 + e];
      double acc[T];
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = 0.0;
      for (int c = 0; c < n; ++c) {
        const float4 q = corr[c];  // the same address in every lane of a wave whose lanes are all here
        const double r2 = rp_sampson2(E, q.x, q.y, q.z, q.w);
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] += (r2 < t2[t]) ? r2 : t2[t];
      }
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (acc[t] < best[t]) { best[t] = acc[t]; best_hk[t] = rp_pack(h, k); }
    }
  }
}

template <int T>
__global__ __launch_bounds__(EM_THREADS) void relpose_score_kernel(const float4* __restrict__ corr_all,
                                                                   const int* __restrict__ cnt,
                                                                   const long long* __restrict__ stream_id,
                                                                   const float* __restrict__ cam0,
                                                                   const float* __restrict__ cam1,
                                                                   unsigned long long seed, int M, int S, int NH,
                                                                   int use_lds, rp_thresholds th,
                                                                   double* __restrict__ part_score,
                                                                   int* __restrict__ part_hk) {
  extern __shared__ __attribute__((aligned(16))) float4 lds_corr[];
  __shared__ double ws[4 * RS_MAX_T];
  __shared__ int wh[4 * RS_MAX_T];
  const int b = blockIdx.x / S, s = blockIdx.x % S, tid = threadIdx.x;
  const int n = cnt[b];
  const float4* corr = corr_all + (size_t)b * M;
  double* ps = part_score + (size_t)blockIdx.x * T;
  int* ph = part_hk + (size_t)blockIdx.x * T;
  if (n < 5) {
    if (tid < T) { ps[tid] = INFINITY; ph[tid] = -1; }
    return;
  }
  const unsigned long long key = rs_key(seed, stream_id ? (unsigned long long)stream_id[b] : (unsigned long long)b);
  const int chunk = (NH + S - 1) / S;
  const int h_lo = s * chunk, h_hi = min(NH, h_lo + chunk);
  double t2[T];
#pragma unroll
  for (int t = 0; t < T; ++t) t2[t] = rp_t2(th.th[t], cam0 + (size_t)b * 10, cam1 + (size_t)b * 10);
  double best[T];
  int best_hk[T];
  if (use_lds) {
    for (int c = tid; c < n; c += EM_THREADS) lds_corr[c] = corr[c];
    __syncthreads();
    rp_score_range<T>(lds_corr, n, key, h_lo, h_hi, t2, best, best_hk);
  } else {
    rp_score_range<T>(corr, n, key, h_lo, h_hi, t2, best, best_hk);
  }
  // argmin over the block by (score, h, k)
#pragma unroll
  for (int t = 0; t < T; ++t) {
    double sc = best[t];
    int hh = best_hk[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(sc, o, 64);
      const int oh = __shfl_xor(hh, o, 64);
      if (os < sc || (os == sc && oh < hh)) { sc = os; hh = oh; }
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
      if (os < sc || (os == sc && oh < hh)) { sc = os; hh = oh; }
    }
    ps[tid] = sc;
    ph[tid] = (sc < INFINITY) ? hh : -1;
  }
}

// MSAC score of E over the n records, block-wide (thread-strided partial sums, then block_sum_f64)
__device__ __forceinline__ double rp_block_msac(const double* E, const float4* corr, int n, double t2, double* red,
                                                int tid) {
  double v[1] = {0.0};
  for (int c = tid; c < n; c += EM_THREADS) {
    const float4 q = corr[c];
    const double r2 = rp_sampson2(E, q.x, q.y, q.z, q.w);
    v[0] += (r2 < t2) ? r2 : t2;
  }
  block_sum_f64<1>(v, red, tid);
  return v[0];
}

__global__ __launch_bounds__(EM_THREADS) void relpose_lo_kernel(
    const float4* __restrict__ corr_all, const int* __restrict__ cidx_all, const int* __restrict__ cnt,
    const long long* __restrict__ m0, const long long* __restrict__ stream_id, const float* __restrict__ cam0,
    const float* __restrict__ cam1, const float* __restrict__ T_gt, unsigned long long seed, int M, int N, int S, int T,
    int lo_iters, rp_thresholds th, double ignore_gt_t_thr, const double* __restrict__ part_score,
    const int* __restrict__ part_hk, double* __restrict__ solve_ws, double* __restrict__ R_out,
    double* __restrict__ t_out, double* __restrict__ E_out, double* __restrict__ Emin_out,
    unsigned char* __restrict__ inl_out, int* __restrict__ ninl_out, unsigned char* __restrict__ success_out,
    int* __restrict__ besth_out, int* __restrict__ bestk_out, double* __restrict__ rerr_out,
    double* __restrict__ terr_out) {
  __shared__ double red[4 * 20];
  __shared__ double sRt[4 * 12];
  __shared__ double sE[9];
  __shared__ double sCand[12];
  __shared__ int sflag;
  const int b = blockIdx.x / T, t = blockIdx.x % T, tid = threadIdx.x;
  const size_t o = blockIdx.x;  // (b, t)
  const int n = cnt[b];
  const float4* corr = corr_all + (size_t)b * M;
  const int* cidx = cidx_all + (size_t)b * M;
  const long long* mm = m0 + (size_t)b * M;
  unsigned char* inl = inl_out + o * M;
  double thv = th.th[0];
#pragma unroll
  for (int q = 1; q < RS_MAX_T; ++q) thv = (q == t) ? th.th[q] : thv;
  const double t2 = rp_t2(thv, cam0 + (size_t)b * 10, cam1 + (size_t)b * 10);
  // winner over the hypothesis ranges: lowest score, ties to the lower (h, k)
  double bs = INFINITY;
  int bhk = -1;
  if (n >= 5)
    for (int s = 0; s < S; ++s) {
      const double os = part_score[((size_t)b * S + s) * T + t];
      const int oh = part_hk[((size_t)b * S + s) * T + t];
      if (oh >= 0 && (os < bs || (os == bs && oh < bhk))) { bs = os; bhk = oh; }
    }
  // thread 0 re-solves the winner (its matrix in the block's slice of the workspace)
  if (tid == 0) {
    int flag = 0;
    if (bhk >= 0) {
      const unsigned long long key = rs_key(seed, stream_id ? (unsigned long long)stream_id[b] : (unsigned long long)b);
      double* work = solve_ws + o * (size_t)(RP_WORK_DOUBLES + RP_MAX_SOL * 9);
      double* Es = work + RP_WORK_DOUBLES;
      bool okk[RP_MAX_SOL];
      const int ns = rp_hypothesis(corr, key, bhk >> 4, n, work, Es, okk);
      const int k = bhk & 15;
      if (k < ns && okk[k]) {
        flag = 1;
        for (int e = 0; e < 9; ++e) sE[e] = Es[k * 9 + e];
        rp_decompose(sE, sRt);
      }
    }
    sflag = flag;
  }
  __syncthreads();
  const bool ok = sflag != 0;
  if (!ok) {  // uniform over the block
    for (int i = tid; i < M; i += EM_THREADS) inl[i] = 0;
    if (tid < 9) {
      R_out[o * 9 + tid] = (tid % 4 == 0) ? 1.0 : 0.0;
      E_out[o * 9 + tid] = 0.0;
      Emin_out[o * 9 + tid] = 0.0;
    }
    if (tid < 3) t_out[o * 3 + tid] = 0.0;
    if (tid == 0) {
      ninl_out[o] = 0; success_out[o] = 0; besth_out[o] = -1; bestk_out[o] = -1;
      if (rerr_out) { rerr_out[o] = INFINITY; terr_out[o] = INFINITY; }
    }
    return;
  }
  double Emin[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) Emin[e] = sE[e];
  // cheirality vote over the inliers of the minimal model
  double votes[4] = {0, 0, 0, 0};
  for (int c = tid; c < n; c += EM_THREADS) {
    const float4 q = corr[c];
    if (rp_sampson2(Emin, q.x, q.y, q.z, q.w) < t2) {
#pragma unroll
      for (int k = 0; k < 4; ++k) votes[k] += rp_cheiral(sRt + 12 * k, sRt + 12 * k + 9, q.x, q.y, q.z, q.w) ? 1.0 : 0.0;
    }
  }
  block_sum_f64<4>(votes, red, tid);
  int win = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (votes[k] > votes[win]) win = k;
  double R[9], tv[3], cur[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) R[e] = sRt[12 * win + e];
#pragma unroll
  for (int e = 0; e < 3; ++e) tv[e] = sRt[12 * win + 9 + e];
  __syncthreads();
  rp_essential(R, tv, cur);
  double cur_score = rp_block_msac(cur, corr, n, t2, red, tid);
  for (int it = 0; it < lo_iters; ++it) {
    double b3[3], b4[3];
    rp_tangent(tv, b3, b4);
    double acc[20];
#pragma unroll
    for (int q = 0; q < 20; ++q) acc[q] = 0.0;
    for (int c = tid; c < n; c += EM_THREADS) {
      const float4 q = corr[c];
      if (rp_sampson2(cur, q.x, q.y, q.z, q.w) < t2) rp_gn_accumulate(acc, R, tv, cur, b3, b4, q.x, q.y, q.z, q.w);
    }
    block_sum_f64<20>(acc, red, tid);
    if (tid == 0) {
      double Rn[9], tn[3];
      for (int e = 0; e < 9; ++e) Rn[e] = R[e];
      for (int e = 0; e < 3; ++e) tn[e] = tv[e];
      const bool fin = rp_gn_update(acc, b3, b4, Rn, tn);
      for (int e = 0; e < 9; ++e) sCand[e] = Rn[e];
      for (int e = 0; e < 3; ++e) sCand[9 + e] = tn[e];
      sflag = fin ? 1 : 0;
    }
    __syncthreads();
    double Rc[9], tc[3], cand[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Rc[e] = sCand[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) tc[e] = sCand[9 + e];
    const int fin = sflag;
    __syncthreads();
    if (!fin) break;
    rp_essential(Rc, tc, cand);
    const double cand_score = rp_block_msac(cand, corr, n, t2, red, tid);
    if (!(cand_score < cur_score)) break;
#pragma unroll
    for (int e = 0; e < 9; ++e) { R[e] = Rc[e]; cur[e] = cand[e]; }
#pragma unroll
    for (int e = 0; e < 3; ++e) tv[e] = tc[e];
    cur_score = cand_score;
  }
  // outputs: inliers in key-point-0 indexing (every i is written exactly once: unmatched rows here, matched rows below)
  for (int i = tid; i < M; i += EM_THREADS) {
    const long long j = mm[i];
    if (!(j > -1 && j < N)) inl[i] = 0;
  }
  double cntv[1] = {0.0};
  for (int c = tid; c < n; c += EM_THREADS) {
    const float4 q = corr[c];
    const bool in = rp_sampson2(cur, q.x, q.y, q.z, q.w) < t2;
    inl[cidx[c]] = in ? 1 : 0;  // cidx[c] < M by construction (ransac_compact_kernel)
    cntv[0] += in ? 1.0 : 0.0;
  }
  block_sum_f64<1>(cntv, red, tid);
  if (tid == 0) {
    // E_minimal: unit norm, its largest-magnitude entry (the first such) positive
    int big = 0;
    for (int e = 1; e < 9; ++e)
      if (fabs(Emin[e]) > fabs(Emin[big])) big = e;
    const double sg = Emin[big] < 0.0 ? -1.0 : 1.0;
    for (int e = 0; e < 9; ++e) {
      R_out[o * 9 + e] = R[e];
      E_out[o * 9 + e] = cur[e];
      Emin_out[o * 9 + e] = sg * Emin[e];
    }
    for (int e = 0; e < 3; ++e) t_out[o * 3 + e] = tv[e];
    ninl_out[o] = (int)cntv[0];
    success_out[o] = 1;
    besth_out[o] = bhk >> 4;
    bestk_out[o] = bhk & 15;
    if (rerr_out) {
      double Rg[9], tg[3], re, te;
      for (int e = 0; e < 9; ++e) Rg[e] = (double)T_gt[(size_t)b * 12 + e];
      for (int e = 0; e < 3; ++e) tg[e] = (double)T_gt[(size_t)b * 12 + 9 + e];
      rp_pose_error(R, tv, Rg, tg, ignore_gt_t_thr, re, te);
      rerr_out[o] = re;
      terr_out[o] = te;
    }
  }
}

// ---- C ABI -------------------------------------------------------------------------------------------------
// hypothesis ranges per pair, as rs_splits of ransac.hip
static int rp_splits(int B, int NH) {
  const int want = (512 + B - 1) / B, most = NH / EM_THREADS;
  return (want < most ? want : most) < 1 ? 1 : (want < most ? want : most);
}

struct rp_layout { size_t corr, cidx, cnt, pscore, ph, solve, total; };
static rp_layout rp_plan(int B, int M, int T, int NH) {
  const size_t S = (size_t)rp_splits(B, NH);
  gfc_slots s;
  return {s.take((size_t)B * M * sizeof(float4)), s.take((size_t)B * M * sizeof(int)), s.take((size_t)B * sizeof(int)),
          s.take((size_t)B * S * T * sizeof(double)), s.take((size_t)B * S * T * sizeof(int)),
          s.take((size_t)B * T * (RP_WORK_DOUBLES + RP_MAX_SOL * 9) * sizeof(double)), s.off};
}

extern "C" int gfc_eval_pose_image2cam(const float* kp, const float* cam, int model, int B, int K, float* out,
                                       void* stream) {
  if (B <= 0 || B > 65535 || K < 0 || model < GFC_CAM_PINHOLE || model > GFC_CAM_OPENCV_FISHEYE || !cam) return GFC_ERR_INVALID;
  if (K == 0) return GFC_OK;
  if (!kp || !out) return GFC_ERR_INVALID;
  hipLaunchKernelGGL(relpose_image2cam_kernel, dim3((K + EM_THREADS - 1) / EM_THREADS, B), dim3(EM_THREADS), 0,
                     (hipStream_t)stream, kp, cam, model, K, out);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

extern "C" size_t gfc_eval_relative_pose_ransac_workspace_bytes(int B, int M, int T, int num_hypotheses) {
  if (B <= 0 || M < 0 || T <= 0 || T > RS_MAX_T || num_hypotheses <= 0) return 0;
  return rp_plan(B, M, T, num_hypotheses).total;
}

template <int T>
static int rp_launch_score(int blocks, size_t lds, hipStream_t st, const float4* corr, const int* cnt,
                           const long long* stream_id, const float* cam0, const float* cam1, unsigned long long seed,
                           int M, int S, int NH, int use_lds, const rp_thresholds& th, double* ps, int* ph) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)relpose_score_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GFC_ERR_LAUNCH;
  hipLaunchKernelGGL(relpose_score_kernel<T>, dim3(blocks), dim3(EM_THREADS), lds, st, corr, cnt, stream_id, cam0, cam1,
                     seed, M, S, NH, use_lds, th, ps, ph);
  return GFC_OK;
}

extern "C" int gfc_eval_relative_pose_ransac(const float* kp0, const float* kp1, const int64_t* m0,
                                             const int64_t* stream_id, const float* cam0, int model0, const float* cam1,
                                             int model1, const float* T_gt, int B, int M, int N, const float* thresholds,
                                             int T, int num_hypotheses, int lo_iters, uint64_t seed,
                                             double ignore_gt_t_thr, double* R_out, double* t_out, double* E_out,
                                             double* E_minimal, uint8_t* inliers, int32_t* num_inliers, uint8_t* success,
                                             int32_t* best_hypothesis, int32_t* best_solution, double* r_err,
                                             double* t_err, void* ws, size_t ws_bytes, void* stream) {
  if (B <= 0 || M < 0 || N < 0 || T <= 0 || T > RS_MAX_T || num_hypotheses <= 0 || lo_iters < 0) return GFC_ERR_INVALID;
  if (num_hypotheses > (0x7fffffff >> 4)) return GFC_ERR_INVALID;  // (h, k) is packed into one int
  if (model0 < GFC_CAM_PINHOLE || model0 > GFC_CAM_OPENCV_FISHEYE || model1 < GFC_CAM_PINHOLE ||
      model1 > GFC_CAM_OPENCV_FISHEYE)
    return GFC_ERR_INVALID;
  // an empty side has nothing to point at: its arrays may be NULL
  if ((M > 0 && (!kp0 || !m0 || !inliers)) || (N > 0 && !kp1) || !cam0 || !cam1 || !thresholds || !R_out || !t_out ||
      !E_out || !E_minimal || !num_inliers || !success || !best_hypothesis || !best_solution || !ws)
    return GFC_ERR_INVALID;
  if ((T_gt == nullptr) != (r_err == nullptr) || (T_gt == nullptr) != (t_err == nullptr)) return GFC_ERR_INVALID;
  if (!(ignore_gt_t_thr >= 0.0)) return GFC_ERR_INVALID;
  if ((size_t)B * (size_t)T > 0x7fffffffull || (size_t)B * (size_t)rp_splits(B, num_hypotheses) > 0x7fffffffull ||
      B > 65535)
    return GFC_ERR_INVALID;
  rp_thresholds th;
  for (int t = 0; t < RS_MAX_T; ++t) {
    const float v = thresholds[t < T ? t : T - 1];
    if (!(v > 0.f) || !(v < INFINITY)) return GFC_ERR_INVALID;
    th.th[t] = (double)v;
  }
  const rp_layout L = rp_plan(B, M, T, num_hypotheses);
  if (ws_bytes < L.total) return GFC_ERR_WORKSPACE;
  char* w = (char*)ws;
  float4* corr = (float4*)(w + L.corr);
  int* cidx = (int*)(w + L.cidx);
  int* cnt = (int*)(w + L.cnt);
  double* ps = (double*)(w + L.pscore);
  int* ph = (int*)(w + L.ph);
  double* solve = (double*)(w + L.solve);
  hipStream_t st = (hipStream_t)stream;
  const int S = rp_splits(B, num_hypotheses);
  const long long* sid = (const long long*)stream_id;
  hipLaunchKernelGGL(ransac_compact_kernel, dim3(B), dim3(EM_THREADS), 0, st, kp0, kp1, (const long long*)m0, M, N, corr,
                     cidx, cnt);
  GFC_LAUNCH_CHECK();
  if (M > 0) {
    hipLaunchKernelGGL(relpose_bearings_kernel, dim3((M + EM_THREADS - 1) / EM_THREADS, B), dim3(EM_THREADS), 0, st, corr,
                       cnt, cam0, model0, cam1, model1, M);
    GFC_LAUNCH_CHECK();
  }
  const size_t corr_bytes = (size_t)M * sizeof(float4);
  const int use_lds = corr_bytes <= RS_LDS_CORR_BYTES ? 1 : 0;  // beyond: the records are read through L2
  const size_t lds = use_lds ? corr_bytes : 0;
  const int blocks = B * S;
  int rc;
#define RP_CASE(TT) \
  case TT: rc = rp_launch_score<TT>(blocks, lds, st, corr, cnt, sid, cam0, cam1, seed, M, S, num_hypotheses, use_lds, th, ps, ph); break;
  switch (T) {
    RP_CASE(1) RP_CASE(2) RP_CASE(3) RP_CASE(4) RP_CASE(5) RP_CASE(6) RP_CASE(7)
    default: rc = rp_launch_score<8>(blocks, lds, st, corr, cnt, sid, cam0, cam1, seed, M, S, num_hypotheses, use_lds, th, ps, ph); break;
  }
#undef RP_CASE
  if (rc != GFC_OK) return rc;
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(relpose_lo_kernel, dim3(B * T), dim3(EM_THREADS), 0, st, corr, cidx, cnt, (const long long*)m0, sid,
                     cam0, cam1, T_gt, (unsigned long long)seed, M, N, S, T, lo_iters, th, ignore_gt_t_thr, ps, ph, solve,
                     R_out, t_out, E_out, E_minimal, inliers, num_inliers, success, best_hypothesis, best_solution, r_err,
                     t_err);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
