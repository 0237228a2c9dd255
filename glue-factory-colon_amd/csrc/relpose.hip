// Robust relative pose on the GPU: five-point RANSAC with MSAC scoring at T thresholds at once, cheirality vote and a
// Gauss-Newton local optimisation on the Sampson residual.  Counterpart of the estimators behind
// eval_relative_pose_robust (reference gluefactory/eval/utils.py:188-222; there OpenCV / PoseLib / pycolmap on the CPU
// -- randomised third-party code, parity with them is unpinned).  The algorithm is written down in DESIGN.md ("Robust
// relative pose"); a float64 restatement of it is tests/relpose_reference.py; the arithmetic is relpose_solver.h.  The
// RANSAC frame -- sampler, compaction, ranges, workspace, scoring kernel, reductions, inlier epilogue, argument checks
// -- is ransac_common.h; this file holds what is the relative pose's own:
//
//   relpose_bearings_kernel   the records through ep_image2cam of their own camera, in place: (u0, v0, u1, v1).
//   rp_model                  the model of the frame: sample of five -> five-point solve (fp64; the 10x20 matrix and the
//                             Sturm chain are per-lane scratch) -> <= 10 models per hypothesis, packed index 16 h + k,
//                             squared Sampson distance, pixel thresholds scaled by the pair's cameras.
//   relpose_lo_kernel         one workgroup per (pair, threshold): merge the ranges, re-solve the winner, decompose,
//                             cheirality vote, up to lo_iters Gauss-Newton rounds, outputs.
#include "ransac_common.h"
#include "relpose_solver.h"

#define RP_WORK_DOUBLES (200 + 121)
#define RP_SOLVE_DOUBLES (RP_WORK_DOUBLES + RP_MAX_SOL * 9)  // the workspace slice of one (pair, threshold) block

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

// the relative pose as a model of the frame (ransac_common.h); args.th holds the thresholds in pixels
struct rp_model {
  static constexpr int K = 5, MAX_SOL = RP_MAX_SOL;
  struct args { rs_thresholds th; const float* cam0; const float* cam1; };
  struct work { double d[RP_WORK_DOUBLES]; };
  static __device__ __forceinline__ int pack(int h, int k) { return h * 16 + k; }
  static __device__ __forceinline__ double t2(const args& a, int b, int t) {
    return rp_t2(a.th.v[t], a.cam0 + (size_t)b * 10, a.cam1 + (size_t)b * 10);
  }
  static __device__ __forceinline__ int solve(const float4* corr, unsigned long long key, int h, int n, work& w,
                                              double* m, bool* ok) {
    return rp_hypothesis(corr, key, h, n, w.d, m, ok);
  }
  static __device__ __forceinline__ double residual2(const double* E, double x0, double y0, double x1, double y1) {
    return rp_sampson2(E, x0, y0, x1, y1);
  }
};

__global__ __launch_bounds__(EM_THREADS) void relpose_lo_kernel(
    const float4* __restrict__ corr_all, const int* __restrict__ cidx_all, const int* __restrict__ cnt,
    const long long* __restrict__ m0, const long long* __restrict__ stream_id, const float* __restrict__ cam0,
    const float* __restrict__ cam1, const float* __restrict__ T_gt, unsigned long long seed, int M, int N, int S, int T,
    int lo_iters, rs_thresholds th, double ignore_gt_t_thr, const double* __restrict__ part_score,
    const int* __restrict__ part_idx, double* __restrict__ solve_ws, double* __restrict__ R_out,
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
  const double t2 = rp_t2(rs_pick(th, t), cam0 + (size_t)b * 10, cam1 + (size_t)b * 10);
  const int bhk = n >= 5 ? rs_merge_ranges(part_score, part_idx, b, S, T, t) : -1;  // 16 h + k
  // thread 0 re-solves the winner (its matrix in the block's slice of the workspace)
  if (tid == 0) {
    int flag = 0;
    if (bhk >= 0) {
      const unsigned long long key = rs_pair_key(seed, stream_id, b);
      double* work = solve_ws + o * (size_t)RP_SOLVE_DOUBLES;
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
  double cur_score = rs_block_msac<rp_model>(cur, corr, n, t2, red, tid);
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
    if (!rs_lo_accept<rp_model>(cand, cur_score, corr, n, t2, red, tid)) break;
#pragma unroll
    for (int e = 0; e < 9; ++e) { R[e] = Rc[e]; cur[e] = cand[e]; }
#pragma unroll
    for (int e = 0; e < 3; ++e) tv[e] = tc[e];
  }
  const int ninl = rs_write_inliers<rp_model>(cur, corr, cidx, mm, inl, n, M, N, t2, red, tid);
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
    ninl_out[o] = ninl;
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
  return rs_workspace_bytes(B, M, T, num_hypotheses, RP_SOLVE_DOUBLES * sizeof(double));
}

extern "C" int gfc_eval_relative_pose_ransac(const float* kp0, const float* kp1, const int64_t* m0,
                                             const int64_t* stream_id, const float* cam0, int model0, const float* cam1,
                                             int model1, const float* T_gt, int B, int M, int N, const float* thresholds,
                                             int T, int num_hypotheses, int lo_iters, uint64_t seed,
                                             double ignore_gt_t_thr, double* R_out, double* t_out, double* E_out,
                                             double* E_minimal, uint8_t* inliers, int32_t* num_inliers, uint8_t* success,
                                             int32_t* best_hypothesis, int32_t* best_solution, double* r_err,
                                             double* t_err, void* ws, size_t ws_bytes, void* stream) {
  if (num_hypotheses > (0x7fffffff >> 4)) return GFC_ERR_INVALID;  // (h, k) is packed into one int
  if (model0 < GFC_CAM_PINHOLE || model0 > GFC_CAM_OPENCV_FISHEYE || model1 < GFC_CAM_PINHOLE ||
      model1 > GFC_CAM_OPENCV_FISHEYE)
    return GFC_ERR_INVALID;
  if (!cam0 || !cam1 || !R_out || !t_out || !E_out || !E_minimal || !best_solution) return GFC_ERR_INVALID;
  if ((T_gt == nullptr) != (r_err == nullptr) || (T_gt == nullptr) != (t_err == nullptr)) return GFC_ERR_INVALID;
  if (!(ignore_gt_t_thr >= 0.0)) return GFC_ERR_INVALID;
  if (B > 65535) return GFC_ERR_INVALID;  // pairs are the y dimension of the bearings grid
  rs_frame f;
  const int rc = rs_begin(kp0, kp1, m0, B, M, N, thresholds, T, num_hypotheses, lo_iters, inliers, num_inliers, success,
                          best_hypothesis, RP_SOLVE_DOUBLES * sizeof(double), ws, ws_bytes, stream, f);
  if (rc != GFC_OK) return rc;
  if (M > 0) {
    hipLaunchKernelGGL(relpose_bearings_kernel, dim3((M + EM_THREADS - 1) / EM_THREADS, B), dim3(EM_THREADS), 0, f.st,
                       f.corr, f.cnt, cam0, model0, cam1, model1, M);
    GFC_LAUNCH_CHECK();
  }
  const rp_model::args a = {f.th, cam0, cam1};
  const long long* sid = (const long long*)stream_id;
  const int rs = rs_score<rp_model>(T, f, sid, (unsigned long long)seed, B, M, num_hypotheses, a);
  if (rs != GFC_OK) return rs;
  hipLaunchKernelGGL(relpose_lo_kernel, dim3(B * T), dim3(EM_THREADS), 0, f.st, f.corr, f.cidx, f.cnt, (const long long*)m0,
                     sid, cam0, cam1, T_gt, (unsigned long long)seed, M, N, f.S, T, lo_iters, f.th, ignore_gt_t_thr,
                     f.part_score, f.part_idx, (double*)f.tail, R_out, t_out, E_out, E_minimal, inliers, num_inliers,
                     success, best_hypothesis, best_solution, r_err, t_err);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
