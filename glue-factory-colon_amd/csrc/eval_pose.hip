// Pose / depth match metrics on the GPU: what the reference's pose benchmarks (megadepth1500, scannet1500, eth3d,
// endomapper_dense1500) score matches with.
//
// Replaces eval_matches_depth and eval_matches_epipolar (reference gluefactory/eval/utils.py:45-138) with their helpers
// symmetric_reprojection_error / sample_depth / project (geometry/depth.py), gt_matches_from_pose_depth with
// epi_th = cc_th = None (geometry/gt_generation.py:594-727), generalized_epi_dist (geometry/epipolar.py:32-85) and the
// camera models of geometry/wrappers.py (PINHOLE, RADIAL, OPENCV, OPENCV_FISHEYE = KB4).  The per-point arithmetic is
// in eval_common.h.  One workgroup per pair, no workspace: projections, flags and argmins of a pair live in LDS, and
// the M x N distance matrix is never materialised (a column sweep and a row sweep keep running (min, argmin) per key
// point in registers; the first index wins ties, like torch.min).
#include "eval_common.h"

#define EP_VALID 1    // the key point has a valid sampled depth
#define EP_VISIBLE 2  // ... and projects to a valid pixel of the other view
#define EP_NANPROJ 4  // its projection is NaN: every distance to it is NaN, and min() of its row is NaN

__global__ __launch_bounds__(EM_THREADS) void eval_pose_project_kernel(
    const float* __restrict__ kp, const float* __restrict__ depth_i, const float* __restrict__ cam_i, int model_i,
    const float* __restrict__ cam_j, int model_j, const float* __restrict__ T_itoj, int K, int Hi, int Wi,
    float* __restrict__ depth_kp, uint8_t* __restrict__ valid_out, float* __restrict__ proj,
    uint8_t* __restrict__ visible_out) {
  const int b = blockIdx.x;
  const EpCam ci = ep_load_cam(cam_i + (size_t)b * 10), cj = ep_load_cam(cam_j + (size_t)b * 10);
  const EpPose T = ep_load_pose(T_itoj + (size_t)b * 12);
  const float* dep = depth_i + (size_t)b * Hi * Wi;
  for (int i = threadIdx.x; i < K; i += EM_THREADS) {
    const size_t g = (size_t)b * K + i;
    float d, px, py;
    bool valid, visible;
    ep_project_point(dep, Hi, Wi, ci, model_i, cj, model_j, T, kp[2 * g], kp[2 * g + 1], d, valid, px, py, visible);
    depth_kp[g] = d;
    valid_out[g] = valid ? 1 : 0;
    proj[2 * g] = px;
    proj[2 * g + 1] = py;
    visible_out[g] = visible ? 1 : 0;
  }
}

__global__ __launch_bounds__(EM_THREADS) void eval_matches_depth_kernel(
    const float* __restrict__ kp0, const float* __restrict__ kp1, const long long* __restrict__ m0,
    const float* __restrict__ depth0, const float* __restrict__ depth1, const float* __restrict__ cam0, int model0,
    const float* __restrict__ cam1, int model1, const float* __restrict__ T01, const float* __restrict__ T10, int M,
    int N, int H0, int W0, int H1, int W1, float pos_th, float neg_th, float* __restrict__ out,
    long long* __restrict__ gt_m0_out, long long* __restrict__ gt_m1_out) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* a0 = sm;                                       // [M][2] kp0
  float* k01 = a0 + 2 * M;                              // [M][2] kp0 projected into view 1
  float* a1 = k01 + 2 * M;                              // [N][2] kp1
  float* k10 = a1 + 2 * N;                              // [N][2] kp1 projected into view 0
  float* best1 = k10 + 2 * N;                           // [N] min over rows of the masked distance
  int* flag0 = reinterpret_cast<int*>(best1 + N);       // [M] EP_* bits
  int* flag1 = flag0 + M;                               // [N]; after the column sweep also bit 8: negative
  int* min0 = flag1 + N;                                // [M] argmin over columns
  int* min1 = min0 + M;                                 // [N] argmin over rows
  __shared__ EdStaticLds st;
  float* acc = st.acc;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* p0 = kp0 + (size_t)b * M * 2;
  const float* p1 = kp1 + (size_t)b * N * 2;
  const long long* mm = m0 + (size_t)b * M;
  const EpCam c0 = ep_load_cam(cam0 + (size_t)b * 10), c1 = ep_load_cam(cam1 + (size_t)b * 10);
  const float pos2 = pos_th * pos_th, neg2 = neg_th * neg_th;
  {
    const EpPose T = ep_load_pose(T01 + (size_t)b * 12);
    const float* dep = depth0 + (size_t)b * H0 * W0;
    for (int i = tid; i < M; i += EM_THREADS) {
      const float x = p0[2 * i], y = p0[2 * i + 1];
      float d, px, py;
      bool valid, visible;
      ep_project_point(dep, H0, W0, c0, model0, c1, model1, T, x, y, d, valid, px, py, visible);
      a0[2 * i] = x; a0[2 * i + 1] = y;
      k01[2 * i] = px; k01[2 * i + 1] = py;
      flag0[i] = (valid ? EP_VALID : 0) | (visible ? EP_VISIBLE : 0) | ((isnan(px) || isnan(py)) ? EP_NANPROJ : 0);
    }
  }
  {
    const EpPose T = ep_load_pose(T10 + (size_t)b * 12);
    const float* dep = depth1 + (size_t)b * H1 * W1;
    for (int j = tid; j < N; j += EM_THREADS) {
      const float x = p1[2 * j], y = p1[2 * j + 1];
      float d, px, py;
      bool valid, visible;
      ep_project_point(dep, H1, W1, c1, model1, c0, model0, T, x, y, d, valid, px, py, visible);
      a1[2 * j] = x; a1[2 * j + 1] = y;
      k10[2 * j] = px; k10[2 * j + 1] = py;
      flag1[j] = (valid ? EP_VALID : 0) | (visible ? EP_VISIBLE : 0) | ((isnan(px) || isnan(py)) ? EP_NANPROJ : 0);
    }
  }
  __syncthreads();
  // column sweep: argmin_i of the masked max(d0, d1), and min_i d1 WITHOUT the mask for the negatives of view 1
  for (int j = tid; j < N; j += EM_THREADS) {
    const float x1 = a1[2 * j], y1 = a1[2 * j + 1], xb = k10[2 * j], yb = k10[2 * j + 1];
    const int fj = flag1[j];
    float best = INFINITY, best_d1 = INFINITY;
    int bi = 0;
    for (int i = 0; i < M; ++i) {
      const float dx0 = k01[2 * i] - x1, dy0 = k01[2 * i + 1] - y1;
      const float dx1 = a0[2 * i] - xb, dy1 = a0[2 * i + 1] - yb;
      const float d1 = dx1 * dx1 + dy1 * dy1;
      const float d = (fj & flag0[i] & EP_VISIBLE) ? fmaxf(dx0 * dx0 + dy0 * dy0, d1) : INFINITY;
      if (d < best) { best = d; bi = i; }
      best_d1 = fminf(best_d1, d1);
    }
    min1[j] = bi;
    best1[j] = best;
    const bool negative = (fj & EP_VALID) && !(fj & EP_NANPROJ) && best_d1 > neg2;
    flag1[j] = fj | (negative ? 8 : 0);
  }
  __syncthreads();
  // row sweep + per-row verdicts
  float s[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < M; i += EM_THREADS) {
    const float x0 = a0[2 * i], y0 = a0[2 * i + 1], xa = k01[2 * i], ya = k01[2 * i + 1];
    const int fi = flag0[i];
    float best = INFINITY, best_d0 = INFINITY;
    int bj = 0;
    for (int j = 0; j < N; ++j) {
      const float dx0 = xa - a1[2 * j], dy0 = ya - a1[2 * j + 1];
      const float dx1 = x0 - k10[2 * j], dy1 = y0 - k10[2 * j + 1];
      const float d0 = dx0 * dx0 + dy0 * dy0;
      const float d = (fi & flag1[j] & EP_VISIBLE) ? fmaxf(d0, dx1 * dx1 + dy1 * dy1) : INFINITY;
      if (d < best) { best = d; bj = j; }
      best_d0 = fminf(best_d0, d0);
    }
    min0[i] = bj;
    long long gt = -2;  // ignore
    if (N > 0 && min1[bj] == i && best < pos2) gt = bj;
    if ((fi & EP_VALID) && !(fi & EP_NANPROJ) && best_d0 > neg2) gt = -1;  // unmatched
    if (N == 0) gt = -1;
    if (gt_m0_out) gt_m0_out[(size_t)b * M + i] = gt;
    const long long m = mm[i];
    if (m > -1) s[0] += 1.f;
    if (m > -1 && m < N) {
      // symmetric reprojection error of the predicted match: the projections are the ones already in LDS
      if (fi & flag1[m] & EP_VALID) {
        const float ex = xa - a1[2 * m], ey = ya - a1[2 * m + 1];
        const float fx = k10[2 * m] - x0, fy = k10[2 * m + 1] - y0;
        float err = 0.5f * (sqrtf(ex * ex + ey * ey) + sqrtf(fx * fx + fy * fy));
        if (isnan(err)) err = INFINITY;
        s[1] += 1.f;
        s[2] += err < 1.f ? 1.f : 0.f;
        s[3] += err < 3.f ? 1.f : 0.f;
        s[4] += err < 5.f ? 1.f : 0.f;
      }
    }
    if (gt > -1) { s[5] += 1.f; s[6] += (m == gt) ? 1.f : 0.f; }
    if (m > -1 && gt >= -1) { s[7] += 1.f; s[8] += (m == gt) ? 1.f : 0.f; }
  }
  block_sum_f32<9>(s, acc, tid);  // its barriers also publish min0
  if (gt_m1_out) {
    for (int j = tid; j < N; j += EM_THREADS) {
      long long gt = -2;
      if (M > 0 && min0[min1[j]] == j && best1[j] < pos2) gt = min1[j];
      if (flag1[j] & 8) gt = -1;
      if (M == 0) gt = -1;
      gt_m1_out[(size_t)b * N + j] = gt;
    }
  }
  if (tid == 0) {
    float* o = out + (size_t)b * 7;
    const float nm = acc[0], nv = acc[1];
    o[0] = nv > 0.f ? acc[2] / nv : 0.f;           // reproj_prec@1px (mean over covisible matches, nan -> 0)
    o[1] = nv > 0.f ? acc[3] / nv : 0.f;           // reproj_prec@3px
    o[2] = nv > 0.f ? acc[4] / nv : 0.f;           // reproj_prec@5px
    o[3] = nv;                                     // covisible
    o[4] = nm > 0.f ? (nv / nm) * 100.f : 0.f;     // covisible_percent
    o[5] = acc[6] / (1e-8f + acc[5]);              // gt_match_recall
    o[6] = acc[8] / (1e-8f + acc[7]);              // gt_match_precision
  }
}

__global__ __launch_bounds__(EM_THREADS) void eval_matches_epipolar_kernel(
    const float* __restrict__ kp0, const float* __restrict__ kp1, const long long* __restrict__ m0,
    const float* __restrict__ cam0, int model0, const float* __restrict__ cam1, int model1,
    const float* __restrict__ T01, int M, int N, float* __restrict__ out) {
  __shared__ float acc[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* p0 = kp0 + (size_t)b * M * 2;
  const float* p1 = kp1 + (size_t)b * N * 2;
  const long long* mm = m0 + (size_t)b * M;
  const EpCam c0 = ep_load_cam(cam0 + (size_t)b * 10), c1 = ep_load_cam(cam1 + (size_t)b * 10);
  const EpPose T = ep_load_pose(T01 + (size_t)b * 12);
  // E = [t]x R, the zero entries of the skew matrix multiplied out like the matrix product does
  const float S[9] = {0.f, -T.t[2], T.t[1], T.t[2], 0.f, -T.t[0], -T.t[1], T.t[0], 0.f};
  float E[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) E[r * 3 + c] = S[r * 3] * T.r[c] + S[r * 3 + 1] * T.r[3 + c] + S[r * 3 + 2] * T.r[6 + c];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < M; i += EM_THREADS) {
    const long long m = mm[i];
    if (m > -1) s[0] += 1.f;
    if (m > -1 && m < N) {
      float ax, ay, bx, by;
      ep_image2cam(c0, model0, p0[2 * i], p0[2 * i + 1], ax, ay);
      ep_image2cam(c1, model1, p1[2 * m], p1[2 * m + 1], bx, by);
      const float e0 = E[0] * ax + E[1] * ay + E[2], e1 = E[3] * ax + E[4] * ay + E[5], e2 = E[6] * ax + E[7] * ay + E[8];
      const float g0 = E[0] * bx + E[3] * by + E[6], g1 = E[1] * bx + E[4] * by + E[7];
      const float num = fabsf(bx * e0 + by * e1 + e2);
      const float d0 = fmaxf(e0 * e0 + e1 * e1, 1e-6f), d1 = fmaxf(g0 * g0 + g1 * g1, 1e-6f);
      const float d = num * (1.f / sqrtf(d0) + 1.f / sqrtf(d1)) / 2.f;
      s[1] += d < 1e-4f ? 1.f : 0.f;
      s[2] += d < 5e-4f ? 1.f : 0.f;
      s[3] += d < 1e-3f ? 1.f : 0.f;
    }
  }
  block_sum_f32<4>(s, acc, tid);
  if (tid == 0) {
    float* o = out + (size_t)b * 5;
    const float nm = acc[0];
    o[0] = nm > 0.f ? acc[1] / nm : 0.f;  // epi_prec@1e-4
    o[1] = nm > 0.f ? acc[2] / nm : 0.f;  // epi_prec@5e-4
    o[2] = nm > 0.f ? acc[3] / nm : 0.f;  // epi_prec@1e-3
    o[3] = nm;                            // num_matches
    o[4] = (M + N) / 2.f;                 // num_keypoints
  }
}

static bool ep_model_ok(int m) { return m >= GFC_CAM_PINHOLE && m <= GFC_CAM_OPENCV_FISHEYE; }

extern "C" int gfc_eval_pose_project(const float* kp, const float* depth_i, const float* cam_i, int model_i,
                                     const float* cam_j, int model_j, const float* T_itoj, int B, int K, int Hi, int Wi,
                                     float* depth_kp, uint8_t* valid, float* proj, uint8_t* visible, void* stream) {
  if (!depth_i || !cam_i || !cam_j || !T_itoj || B <= 0 || K < 0 || Hi <= 0 || Wi <= 0 || !ep_model_ok(model_i) ||
      !ep_model_ok(model_j) || (K > 0 && (!kp || !depth_kp || !valid || !proj || !visible)))
    return GFC_ERR_INVALID;
  if (K == 0) return GFC_OK;  // nothing to write
  hipLaunchKernelGGL(eval_pose_project_kernel, dim3(B), dim3(EM_THREADS), 0, (hipStream_t)stream, kp, depth_i, cam_i,
                     model_i, cam_j, model_j, T_itoj, K, Hi, Wi, depth_kp, valid, proj, visible);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

extern "C" size_t gfc_eval_matches_depth_lds_bytes(int M, int N) {
  return (M < 0 || N < 0) ? 0 : ed_dynamic_lds(M, N) + ED_STATIC_LDS;
}

extern "C" int gfc_eval_matches_depth(const float* kp0, const float* kp1, const int64_t* matches0, const float* depth0,
                                      const float* depth1, const float* cam0, int model0, const float* cam1, int model1,
                                      const float* T_0to1, const float* T_1to0, int B, int M, int N, int H0, int W0,
                                      int H1, int W1, float pos_th, float neg_th, float* out, int64_t* gt_matches0,
                                      int64_t* gt_matches1, void* stream) {
  // an empty side has no array to point at: its pointers may be NULL
  if (!depth0 || !depth1 || !cam0 || !cam1 || !T_0to1 || !T_1to0 || !out || B <= 0 || M < 0 || N < 0 || H0 <= 0 ||
      W0 <= 0 || H1 <= 0 || W1 <= 0 || !ep_model_ok(model0) || !ep_model_ok(model1) ||
      (M > 0 && (!kp0 || !matches0)) || (N > 0 && !kp1))
    return GFC_ERR_INVALID;
  const size_t lds = ed_dynamic_lds(M, N);  // the dynamic arrays only: the launch adds the static ones itself
  if (lds + ED_STATIC_LDS > EVAL_LDS_LIMIT) return GFC_ERR_UNSUPPORTED;
  static std::atomic<unsigned long long> lds_ok{0};
  if (lds > 64 * 1024 &&
      !gfc_allow_dynamic_lds((const void*)eval_matches_depth_kernel, EVAL_LDS_LIMIT - ED_STATIC_LDS, lds_ok)) {
    (void)hipGetLastError();
    return GFC_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(eval_matches_depth_kernel, dim3(B), dim3(EM_THREADS), lds, (hipStream_t)stream, kp0, kp1,
                     (const long long*)matches0, depth0, depth1, cam0, model0, cam1, model1, T_0to1, T_1to0, M, N, H0,
                     W0, H1, W1, pos_th, neg_th, out, (long long*)gt_matches0, (long long*)gt_matches1);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

extern "C" int gfc_eval_matches_epipolar(const float* kp0, const float* kp1, const int64_t* matches0, const float* cam0,
                                         int model0, const float* cam1, int model1, const float* T_0to1, int B, int M,
                                         int N, float* out, void* stream) {
  if (!cam0 || !cam1 || !T_0to1 || !out || B <= 0 || M < 0 || N < 0 || !ep_model_ok(model0) || !ep_model_ok(model1) ||
      (M > 0 && (!kp0 || !matches0)) || (N > 0 && !kp1))
    return GFC_ERR_INVALID;
  hipLaunchKernelGGL(eval_matches_epipolar_kernel, dim3(B), dim3(EM_THREADS), 0, (hipStream_t)stream, kp0, kp1,
                     (const long long*)matches0, cam0, model0, cam1, model1, T_0to1, M, N, out);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
