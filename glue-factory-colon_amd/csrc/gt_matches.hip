// Ground-truth matches for the validation pass: gt_matches_from_homography (reference gluefactory/geometry/
// gt_generation.py:730-801) and the matching part of gt_matches_from_pose_depth (gt_generation.py:666-727, with epi_th)
// in full -- both views, masks, independent pos_th / neg_th, and on request the dense assignment / reward.
//
// gt_matches_kernel: one workgroup per pair, every key point of the pair in LDS, the M x N distance matrix never stored.
// A row sweep and a column sweep keep (min, argmin) of the MASKED distance and the min of the UNMASKED one-way distance
// per key point in registers (the arg-min rule of gt_sweep.h, one thread walking the whole row); a third pass gives the
// verdicts.  With a fundamental matrix a fourth pass is the
// epi_th rule: a row / column minimum of the symmetric epipolar distance over ignore x ignore, again never stored.
// The two projections come from a homography (computed here) or from pose and depth (given: gfc_eval_pose_project or
// gt_project_kernel).  No static LDS: the dynamic region is all there is.
// LDS = 21 (M + N) bytes <= 160 KB: M + N <= 7801 is admitted, 3901 x 3901 is the first square shape refused.
// gt_dense_kernel: plain writes of assignment / reward, one thread per element, gridded over (column blocks, rows, B).
#include "gt_sweep.h"
#include "../../include/gfc_amd_validation.h"

#define GT_THREADS 1024  // 16 waves on the one CU a pair occupies: four per SIMD to hide the LDS latency of the sweeps

// r0 [M] float4 = (kp0 projected into image 1, kp0), c1 [N] float4 = (kp1, kp1 projected into image 0): one 128-bit LDS
// read per distance; min0 [M], min1 [N] ints; then the two flag byte rows v0 [M], v1 [N]
inline size_t gt_dynamic_lds(int M, int N) { return (size_t)21 * M + (size_t)21 * N; }
// flag bytes: the key point takes part in the masked distance (valid mask of the homography matcher, `visible` of the
// depth matcher) / it is `negative` (its smallest UNMASKED one-way distance exceeds neg_th^2 and it may be: GT_MAY_NEG) /
// its smallest masked distance is below pos_th^2 / it may be negative (the same mask for a homography, `valid` depth
// for the depth matcher) / its match is `ignore` before the epi_th rule
enum : unsigned char { GT_VALID = 1, GT_NEGATIVE = 2, GT_BELOW_POS = 4, GT_MAY_NEG = 8, GT_IGNORE = 16 };

__global__ __launch_bounds__(GT_THREADS) void gt_matches_kernel(
    const float* __restrict__ kp0, const float* __restrict__ kp1, const float* __restrict__ H,
    const float* __restrict__ Hinv, const float* __restrict__ proj_in01, const float* __restrict__ proj_in10,
    const unsigned char* __restrict__ mask0, const unsigned char* __restrict__ mask1,
    const unsigned char* __restrict__ mayneg0, const unsigned char* __restrict__ mayneg1,
    const float* __restrict__ Fm, float epi_th, int M, int N, float pos2, float neg2, long long* __restrict__ m0_out,
    long long* __restrict__ m1_out, float* __restrict__ proj01, float* __restrict__ proj10,
    int* __restrict__ positive0) {
  extern __shared__ __attribute__((aligned(16))) float4 sm4[];
  float4* r0 = sm4;      // [M] (k01.x, k01.y, kp0.x, kp0.y); k01 = kp0 in image 1
  float4* c1 = r0 + M;   // [N] (kp1.x, kp1.y, k10.x, k10.y); k10 = kp1 in image 0
  int* min0 = reinterpret_cast<int*>(c1 + N);  // [M] argmin over the columns of the masked distance
  int* min1 = min0 + M;                        // [N] argmin over its rows
  unsigned char* v0 = reinterpret_cast<unsigned char*>(min1 + N);  // [M]
  unsigned char* v1 = v0 + M;                                      // [N]
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* p0 = kp0 + (size_t)b * M * 2;
  const float* p1 = kp1 + (size_t)b * N * 2;
  float Hm[9], Hi[9];
  if (H) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { Hm[i] = H[b * 9 + i]; Hi[i] = Hinv[b * 9 + i]; }
  }
  for (int i = tid; i < M; i += GT_THREADS) {
    const size_t g = (size_t)b * M + i;
    const float x = p0[2 * i], y = p0[2 * i + 1];
    float wx, wy;
    if (H) {  // warp_points_torch, eps 1e-5
      warp_pt(Hm, x, y, 1e-5f, wx, wy);
      proj01[2 * g] = wx; proj01[2 * g + 1] = wy;
    } else {
      wx = proj_in01[2 * g]; wy = proj_in01[2 * g + 1];
    }
    r0[i] = make_float4(wx, wy, x, y);
    const bool in_mask = mask0 ? (mask0[g] != 0) : true;
    const bool may_neg = mayneg0 ? (mayneg0[g] != 0) : in_mask;
    v0[i] = (in_mask ? GT_VALID : 0) | (may_neg ? GT_MAY_NEG : 0);
  }
  for (int j = tid; j < N; j += GT_THREADS) {
    const size_t g = (size_t)b * N + j;
    const float x = p1[2 * j], y = p1[2 * j + 1];
    float wx, wy;
    if (H) {
      warp_pt(Hi, x, y, 1e-5f, wx, wy);
      proj10[2 * g] = wx; proj10[2 * g + 1] = wy;
    } else {
      wx = proj_in10[2 * g]; wy = proj_in10[2 * g + 1];
    }
    c1[j] = make_float4(x, y, wx, wy);
    const bool in_mask = mask1 ? (mask1[g] != 0) : true;
    const bool may_neg = mayneg1 ? (mayneg1[g] != 0) : in_mask;
    v1[j] = (in_mask ? GT_VALID : 0) | (may_neg ? GT_MAY_NEG : 0);
  }
  __syncthreads();
  // column sweep: reads the mask bit of every row, adds the two flags of its own column afterwards
  for (int j = tid; j < N; j += GT_THREADS) {
    const float4 c = c1[j];
    const unsigned char fj = v1[j];
    const bool vj = fj & GT_VALID;
    float best = INFINITY, best_d1 = INFINITY;
    int bi = 0;
    for (int i = 0; i < M; ++i) {
      const float4 r = r0[i];
      float d0, d1;
      gt_pair_dists(r, c, d0, d1);
      const float d = (vj && (v0[i] & GT_VALID)) ? fmaxf(d0, d1) : INFINITY;
      if (d < best) { best = d; bi = i; }
      best_d1 = fminf(best_d1, d1);
    }
    min1[j] = bi;
    v1[j] = fj | ((best_d1 > neg2 && (fj & GT_MAY_NEG)) ? GT_NEGATIVE : 0) | (best < pos2 ? GT_BELOW_POS : 0);
  }
  __syncthreads();  // the row sweep reads v1 of every column and rewrites v0 of its own row
  for (int i = tid; i < M; i += GT_THREADS) {
    const float4 r = r0[i];
    const unsigned char fi = v0[i];
    const bool vi = fi & GT_VALID;
    float best = INFINITY, best_d0 = INFINITY;
    int bj = 0;
    for (int j = 0; j < N; ++j) {
      const float4 c = c1[j];
      float d0, d1;
      gt_pair_dists(r, c, d0, d1);
      const float d = (vi && (v1[j] & GT_VALID)) ? fmaxf(d0, d1) : INFINITY;
      if (d < best) { best = d; bj = j; }
      best_d0 = fminf(best_d0, d0);
    }
    min0[i] = bj;
    v0[i] = fi | ((best_d0 > neg2 && (fi & GT_MAY_NEG)) ? GT_NEGATIVE : 0) | (best < pos2 ? GT_BELOW_POS : 0);
  }
  __syncthreads();
  // verdicts.  positive.any(-1) of row i: the one column ismin0 marks there (min0[i]) is marked by ismin1 too, and
  // dist[i, min0[i]] -- the row minimum -- is below pos_th^2.  negative overrides positive in matches.
  for (int i = tid; i < M; i += GT_THREADS) {
    const int bj = min0[i];
    const bool positive = gt_mutual_positive(v0[i] & GT_BELOW_POS, min1, bj, i);
    const long long m = (v0[i] & GT_NEGATIVE) ? -1 : (positive ? bj : -2);
    m0_out[(size_t)b * M + i] = m;
    if (positive0) positive0[(size_t)b * M + i] = positive ? bj : -1;
    if (m == -2) v0[i] |= GT_IGNORE;
  }
  for (int j = tid; j < N; j += GT_THREADS) {
    const int bi = min1[j];
    const bool positive = gt_mutual_positive(v1[j] & GT_BELOW_POS, min0, bi, j);
    const long long m = (v1[j] & GT_NEGATIVE) ? -1 : (positive ? bi : -2);
    m1_out[(size_t)b * N + j] = m;
    if (m == -2) v1[j] |= GT_IGNORE;
  }
  if (!Fm) return;  // uniform
  // epi_th (gt_generation.py:705-712): a point without valid depth -- always `ignore` so far: a match needs it visible,
  // `negative` needs its depth valid -- becomes unmatched when its smallest symmetric epipolar distance to the ignored
  // points of the other image exceeds epi_th (+inf when there is none).  The flags are not touched any more.
  __syncthreads();
  float Ff[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) Ff[q] = Fm[b * 9 + q];
  for (int i = tid; i < M; i += GT_THREADS) {
    if (v0[i] & GT_MAY_NEG) continue;
    const float4 r = r0[i];
    float best = INFINITY;
    if (v0[i] & GT_IGNORE)
      for (int j = 0; j < N; ++j)
        if (v1[j] & GT_IGNORE) best = fminf(best, gt_epi_dist(Ff, r.z, r.w, c1[j].x, c1[j].y));
    if (best > epi_th) m0_out[(size_t)b * M + i] = -1;
  }
  for (int j = tid; j < N; j += GT_THREADS) {
    if (v1[j] & GT_MAY_NEG) continue;
    const float4 c = c1[j];
    float best = INFINITY;
    if (v1[j] & GT_IGNORE)
      for (int i = 0; i < M; ++i)
        if (v0[i] & GT_IGNORE) best = fminf(best, gt_epi_dist(Ff, r0[i].z, r0[i].w, c.x, c.y));
    if (best > epi_th) m1_out[(size_t)b * N + j] = -1;
  }
}

// assignment[b, i, j] = (positive0[b, i] == j); reward on the masked distance, recomputed from the projections.
// Homography (Fm null): reward = (dist < pos_th^2) - (dist > neg_th^2).  Pose and depth: reward = (dist < pos_th^2) -
// (epi > epi_val), epi the symmetric epipolar distance -- with epi_th set (masked_epi) it is +inf outside ignore x ignore
// of the matches BEFORE the epi_th rule: final -2, or final -1 without valid depth.  blockIdx = (column block, row, pair).
__global__ __launch_bounds__(EM_THREADS) void gt_dense_kernel(
    const float* __restrict__ kp0, const float* __restrict__ kp1, const float* __restrict__ proj01,
    const float* __restrict__ proj10, const unsigned char* __restrict__ mask0,
    const unsigned char* __restrict__ mask1, const unsigned char* __restrict__ mayneg0,
    const unsigned char* __restrict__ mayneg1, const long long* __restrict__ m0, const long long* __restrict__ m1,
    const float* __restrict__ Fm, float epi_val, int masked_epi, const int* __restrict__ positive0, int M, int N,
    float pos2, float neg2, unsigned char* __restrict__ assignment, float* __restrict__ reward) {
  const int j = blockIdx.x * EM_THREADS + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
  if (j >= N) return;
  const size_t r = (size_t)b * M + i, c = (size_t)b * N + j;
  const size_t o = r * N + j;
  if (assignment) assignment[o] = positive0[r] == j;
  if (!reward) return;
  float d0, d1;
  gt_pair_dists(gt_coords(kp0, proj01, 0, r), gt_coords(kp1, proj10, 1, c), d0, d1);
  const bool vis = (!mask0 || mask0[r]) && (!mask1 || mask1[c]);
  const float d = vis ? fmaxf(d0, d1) : INFINITY;
  float penalty;
  if (!Fm) {
    penalty = d > neg2 ? 1.f : 0.f;
  } else {
    float Ff[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Ff[q] = Fm[b * 9 + q];
    float e = gt_epi_dist(Ff, kp0[2 * r], kp0[2 * r + 1], kp1[2 * c], kp1[2 * c + 1]);
    if (masked_epi) {
      const bool ig0 = m0[r] == -2 || (m0[r] == -1 && !mayneg0[r]);
      const bool ig1 = m1[c] == -2 || (m1[c] == -1 && !mayneg1[c]);
      if (!(ig0 && ig1)) e = INFINITY;
    }
    penalty = e > epi_val ? 1.f : 0.f;
  }
  reward[o] = (d < pos2 ? 1.f : 0.f) - penalty;
}

// project() of the reference (geometry/depth.py) for key points whose depth is GIVEN (the cached-depth input of the
// depth matcher): image2cam, the depth, the pose, cam2image; visible = valid depth and a valid projection.
__global__ __launch_bounds__(EM_THREADS) void gt_project_kernel(
    const float* __restrict__ kp, const float* __restrict__ depth_kp, const unsigned char* __restrict__ valid,
    const float* __restrict__ cam_i, int model_i, const float* __restrict__ cam_j, int model_j,
    const float* __restrict__ T_itoj, int K, float* __restrict__ proj, unsigned char* __restrict__ visible) {
  const int b = blockIdx.x;
  const EpCam ci = ep_load_cam(cam_i + (size_t)b * 10), cj = ep_load_cam(cam_j + (size_t)b * 10);
  const EpPose T = ep_load_pose(T_itoj + (size_t)b * 12);
  for (int i = threadIdx.x; i < K; i += EM_THREADS) {
    const size_t g = (size_t)b * K + i;
    const float d = depth_kp[g];
    float nx, ny, px, py;
    ep_image2cam(ci, model_i, kp[2 * g], kp[2 * g + 1], nx, ny);
    const float a = nx * d, bb = ny * d, c = 1.0f * d;
    const float X = a * T.r[0] + bb * T.r[1] + c * T.r[2] + T.t[0];
    const float Y = a * T.r[3] + bb * T.r[4] + c * T.r[5] + T.t[1];
    const float Z = a * T.r[6] + bb * T.r[7] + c * T.r[8] + T.t[2];
    const bool ok = ep_cam2image(cj, model_j, X, Y, Z, px, py) && valid[g] != 0;
    proj[2 * g] = px;
    proj[2 * g + 1] = py;
    visible[g] = ok ? 1 : 0;
  }
}

extern "C" size_t gfc_gt_matches_homography_lds_bytes(int M, int N) {
  return (M < 0 || N < 0) ? 0 : gt_dynamic_lds(M, N);
}

static int gt_launch(const float* kp0, const float* kp1, const float* H, const float* Hinv, const float* in01,
                     const float* in10, const uint8_t* mask0, const uint8_t* mask1, const uint8_t* mayneg0,
                     const uint8_t* mayneg1, const float* F, int use_epi, double epi_th, int B, int M, int N,
                     double pos_th, double neg_th, int64_t* matches0, int64_t* matches1, float* proj01, float* proj10,
                     int32_t* positive0, uint8_t* assignment, float* reward, hipStream_t s) {
  const size_t lds = gt_dynamic_lds(M, N);
  if (lds > EVAL_LDS_LIMIT) return GFC_ERR_UNSUPPORTED;
  static std::atomic<unsigned long long> lds_ok{0};
  if (lds > 64 * 1024 && !gfc_allow_dynamic_lds((const void*)gt_matches_kernel, EVAL_LDS_LIMIT, lds_ok)) {
    (void)hipGetLastError();
    return GFC_ERR_LAUNCH;
  }
  // the reference squares the Python double and compares the float32 tensor with it: the double square, rounded once
  const float pos2 = (float)(pos_th * pos_th), neg2 = (float)(neg_th * neg_th);
  hipLaunchKernelGGL(gt_matches_kernel, dim3(B), dim3(GT_THREADS), lds, s, kp0, kp1, H, Hinv, in01, in10, mask0, mask1,
                     mayneg0, mayneg1, use_epi ? F : nullptr, (float)epi_th, M, N, pos2, neg2, (long long*)matches0,
                     (long long*)matches1, proj01, proj10, positive0);
  GFC_LAUNCH_CHECK();
  if (assignment || reward) {
    hipLaunchKernelGGL(gt_dense_kernel, dim3((N + EM_THREADS - 1) / EM_THREADS, M, B), dim3(EM_THREADS), 0, s, kp0, kp1,
                       H ? proj01 : in01, H ? proj10 : in10, mask0, mask1, mayneg0, mayneg1,
                       (const long long*)matches0, (const long long*)matches1, F, (float)(use_epi ? epi_th : neg_th),
                       use_epi, positive0, M, N, pos2, neg2, assignment, reward);
    GFC_LAUNCH_CHECK();
  }
  return GFC_OK;
}

extern "C" int gfc_gt_matches_homography(const float* kp0, const float* kp1, const float* H, const float* Hinv,
                                         const uint8_t* valid0, const uint8_t* valid1, int B, int M, int N,
                                         double pos_th, double neg_th, int64_t* matches0, int64_t* matches1,
                                         float* proj_0to1, float* proj_1to0, int32_t* positive0, uint8_t* assignment,
                                         float* reward, void* stream) {
  if (B <= 0 || M < 0 || N < 0 || B > 65535 || M > 65535) return GFC_ERR_INVALID;
  if (M == 0 || N == 0)
    return gt_empty_side(B, M, N, matches0, matches1, positive0, nullptr, nullptr, nullptr, nullptr, nullptr,
                         (hipStream_t)stream);
  if (!kp0 || !kp1 || !H || !Hinv || !matches0 || !matches1 || !proj_0to1 || !proj_1to0) return GFC_ERR_INVALID;
  if (assignment && !positive0) return GFC_ERR_INVALID;
  return gt_launch(kp0, kp1, H, Hinv, nullptr, nullptr, valid0, valid1, nullptr, nullptr, nullptr, 0, 0.0, B, M, N,
                   pos_th, neg_th, matches0, matches1, proj_0to1, proj_1to0, positive0, assignment, reward,
                   (hipStream_t)stream);
}

extern "C" int gfc_gt_matches_depth(const float* kp0, const float* kp1, const float* proj_0to1, const float* proj_1to0,
                                    const uint8_t* visible0, const uint8_t* visible1, const uint8_t* valid0,
                                    const uint8_t* valid1, const float* F, int B, int M, int N, double pos_th,
                                    double neg_th, double epi_th, int64_t* matches0, int64_t* matches1,
                                    int32_t* positive0, uint8_t* assignment, float* reward, void* stream) {
  if (B <= 0 || M < 0 || N < 0 || B > 65535 || M > 65535) return GFC_ERR_INVALID;
  if (M == 0 || N == 0)
    return gt_empty_side(B, M, N, matches0, matches1, positive0, nullptr, nullptr, nullptr, nullptr, nullptr,
                         (hipStream_t)stream);
  if (!kp0 || !kp1 || !proj_0to1 || !proj_1to0 || !visible0 || !visible1 || !valid0 || !valid1 || !matches0 || !matches1)
    return GFC_ERR_INVALID;
  const int use_epi = epi_th >= 0.0;
  if ((use_epi || reward) && !F) return GFC_ERR_INVALID;
  if (assignment && !positive0) return GFC_ERR_INVALID;
  return gt_launch(kp0, kp1, nullptr, nullptr, proj_0to1, proj_1to0, visible0, visible1, valid0, valid1, F, use_epi,
                   epi_th, B, M, N, pos_th, neg_th, matches0, matches1, nullptr, nullptr, positive0, assignment, reward,
                   (hipStream_t)stream);
}

extern "C" int gfc_gt_project_depth(const float* kp, const float* depth_kp, const uint8_t* valid, const float* cam_i,
                                    int model_i, const float* cam_j, int model_j, const float* T_itoj, int B, int K,
                                    float* proj, uint8_t* visible, void* stream) {
  if (!cam_i || !cam_j || !T_itoj || B <= 0 || K < 0 || model_i < GFC_CAM_PINHOLE || model_i > GFC_CAM_OPENCV_FISHEYE ||
      model_j < GFC_CAM_PINHOLE || model_j > GFC_CAM_OPENCV_FISHEYE ||
      (K > 0 && (!kp || !depth_kp || !valid || !proj || !visible)))
    return GFC_ERR_INVALID;
  if (K == 0) return GFC_OK;
  hipLaunchKernelGGL(gt_project_kernel, dim3(B), dim3(EM_THREADS), 0, (hipStream_t)stream, kp, depth_kp, valid, cam_i,
                     model_i, cam_j, model_j, T_itoj, K, proj, visible);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
