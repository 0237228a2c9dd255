// Device functions shared by the evaluation kernels (eval_metrics.hip: match metrics + weighted DLT; ransac.hip:
// the robust estimator, whose local optimisation is the same normalised DLT over the inliers).  One copy of the
// fp64 normal-matrix accumulation, the Jacobi eigen-solve and the corner error, so both kernels compute them alike.
#pragma once
#include "common.h"

#define EM_THREADS 256

// LDS of the two match-metric kernels (eval_metrics.hip, eval_pose.hip).  A workgroup of this part has 160 KB in all:
// the dynamic arrays (every key point of the pair) PLUS the kernel's static variables.  Each kernel declares ALL its
// static LDS as one struct, so that the size the launcher counts is tied to the declaration; the dynamic array is
// 16-byte aligned and follows it.  A pair is refused (nothing launched) exactly when the sum exceeds the limit, and the
// launch asks for the dynamic part only.
constexpr size_t EVAL_LDS_LIMIT = 160 * 1024;
constexpr size_t eval_static_lds(size_t bytes) { return (bytes + 15) / 16 * 16; }
struct EmStaticLds { float acc7[7]; };  // eval_matches_kernel: the seven block sums
struct EdStaticLds { float acc[9]; };   // eval_matches_depth_kernel: the nine block sums
constexpr size_t EM_STATIC_LDS = eval_static_lds(sizeof(EmStaticLds));
constexpr size_t ED_STATIC_LDS = eval_static_lds(sizeof(EdStaticLds));
// k01, a0 [M][2], k10, a1 [N][2] floats and min1 [N] ints
inline size_t em_dynamic_lds(int M, int N) { return (size_t)16 * M + (size_t)20 * N; }
// a0, k01 [M][2], a1, k10 [N][2], best1 [N] floats and flag0, min0 [M], flag1, min1 [N] ints
inline size_t ed_dynamic_lds(int M, int N) { return (size_t)24 * M + (size_t)28 * N; }

__device__ __forceinline__ void warp_pt(const float* Hm, float x, float y, float eps, float& ox, float& oy) {
  // to_homogeneous(p) @ H^T then division by (w + eps): einsum order x*H[r][0] + y*H[r][1] + 1*H[r][2]
  const float wx = x * Hm[0] + y * Hm[1] + Hm[2];
  const float wy = x * Hm[3] + y * Hm[4] + Hm[5];
  const float ww = x * Hm[6] + y * Hm[7] + Hm[8];
  ox = wx / (ww + eps);
  oy = wy / (ww + eps);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide sum of NV doubles per thread; result valid in every thread (via LDS)
template <int NV>
__device__ __forceinline__ void block_sum_f64(double* v, double* lds /* [4][NV] */, int tid) {
  const int wave = tid >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const double t = wave_sum_f64(v[q]);
    if ((tid & 63) == 0) lds[wave * NV + q] = t;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = lds[q] + lds[NV + q] + lds[2 * NV + q] + lds[3 * NV + q];
  __syncthreads();
}

// One correspondence (Hartley-normalised (x1, y1) -> (x2, y2), weight w) into the 45 unique entries of the 9x9 normal
// matrix A^T diag(w) A, upper triangle row-major (r <= c); the two design rows are never stored.
__device__ __forceinline__ void dlt_accumulate(double* acc /* [45] */, double w, double x1, double y1, double x2,
                                               double y2) {
  const double rx[9] = {0, 0, 0, -x1, -y1, -1.0, y2 * x1, y2 * y1, y2};
  const double ry[9] = {x1, y1, 1.0, 0, 0, 0, -x2 * x1, -x2 * y1, -x2};
  int q = 0;
#pragma unroll
  for (int r = 0; r < 9; ++r)
#pragma unroll
    for (int c = r; c < 9; ++c) acc[q++] += w * (rx[r] * rx[c] + ry[r] * ry[c]);
}

// ONE thread: eigenvector of the smallest eigenvalue of the normal matrix (cyclic Jacobi in LDS: A, V [81]) and the
// de-normalisation H = T2^-1 (Hn T1), T = [[s,0,-s mx],[0,s,-s my],[0,0,1]].  f [9] row-major, not yet divided by f[8].
__device__ __forceinline__ void dlt_solve(const double* acc /* [45] */, double* A, double* V, double sc_a, double mx0,
                                          double my0, double sc_b, double mx1, double my1, double* f) {
  int q = 0;
  for (int r = 0; r < 9; ++r)
    for (int c = r; c < 9; ++c) { A[r * 9 + c] = acc[q]; A[c * 9 + r] = acc[q]; ++q; }
  for (int r = 0; r < 81; ++r) V[r] = (r % 10 == 0) ? 1.0 : 0.0;
  // cyclic Jacobi: A <- J^T A J, V <- V J
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 9; ++c) { if (r == c) dg += A[r * 9 + c] * A[r * 9 + c]; else off += A[r * 9 + c] * A[r * 9 + c]; }
    if (!(off > 1e-40 * dg)) break;  // also leaves on NaN
    for (int p = 0; p < 8; ++p)
      for (int r = p + 1; r < 9; ++r) {
        const double apq = A[p * 9 + r];
        if (fabs(apq) < 1e-300) continue;
        const double theta = (A[r * 9 + r] - A[p * 9 + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 9; ++k) {  // columns p, r
          const double akp = A[k * 9 + p], akr = A[k * 9 + r];
          A[k * 9 + p] = c * akp - s * akr;
          A[k * 9 + r] = s * akp + c * akr;
        }
        for (int k = 0; k < 9; ++k) {  // rows p, r
          const double apk = A[p * 9 + k], ark = A[r * 9 + k];
          A[p * 9 + k] = c * apk - s * ark;
          A[r * 9 + k] = s * apk + c * ark;
        }
        for (int k = 0; k < 9; ++k) {
          const double vkp = V[k * 9 + p], vkr = V[k * 9 + r];
          V[k * 9 + p] = c * vkp - s * vkr;
          V[k * 9 + r] = s * vkp + c * vkr;
        }
      }
  }
  int best = 0;
  for (int r = 1; r < 9; ++r)
    if (A[r * 9 + r] < A[best * 9 + best]) best = r;
  double h[9];
  for (int r = 0; r < 9; ++r) h[r] = V[r * 9 + best];
  double g[9];
  for (int r = 0; r < 3; ++r) {
    g[r * 3 + 0] = h[r * 3 + 0] * sc_a;
    g[r * 3 + 1] = h[r * 3 + 1] * sc_a;
    g[r * 3 + 2] = -h[r * 3 + 0] * sc_a * mx0 - h[r * 3 + 1] * sc_a * my0 + h[r * 3 + 2];
  }
  for (int c = 0; c < 3; ++c) {
    f[0 * 3 + c] = g[0 * 3 + c] / sc_b + mx1 * g[2 * 3 + c];
    f[1 * 3 + c] = g[1 * 3 + c] / sc_b + my1 * g[2 * 3 + c];
    f[2 * 3 + c] = g[2 * 3 + c];
  }
}

// homography_corner_error (gluefactory/geometry/homography.py:336-342): corners (0,0) (W,0) (W,H) (0,H), plain
// division, mean distance, fp32 like the reference; +inf when not finite.  Hf must be finite.
__device__ __forceinline__ float corner_error(const float* Hf, const float* Hgt /* [9] */, float Wd, float Hd) {
  const float cx[4] = {0.f, Wd, Wd, 0.f}, cy[4] = {0.f, 0.f, Hd, Hd};
  float Hg[9];
  for (int r = 0; r < 9; ++r) Hg[r] = Hgt[r];
  float sum = 0.f;
  for (int k = 0; k < 4; ++k) {
    float ax, ay, gx, gy;
    warp_pt(Hf, cx[k], cy[k], 0.f, ax, ay);
    warp_pt(Hg, cx[k], cy[k], 0.f, gx, gy);
    sum += sqrtf((ax - gx) * (ax - gx) + (ay - gy) * (ay - gy));
  }
  float err = sum / 4.f;
  if (!isfinite(err)) err = INFINITY;
  return err;
}

// ---- cameras, poses and depth sampling (eval_pose.hip) -----------------------------------------------------------------
// Restated in fp32 and in the operation order of the reference (gluefactory/geometry/wrappers.py:407-481, utils.py:92-248,
// depth.py:8-59).  A camera is float[10] = w, h, fx, fy, cx, cy, d0..d3; a pose float[12] = R row-major, t.
struct EpCam { float w, h, fx, fy, cx, cy, d0, d1, d2, d3; };
struct EpPose { float r[9], t[3]; };

__device__ __forceinline__ EpCam ep_load_cam(const float* p) {
  return EpCam{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]};
}
__device__ __forceinline__ EpPose ep_load_pose(const float* p) {
  EpPose T;
#pragma unroll
  for (int i = 0; i < 9; ++i) T.r[i] = p[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) T.t[i] = p[9 + i];
  return T;
}

// Camera.image2cam: pixel -> point on the z = 1 plane.  Only the KB4 fisheye model removes its distortion: Newton on
// theta from theta = |p|, 10 rounds, a point frozen once its own |step| < 1e-12 (undistort_points_fisheye_kb4).
__device__ __forceinline__ void ep_image2cam(const EpCam& c, int model, float x, float y, float& nx, float& ny) {
  nx = (x - c.cx) / c.fx;
  ny = (y - c.cy) / c.fy;
  if (model != GFC_CAM_OPENCV_FISHEYE) return;
  const float theta_d = sqrtf(nx * nx + ny * ny);
  float theta = theta_d;
  bool active = theta_d > 1e-12f;
  for (int it = 0; it < 10; ++it) {
    const float t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
    const float f = theta * (1.0f + c.d0 * t2 + c.d1 * t4 + c.d2 * t6 + c.d3 * t8) - theta_d;
    const float fp = 1.0f + 3.0f * c.d0 * t2 + 5.0f * c.d1 * t4 + 7.0f * c.d2 * t6 + 9.0f * c.d3 * t8;
    const float step = f / fp;
    if (active) theta = theta - step;
    active = active && (fabsf(step) >= 1e-12f);
  }
  const float scale = theta_d > 1e-12f ? tanf(theta) / theta_d : 1.0f;
  nx *= scale;
  ny *= scale;
}

// Camera.cam2image: project (eps 1e-4, clamp), distort with the model's validity, denormalise, 0 <= p <= size - 1.
__device__ __forceinline__ bool ep_cam2image(const EpCam& c, int model, float X, float Y, float Z, float& px, float& py) {
  bool ok = Z > 1e-4f;
  const float z = Z < 1e-4f ? 1e-4f : Z;  // clamp(min) that keeps a NaN
  float u = X / z, v = Y / z;
  if (model == GFC_CAM_OPENCV_FISHEYE) {
    const float r = sqrtf(u * u + v * v);
    const float th = atanf(r);
    const float t2 = th * th, t3 = th * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const float theta_d = th + c.d0 * t3 + c.d1 * t5 + c.d2 * t7 + c.d3 * t9;
    const float scale = r > 1e-12f ? theta_d / r : 1.0f;
    u *= scale;
    v *= scale;
    ok = ok && isfinite(u) && isfinite(v);
  } else if (model != GFC_CAM_PINHOLE) {
    const float k1 = c.d0, k2 = c.d1;
    const float r2 = u * u + v * v;
    const float radial = k1 * r2 + k2 * (r2 * r2);
    float du = u + u * radial, dv = v + v * radial;
    // beyond the inflection point of r + k1 r^3 + k2 r^5 the model maps far points back into the image
    const float disc = 9.f * (k1 * k1) - 20.f * k2;
    const bool limited = (k2 > 0.f && disc > 0.f) || (k2 <= 0.f && k1 > 0.f);
    if (limited) {
      const float limit = fabsf(k2 > 0.f ? (sqrtf(disc) - 3.f * k1) / (10.f * k2) : 1.f / (3.f * k1));
      ok = ok && (r2 < limit);
    }
    if (model == GFC_CAM_OPENCV) {
      const float p1 = c.d2, p2 = c.d3, uv = u * v;
      du = du + 2.f * p1 * uv + p2 * (r2 + 2.f * (u * u));
      dv = dv + 2.f * p2 * uv + p1 * (r2 + 2.f * (v * v));
    }
    u = du;
    v = dv;
  }
  px = u * c.fx + c.cx;
  py = v * c.fy + c.cy;
  return ok && px >= 0.f && px <= c.w - 1.f && py >= 0.f && py <= c.h - 1.f;
}

// sample_depth: holes (<= 0) are NaN; bilinear grid_sample(align_corners=False, zero padding) at p / (W, H) * 2 - 1
// (a corner outside the map adds nothing, a hole inside it makes the sum NaN whatever its weight); where that is NaN,
// the nearest sample (round half to even, 0 outside).  H, W > 0.
__device__ __forceinline__ float ep_depth_at(const float* __restrict__ depth, int H, int W, float fx, float fy,
                                             bool& inside) {
  inside = fx >= 0.f && fx <= (float)(W - 1) && fy >= 0.f && fy <= (float)(H - 1);
  if (!inside) return 0.f;
  const float d = depth[(size_t)(int)fy * W + (int)fx];
  return d > 0.f ? d : NAN;
}

__device__ __forceinline__ float ep_sample_depth(const float* __restrict__ depth, int H, int W, float x, float y,
                                                 bool& valid) {
  const float gx = x / (float)W * 2.f - 1.f, gy = y / (float)H * 2.f - 1.f;
  const float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f, iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
  const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.f, y1 = y0 + 1.f;
  float lin = 0.f;
  bool in;
  float d = ep_depth_at(depth, H, W, x0, y0, in);
  if (in) lin += d * ((x1 - ix) * (y1 - iy));
  d = ep_depth_at(depth, H, W, x1, y0, in);
  if (in) lin += d * ((ix - x0) * (y1 - iy));
  d = ep_depth_at(depth, H, W, x0, y1, in);
  if (in) lin += d * ((x1 - ix) * (iy - y0));
  d = ep_depth_at(depth, H, W, x1, y1, in);
  if (in) lin += d * ((ix - x0) * (iy - y0));
  if (isnan(lin)) lin = ep_depth_at(depth, H, W, rintf(ix), rintf(iy), in);  // 0 outside
  valid = !isnan(lin) && lin > 0.f;
  return lin;
}

// sample_depth + project(ccth=None) for one key point of view i: depth, its validity, the pixel in view j, visibility.
__device__ __forceinline__ void ep_project_point(const float* __restrict__ depth_i, int Hi, int Wi, const EpCam& ci,
                                                 int model_i, const EpCam& cj, int model_j, const EpPose& T, float x,
                                                 float y, float& d, bool& valid, float& px, float& py, bool& visible) {
  d = ep_sample_depth(depth_i, Hi, Wi, x, y, valid);
  float nx, ny;
  ep_image2cam(ci, model_i, x, y, nx, ny);
  const float a = nx * d, b = ny * d, c = 1.0f * d;
  const float X = a * T.r[0] + b * T.r[1] + c * T.r[2] + T.t[0];
  const float Y = a * T.r[3] + b * T.r[4] + c * T.r[5] + T.t[1];
  const float Z = a * T.r[6] + b * T.r[7] + c * T.r[8] + T.t[2];
  visible = ep_cam2image(cj, model_j, X, Y, Z, px, py) && valid;
}

// block-wide sums of NV floats per thread (EM_THREADS threads): wave shuffle, then LDS atomics; acc [NV] in LDS holds
// the totals after the call, visible to every thread
template <int NV>
__device__ __forceinline__ void block_sum_f32(const float* v, float* acc, int tid) {
  if (tid < NV) acc[tid] = 0.f;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const float t = wave_sum(v[q]);
    if ((tid & 63) == 0) atomicAdd(&acc[q], t);
  }
  __syncthreads();
}
