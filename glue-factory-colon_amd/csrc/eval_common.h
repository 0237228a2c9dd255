// Device functions shared by the evaluation kernels (eval_metrics.hip: match metrics + weighted DLT; ransac.hip:
// the robust estimator, whose local optimisation is the same normalised DLT over the inliers).  One copy of the
// fp64 normal-matrix accumulation, the Jacobi eigen-solve and the corner error, so both kernels compute them alike.
#pragma once
#include "common.h"

#define EM_THREADS 256

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
