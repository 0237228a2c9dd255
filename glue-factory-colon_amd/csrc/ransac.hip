// Robust homography estimation on the GPU: RANSAC with MSAC scoring at T thresholds at once and a local
// optimisation by the normalised DLT of eval_common.h.  Counterpart of the estimators behind eval_homography_robust
// (reference gluefactory/eval/utils.py:225-273; there OpenCV / PoseLib on the CPU -- randomised third-party code,
// parity with them is unpinned).  The algorithm is written down in DESIGN.md ("Robust homography"); a float64
// restatement of it is tests/ransac_reference.py.  The RANSAC frame -- sampler, ranges, workspace, scoring kernel,
// reductions, inlier epilogue, argument checks -- is ransac_common.h; this file holds what is the homography's own:
//
//   ransac_compact_kernel  one workgroup per pair: the matches (i, m0[i]) with 0 <= m0[i] < N in ascending i
//                          -> (x0, y0, x1, y1) records + their key-point-0 index + the count n (both estimators' first
//                          step; declared in ransac_common.h).
//   rs_homography          the model of the frame: sample of 4 -> closed-form 4-point homography (fp64), one model per
//                          hypothesis, packed index h, squared forward transfer error, thresholds squared on the host.
//   ransac_lo_kernel       one workgroup per (pair, threshold): merge the ranges (score, then h), re-solve the winner,
//                          up to lo_iters rounds of {inliers -> DLT -> accept iff the MSAC score drops}, outputs.
#include "block_select.h"
#include "ransac_common.h"

#define RS_DET_EPS 1e-10

// ---- minimal solve ---------------------------------------------------------------------------------------
// twice the signed area of the triangle (a, b, c)
__device__ __forceinline__ double rs_area2(double ax, double ay, double bx, double by, double cx, double cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// Hartley normalisation of 4 points: centroid, mean distance -> sqrt 2 (the scale of find_homography_dlt)
__device__ __forceinline__ void rs_normalise4(const double* x, const double* y, double* u, double* v, double& mx,
                                              double& my, double& s) {
  mx = (((x[0] + x[1]) + x[2]) + x[3]) * 0.25;
  my = (((y[0] + y[1]) + y[2]) + y[3]) * 0.25;
  double d = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double ax = x[k] - mx, ay = y[k] - my;
    d += sqrt(ax * ax + ay * ay);
  }
  s = 1.4142135623730951 / (d * 0.25 + 1e-8);
#pragma unroll
  for (int k = 0; k < 4; ++k) { u[k] = s * (x[k] - mx); v[k] = s * (y[k] - my); }
}

// The projective map that sends the basis e1, e2, e3, (1,1,1) to the four points: columns l_k * (u_k, v_k, 1), with
// l = adj([p1 p2 p3]) p4 (Cramer; the common factor det[p1 p2 p3] is an overall scale).  Returns the smallest of the
// four |triangle areas| (any three points collinear <=> the 8x8 system is singular).
__device__ __forceinline__ double rs_basis(const double* u, const double* v, double* Bm) {
  const double d = rs_area2(u[0], v[0], u[1], v[1], u[2], v[2]);
  const double l0 = rs_area2(u[3], v[3], u[1], v[1], u[2], v[2]);
  const double l1 = rs_area2(u[0], v[0], u[3], v[3], u[2], v[2]);
  const double l2 = rs_area2(u[0], v[0], u[1], v[1], u[3], v[3]);
  Bm[0] = l0 * u[0]; Bm[1] = l1 * u[1]; Bm[2] = l2 * u[2];
  Bm[3] = l0 * v[0]; Bm[4] = l1 * v[1]; Bm[5] = l2 * v[2];
  Bm[6] = l0;        Bm[7] = l1;        Bm[8] = l2;
  return fmin(fmin(fabs(d), fabs(l0)), fmin(fabs(l1), fabs(l2)));
}

// Homography through 4 correspondences (x0, y0) -> (x1, y1), fp64, closed form on Hartley-normalised points:
// Hn = B1 adj(B0), H = T1^-1 Hn T0, divided by H[2][2].  false: singular (three points collinear in either image)
// or a non-finite entry.
__device__ __forceinline__ bool rs_homography_4pt(const double* x0, const double* y0, const double* x1,
                                                  const double* y1, double* H) {
  double u0[4], v0[4], u1[4], v1[4], mx0, my0, s0, mx1, my1, s1, A[9], Bq[9];
  rs_normalise4(x0, y0, u0, v0, mx0, my0, s0);
  rs_normalise4(x1, y1, u1, v1, mx1, my1, s1);
  const double e0 = rs_basis(u0, v0, A);
  const double e1 = rs_basis(u1, v1, Bq);
  double C[9];  // adj(A)
  C[0] = A[4] * A[8] - A[5] * A[7]; C[1] = A[2] * A[7] - A[1] * A[8]; C[2] = A[1] * A[5] - A[2] * A[4];
  C[3] = A[5] * A[6] - A[3] * A[8]; C[4] = A[0] * A[8] - A[2] * A[6]; C[5] = A[2] * A[3] - A[0] * A[5];
  C[6] = A[3] * A[7] - A[4] * A[6]; C[7] = A[1] * A[6] - A[0] * A[7]; C[8] = A[0] * A[4] - A[1] * A[3];
  double h[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) h[r * 3 + c] = (Bq[r * 3] * C[c] + Bq[r * 3 + 1] * C[3 + c]) + Bq[r * 3 + 2] * C[6 + c];
  double g[9], f[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g[r * 3 + 0] = h[r * 3 + 0] * s0;
    g[r * 3 + 1] = h[r * 3 + 1] * s0;
    g[r * 3 + 2] = (h[r * 3 + 2] - g[r * 3 + 0] * mx0) - g[r * 3 + 1] * my0;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f[0 * 3 + c] = g[0 * 3 + c] / s1 + mx1 * g[2 * 3 + c];
    f[1 * 3 + c] = g[1 * 3 + c] / s1 + my1 * g[2 * 3 + c];
    f[2 * 3 + c] = g[2 * 3 + c];
  }
  bool ok = (e0 > RS_DET_EPS) && (e1 > RS_DET_EPS);
  const double inv = 1.0 / f[8];
#pragma unroll
  for (int r = 0; r < 9; ++r) { H[r] = f[r] * inv; ok = ok && isfinite(H[r]); }
  return ok;
}

// squared forward transfer error; +inf when the projective denominator is <= 0 or not finite
__device__ __forceinline__ double rs_residual2(const double* H, double x0, double y0, double x1, double y1) {
  const double X = (H[0] * x0 + H[1] * y0) + H[2];
  const double Y = (H[3] * x0 + H[4] * y0) + H[5];
  const double W = (H[6] * x0 + H[7] * y0) + H[8];
  const double iw = 1.0 / W;
  const double dx = X * iw - x1, dy = Y * iw - y1;
  const double r2 = dx * dx + dy * dy;
  return (W > 0.0 && W < INFINITY) ? r2 : INFINITY;
}

// the four sampled correspondences of hypothesis h -> model
__device__ __forceinline__ bool rs_hypothesis(const float4* corr, unsigned long long key, int h, int n, double* H) {
  int i[4];
  rs_sample_k<4>(key, h, n, i);
  const float4 c0 = corr[i[0]], c1 = corr[i[1]], c2 = corr[i[2]], c3 = corr[i[3]];
  const double x0[4] = {c0.x, c1.x, c2.x, c3.x}, y0[4] = {c0.y, c1.y, c2.y, c3.y};
  const double x1[4] = {c0.z, c1.z, c2.z, c3.z}, y1[4] = {c0.w, c1.w, c2.w, c3.w};
  return rs_homography_4pt(x0, y0, x1, y1, H);
}

// the homography as a model of the frame (ransac_common.h); args.th holds the squared thresholds
struct rs_homography {
  static constexpr int K = 4, MAX_SOL = 1;
  struct args { rs_thresholds th; };
  struct work {};
  static __device__ __forceinline__ int pack(int h, int) { return h; }
  static __device__ __forceinline__ double t2(const args& a, int, int t) { return a.th.v[t]; }
  static __device__ __forceinline__ int solve(const float4* corr, unsigned long long key, int h, int n, work&,
                                              double* m, bool* ok) {
    ok[0] = rs_hypothesis(corr, key, h, n, m);
    return 1;
  }
  static __device__ __forceinline__ double residual2(const double* H, double x0, double y0, double x1, double y1) {
    return rs_residual2(H, x0, y0, x1, y1);
  }
};

// ---- kernels -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EM_THREADS) void ransac_compact_kernel(const float* __restrict__ kp0,
                                                                    const float* __restrict__ kp1,
                                                                    const long long* __restrict__ m0, int M, int N,
                                                                    float4* __restrict__ corr, int* __restrict__ cidx,
                                                                    int* __restrict__ cnt) {
  __shared__ int wsum[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* p0 = kp0 + (size_t)b * M * 2;
  const float* p1 = kp1 + (size_t)b * N * 2;
  const long long* mm = m0 + (size_t)b * M;
  float4* cc = corr + (size_t)b * M;
  int* ci = cidx + (size_t)b * M;
  int base = 0;
  for (int i0 = 0; i0 < M; i0 += EM_THREADS) {
    const int i = i0 + tid;
    long long j = -1;
    if (i < M) j = mm[i];
    const bool valid = (i < M) && j > -1 && j < N;
    int total;
    const int pos = base + gfc_block_rank<EM_THREADS / 64>(valid, wsum, total);  // < M: at most one slot per valid i
    if (valid) {
      cc[pos] = make_float4(p0[2 * i], p0[2 * i + 1], p1[2 * j], p1[2 * j + 1]);
      ci[pos] = i;
    }
    base += total;
  }
  if (tid == 0) cnt[b] = base;
}

__global__ __launch_bounds__(EM_THREADS) void ransac_lo_kernel(
    const float4* __restrict__ corr_all, const int* __restrict__ cidx_all, const int* __restrict__ cnt,
    const long long* __restrict__ m0, const long long* __restrict__ stream_id, unsigned long long seed, int M, int N,
    int S, int T, int lo_iters, rs_thresholds th, const double* __restrict__ part_score,
    const int* __restrict__ part_idx, const float* __restrict__ Hgt, const float* __restrict__ size0,
    double* __restrict__ Hout, unsigned char* __restrict__ inl_out, int* __restrict__ ninl_out,
    unsigned char* __restrict__ success_out, int* __restrict__ besth_out, double* __restrict__ Hmin_out,
    float* __restrict__ err_out) {
  __shared__ double red[4 * 45];
  __shared__ double A[81], V[81];
  __shared__ double sH[9];
  __shared__ int sflag;
  const int b = blockIdx.x / T, t = blockIdx.x % T, tid = threadIdx.x;
  const size_t o = blockIdx.x;  // (b, t)
  const int n = cnt[b];
  const float4* corr = corr_all + (size_t)b * M;
  const int* cidx = cidx_all + (size_t)b * M;
  const long long* mm = m0 + (size_t)b * M;
  unsigned char* inl = inl_out + o * M;
  const double t2 = rs_pick(th, t);  // squared on the host
  const int bh = n >= 4 ? rs_merge_ranges(part_score, part_idx, b, S, T, t) : -1;
  double cur[9];
  bool ok = bh >= 0;
  if (ok) ok = rs_hypothesis(corr, rs_pair_key(seed, stream_id, b), bh, n, cur);
  if (!ok) {  // uniform over the block
    for (int i = tid; i < M; i += EM_THREADS) inl[i] = 0;
    if (tid < 9) { Hout[o * 9 + tid] = (tid % 4 == 0) ? 1.0 : 0.0; Hmin_out[o * 9 + tid] = (tid % 4 == 0) ? 1.0 : 0.0; }
    if (tid == 0) {
      ninl_out[o] = 0; success_out[o] = 0; besth_out[o] = -1;
      if (err_out) err_out[o] = INFINITY;
    }
    return;
  }
  if (tid < 9) Hmin_out[o * 9 + tid] = cur[tid];
  double cur_score = rs_block_msac<rs_homography>(cur, corr, n, t2, red, tid);
  for (int it = 0; it < lo_iters; ++it) {
    // normalised DLT over the inliers of the current model (unit weights), as dlt_kernel
    double s5[5] = {0, 0, 0, 0, 0};
    for (int c = tid; c < n; c += EM_THREADS) {
      const float4 q = corr[c];
      if (rs_residual2(cur, q.x, q.y, q.z, q.w) < t2) { s5[0] += 1.0; s5[1] += q.x; s5[2] += q.y; s5[3] += q.z; s5[4] += q.w; }
    }
    block_sum_f64<5>(s5, red, tid);
    const double ni = s5[0];
    if (ni < 4.0) break;
    const double mx0 = s5[1] / ni, my0 = s5[2] / ni, mx1 = s5[3] / ni, my1 = s5[4] / ni;
    double d2[2] = {0, 0};
    for (int c = tid; c < n; c += EM_THREADS) {
      const float4 q = corr[c];
      if (rs_residual2(cur, q.x, q.y, q.z, q.w) < t2) {
        const double ax = q.x - mx0, ay = q.y - my0, bx = q.z - mx1, by = q.w - my1;
        d2[0] += sqrt(ax * ax + ay * ay);
        d2[1] += sqrt(bx * bx + by * by);
      }
    }
    block_sum_f64<2>(d2, red, tid);
    const double sc_a = 1.4142135623730951 / (d2[0] / ni + 1e-8), sc_b = 1.4142135623730951 / (d2[1] / ni + 1e-8);
    double acc[45];
#pragma unroll
    for (int q = 0; q < 45; ++q) acc[q] = 0.0;
    for (int c = tid; c < n; c += EM_THREADS) {
      const float4 q = corr[c];
      if (rs_residual2(cur, q.x, q.y, q.z, q.w) < t2)
        dlt_accumulate(acc, 1.0, sc_a * (q.x - mx0), sc_a * (q.y - my0), sc_b * (q.z - mx1), sc_b * (q.w - my1));
    }
    block_sum_f64<45>(acc, red, tid);
    if (tid == 0) {
      double f[9];
      dlt_solve(acc, A, V, sc_a, mx0, my0, sc_b, mx1, my1, f);
      const double inv = 1.0 / f[8];
      bool fin = true;
      for (int r = 0; r < 9; ++r) { sH[r] = f[r] * inv; fin = fin && isfinite(sH[r]); }
      sflag = fin ? 1 : 0;
    }
    __syncthreads();
    double cand[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) cand[r] = sH[r];
    const int fin = sflag;
    __syncthreads();
    if (!fin) break;
    if (!rs_lo_accept<rs_homography>(cand, cur_score, corr, n, t2, red, tid)) break;
#pragma unroll
    for (int r = 0; r < 9; ++r) cur[r] = cand[r];
  }
  const int ninl = rs_write_inliers<rs_homography>(cur, corr, cidx, mm, inl, n, M, N, t2, red, tid);
  if (tid == 0) {
    float Hf[9];
    bool fin = true;
    for (int r = 0; r < 9; ++r) { Hf[r] = (float)cur[r]; fin = fin && isfinite(Hf[r]); }
    for (int r = 0; r < 9; ++r) Hout[o * 9 + r] = cur[r];  // fp64, as computed; the corner error is fp32 like dlt_kernel's
    ninl_out[o] = ninl;
    success_out[o] = 1;
    besth_out[o] = bh;
    if (err_out) err_out[o] = fin ? corner_error(Hf, Hgt + (size_t)b * 9, size0[b * 2], size0[b * 2 + 1]) : INFINITY;
  }
}

// ---- C ABI -------------------------------------------------------------------------------------------------
extern "C" size_t gfc_eval_homography_ransac_workspace_bytes(int B, int M, int T, int num_hypotheses) {
  return rs_workspace_bytes(B, M, T, num_hypotheses, 0);
}

extern "C" int gfc_eval_homography_ransac(const float* kp0, const float* kp1, const int64_t* m0,
                                          const int64_t* stream_id, const float* H_gt, const float* image_size0, int B,
                                          int M, int N, const float* thresholds, int T, int num_hypotheses, int lo_iters,
                                          uint64_t seed, double* H_out, uint8_t* inliers, int32_t* num_inliers,
                                          uint8_t* success, int32_t* best_hypothesis, double* H_minimal, float* err_out,
                                          void* ws, size_t ws_bytes, void* stream) {
  if (!H_out || !H_minimal) return GFC_ERR_INVALID;
  if ((H_gt == nullptr) != (image_size0 == nullptr) || (H_gt == nullptr) != (err_out == nullptr)) return GFC_ERR_INVALID;
  rs_frame f;
  const int rc = rs_begin(kp0, kp1, m0, B, M, N, thresholds, T, num_hypotheses, lo_iters, inliers, num_inliers, success,
                          best_hypothesis, 0, ws, ws_bytes, stream, f);
  if (rc != GFC_OK) return rc;
  rs_homography::args a;
  for (int t = 0; t < RS_MAX_T; ++t) a.th.v[t] = f.th.v[t] * f.th.v[t];
  const long long* sid = (const long long*)stream_id;
  const int rs = rs_score<rs_homography>(T, f, sid, (unsigned long long)seed, B, M, num_hypotheses, a);
  if (rs != GFC_OK) return rs;
  hipLaunchKernelGGL(ransac_lo_kernel, dim3(B * T), dim3(EM_THREADS), 0, f.st, f.corr, f.cidx, f.cnt, (const long long*)m0,
                     sid, (unsigned long long)seed, M, N, f.S, T, lo_iters, a.th, f.part_score, f.part_idx, H_gt,
                     image_size0, H_out, inliers, num_inliers, success, best_hypothesis, H_minimal, err_out);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
