// Ground-truth labels from dense warps (RoMa): cycle_dist (reference gluefactory/utils/image.py:260-270), sample_dense
// and the label part of gt_matches_from_roma (gluefactory/geometry/gt_generation.py:127-134, 149-269).  The sampling
// rule, the order of decisions and the launch plan are stated in include/gfc_amd_dense_warp.h.
//
// A pair is split over workgroups by the sweep of gt_sweep.h, which also states the arg-min rule (ties, a row of +inf,
// NaN) and the known difference from the reference.  Here: the samplers, what a RoMa key point brings to that sweep (one
// flag, `valid_pos`, for the masked distance and the one-way minimum alike), the verdicts and the dense outputs.
#include "gt_sweep.h"
#include "../../include/gfc_amd_dense_warp.h"

#define DW_THREADS 256  // every kernel here but the sweep, which has gt_sweep.h's shape

// ---- F.grid_sample(bilinear, zeros, align_corners=False) --------------------------------------------------------------
struct DwTaps {
  float x0, y0, x1, y1;      // tap coordinates, as floats: compared with the field's size before any cast
  float nw, ne, sw, se;      // weights
  bool finite;               // a position that is not finite samples NaN
};

__device__ __forceinline__ DwTaps dw_taps(float cx, float cy, int H, int W) {
  DwTaps t;
  const float ix = ((cx + 1.f) * (float)W - 1.f) / 2.f, iy = ((cy + 1.f) * (float)H - 1.f) / 2.f;
  t.finite = isfinite(ix) && isfinite(iy);
  t.x0 = floorf(ix); t.y0 = floorf(iy);
  t.x1 = t.x0 + 1.f; t.y1 = t.y0 + 1.f;
  t.nw = (t.x1 - ix) * (t.y1 - iy);
  t.ne = (ix - t.x0) * (t.y1 - iy);
  t.sw = (t.x1 - ix) * (iy - t.y0);
  t.se = (ix - t.x0) * (iy - t.y0);
  return t;
}

__device__ __forceinline__ bool dw_inside(float x, float y, int H, int W) {
  return x >= 0.f && x <= (float)(W - 1) && y >= 0.f && y <= (float)(H - 1);
}

// sum of value(x, y) * weight over the taps inside the field, in torch's order; `at` is called for inside taps only
template <class F>
__device__ __forceinline__ float dw_combine(const DwTaps& t, int H, int W, F at) {
  if (!t.finite) return NAN;
  float acc = 0.f;
  if (dw_inside(t.x0, t.y0, H, W)) acc += at((int)t.x0, (int)t.y0) * t.nw;
  if (dw_inside(t.x1, t.y0, H, W)) acc += at((int)t.x1, (int)t.y0) * t.ne;
  if (dw_inside(t.x0, t.y1, H, W)) acc += at((int)t.x0, (int)t.y1) * t.sw;
  if (dw_inside(t.x1, t.y1, H, W)) acc += at((int)t.x1, (int)t.y1) * t.se;
  return acc;
}

// the same for the two channels of a warp, fetched as one float2; per channel the operations of dw_combine
template <class F>
__device__ __forceinline__ float2 dw_combine2(const DwTaps& t, int H, int W, F at) {
  if (!t.finite) return make_float2(NAN, NAN);
  float2 acc = make_float2(0.f, 0.f);
  if (dw_inside(t.x0, t.y0, H, W)) { const float2 v = at((int)t.x0, (int)t.y0); acc.x += v.x * t.nw; acc.y += v.y * t.nw; }
  if (dw_inside(t.x1, t.y0, H, W)) { const float2 v = at((int)t.x1, (int)t.y0); acc.x += v.x * t.ne; acc.y += v.y * t.ne; }
  if (dw_inside(t.x0, t.y1, H, W)) { const float2 v = at((int)t.x0, (int)t.y1); acc.x += v.x * t.sw; acc.y += v.y * t.sw; }
  if (dw_inside(t.x1, t.y1, H, W)) { const float2 v = at((int)t.x1, (int)t.y1); acc.x += v.x * t.se; acc.y += v.y * t.se; }
  return acc;
}

// a warp field [H,W,2] as float2 per pixel (the launchers refuse a pointer that is not 8-byte aligned)
__device__ __forceinline__ float2 dw_warp_at(const float* __restrict__ f, int W, int x, int y) {
  return *(const float2*)(f + 2 * ((size_t)y * W + x));
}

// cycle_dist of pixel (x, y) of q [H,W,2] against r [Hr,Wr,2], both of one pair; 0 <= x < W, 0 <= y < H
__device__ __forceinline__ float dw_cycle_at(const float* __restrict__ q, const float* __restrict__ r, int H, int W,
                                             int Hr, int Wr, int x, int y) {
  const float2 c = dw_warp_at(q, W, x, y);
  const DwTaps t = dw_taps(c.x, c.y, Hr, Wr);
  const float2 s = dw_combine2(t, Hr, Wr, [&](int u, int v) { return dw_warp_at(r, Wr, u, v); });
  const float sx = s.x, sy = s.y;
  // denormalize_coords(hw=None) takes the size from the sampled tensor, which has the shape of q
  const float bx = (sx + 1.f) / 2.f * (float)(W - 1), by = (sy + 1.f) / 2.f * (float)(H - 1);
  const float ex = ((float)x + 0.5f) - bx, ey = ((float)y + 0.5f) - by;
  return sqrtf(ex * ex + ey * ey);
}

__global__ __launch_bounds__(DW_THREADS) void dw_cycle_kernel(const float* __restrict__ q, const float* __restrict__ r,
                                                              float* __restrict__ out, int H, int W, int Hr, int Wr) {
  const size_t p = (size_t)blockIdx.x * DW_THREADS + threadIdx.x, hw = (size_t)H * W;
  if (p >= hw) return;
  const int b = blockIdx.y;
  out[b * hw + p] = dw_cycle_at(q + 2 * b * hw, r + 2 * (size_t)b * Hr * Wr, H, W, Hr, Wr, (int)(p % W), (int)(p / W));
}

// CYCLE 0: cycle_kp = 0; 1: sampled from the field `cyc`; 2: from the cycle error of the tap pixels, computed here
template <int CYCLE>
__global__ __launch_bounds__(DW_THREADS) void dw_sample_kernel(const float* __restrict__ kp,
                                                               const float* __restrict__ warp,
                                                               const float* __restrict__ cert,
                                                               const float* __restrict__ cyc,
                                                               const float* __restrict__ other, int M, int H, int W,
                                                               int Hr, int Wr, float qh1, float qw1, float th1, float tw1,
                                                               float* __restrict__ proj, float* __restrict__ cert_kp,
                                                               float* __restrict__ cyc_kp) {
  const int k = blockIdx.x * DW_THREADS + threadIdx.x, b = blockIdx.y;
  if (k >= M) return;
  const size_t g = (size_t)b * M + k, hw = (size_t)H * W;
  const float* wb = warp + 2 * b * hw;
  const float* cb = cert + b * hw;
  const float cx = kp[2 * g] / qw1 * 2.f - 1.f, cy = kp[2 * g + 1] / qh1 * 2.f - 1.f;
  const DwTaps t = dw_taps(cx, cy, H, W);
  const float2 s = dw_combine2(t, H, W, [&](int u, int v) { return dw_warp_at(wb, W, u, v); });
  proj[2 * g] = (s.x + 1.f) / 2.f * tw1;
  proj[2 * g + 1] = (s.y + 1.f) / 2.f * th1;
  cert_kp[g] = dw_combine(t, H, W, [&](int u, int v) { return cb[(size_t)v * W + u]; });
  float ce = 0.f;
  if (CYCLE == 1) {
    const float* eb = cyc + b * hw;
    ce = dw_combine(t, H, W, [&](int u, int v) { return eb[(size_t)v * W + u]; });
  } else if (CYCLE == 2) {
    const float* ob = other + 2 * (size_t)b * Hr * Wr;
    ce = dw_combine(t, H, W, [&](int u, int v) { return dw_cycle_at(wb, ob, H, W, Hr, Wr, u, v); });
  }
  cyc_kp[g] = ce;
}

// ---- labels -----------------------------------------------------------------------------------------------------------
struct DwSide {  // one image of the batch
  const float* kp;
  const float* proj;
  const float* cert;
  const float* cyc;
  const unsigned char* valid;
  int n;
};
struct DwTh { float pos2, neg2, pos_cert, pos_cyc, neg_cert, neg_cyc; int has_pos_cert, has_pos_cyc, has_unrel; };

// step 1
__device__ __forceinline__ bool dw_valid_pos(const DwSide& s, const DwTh& th, size_t g) {
  const float c = s.cert[g], e = s.cyc[g];
  bool v = s.valid[g] != 0 && isfinite(s.proj[2 * g]) && isfinite(s.proj[2 * g + 1]) && isfinite(c);
  if (th.has_pos_cert) v = v && c > th.pos_cert;
  if (th.has_pos_cyc) v = v && isfinite(e) && e < th.pos_cyc;
  return v;
}

struct DwLabeller {  // for gt_sweep: valid_pos masks the distance and admits a key point to the one-way minimum
  using Side = DwSide;
  const DwTh& th;
  __device__ __forceinline__ unsigned char flags(const DwSide& s, size_t g) const {
    return dw_valid_pos(s, th, g) ? GTS_MASKED : 0;
  }
  static __device__ __forceinline__ bool own_min(unsigned char f) { return f & GTS_MASKED; }
};

__global__ __launch_bounds__(GTS_THREADS) void dw_sweep_kernel(DwSide s0, DwSide s1, DwTh th, int row_blocks, size_t side1,
                                                               GtsOut w) {
  __shared__ __attribute__((aligned(16))) GtsTile tile;
  GtsNoExtra none;
  gt_sweep_pair(DwLabeller{th}, s0, s1, row_blocks, side1, tile, w, none);
}

// Steps 3-8 per key point.  grid (ceil((M + N) / DW_THREADS), B): threads 0..M-1 of a pair are its rows, then its columns.
__global__ __launch_bounds__(DW_THREADS) void dw_finish_kernel(DwSide s0, DwSide s1, DwTh th, size_t side1,
                                                               const float* __restrict__ w_best,
                                                               const int* __restrict__ w_arg,
                                                               const float* __restrict__ w_own,
                                                               unsigned char* __restrict__ w_vp, int* __restrict__ w_pos0,
                                                               long long* __restrict__ m0_out,
                                                               long long* __restrict__ m1_out, float* __restrict__ sc0,
                                                               float* __restrict__ sc1, unsigned char* __restrict__ masks0,
                                                               unsigned char* __restrict__ masks1) {
  const int b = blockIdx.y, M = s0.n, N = s1.n;
  const int t = blockIdx.x * DW_THREADS + threadIdx.x;
  if (t >= M + N) return;
  const int side = t >= M, k = side ? t - M : t;
  const DwSide& me = side ? s1 : s0;
  const DwSide& ot = side ? s0 : s1;
  const size_t g = (size_t)b * me.n + k;                    // in the arrays of the caller
  const size_t w = (side ? side1 : 0) + g;                  // in the workspace
  const size_t wo = (side ? 0 : side1) + (size_t)b * ot.n;  // the other side's key points of this pair in the workspace
  const int a = w_arg[w];
  const int p = gt_mutual_positive(w_best[w] < th.pos2, w_arg + wo, a, k) ? a : -1;
  const bool vp = dw_valid_pos(me, th, g);
  const bool valid = me.valid[g] != 0;
  const float c = me.cert[g], e = me.cyc[g];
  const bool far = vp && w_own[w] > th.neg2;
  const bool unrel = th.has_unrel && valid && isfinite(c) && isfinite(e) && c < th.neg_cert && e > th.neg_cyc;
  const bool neg = (far || unrel) && p < 0;
  (side ? m1_out : m0_out)[g] = p >= 0 ? p : (neg ? -1 : -2);
  (side ? sc1 : sc0)[g] = p >= 0 ? c : 0.f;
  w_vp[w] = vp;
  unsigned char* masks = side ? masks1 : masks0;
  if (masks) {
    unsigned char* row = masks + (size_t)b * 4 * me.n + k;
    row[0] = vp;
    row[(size_t)me.n] = far;
    row[(size_t)2 * me.n] = unrel;
    row[(size_t)3 * me.n] = valid && p < 0 && !neg;
  }
  if (!side) w_pos0[g] = p;
}

// Step 9: plain writes, one thread per element, blockIdx = (column block, row, pair)
__global__ __launch_bounds__(DW_THREADS) void dw_dense_kernel(DwSide s0, DwSide s1, DwTh th, size_t side1,
                                                              const unsigned char* __restrict__ w_vp,
                                                              const int* __restrict__ w_pos0,
                                                              unsigned char* __restrict__ assignment,
                                                              float* __restrict__ reward) {
  const int j = blockIdx.x * DW_THREADS + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
  const int M = s0.n, N = s1.n;
  if (j >= N) return;
  const size_t r = (size_t)b * M + i, c = (size_t)b * N + j;
  const size_t o = r * N + j;
  const bool pos = w_pos0[r] == j;
  if (assignment) assignment[o] = pos;
  if (!reward) return;
  float d0, d1;
  gt_pair_dists(gt_coords(s0.kp, s0.proj, 0, r), gt_coords(s1.kp, s1.proj, 1, c), d0, d1);
  const bool pair = w_vp[r] && w_vp[side1 + c];
  const float d = pair ? fmaxf(d0, d1) : INFINITY;
  const float gain = fmaxf((pair && d < th.pos2) ? 1.f : 0.f, pos ? 1.f : 0.f);
  reward[o] = gain - ((pair && d > th.neg2) ? 1.f : 0.f);
}

// Workspace: one description, used by gfc_gt_matches_roma_workspace_bytes and by the launcher: the head every split
// labeller has (gt_sweep.h), then vp over the same K = B (M + N) key points, and pos0 [B,M].
struct DwWs { GtsSlots sweep; size_t vp, pos0, total; };
static DwWs dw_ws(int B, int M, int N) {
  gfc_slots s;
  return {gts_slots(s, B, M, N), s.take(gts_points(B, M, N)), s.take((size_t)B * M * sizeof(int)), s.off};
}

static bool dw_aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
static bool dw_field_ok(int H, int W) { return H >= 1 && W >= 1 && H <= 32768 && W <= 32768; }
static bool dw_sizes_ok(int B, int M, int N) { return B > 0 && M >= 0 && N >= 0 && B <= 65535 && M <= 65535 && N <= 65535; }

extern "C" int gfc_dense_cycle_error(const float* q_to_ref, const float* ref_to_q, float* out, int B, int H, int W, int Hr,
                                     int Wr, void* stream) {
  if (B <= 0 || B > 65535 || !dw_field_ok(H, W) || !dw_field_ok(Hr, Wr) || !q_to_ref || !ref_to_q || !out ||
      !dw_aligned8(q_to_ref) || !dw_aligned8(ref_to_q))
    return GFC_ERR_INVALID;
  const unsigned blocks = (unsigned)(((size_t)H * W + DW_THREADS - 1) / DW_THREADS);
  hipLaunchKernelGGL(dw_cycle_kernel, dim3(blocks, B), dim3(DW_THREADS), 0, (hipStream_t)stream, q_to_ref, ref_to_q, out,
                     H, W, Hr, Wr);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

extern "C" int gfc_gt_sample_dense_warp(const float* kp, const float* warp, const float* certainty,
                                        const float* cycle_error, const float* other_warp, int B, int M, int H, int W,
                                        int Hr, int Wr, int q_h, int q_w, int t_h, int t_w, float* proj,
                                        float* certainty_kp, float* cycle_kp, void* stream) {
  if (B <= 0 || B > 65535 || M < 0 || M > 65535 || !dw_field_ok(H, W) || q_h < 1 || q_w < 1 || t_h < 1 || t_w < 1)
    return GFC_ERR_INVALID;
  const int mode = cycle_error ? 1 : (other_warp ? 2 : 0);
  if (mode == 2 && !dw_field_ok(Hr, Wr)) return GFC_ERR_INVALID;
  if (M == 0) return GFC_OK;
  if (!kp || !warp || !certainty || !proj || !certainty_kp || !cycle_kp || !dw_aligned8(warp) || !dw_aligned8(other_warp))
    return GFC_ERR_INVALID;
  const dim3 grid((M + DW_THREADS - 1) / DW_THREADS, B), block(DW_THREADS);
  hipStream_t s = (hipStream_t)stream;
  const float qh1 = (float)(q_h - 1), qw1 = (float)(q_w - 1), th1 = (float)(t_h - 1), tw1 = (float)(t_w - 1);
  if (mode == 0)
    hipLaunchKernelGGL(dw_sample_kernel<0>, grid, block, 0, s, kp, warp, certainty, cycle_error, other_warp, M, H, W, Hr,
                       Wr, qh1, qw1, th1, tw1, proj, certainty_kp, cycle_kp);
  else if (mode == 1)
    hipLaunchKernelGGL(dw_sample_kernel<1>, grid, block, 0, s, kp, warp, certainty, cycle_error, other_warp, M, H, W, Hr,
                       Wr, qh1, qw1, th1, tw1, proj, certainty_kp, cycle_kp);
  else
    hipLaunchKernelGGL(dw_sample_kernel<2>, grid, block, 0, s, kp, warp, certainty, cycle_error, other_warp, M, H, W, Hr,
                       Wr, qh1, qw1, th1, tw1, proj, certainty_kp, cycle_kp);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

extern "C" size_t gfc_gt_matches_roma_workspace_bytes(int B, int M, int N) {
  if (!dw_sizes_ok(B, M, N) || M == 0 || N == 0) return 0;
  return dw_ws(B, M, N).total;
}

extern "C" int gfc_gt_matches_roma(const float* kp0, const float* kp1, const float* proj_0to1, const float* proj_1to0,
                                   const float* certainty_kp0, const float* certainty_kp1, const float* cycle_kp0,
                                   const float* cycle_kp1, const uint8_t* valid0, const uint8_t* valid1, int B, int M,
                                   int N, double pos_th, double neg_th, double pos_cert_th, double pos_cycle_error_th,
                                   double neg_cert_th, double neg_cycle_error_th, int64_t* matches0, int64_t* matches1,
                                   float* scores0, float* scores1, uint8_t* masks0, uint8_t* masks1, uint8_t* assignment,
                                   float* reward, void* workspace, size_t workspace_bytes, void* stream) {
  if (!dw_sizes_ok(B, M, N) || !(pos_th >= 0.0) || !(neg_th >= 0.0)) return GFC_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (M == 0 || N == 0) {
    if ((M > 0 && !scores0) || (N > 0 && !scores1)) return GFC_ERR_INVALID;
    return gt_empty_side(B, M, N, matches0, matches1, nullptr, scores0, scores1, masks0, masks1, nullptr, s);
  }
  if (!kp0 || !kp1 || !proj_0to1 || !proj_1to0 || !certainty_kp0 || !certainty_kp1 || !cycle_kp0 || !cycle_kp1 ||
      !valid0 || !valid1 || !matches0 || !matches1 || !scores0 || !scores1)
    return GFC_ERR_INVALID;
  const DwWs L = dw_ws(B, M, N);
  if (!workspace || workspace_bytes < L.total) return GFC_ERR_WORKSPACE;
  char* ws = (char*)workspace;
  const GtsOut w = gts_out(workspace, L.sweep);
  unsigned char* w_vp = (unsigned char*)(ws + L.vp);
  int* w_pos0 = (int*)(ws + L.pos0);
  const size_t side1 = (size_t)B * M;  // where the [B,N] part of a workspace array starts
  const DwSide s0{kp0, proj_0to1, certainty_kp0, cycle_kp0, valid0, M};
  const DwSide s1{kp1, proj_1to0, certainty_kp1, cycle_kp1, valid1, N};
  // the reference compares a float32 tensor with a Python double: the double (or its double square), rounded once
  DwTh th;
  th.pos2 = (float)(pos_th * pos_th);
  th.neg2 = (float)(neg_th * neg_th);
  th.has_pos_cert = pos_cert_th >= 0.0;
  th.has_pos_cyc = pos_cycle_error_th >= 0.0;
  th.has_unrel = neg_cert_th >= 0.0 && neg_cycle_error_th >= 0.0;
  th.pos_cert = (float)pos_cert_th;
  th.pos_cyc = (float)pos_cycle_error_th;
  th.neg_cert = (float)neg_cert_th;
  th.neg_cyc = (float)neg_cycle_error_th;
  const int row_blocks = gts_blocks(M), col_blocks = gts_blocks(N);
  hipLaunchKernelGGL(dw_sweep_kernel, dim3(row_blocks + col_blocks, B), dim3(GTS_THREADS), 0, s, s0, s1, th, row_blocks,
                     side1, w);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(dw_finish_kernel, dim3((M + N + DW_THREADS - 1) / DW_THREADS, B), dim3(DW_THREADS), 0, s, s0, s1, th,
                     side1, w.best, w.arg, w.own, w_vp, w_pos0, (long long*)matches0, (long long*)matches1, scores0,
                     scores1, masks0, masks1);
  GFC_LAUNCH_CHECK();
  if (assignment || reward) {
    hipLaunchKernelGGL(dw_dense_kernel, dim3((N + DW_THREADS - 1) / DW_THREADS, M, B), dim3(DW_THREADS), 0, s, s0, s1, th,
                       side1, w_vp, w_pos0, assignment, reward);
    GFC_LAUNCH_CHECK();
  }
  return GFC_OK;
}
