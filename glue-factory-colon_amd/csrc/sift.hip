// SIFT on the GPU: Gaussian / DoG pyramid, extremum detection with fp64 refinement, orientation assignment, descriptor.
//
// The algorithm is the one stated in tests/sift_reference.py (Lowe's detector and descriptor with pycolmap's meaning of
// the reference's conf keys, gluefactory/models/extractors/sift.py:139-144).  OpenCV, pycolmap and CudaSift are absent
// -> parity with them is UNPINNED; the pin is that float64 restatement.
//
// Memory: one float array per image for the Gaussian levels and one for the DoG levels, laid out by sift_plan() from
// the PADDED size (H, W): octave o is a stack of S + 3 (S + 2) planes of (h_o, w_o) floats, row stride w_o.  An image
// whose valid size is smaller fills the top-left (h, w) of each plane with ITS OWN pyramid (its own octave sizes, its
// own replicate border) and may have fewer octaves; the rest of a plane is never read.
//
// pyramid  one launch per level.  256 threads own a 32 x 64 output tile: the input tile with its halo goes through LDS
//          once (read with the replicate clamp, or through the 2x bilinear up-sample for the first level), the row pass
//          writes a second LDS tile, the column pass writes the level, the DoG level (this level minus the LDS copy of
//          its input) and, for level S, every second pixel into level 0 of the next octave.  HBM: one read, one write
//          (+ DoG) per level.
// detect   26-neighbour test per sample behind the |v| > 0.8 thr test -> candidate keys (octave, layer, y, x) appended
//          with one vector atomic per candidate; each candidate then RANKS its key among the image's keys (the order of
//          the output never depends on the arrival of the atomics), is refined in fp64 and is compacted by a block scan.
//          A candidate beyond `cap` is counted, never stored: counts[b][2] reports how many.
// orient / describe   one wave per key point.  Histogram bins are 64-bit fixed-point (2^-40) LDS integers: integer
//          addition commutes, so the sums do not depend on the order in which the lanes arrive.
#include <math.h>

#include "block_select.h"
#include "common.h"

namespace {

constexpr int S_LAYERS = 3;
constexpr int N_GAUSS = S_LAYERS + 3, N_DOG = S_LAYERS + 2;
constexpr int MAX_OCT = 8;
constexpr int MIN_SIDE = 16;
constexpr int RMAX = 13;  // ceil(4 * 1.6 * sqrt(2^(10/3) - 2^(8/3))) = 13: the widest incremental blur (level S + 2)
constexpr int PT_H = 32, PT_W = 64;
constexpr int MAX_SIDE = 16384;  // of the (up-sampled) base level: keys hold y and x in 20 bits each
constexpr double SIGMA0 = 1.6;
constexpr float FIX = 1099511627776.f;  // 2^40
constexpr double UNFIX = 1.0 / 1099511627776.0;

struct sift_layout {
  int n_oct;
  int h[MAX_OCT], w[MAX_OCT];
  long long goff[MAX_OCT], doff[MAX_OCT];  // in floats, per image
  long long gauss_floats, dog_floats;
};

// GFC_OK, or why the shape cannot be served
int sift_plan(int H, int W, int first_octave, int num_octaves, sift_layout& L) {
  if (H <= 0 || W <= 0) return GFC_ERR_INVALID;
  if ((first_octave != -1 && first_octave != 0) || num_octaves < 1 || num_octaves > MAX_OCT) return GFC_ERR_UNSUPPORTED;
  long long h = H, w = W;
  if (first_octave < 0) { h *= 2; w *= 2; }
  if (h > MAX_SIDE || w > MAX_SIDE || (h < w ? h : w) < MIN_SIDE) return GFC_ERR_UNSUPPORTED;
  L = sift_layout();
  while (L.n_oct < num_octaves && (h < w ? h : w) >= MIN_SIDE) {
    const int o = L.n_oct++;
    L.h[o] = (int)h; L.w[o] = (int)w;
    L.goff[o] = L.gauss_floats; L.doff[o] = L.dog_floats;
    L.gauss_floats += (long long)N_GAUSS * h * w;
    L.dog_floats += (long long)N_DOG * h * w;
    h /= 2; w /= 2;
  }
  return GFC_OK;
}

// the image's own size at octave o; false when it has no such octave
__device__ __forceinline__ bool own_size(const int32_t* valid_wh, int b, int H, int W, int up, int o, int& h, int& w) {
  w = valid_wh ? valid_wh[2 * b] : W;
  h = valid_wh ? valid_wh[2 * b + 1] : H;
  w = min(max(w, 0), W); h = min(max(h, 0), H);  // device data the entry point cannot check
  if (up) { h *= 2; w *= 2; }
  h >>= o; w >>= o;
  return min(h, w) >= MIN_SIDE;
}

struct sift_taps { float t[2 * RMAX + 1]; int r; };

sift_taps make_taps(double sigma) {
  sift_taps T = {};
  T.r = (int)ceil(4.0 * sigma);
  double v[2 * RMAX + 1], sum = 0.0;
  for (int k = 0; k <= 2 * T.r; ++k) { const double x = k - T.r; v[k] = exp(-(x * x) / (2.0 * sigma * sigma)); sum += v[k]; }
  for (int k = 0; k <= 2 * T.r; ++k) T.t[k] = (float)(v[k] / sum);
  return T;
}

__device__ __forceinline__ float lerp2(float a, float b, float f) { return a * (1.f - f) + b * f; }

// One level.  UP: src is the input image and the level is blurred from its 2x bilinear up-sample.  first: src is the
// input image at its own size (octave 0, level 0); otherwise src is the previous level.
template <bool UP>
__global__ __launch_bounds__(256) void sift_level_kernel(const float* __restrict__ src, long long src_bstride, int src_ld,
                                                         float* __restrict__ dst, float* __restrict__ dog,
                                                         long long dst_bstride, long long dog_bstride, int ld,
                                                         float* __restrict__ dec, int dec_ld, const int32_t* __restrict__ valid_wh,
                                                         int H, int W, int up, int o, sift_taps T) {
  __shared__ float in[(PT_H + 2 * RMAX) * (PT_W + 2 * RMAX)];
  __shared__ float mid[(PT_H + 2 * RMAX) * PT_W];
  const int b = blockIdx.z;
  int h, w;
  if (!own_size(valid_wh, b, H, W, up, o, h, w)) return;
  const int x0 = blockIdx.x * PT_W, y0 = blockIdx.y * PT_H;
  if (x0 >= w || y0 >= h) return;
  const int R = T.r, IW = PT_W + 2 * R, IH = PT_H + 2 * R;
  const float* sb = src + (size_t)b * src_bstride;
  // the first level reads the input image: clipped to [0, 1] like the reference's np.clip (sift.py:208)
  const float lo = dog ? -INFINITY : 0.f, hi = dog ? INFINITY : 1.f;
  for (int i = threadIdx.x; i < IW * IH; i += 256) {
    const int ty = i / IW, tx = i - ty * IW;
    const int y = min(max(y0 + ty - R, 0), h - 1), x = min(max(x0 + tx - R, 0), w - 1);
    float v;
    if (UP) {
      const int sh = h >> 1, sw = w >> 1;  // the source's own size
      const int ix = (x & 1) ? (x - 1) / 2 : x / 2 - 1, iy = (y & 1) ? (y - 1) / 2 : y / 2 - 1;
      const float fx = (x & 1) ? 0.25f : 0.75f, fy = (y & 1) ? 0.25f : 0.75f;
      const int xa = max(ix, 0), xb = min(ix + 1, sw - 1), ya = max(iy, 0), yb = min(iy + 1, sh - 1);
      const float t00 = fminf(fmaxf(sb[(size_t)ya * src_ld + xa], lo), hi), t01 = fminf(fmaxf(sb[(size_t)ya * src_ld + xb], lo), hi);
      const float t10 = fminf(fmaxf(sb[(size_t)yb * src_ld + xa], lo), hi), t11 = fminf(fmaxf(sb[(size_t)yb * src_ld + xb], lo), hi);
      v = lerp2(lerp2(t00, t01, fx), lerp2(t10, t11, fx), fy);
    } else {
      v = fminf(fmaxf(sb[(size_t)y * src_ld + x], lo), hi);
    }
    in[ty * IW + tx] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int ty = wv; ty < IH; ty += 4) {  // rows: along x
    const float* p = in + ty * IW + lane;
    float acc = 0.f;
    for (int k = 0; k <= 2 * R; ++k) acc = fmaf(T.t[k], p[k], acc);
    mid[ty * PT_W + lane] = acc;
  }
  __syncthreads();
  const int x = x0 + lane;
  float* db = dst + (size_t)b * dst_bstride;
  // columns: along y.  (Sliding one LDS read over the eight rows a thread owns was measured and bought nothing: 2.87 ms
  // against 2.76 ms for the B = 32 up-sampled VGA pyramid.)
  for (int j = 0; j < PT_H / 4; ++j) {
    const int ty = wv * (PT_H / 4) + j, y = y0 + ty;
    if (y >= h || x >= w) continue;
    const float* p = mid + ty * PT_W + lane;
    float acc = 0.f;
    for (int k = 0; k <= 2 * R; ++k) acc = fmaf(T.t[k], p[k * PT_W], acc);
    db[(size_t)y * ld + x] = acc;
    if (dog) dog[(size_t)b * dog_bstride + (size_t)y * ld + x] = acc - in[(ty + R) * IW + lane + R];
    if (dec && !(y & 1) && !(x & 1) && (y >> 1) < (h >> 1) && (x >> 1) < (w >> 1))
      dec[(size_t)b * dst_bstride + (size_t)(y >> 1) * dec_ld + (x >> 1)] = acc;
  }
}

// ------------------------------------------------------------------------------------------------------------ detect
struct detect_layout { size_t keys, tmp_f, tmp_i, flag, total; };
detect_layout detect_plan(int B, int cap) {
  gfc_slots s;
  const size_t n = (size_t)B * cap;
  return {s.take(n * 8), s.take(n * 8 * 4), s.take(n * 8 * 4), s.take(n * 4), s.off};
}

__global__ __launch_bounds__(256) void sift_candidates_kernel(const float* __restrict__ dog, long long dog_bstride,
                                                              long long doff, int ld, int plane_h,
                                                              const int32_t* __restrict__ valid_wh, int H, int W, int up, int o,
                                                              double thr08, int cap, unsigned long long* __restrict__ keys,
                                                              int32_t* __restrict__ counts) {
  const int b = blockIdx.z / S_LAYERS, l = blockIdx.z % S_LAYERS + 1;
  int h, w;
  if (!own_size(valid_wh, b, H, W, up, o, h, w)) return;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x < 1 || y < 1 || x > w - 2 || y > h - 2) return;
  const size_t plane = (size_t)plane_h * ld;
  const float* d = dog + (size_t)b * dog_bstride + doff + (size_t)l * plane + (size_t)y * ld + x;
  const float v = *d;
  if (!((double)fabsf(v) > thr08)) return;
  bool gt = true, lt = true;
  for (int ds = -1; ds <= 1; ++ds)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (!ds && !dy && !dx) continue;
        const float n = d[(long long)ds * (long long)plane + (long long)dy * ld + dx];
        gt = gt && v > n;
        lt = lt && v < n;
      }
  if (!gt && !lt) return;
  const int pos = atomicAdd(&counts[4 * b + 1], 1);
  if (pos < cap)
    keys[(size_t)b * cap + pos] = ((unsigned long long)(o * 4 + l) << 40) | ((unsigned long long)y << 20) | (unsigned long long)x;
}

// Gaussian elimination with partial pivoting, in the order of tests/sift_reference.py: _solve3
__device__ bool solve3(double A[3][3], double b[3], double x[3]) {
  for (int j = 0; j < 3; ++j) {
    int piv = j;
    double big = fabs(A[j][j]);
    for (int i = j + 1; i < 3; ++i)
      if (fabs(A[i][j]) > big) { big = fabs(A[i][j]); piv = i; }
    if (big < 1e-30) return false;
    if (piv != j) {
      for (int k = 0; k < 3; ++k) { const double t = A[j][k]; A[j][k] = A[piv][k]; A[piv][k] = t; }
      const double t = b[j]; b[j] = b[piv]; b[piv] = t;
    }
    for (int i = j + 1; i < 3; ++i) {
      const double f = A[i][j] / A[j][j];
      for (int k = j; k < 3; ++k) A[i][k] -= f * A[j][k];
      b[i] -= f * b[j];
    }
  }
  for (int i = 2; i >= 0; --i) {
    double s = b[i];
    for (int k = i + 1; k < 3; ++k) s -= A[i][k] * x[k];
    x[i] = s / A[i][i];
  }
  return true;
}

struct plan_dev { int h[MAX_OCT], w[MAX_OCT]; long long doff[MAX_OCT]; };

__global__ __launch_bounds__(256) void sift_refine_kernel(const float* __restrict__ dog, long long dog_bstride, plan_dev P,
                                                          const int32_t* __restrict__ valid_wh, int H, int W, int up,
                                                          double thr, double edge_limit, int cap,
                                                          const unsigned long long* __restrict__ keys,
                                                          const int32_t* __restrict__ counts, float* __restrict__ tmp_f,
                                                          int32_t* __restrict__ tmp_i, int32_t* __restrict__ flag) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int n = min(counts[4 * b + 1], cap);
  if (i >= n) return;
  const unsigned long long* kb = keys + (size_t)b * cap;
  const unsigned long long key = kb[i];
  int rank = 0;
  for (int j = 0; j < n; ++j) rank += kb[j] < key;  // keys are distinct: a permutation
  const size_t slot = (size_t)b * cap + rank;
  flag[slot] = 0;
  const int o = (int)(key >> 42), l0 = (int)(key >> 40) & 3, y0 = (int)(key >> 20) & 0xFFFFF, x0 = (int)key & 0xFFFFF;
  int h, w;
  own_size(valid_wh, b, H, W, up, o, h, w);
  const int ld = P.w[o];
  const size_t plane = (size_t)P.h[o] * ld;
  const float* base = dog + (size_t)b * dog_bstride + P.doff[o];
#define D(L_, Y_, X_) ((double)base[(size_t)(L_) * plane + (size_t)(Y_) * ld + (X_)])
  int l = l0, y = y0, x = x0, moves = 0;
  double off[3], v, gx, gy, gs, hxx, hyy, hxy;
  bool ok = false;
  while (true) {
    v = D(l, y, x);
    gx = 0.5 * (D(l, y, x + 1) - D(l, y, x - 1));
    gy = 0.5 * (D(l, y + 1, x) - D(l, y - 1, x));
    gs = 0.5 * (D(l + 1, y, x) - D(l - 1, y, x));
    hxx = D(l, y, x + 1) + D(l, y, x - 1) - 2.0 * v;
    hyy = D(l, y + 1, x) + D(l, y - 1, x) - 2.0 * v;
    const double hss = D(l + 1, y, x) + D(l - 1, y, x) - 2.0 * v;
    hxy = 0.25 * (D(l, y + 1, x + 1) + D(l, y - 1, x - 1) - D(l, y - 1, x + 1) - D(l, y + 1, x - 1));
    const double hxs = 0.25 * (D(l + 1, y, x + 1) + D(l - 1, y, x - 1) - D(l - 1, y, x + 1) - D(l + 1, y, x - 1));
    const double hys = 0.25 * (D(l + 1, y + 1, x) + D(l - 1, y - 1, x) - D(l - 1, y + 1, x) - D(l + 1, y - 1, x));
    double A[3][3] = {{hxx, hxy, hxs}, {hxy, hyy, hys}, {hxs, hys, hss}}, rhs[3] = {-gx, -gy, -gs};
    if (!solve3(A, rhs, off)) break;
    const int mx = off[0] > 0.6 ? 1 : off[0] < -0.6 ? -1 : 0;
    const int my = off[1] > 0.6 ? 1 : off[1] < -0.6 ? -1 : 0;
    const int ml = off[2] > 0.6 ? 1 : off[2] < -0.6 ? -1 : 0;
    if (!mx && !my && !ml) { ok = true; break; }
    if (moves == 5) break;
    ++moves;
    x += mx; y += my; l += ml;
    if (x < 1 || x > w - 2 || y < 1 || y > h - 2 || l < 1 || l > S_LAYERS) break;
  }
#undef D
  if (!ok) return;
  const double val = v + 0.5 * (gx * off[0] + gy * off[1] + gs * off[2]);
  const double score = fabs(val);
  if (score < thr) return;
  const double tr = hxx + hyy, det = hxx * hyy - hxy * hxy;
  if (!(det > 0.0)) return;
  if (!(tr * tr / det < edge_limit)) return;
  const double step = (double)(1 << o), s0 = up ? 0.5 : 1.0;
  const double xo = x + off[0], yo = y + off[1], so = SIGMA0 * exp2((l + off[2]) / (double)S_LAYERS);
  float* f = tmp_f + slot * 8;
  f[0] = (float)((xo * step + 0.5) * s0); f[1] = (float)((yo * step + 0.5) * s0); f[2] = (float)(so * step * s0);
  f[3] = (float)score; f[4] = (float)xo; f[5] = (float)yo; f[6] = (float)so; f[7] = 0.f;
  int32_t* q = tmp_i + slot * 8;
  q[0] = o; q[1] = l0; q[2] = y0; q[3] = x0; q[4] = l; q[5] = y; q[6] = x; q[7] = 0;
  flag[slot] = 1;
}

__global__ __launch_bounds__(1024) void sift_compact_kernel(int cap, const float* __restrict__ tmp_f,
                                                            const int32_t* __restrict__ tmp_i, const int32_t* __restrict__ flag,
                                                            float* __restrict__ raw_f, int32_t* __restrict__ raw_i,
                                                            int32_t* __restrict__ counts) {
  __shared__ int wave_lds[16];
  const int b = blockIdx.x;
  const int found = counts[4 * b + 1], n = min(found, cap);
  int done = 0;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const size_t slot = (size_t)b * cap + i;
    const bool f = i < n && flag[slot];
    int total;
    const int at = done + gfc_block_rank<16>(f, wave_lds, total);
    if (f) {
      const size_t out = (size_t)b * cap + at;
      for (int k = 0; k < 8; ++k) { raw_f[out * 8 + k] = tmp_f[slot * 8 + k]; raw_i[out * 8 + k] = tmp_i[slot * 8 + k]; }
    }
    done += total;
  }
  if (threadIdx.x == 0) { counts[4 * b] = done; counts[4 * b + 2] = max(found - cap, 0); counts[4 * b + 3] = 0; }
}

// ------------------------------------------------------------------------------------------------------------ orient
struct orient_layout { size_t n_ori, angles, total; };
orient_layout orient_plan(int B, int cap) {
  gfc_slots s;
  const size_t n = (size_t)B * cap;
  return {s.take(n * 4), s.take(n * 4 * 4), s.off};
}

struct plan_gauss { int h[MAX_OCT], w[MAX_OCT]; long long goff[MAX_OCT]; };

// what detect writes: a position inside MAX_SIDE, sigma_oct in (0, 16), an octave and a level of the layout
__device__ __forceinline__ bool record_ok(float xo, float yo, float so, int o, int l) {
  return fabsf(xo) <= (float)MAX_SIDE && fabsf(yo) <= (float)MAX_SIDE && so > 0.f && so < 16.f && o >= 0 && o < MAX_OCT &&
         l >= 0 && l < N_GAUSS;
}

__device__ __forceinline__ void fix_add(unsigned long long* bin, float c) {
  atomicAdd(bin, (unsigned long long)(long long)(c * FIX));
}

__global__ __launch_bounds__(256) void sift_orient_kernel(const float* __restrict__ gauss, long long g_bstride, plan_gauss P,
                                                          const int32_t* __restrict__ valid_wh, int H, int W, int up,
                                                          const float* __restrict__ raw_f, const int32_t* __restrict__ raw_i,
                                                          const int32_t* __restrict__ counts, int cap,
                                                          int32_t* __restrict__ n_ori, float* __restrict__ angles) {
  __shared__ unsigned long long hist[4][36];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv;
  const bool active = i < min(counts[4 * b], cap);
  if (lane < 36) hist[wv][lane] = 0ull;
  __syncthreads();
  const size_t rec = (size_t)b * cap + i;
  bool sane = false;  // a record this library did not write is answered with no orientation, never followed
  if (active) {
    const float xo = raw_f[rec * 8 + 4], yo = raw_f[rec * 8 + 5], so = raw_f[rec * 8 + 6];
    const int o = raw_i[rec * 8], l = raw_i[rec * 8 + 4];
    sane = record_ok(xo, yo, so, o, l) && P.w[o] > 0;
  }
  if (sane) {
    const float xo = raw_f[rec * 8 + 4], yo = raw_f[rec * 8 + 5], so = raw_f[rec * 8 + 6];
    const int o = raw_i[rec * 8], l = raw_i[rec * 8 + 4];
    int h, w;
    own_size(valid_wh, b, H, W, up, o, h, w);
    const int ld = P.w[o];
    const float* g = gauss + (size_t)b * g_bstride + P.goff[o] + (size_t)l * P.h[o] * ld;
    const float sw = 1.5f * so;
    const int Wr = (int)floor(3.0 * 1.5 * (double)so + 0.5);
    const int xi = (int)floor((double)xo + 0.5), yi = (int)floor((double)yo + 0.5);
    const int side = 2 * Wr + 1;
    const float lim = (float)(Wr * Wr) + 0.6f, inv = 2.f * sw * sw;
    for (int s = lane; s < side * side; s += 64) {
      const int y = yi - Wr + s / side, x = xi - Wr + s % side;
      if (x < 1 || x > w - 2 || y < 1 || y > h - 2) continue;
      const float dx = (float)x - xo, dy = (float)y - yo;
      const float r2 = dx * dx + dy * dy;
      if (!(r2 < lim)) continue;
      const float gx = 0.5f * (g[(size_t)y * ld + x + 1] - g[(size_t)y * ld + x - 1]);
      const float gy = 0.5f * (g[(size_t)(y + 1) * ld + x] - g[(size_t)(y - 1) * ld + x]);
      const float mag = sqrtf(gx * gx + gy * gy);
      if (!(mag <= 3.0e38f)) continue;  // NaN / inf in the level
      float ang = atan2f(gy, gx);
      if (ang < 0.f) ang += 6.283185307179586f;
      const float wgt = mag * expf(-r2 / inv);
      const float fbin = ang * 5.729577951308232f - 0.5f;  // 36 / (2 pi)
      const float b0f = floorf(fbin), rb = fbin - b0f;
      const int b0 = (int)b0f;
      fix_add(&hist[wv][(b0 + 36) % 36], wgt * (1.f - rb));
      fix_add(&hist[wv][(b0 + 1) % 36], wgt * rb);
    }
  }
  __syncthreads();
  if (!active) return;
  if (!sane) {
    if (lane == 0) n_ori[rec] = 0;
    return;
  }
  const int bin = lane < 36 ? lane : 0;
  float hv = (float)((double)(long long)hist[wv][bin] * UNFIX);
  const float third = 1.f / 3.f;
  const int lm = (bin + 35) % 36, lp = (bin + 1) % 36;
  for (int it = 0; it < 6; ++it) hv = (__shfl(hv, lm) + hv + __shfl(hv, lp)) * third;
  const float hm = __shfl(hv, lm), hp = __shfl(hv, lp);
  const float top = wave_max(lane < 36 ? hv : -INFINITY);
  const bool peak = lane < 36 && top > 0.f && hv > hm && hv > hp && hv >= 0.8f * top;
  int peaks;
  const int before = gfc_wave_rank(peak, peaks);
  if (peak && before < 4) {
    const float di = -0.5f * (hp - hm) / (hp + hm - 2.f * hv);
    float th = 6.283185307179586f * ((float)lane + di + 0.5f) / 36.f;
    if (th > 3.141592653589793f) th -= 6.283185307179586f;
    angles[rec * 4 + before] = th;
  }
  if (lane == 0) n_ori[rec] = min(peaks, 4);
}

__global__ __launch_bounds__(1024) void sift_orient_compact_kernel(int cap, int ocap, const float* __restrict__ raw_f,
                                                                   const int32_t* __restrict__ raw_i,
                                                                   const int32_t* __restrict__ counts,
                                                                   const int32_t* __restrict__ n_ori,
                                                                   const float* __restrict__ angles, float* __restrict__ ori_f,
                                                                   int32_t* __restrict__ ori_i, int32_t* __restrict__ ocounts) {
  __shared__ int wave_lds[16];
  const int b = blockIdx.x;
  const int n = min(counts[4 * b], cap);
  int done = 0;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const size_t rec = (size_t)b * cap + i;
    const int k = i < n ? n_ori[rec] : 0;
    int total;
    const int at = done + gfc_block_scan_excl<16>(k, wave_lds, total);
    for (int j = 0; j < k; ++j) {
      if (at + j >= ocap) break;
      const size_t out = (size_t)b * ocap + at + j;
      for (int c = 0; c < 7; ++c) ori_f[out * 8 + c] = raw_f[rec * 8 + c];
      ori_f[out * 8 + 7] = angles[rec * 4 + j];
      ori_i[out * 4] = i; ori_i[out * 4 + 1] = raw_i[rec * 8]; ori_i[out * 4 + 2] = raw_i[rec * 8 + 4]; ori_i[out * 4 + 3] = j;
    }
    done += total;
  }
  if (threadIdx.x == 0) { ocounts[2 * b] = min(done, ocap); ocounts[2 * b + 1] = max(done - ocap, 0); }
}

// ---------------------------------------------------------------------------------------------------------- describe
__global__ __launch_bounds__(256) void sift_describe_kernel(const float* __restrict__ gauss, long long g_bstride, plan_gauss P,
                                                            const int32_t* __restrict__ valid_wh, int H, int W, int up,
                                                            const float* __restrict__ ori_f, const int32_t* __restrict__ ori_i,
                                                            const int32_t* __restrict__ ocounts, int ocap, float* __restrict__ desc) {
  __shared__ unsigned long long hist[4][128];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv;
  const bool active = i < min(ocounts[2 * b], ocap);
  hist[wv][lane] = 0ull; hist[wv][lane + 64] = 0ull;
  __syncthreads();
  const size_t rec = (size_t)b * ocap + i;
  bool sane = false;  // a record this library did not write gets a zero descriptor
  if (active) {
    const float xo = ori_f[rec * 8 + 4], yo = ori_f[rec * 8 + 5], so = ori_f[rec * 8 + 6], theta = ori_f[rec * 8 + 7];
    const int o = ori_i[rec * 4 + 1], l = ori_i[rec * 4 + 2];
    sane = record_ok(xo, yo, so, o, l) && P.w[o] > 0 && fabsf(theta) <= 7.f;
  }
  if (sane) {
    const float xo = ori_f[rec * 8 + 4], yo = ori_f[rec * 8 + 5], so = ori_f[rec * 8 + 6], theta = ori_f[rec * 8 + 7];
    const int o = ori_i[rec * 4 + 1], l = ori_i[rec * 4 + 2];
    int h, w;
    own_size(valid_wh, b, H, W, up, o, h, w);
    const int ld = P.w[o];
    const float* g = gauss + (size_t)b * g_bstride + P.goff[o] + (size_t)l * P.h[o] * ld;
    const float sbp = 3.f * so;
    const int Wr = (int)floor(sqrt(2.0) * (double)sbp * 2.5 + 0.5);
    const int xi = (int)floor((double)xo + 0.5), yi = (int)floor((double)yo + 0.5);
    const float ct = cosf(theta), st = sinf(theta);
    const int side = 2 * Wr + 1;
    const float two_pi = 6.283185307179586f;
    for (int s = lane; s < side * side; s += 64) {
      const int y = yi - Wr + s / side, x = xi - Wr + s % side;
      if (x < 1 || x > w - 2 || y < 1 || y > h - 2) continue;
      const float dx = (float)x - xo, dy = (float)y - yo;
      const float gx = 0.5f * (g[(size_t)y * ld + x + 1] - g[(size_t)y * ld + x - 1]);
      const float gy = 0.5f * (g[(size_t)(y + 1) * ld + x] - g[(size_t)(y - 1) * ld + x]);
      const float mag = sqrtf(gx * gx + gy * gy);
      if (!(mag <= 3.0e38f)) continue;  // NaN / inf in the level
      float ang = atan2f(gy, gx) - theta;
      if (ang < 0.f) ang += two_pi;
      if (ang < 0.f) ang += two_pi;
      if (ang >= two_pi) ang -= two_pi;
      const float nx = (ct * dx + st * dy) / sbp, ny = (-st * dx + ct * dy) / sbp;
      const float nt = ang * 1.2732395447351628f;  // 8 / (2 pi)
      const float wgt = mag * expf(-(nx * nx + ny * ny) / 8.f);
      const float bxf = floorf(nx - 0.5f), byf = floorf(ny - 0.5f), btf = floorf(nt);
      const float rx = nx - (bxf + 0.5f), ry = ny - (byf + 0.5f), rt = nt - btf;
      const int bx = (int)bxf, by = (int)byf, bt = (int)btf;
      for (int ddy = 0; ddy < 2; ++ddy)
        for (int ddx = 0; ddx < 2; ++ddx) {
          const int cx = bx + ddx + 2, cy = by + ddy + 2;
          if (cx < 0 || cx >= 4 || cy < 0 || cy >= 4) continue;
          const float wxy = wgt * (ddx ? rx : 1.f - rx) * (ddy ? ry : 1.f - ry);
          fix_add(&hist[wv][(cy * 4 + cx) * 8 + (bt & 7)], wxy * (1.f - rt));
          fix_add(&hist[wv][(cy * 4 + cx) * 8 + ((bt + 1) & 7)], wxy * rt);
        }
    }
  }
  __syncthreads();
  if (!active) return;
  float a = (float)((double)(long long)hist[wv][lane] * UNFIX), c = (float)((double)(long long)hist[wv][lane + 64] * UNFIX);
  float n = sqrtf(wave_sum(a * a + c * c));
  if (n > 0.f) { a /= n; c /= n; }
  a = fminf(a, 0.2f); c = fminf(c, 0.2f);
  n = sqrtf(wave_sum(a * a + c * c));
  if (n > 0.f) { a /= n; c /= n; }
  desc[rec * 128 + lane] = a;
  desc[rec * 128 + lane + 64] = c;
}

plan_gauss gauss_plan(const sift_layout& L) {
  plan_gauss P = {};
  for (int o = 0; o < L.n_oct; ++o) { P.h[o] = L.h[o]; P.w[o] = L.w[o]; P.goff[o] = L.goff[o]; }
  return P;
}

}  // namespace

extern "C" int gfc_sift_pyramid_layout(int H, int W, int first_octave, int num_octaves, int64_t* out) {
  if (!out) return GFC_ERR_INVALID;
  sift_layout L;
  const int s = sift_plan(H, W, first_octave, num_octaves, L);
  if (s != GFC_OK) return s;
  for (int i = 0; i < 3 + 4 * MAX_OCT; ++i) out[i] = 0;
  out[0] = L.n_oct; out[1] = L.gauss_floats; out[2] = L.dog_floats;
  for (int o = 0; o < L.n_oct; ++o) {
    out[3 + 4 * o] = L.h[o]; out[4 + 4 * o] = L.w[o]; out[5 + 4 * o] = L.goff[o]; out[6 + 4 * o] = L.doff[o];
  }
  return GFC_OK;
}

extern "C" int gfc_sift_pyramid(const float* image, int B, int H, int W, const int32_t* valid_wh, int first_octave,
                                int num_octaves, float* gauss, float* dog, void* stream) {
  if (!image || !gauss || !dog || B <= 0 || B > 65535) return GFC_ERR_INVALID;
  sift_layout L;
  const int s = sift_plan(H, W, first_octave, num_octaves, L);
  if (s != GFC_OK) return s;
  const hipStream_t st = (hipStream_t)stream;
  const int up = first_octave < 0;
  const double nominal = up ? 1.0 : 0.5;
  double sig[N_GAUSS];
  for (int k = 0; k < N_GAUSS; ++k) sig[k] = SIGMA0 * pow(2.0, (double)k / S_LAYERS);
  for (int o = 0; o < L.n_oct; ++o) {
    const int h = L.h[o], w = L.w[o];
    const long long plane = (long long)h * w;
    const dim3 grid((w + PT_W - 1) / PT_W, (h + PT_H - 1) / PT_H, B);
    float* g = gauss + L.goff[o];
    float* d = dog + L.doff[o];
    if (o == 0) {
      const sift_taps T = make_taps(sqrt(SIGMA0 * SIGMA0 - nominal * nominal));
      if (up)
        hipLaunchKernelGGL(sift_level_kernel<true>, grid, dim3(256), 0, st, image, (long long)H * W, W, g, (float*)nullptr,
                           L.gauss_floats, L.dog_floats, w, (float*)nullptr, 0, valid_wh, H, W, up, o, T);
      else
        hipLaunchKernelGGL(sift_level_kernel<false>, grid, dim3(256), 0, st, image, (long long)H * W, W, g, (float*)nullptr,
                           L.gauss_floats, L.dog_floats, w, (float*)nullptr, 0, valid_wh, H, W, up, o, T);
      GFC_LAUNCH_CHECK();
    }
    for (int k = 1; k < N_GAUSS; ++k) {
      const sift_taps T = make_taps(sqrt(sig[k] * sig[k] - sig[k - 1] * sig[k - 1]));
      const bool feed = k == S_LAYERS && o + 1 < L.n_oct;  // level S feeds level 0 of the next octave
      hipLaunchKernelGGL(sift_level_kernel<false>, grid, dim3(256), 0, st, g + (k - 1) * plane, L.gauss_floats, w,
                         g + k * plane, d + (k - 1) * plane, L.gauss_floats, L.dog_floats, w,
                         feed ? gauss + L.goff[o + 1] : (float*)nullptr, feed ? L.w[o + 1] : 0, valid_wh, H, W, up, o, T);
      GFC_LAUNCH_CHECK();
    }
  }
  return GFC_OK;
}

extern "C" size_t gfc_sift_detect_workspace_bytes(int B, int cap) {
  if (B <= 0 || cap <= 0 || (long long)B * cap > (1ll << 28)) return 0;
  return detect_plan(B, cap).total;
}

extern "C" int gfc_sift_detect(const float* dog, int B, int H, int W, const int32_t* valid_wh, int first_octave,
                               int num_octaves, double detection_threshold, double edge_threshold, int cap, float* raw_f,
                               int32_t* raw_i, int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (!dog || !raw_f || !raw_i || !counts || B <= 0 || B > 21845 || cap <= 0 || (long long)B * cap > (1ll << 28))
    return GFC_ERR_INVALID;
  if (!(detection_threshold >= 0.0) || !(edge_threshold > 0.0)) return GFC_ERR_INVALID;
  sift_layout L;
  const int s = sift_plan(H, W, first_octave, num_octaves, L);
  if (s != GFC_OK) return s;
  const detect_layout D = detect_plan(B, cap);
  if (!ws || ws_bytes < D.total) return GFC_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)((char*)ws + D.keys);
  float* tmp_f = (float*)((char*)ws + D.tmp_f);
  int32_t* tmp_i = (int32_t*)((char*)ws + D.tmp_i);
  int32_t* flag = (int32_t*)((char*)ws + D.flag);
  const int up = first_octave < 0;
  if (hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(int32_t), st) != hipSuccess) return GFC_ERR_LAUNCH;
  plan_dev P = {};
  for (int o = 0; o < L.n_oct; ++o) {
    P.h[o] = L.h[o]; P.w[o] = L.w[o]; P.doff[o] = L.doff[o];
    const dim3 grid((L.w[o] + 63) / 64, (L.h[o] + 3) / 4, B * S_LAYERS);
    hipLaunchKernelGGL(sift_candidates_kernel, grid, dim3(256), 0, st, dog, L.dog_floats, L.doff[o], L.w[o], L.h[o], valid_wh,
                       H, W, up, o, 0.8 * detection_threshold, cap, keys, counts);
    GFC_LAUNCH_CHECK();
  }
  const double r = edge_threshold;
  hipLaunchKernelGGL(sift_refine_kernel, dim3((cap + 255) / 256, B), dim3(256), 0, st, dog, L.dog_floats, P, valid_wh, H, W,
                     up, detection_threshold, (r + 1.0) * (r + 1.0) / r, cap, keys, counts, tmp_f, tmp_i, flag);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sift_compact_kernel, dim3(B), dim3(1024), 0, st, cap, tmp_f, tmp_i, flag, raw_f, raw_i, counts);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

extern "C" size_t gfc_sift_orient_workspace_bytes(int B, int cap) {
  if (B <= 0 || cap <= 0 || (long long)B * cap > (1ll << 28)) return 0;
  return orient_plan(B, cap).total;
}

extern "C" int gfc_sift_orient(const float* gauss, int B, int H, int W, const int32_t* valid_wh, int first_octave,
                               int num_octaves, const float* raw_f, const int32_t* raw_i, const int32_t* counts, int cap,
                               int ocap, float* ori_f, int32_t* ori_i, int32_t* ocounts, void* ws, size_t ws_bytes,
                               void* stream) {
  if (!gauss || !raw_f || !raw_i || !counts || !ori_f || !ori_i || !ocounts || B <= 0 || B > 65535 || cap <= 0 ||
      ocap <= 0 || (long long)B * cap > (1ll << 28) || (long long)B * ocap > (1ll << 28))
    return GFC_ERR_INVALID;
  sift_layout L;
  const int s = sift_plan(H, W, first_octave, num_octaves, L);
  if (s != GFC_OK) return s;
  const orient_layout O = orient_plan(B, cap);
  if (!ws || ws_bytes < O.total) return GFC_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  int32_t* n_ori = (int32_t*)((char*)ws + O.n_ori);
  float* angles = (float*)((char*)ws + O.angles);
  hipLaunchKernelGGL(sift_orient_kernel, dim3((cap + 3) / 4, B), dim3(256), 0, st, gauss, L.gauss_floats, gauss_plan(L),
                     valid_wh, H, W, (int)(first_octave < 0), raw_f, raw_i, counts, cap, n_ori, angles);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sift_orient_compact_kernel, dim3(B), dim3(1024), 0, st, cap, ocap, raw_f, raw_i, counts, n_ori, angles,
                     ori_f, ori_i, ocounts);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

extern "C" int gfc_sift_describe(const float* gauss, int B, int H, int W, const int32_t* valid_wh, int first_octave,
                                 int num_octaves, const float* ori_f, const int32_t* ori_i, const int32_t* ocounts, int ocap,
                                 float* desc, void* stream) {
  if (!gauss || !ori_f || !ori_i || !ocounts || !desc || B <= 0 || B > 65535 || ocap <= 0 ||
      (long long)B * ocap > (1ll << 24))
    return GFC_ERR_INVALID;
  sift_layout L;
  const int s = sift_plan(H, W, first_octave, num_octaves, L);
  if (s != GFC_OK) return s;
  hipLaunchKernelGGL(sift_describe_kernel, dim3((ocap + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, gauss, L.gauss_floats,
                     gauss_plan(L), valid_wh, H, W, (int)(first_octave < 0), ori_f, ori_i, ocounts, ocap, desc);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

// ------------------------------------------------------------------------------------------------------------ filter
// The reference's post-processing of a SIFT list (gluefactory/models/extractors/sift.py:288-380), per image:
// specular-mask rule (extractors/utils.py:4-42, offset 0.5) -> filter_dog_point (sift.py:29-62) -> top-k by score (or
// score x scale) -> RootSIFT (sift.py:65-68; applied after padding, so a padded row becomes the RootSIFT of zero).
// filter_dog_point keeps, per pixel round(p - 0.5), the points of the largest score, among them those of the smallest
// |angle|, then the ones that equal the (2 r + 1)^2 maximum of the per-pixel score plane.  Scores are >= 0 and |angle|
// >= 0, so their fp32 bit patterns order like the numbers: the planes hold those patterns and are built with vector
// atomic max / min, whose result does not depend on the order of arrival.
namespace {

constexpr int MAX_NMS_RADIUS = 16;

struct filter_layout { size_t score, angle, flag, kept, sel, m, total; };
filter_layout filter_plan(int B, int H, int W, int ocap) {
  gfc_slots s;
  const size_t px = (size_t)B * H * W, n = (size_t)B * ocap;
  return {s.take(px * 4), s.take(px * 4), s.take(n * 4), s.take(n * 4), s.take(n * 4), s.take((size_t)B * 4), s.off};
}

__device__ __forceinline__ void valid_size(const int32_t* valid_wh, int b, int H, int W, int& h, int& w) {
  w = valid_wh ? valid_wh[2 * b] : W;
  h = valid_wh ? valid_wh[2 * b + 1] : H;
  w = min(max(w, 1), W); h = min(max(h, 1), H);
}

__device__ __forceinline__ bool specular_ok(const unsigned char* mask, int ld, int h, int w, float x, float y) {
  const float fx = x - 0.5f, fy = y - 0.5f;
  const float x0 = floorf(fx), x1 = ceilf(fx), y0 = floorf(fy), y1 = ceilf(fy);
  if (!(x0 >= 0.f && x1 < (float)w && y0 >= 0.f && y1 < (float)h)) return false;
  const int ix0 = (int)x0, ix1 = (int)x1, iy0 = (int)y0, iy1 = (int)y1;
  return mask[(size_t)iy0 * ld + ix0] && mask[(size_t)iy0 * ld + ix1] && mask[(size_t)iy1 * ld + ix0] &&
         mask[(size_t)iy1 * ld + ix1];
}

// phase 0: specular rule, per-pixel max of the score; 1: per-pixel min of |angle| among the maxima; 2: the verdict
__global__ __launch_bounds__(256) void sift_filter_mark_kernel(int phase, const float* __restrict__ ori_f,
                                                               const int32_t* __restrict__ ocounts, int ocap, int H, int W,
                                                               const int32_t* __restrict__ valid_wh,
                                                               const unsigned char* __restrict__ specular, int radius,
                                                               unsigned* __restrict__ score_plane, unsigned* __restrict__ angle_plane,
                                                               int32_t* __restrict__ flag) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= min(ocounts[2 * b], ocap)) return;
  const size_t rec = (size_t)b * ocap + i;
  const float x = ori_f[rec * 8], y = ori_f[rec * 8 + 1], score = ori_f[rec * 8 + 3], angle = ori_f[rec * 8 + 7];
  int h, w;
  valid_size(valid_wh, b, H, W, h, w);
  if (phase == 0) {
    bool ok = score >= 0.f && fabsf(x) < 1e9f && fabsf(y) < 1e9f;  // (NaN and negative scores are no key points)
    if (ok && specular) ok = specular_ok(specular + (size_t)b * H * W, W, h, w, x, y);
    flag[rec] = ok;
    if (!ok || radius < 0) return;
  } else if (!flag[rec] || radius < 0) {
    return;
  }
  const int px = min(max((int)rintf(x - 0.5f), 0), w - 1), py = min(max((int)rintf(y - 0.5f), 0), h - 1);
  const size_t at = ((size_t)b * H + py) * W + px;
  const unsigned sb = __float_as_uint(score), ab = __float_as_uint(fabsf(angle));
  if (phase == 0) {
    atomicMax(&score_plane[at], sb);
  } else if (phase == 1) {
    if (score_plane[at] == sb) atomicMin(&angle_plane[at], ab);
  } else {
    bool keep = score_plane[at] == sb && angle_plane[at] == ab;
    for (int dy = -radius; keep && dy <= radius; ++dy)
      for (int dx = -radius; dx <= radius; ++dx) {
        const int yy = py + dy, xx = px + dx;
        if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
        if (score_plane[((size_t)b * H + yy) * W + xx] > sb) { keep = false; break; }
      }
    flag[rec] = keep;
  }
}

__global__ __launch_bounds__(1024) void sift_filter_compact_kernel(int ocap, const int32_t* __restrict__ ocounts,
                                                                   const int32_t* __restrict__ flag, int32_t* __restrict__ kept,
                                                                   int32_t* __restrict__ m) {
  __shared__ int wave_lds[16];
  const int b = blockIdx.x, n = min(ocounts[2 * b], ocap);
  int done = 0;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const bool f = i < n && flag[(size_t)b * ocap + i];
    int total;
    const int at = done + gfc_block_rank<16>(f, wave_lds, total);
    if (f) kept[(size_t)b * ocap + at] = i;
    done += total;
  }
  if (threadIdx.x == 0) m[b] = done;
}

__device__ __forceinline__ float rank_value(const float* ori_f, size_t rec, int weighting) {
  const float s = ori_f[rec * 8 + 3];
  return weighting ? s * ori_f[rec * 8 + 2] : s;
}

__global__ __launch_bounds__(256) void sift_filter_select_kernel(const float* __restrict__ ori_f, int ocap, int k, int out_cap,
                                                                 int weighting, const int32_t* __restrict__ kept,
                                                                 const int32_t* __restrict__ m, int32_t* __restrict__ sel,
                                                                 int32_t* __restrict__ counts_out) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int n = m[b];
  const bool topk = k > 0 && n > k;
  if (i == 0) counts_out[b] = min(topk ? k : n, out_cap);
  if (i >= n) return;
  const int32_t* kb = kept + (size_t)b * ocap;
  int at = i;
  if (topk) {  // torch.topk: descending; equal values by index (the fixtures have no tie at the boundary)
    const float v = rank_value(ori_f, (size_t)b * ocap + kb[i], weighting);
    at = 0;
    for (int j = 0; j < n; ++j) {
      const float u = rank_value(ori_f, (size_t)b * ocap + kb[j], weighting);
      at += u > v || (u == v && j < i);
    }
    if (at >= k) return;
  }
  if (at < out_cap) sel[(size_t)b * ocap + at] = kb[i];
}

__global__ __launch_bounds__(256) void sift_filter_gather_kernel(const float* __restrict__ ori_f, const float* __restrict__ desc,
                                                                 int ocap, int out_cap, int rootsift,
                                                                 const int32_t* __restrict__ sel,
                                                                 const int32_t* __restrict__ counts_out, float* __restrict__ kpts,
                                                                 float* __restrict__ scales, float* __restrict__ oris,
                                                                 float* __restrict__ scores, float* __restrict__ desc_out,
                                                                 int32_t* __restrict__ index) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= out_cap) return;
  const size_t out = (size_t)b * out_cap + r;
  const bool real = r < counts_out[b];
  const int src = real ? sel[(size_t)b * ocap + r] : -1;
  float a = 0.f, c = 0.f;
  if (real) {
    const size_t rec = (size_t)b * ocap + src;
    a = desc[rec * 128 + lane]; c = desc[rec * 128 + lane + 64];
    if (lane == 0) {
      kpts[out * 2] = ori_f[rec * 8]; kpts[out * 2 + 1] = ori_f[rec * 8 + 1];
      scales[out] = ori_f[rec * 8 + 2]; scores[out] = ori_f[rec * 8 + 3]; oris[out] = ori_f[rec * 8 + 7];
    }
  } else if (lane == 0) {
    scales[out] = 0.f; scores[out] = 0.f; oris[out] = 0.f;  // kpts: left to the padding
  }
  if (lane == 0) index[out] = src;
  if (rootsift) {  // normalize(p = 1, eps), clip(min = eps), sqrt, normalize(p = 2, eps); eps = 1e-6
    const float eps = 1e-6f;
    const float l1 = fmaxf(wave_sum(fabsf(a) + fabsf(c)), eps);
    a = sqrtf(fmaxf(a / l1, eps)); c = sqrtf(fmaxf(c / l1, eps));
    const float l2 = fmaxf(sqrtf(wave_sum(a * a + c * c)), eps);
    a /= l2; c /= l2;
  }
  desc_out[out * 128 + lane] = a;
  desc_out[out * 128 + lane + 64] = c;
}

}  // namespace

int gfc_rgb_to_gray(const float* img, float* out, int B, int H, int W, hipStream_t stream);  // conv.hip

extern "C" int gfc_sift_gray(const float* image, float* out, int B, int H, int W, void* stream) {
  if (!image || !out || B <= 0 || H <= 0 || W <= 0) return GFC_ERR_INVALID;
  return gfc_rgb_to_gray(image, out, B, H, W, (hipStream_t)stream);
}

extern "C" size_t gfc_sift_filter_workspace_bytes(int B, int H, int W, int ocap) {
  if (B <= 0 || H <= 0 || W <= 0 || ocap <= 0 || (long long)B * ocap > (1ll << 28) || (long long)B * H * W > (1ll << 31))
    return 0;
  return filter_plan(B, H, W, ocap).total;
}

extern "C" int gfc_sift_filter(const float* ori_f, const float* desc, const int32_t* ocounts, int B, int ocap, int H, int W,
                               const int32_t* valid_wh, const unsigned char* specular, int nms_radius, int scale_weighting,
                               int k, int rootsift, int out_cap, float* kpts, float* scales, float* oris, float* scores,
                               float* desc_out, int32_t* index, int32_t* counts_out, void* ws, size_t ws_bytes, void* stream) {
  if (!ori_f || !desc || !ocounts || !kpts || !scales || !oris || !scores || !desc_out || !index || !counts_out || B <= 0 ||
      B > 65535 || ocap <= 0 || out_cap <= 0 || H <= 0 || W <= 0 || (long long)B * ocap > (1ll << 28) ||
      (long long)B * H * W > (1ll << 31) || (long long)B * out_cap > (1ll << 24))
    return GFC_ERR_INVALID;
  if (out_cap < (k > 0 && k < ocap ? k : ocap)) return GFC_ERR_INVALID;  // every kept point has a row
  if (nms_radius > MAX_NMS_RADIUS) return GFC_ERR_UNSUPPORTED;
  const filter_layout F = filter_plan(B, H, W, ocap);
  if (!ws || ws_bytes < F.total) return GFC_ERR_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  unsigned* score_plane = (unsigned*)((char*)ws + F.score);
  unsigned* angle_plane = (unsigned*)((char*)ws + F.angle);
  int32_t* flag = (int32_t*)((char*)ws + F.flag);
  int32_t* kept = (int32_t*)((char*)ws + F.kept);
  int32_t* sel = (int32_t*)((char*)ws + F.sel);
  int32_t* m = (int32_t*)((char*)ws + F.m);
  const size_t px = (size_t)B * H * W;
  if (nms_radius >= 0) {
    if (hipMemsetAsync(score_plane, 0, px * 4, st) != hipSuccess) return GFC_ERR_LAUNCH;
    if (hipMemsetAsync(angle_plane, 0xFF, px * 4, st) != hipSuccess) return GFC_ERR_LAUNCH;
  }
  const dim3 grid((ocap + 255) / 256, B);
  for (int phase = 0; phase < (nms_radius >= 0 ? 3 : 1); ++phase) {
    hipLaunchKernelGGL(sift_filter_mark_kernel, grid, dim3(256), 0, st, phase, ori_f, ocounts, ocap, H, W, valid_wh, specular,
                       nms_radius, score_plane, angle_plane, flag);
    GFC_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(sift_filter_compact_kernel, dim3(B), dim3(1024), 0, st, ocap, ocounts, flag, kept, m);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sift_filter_select_kernel, grid, dim3(256), 0, st, ori_f, ocap, k, out_cap, scale_weighting, kept, m, sel,
                     counts_out);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sift_filter_gather_kernel, dim3((out_cap + 3) / 4, B), dim3(256), 0, st, ori_f, desc, ocap, out_cap,
                     rootsift, sel, counts_out, kpts, scales, oris, scores, desc_out, index);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

// ----------------------------------------------------------------------------------------------------------- extract
// The stages above in sequence on one stream, every intermediate in ONE workspace, no host read in between.
namespace {

struct extract_layout { size_t gauss, dog, raw_f, raw_i, ori_f, ori_i, desc, stage, total; };
bool extract_plan(int B, int H, int W, int first_octave, int num_octaves, int cap, int ocap, extract_layout& E, int& status) {
  sift_layout L;
  status = sift_plan(H, W, first_octave, num_octaves, L);
  if (status != GFC_OK) return false;
  status = GFC_ERR_INVALID;
  if (B <= 0 || B > 21845 || cap <= 0 || ocap <= 0 || (long long)B * cap > (1ll << 28) || (long long)B * ocap > (1ll << 24) ||
      (long long)B * H * W > (1ll << 31))
    return false;
  const size_t d = detect_plan(B, cap).total, o = orient_plan(B, cap).total, f = filter_plan(B, H, W, ocap).total;
  const size_t stage = d > o ? (d > f ? d : f) : (o > f ? o : f);  // the stages run one after the other
  gfc_slots s;
  const size_t nb = (size_t)B;
  E = {s.take(nb * L.gauss_floats * 4), s.take(nb * L.dog_floats * 4), s.take(nb * cap * 8 * 4), s.take(nb * cap * 8 * 4),
       s.take(nb * ocap * 8 * 4), s.take(nb * ocap * 4 * 4), s.take(nb * ocap * 128 * 4), s.take(stage), s.off};
  status = GFC_OK;
  return true;
}

}  // namespace

extern "C" size_t gfc_sift_extract_workspace_bytes(int B, int H, int W, int first_octave, int num_octaves, int cap, int ocap) {
  extract_layout E;
  int status;
  return extract_plan(B, H, W, first_octave, num_octaves, cap, ocap, E, status) ? E.total : 0;
}

extern "C" int gfc_sift_extract(const float* image, int B, int H, int W, const int32_t* valid_wh, const unsigned char* specular,
                                int first_octave, int num_octaves, double detection_threshold, double edge_threshold, int cap,
                                int ocap, int nms_radius, int scale_weighting, int k, int rootsift, int out_cap, float* kpts,
                                float* scales, float* oris, float* scores, float* desc_out, int32_t* index, int32_t* counts_out,
                                int32_t* counts, int32_t* ocounts, void* ws, size_t ws_bytes, void* stream) {
  if (!image || !counts || !ocounts) return GFC_ERR_INVALID;
  extract_layout E;
  int status;
  if (!extract_plan(B, H, W, first_octave, num_octaves, cap, ocap, E, status)) return status;
  if (nms_radius > MAX_NMS_RADIUS) return GFC_ERR_UNSUPPORTED;
  if (!kpts || !scales || !oris || !scores || !desc_out || !index || !counts_out || out_cap <= 0 ||
      out_cap < (k > 0 && k < ocap ? k : ocap) || (long long)B * out_cap > (1ll << 24))
    return GFC_ERR_INVALID;
  if (!ws || ws_bytes < E.total) return GFC_ERR_WORKSPACE;
  char* base = (char*)ws;
  float* gauss = (float*)(base + E.gauss);
  float* dog = (float*)(base + E.dog);
  float* raw_f = (float*)(base + E.raw_f);
  int32_t* raw_i = (int32_t*)(base + E.raw_i);
  float* ori_f = (float*)(base + E.ori_f);
  int32_t* ori_i = (int32_t*)(base + E.ori_i);
  float* desc = (float*)(base + E.desc);
  void* stage = base + E.stage;
  const size_t stage_bytes = E.total - E.stage;
  int s = gfc_sift_pyramid(image, B, H, W, valid_wh, first_octave, num_octaves, gauss, dog, stream);
  if (s != GFC_OK) return s;
  s = gfc_sift_detect(dog, B, H, W, valid_wh, first_octave, num_octaves, detection_threshold, edge_threshold, cap, raw_f, raw_i,
                      counts, stage, stage_bytes, stream);
  if (s != GFC_OK) return s;
  s = gfc_sift_orient(gauss, B, H, W, valid_wh, first_octave, num_octaves, raw_f, raw_i, counts, cap, ocap, ori_f, ori_i, ocounts,
                      stage, stage_bytes, stream);
  if (s != GFC_OK) return s;
  s = gfc_sift_describe(gauss, B, H, W, valid_wh, first_octave, num_octaves, ori_f, ori_i, ocounts, ocap, desc, stream);
  if (s != GFC_OK) return s;
  return gfc_sift_filter(ori_f, desc, ocounts, B, ocap, H, W, valid_wh, specular, nms_radius, scale_weighting, k, rootsift,
                         out_cap, kpts, scales, oris, scores, desc_out, index, counts_out, stage, stage_bytes, stream);
}
