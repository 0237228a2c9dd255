// What the ground-truth labellers share (gt_matches.hip: homography and pose + depth; gt_sparse_map.hip: Endomapper sparse
// maps; gt_dense_warp.hip: RoMa): the per-pair distances, the split nearest-neighbour sweep, the test for a mutual
// positive, the early return for an empty side and the head of the split labellers' workspace.
//
// Every labeller needs, per key point, the arg-min over the other side of the MASKED distance max(d0, d1) -- d0, d1 the
// squared one-way reprojection distances, +inf where either point is masked out -- and the minimum of its own UNMASKED
// one-way distance.  The rule for the arg-min is torch.min's, and it is stated here once:
//   * a running minimum starts at (+inf, index 0) and is replaced on '<' only, so the first index wins equal distances
//     and a row that is +inf throughout keeps arg-min 0;
//   * fminf and '<' skip a NaN distance where torch.min would propagate it (then `NaN > neg_th^2` is false and the point
//     stays `ignore`, while here it can become `negative`): the one known difference from the reference, for a key point
//     with valid depth whose projection is NaN.
// gt_matches_kernel keeps a whole pair in LDS and applies the rule in one thread per key point.  gt_sweep below SPLITS a
// pair over workgroups, and the rule must hold however a row is split: a workgroup owns GTS_OWN key points of one side,
// GTS_LANES lanes each, and streams the other side through LDS in tiles of GTS_TILE elements.  A lane visits its elements
// (lane, lane + GTS_LANES, ...) in ascending order and keeps the first of equal distances; the lanes of a key point are
// then reduced on (distance, index) with the lower index winning equal distances, so the result is that of one thread
// walking the whole row.  Per-key-point results go to the workspace and a short second launch of the labeller gives the
// verdicts: no workgroup waits for another.
#pragma once
#include "eval_common.h"

// ---- one pair of key points ----------------------------------------------------------------------------------------------
// r = (kp0 projected into image 1, kp0) for a key point of image 0, c = (kp1, kp1 projected into image 0) for one of
// image 1: one 128-bit read per distance
__device__ __forceinline__ float4 gt_coords(const float* kp, const float* proj, int side, size_t g) {
  const float x = kp[2 * g], y = kp[2 * g + 1], px = proj[2 * g], py = proj[2 * g + 1];
  return side == 0 ? make_float4(px, py, x, y) : make_float4(x, y, px, py);
}

// the squared one-way distances: d0 in image 1, d1 in image 0
__device__ __forceinline__ void gt_pair_dists(const float4& r, const float4& c, float& d0, float& d1) {
  const float dx0 = r.x - c.x, dy0 = r.y - c.y;
  const float dx1 = r.z - c.z, dy1 = r.w - c.w;
  d0 = dx0 * dx0 + dy0 * dy0;
  d1 = dx1 * dx1 + dy1 * dy1;
}

// sym_epipolar_distance_all (gluefactory/geometry/epipolar.py:59-72) of one pair of pixels: l0 = F p0, l1 = F^T p1
__device__ __forceinline__ float gt_epi_dist(const float* F, float x0, float y0, float x1, float y1) {
  const float a0 = F[0] * x0 + F[1] * y0 + F[2], b0 = F[3] * x0 + F[4] * y0 + F[5], c0 = F[6] * x0 + F[7] * y0 + F[8];
  const float a1 = F[0] * x1 + F[3] * y1 + F[6], b1 = F[1] * x1 + F[4] * y1 + F[7];
  const float num = fabsf(x1 * a0 + y1 * b0 + c0);
  return (num / sqrtf(a0 * a0 + b0 * b0 + 1e-15f) + num / sqrtf(a1 * a1 + b1 * b1 + 1e-15f)) / 2.f;
}

// positive.any(-1) of key point k, whose masked arg-min is a: its minimum is below pos_th^2 and the arg-min of a, among
// those of the other side, points back.  other_arg[a] is read only when below_pos holds.
__device__ __forceinline__ bool gt_mutual_positive(bool below_pos, const int* other_arg, int a, int k) {
  return below_pos && other_arg[a] == k;
}

// ---- the split sweep -----------------------------------------------------------------------------------------------------
constexpr int GTS_THREADS = 256;
constexpr int GTS_LANES = 16;                    // lanes per owned key point: a quarter of a wave, reduced with __shfl_xor
constexpr int GTS_OWN = GTS_THREADS / GTS_LANES;  // 16 key points per workgroup
constexpr int GTS_TILE = 256;                    // elements of the other side per LDS tile: one per thread

// bit 0 of a key point's flag byte: it takes part in the masked distance.  The other bits are the labeller's.
enum : unsigned char { GTS_MASKED = 1 };

struct GtsTile {  // 256 x (16 + 1) = 4352 bytes of static LDS, one for both instantiations of a kernel
  float4 xy[GTS_TILE];
  unsigned char flag[GTS_TILE];
};

// Head of a split labeller's workspace, over K = B (M + N) key points: side 0 of every pair first ([B,M]), then side 1
// ([B,N]) inside each array, so the side-1 part starts at element side1 = B M.  A labeller's layout takes it first.
struct GtsSlots { size_t best, arg, own; };
static inline size_t gts_points(int B, int M, int N) { return (size_t)B * ((size_t)M + N); }
static inline GtsSlots gts_slots(gfc_slots& s, int B, int M, int N) {
  const size_t K = gts_points(B, M, N);
  return {s.take(K * sizeof(float)), s.take(K * sizeof(int)), s.take(K * sizeof(float))};
}
struct GtsOut {
  float* best;  // minimum of the masked distance
  int* arg;     // its index
  float* own;   // minimum of the key point's own one-way distance
};
static inline GtsOut gts_out(void* workspace, const GtsSlots& L) {
  char* ws = (char*)workspace;
  return {(float*)(ws + L.best), (int*)(ws + L.arg), (float*)(ws + L.own)};
}
static inline int gts_blocks(int n) { return (n + GTS_OWN - 1) / GTS_OWN; }

// a labeller without a further accumulator
struct GtsNoExtra {
  template <class Side> __device__ __forceinline__ void begin(const Side&, size_t, unsigned char) {}
  template <class Side> __device__ __forceinline__ void stage(const Side&, size_t, int) {}
  __device__ __forceinline__ void visit(unsigned char, int, int) {}
  __device__ __forceinline__ void reduce(int) {}
  __device__ __forceinline__ void store(size_t) {}
};

// GTS_OWN key points of side SIDE (`own`, workgroup `blk` of that side, pair b) against every key point of `oth`; results
// at w_off + (index in the caller's arrays), w_off = 0 or side1.  The labeller L gives
//   Side                   one image of the batch, with kp, proj and n
//   flags(side, g)         the flag byte of a key point, formed alike for the owned point and for the tile
//   own_min(flag)          whether a tile element counts in the one-way minimum
// and X is a further accumulator over the same walk (GtsNoExtra: none), called with the owned point and its flag byte
// (begin), for a thread's tile element (stage), per visited element with its flag, tile slot and index (visit), per
// shuffle distance (reduce) and by the lane that stores (store).
template <int SIDE, class L, class X>
__device__ __forceinline__ void gt_sweep(const L& lab, const typename L::Side& own, const typename L::Side& oth, int blk,
                                         int b, GtsTile& t, const GtsOut& w, size_t w_off, X& x) {
  const int tid = threadIdx.x, lane = tid % GTS_LANES;
  const int k = blk * GTS_OWN + tid / GTS_LANES;  // the owned key point
  const bool live = k < own.n;
  const size_t g = (size_t)b * own.n + (live ? k : 0);
  const float4 me = gt_coords(own.kp, own.proj, SIDE, g);
  const unsigned char mine = live ? lab.flags(own, g) : 0;
  const bool masked = mine & GTS_MASKED;
  x.begin(own, g, mine);
  float best = INFINITY, best_own = INFINITY;
  int bi = 0;
  for (int base = 0; base < oth.n; base += GTS_TILE) {
    const int cnt = min(GTS_TILE, oth.n - base);
    __syncthreads();  // the previous tile has been read
    if (tid < cnt) {
      const size_t q = (size_t)b * oth.n + base + tid;
      t.xy[tid] = gt_coords(oth.kp, oth.proj, 1 - SIDE, q);
      t.flag[tid] = lab.flags(oth, q);
      x.stage(oth, q, tid);
    }
    __syncthreads();
    for (int e = lane; e < cnt; e += GTS_LANES) {
      const float4 r = SIDE == 0 ? me : t.xy[e];
      const float4 c = SIDE == 0 ? t.xy[e] : me;
      const unsigned char f = t.flag[e];
      float d0, d1;
      gt_pair_dists(r, c, d0, d1);
      const float d = (masked && (f & GTS_MASKED)) ? fmaxf(d0, d1) : INFINITY;
      if (d < best) { best = d; bi = base + e; }
      if (L::own_min(f)) best_own = fminf(best_own, SIDE == 0 ? d0 : d1);
      x.visit(f, e, base + e);
    }
  }
  // the GTS_LANES lanes of a key point: (distance, index) with the lower index winning equal distances
#pragma unroll
  for (int o = GTS_LANES / 2; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, GTS_LANES);
    const int oi = __shfl_xor(bi, o, GTS_LANES);
    if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    best_own = fminf(best_own, __shfl_xor(best_own, o, GTS_LANES));
    x.reduce(o);
  }
  if (live && lane == 0) {
    w.best[w_off + g] = best; w.arg[w_off + g] = bi; w.own[w_off + g] = best_own;
    x.store(w_off + g);
  }
}

// the body of a sweep kernel, grid (gts_blocks(M) + gts_blocks(N), B): blockIdx.x < row_blocks owns rows of image 0
// against every column, the others own columns against every row
template <class L, class X>
__device__ __forceinline__ void gt_sweep_pair(const L& lab, const typename L::Side& s0, const typename L::Side& s1,
                                              int row_blocks, size_t side1, GtsTile& t, const GtsOut& w, X& x) {
  const int b = blockIdx.y;
  if ((int)blockIdx.x < row_blocks) gt_sweep<0>(lab, s0, s1, blockIdx.x, b, t, w, 0, x);
  else gt_sweep<1>(lab, s1, s0, blockIdx.x - row_blocks, b, t, w, side1, x);
}

// ---- an empty side -------------------------------------------------------------------------------------------------------
// The early return of the reference (gt_generation.py:62-94, 282-314, 598-634, 735-753) for M == 0 or N == 0: every key
// point of the other side unmatched, nothing positive, no projection written, no dense element exists.  No kernel: -1 is
// all bits set in int64 and int32 alike.  positive0, the scores, the masks ([B,4,M], [B,4,N]) and extra_positives ([B])
// may be null; the matches of a side that has key points may not.
static inline int gt_empty_side(int B, int M, int N, int64_t* matches0, int64_t* matches1, int32_t* positive0,
                                float* scores0, float* scores1, uint8_t* masks0, uint8_t* masks1,
                                int32_t* extra_positives, hipStream_t s) {
  if ((M > 0 && !matches0) || (N > 0 && !matches1)) return GFC_ERR_INVALID;
  const size_t m = (size_t)B * M, n = (size_t)B * N;
  const struct { void* p; int byte; size_t bytes; } fills[] = {
      {matches0, 0xFF, m * sizeof(int64_t)}, {matches1, 0xFF, n * sizeof(int64_t)}, {positive0, 0xFF, m * sizeof(int32_t)},
      {scores0, 0, m * sizeof(float)},       {scores1, 0, n * sizeof(float)},       {masks0, 0, 4 * m},
      {masks1, 0, 4 * n},                    {extra_positives, 0, (size_t)B * sizeof(int32_t)}};
  for (const auto& f : fills)
    if (f.p && f.bytes && hipMemsetAsync(f.p, f.byte, f.bytes, s) != hipSuccess) return GFC_ERR_LAUNCH;
  return GFC_OK;
}
