// Ground-truth labels from Endomapper sparse maps: the matching part of gt_matches_from_pose_sparse_map and
// gt_matches_from_pose_sparse_dense_map (reference gluefactory/geometry/gt_generation.py:441-591, 271-438).  The order
// of decisions and the launch plan are stated in include/gfc_amd_sparse_map.h.
//
// A pair is split over workgroups by the sweep of gt_sweep.h, which also states the arg-min rule (ties, a row of +inf,
// NaN) and the one known difference from the reference.  Here: what a sparse-map key point brings to that sweep (its
// flags and the seeding by 3D-point identity), the verdicts, the th_epi rule and the dense outputs.
#include "gt_sweep.h"
#include "../../include/gfc_amd_sparse_map.h"

enum : unsigned char { SM_VISIBLE = GTS_MASKED, SM_VALID3D = 2 };  // flag byte of a key point in the sweep
enum : unsigned char { SM_IGNORE = 1 };                             // state byte: the match is -2 BEFORE the epi_th rule

// Workspace: one description, used by gfc_gt_matches_sparse_map_workspace_bytes and by the launcher: the head every
// split labeller has (gt_sweep.h), then first, count and state over the same K = B (M + N) key points, and pos0 [B,M].
struct SmWs { GtsSlots sweep; size_t first, count, state, pos0, total; };
static SmWs sm_ws(int B, int M, int N) {
  const size_t K = gts_points(B, M, N);
  gfc_slots s;
  return {gts_slots(s, B, M, N), s.take(K * sizeof(int)), s.take(K * sizeof(int)), s.take(K),
          s.take((size_t)B * M * sizeof(int)), s.off};
}

struct SmSide {  // one image of the batch
  const float* kp;
  const float* proj;
  const unsigned char* visible;
  const unsigned char* valid;
  const long long* ids;
  const unsigned char* valid3d;
  int n;
};

__device__ __forceinline__ bool sm_valid3d(const SmSide& s, size_t g) { return s.valid3d ? s.valid3d[g] != 0 : true; }

struct SmLabeller {  // for gt_sweep: `visible` masks the distance, every key point counts in the one-way minimum
  using Side = SmSide;
  __device__ __forceinline__ unsigned char flags(const SmSide& s, size_t g) const {
    return (s.visible[g] ? SM_VISIBLE : 0) | (sm_valid3d(s, g) ? SM_VALID3D : 0);
  }
  static __device__ __forceinline__ bool own_min(unsigned char) { return true; }
};

// The seeding by identity as gt_sweep's further accumulator: the first key point of the other side with the owned point's
// id, both of them valid 3D points, and how many there are.  Without ids nothing is found.
struct SmSeeds {
  long long* t_id;  // [GTS_TILE] in LDS
  int* w_first;
  int* w_count;
  bool use_ids, id_ok;
  long long my_id;
  int first, count;
  __device__ __forceinline__ void begin(const SmSide& own, size_t g, unsigned char mine) {
    use_ids = own.ids != nullptr;
    id_ok = use_ids && (mine & SM_VALID3D);
    my_id = use_ids ? own.ids[g] : 0;
    first = INT_MAX;
    count = 0;
  }
  __device__ __forceinline__ void stage(const SmSide& oth, size_t q, int slot) { t_id[slot] = use_ids ? oth.ids[q] : 0; }
  __device__ __forceinline__ void visit(unsigned char f, int slot, int index) {
    if (id_ok && (f & SM_VALID3D) && t_id[slot] == my_id) {
      first = min(first, index);
      ++count;
    }
  }
  __device__ __forceinline__ void reduce(int o) {
    first = min(first, __shfl_xor(first, o, GTS_LANES));
    count += __shfl_xor(count, o, GTS_LANES);
  }
  __device__ __forceinline__ void store(size_t w) { w_first[w] = first; w_count[w] = count; }
};

__global__ __launch_bounds__(GTS_THREADS) void sm_sweep_kernel(SmSide s0, SmSide s1, int row_blocks, size_t side1, GtsOut w,
                                                               int* __restrict__ w_first, int* __restrict__ w_count) {
  __shared__ __attribute__((aligned(16))) GtsTile tile;  // with the ids 256 x (16 + 1 + 8) = 6400 bytes of static LDS
  __shared__ long long t_id[GTS_TILE];
  SmSeeds seeds{t_id, w_first, w_count};
  gt_sweep_pair(SmLabeller{}, s0, s1, row_blocks, side1, tile, w, seeds);
}

// Steps 2-5 per key point.  grid (ceil((M + N) / GTS_THREADS), B): threads 0..M-1 of a pair are its rows, then its columns.
// extra_positives is zeroed by the launcher.
__global__ __launch_bounds__(GTS_THREADS) void sm_finish_kernel(
    SmSide s0, SmSide s1, size_t side1, const float* __restrict__ w_best, const int* __restrict__ w_arg,
    const float* __restrict__ w_own, const int* __restrict__ w_first, const int* __restrict__ w_count,
    unsigned char* __restrict__ w_state, int* __restrict__ w_pos0, int has_pos, float pos2, int has_neg, float neg2,
    long long* __restrict__ m0_out, long long* __restrict__ m1_out, unsigned char* __restrict__ masks0,
    unsigned char* __restrict__ masks1, int* __restrict__ positive0, int* __restrict__ extra_positives) {
  const int b = blockIdx.y, M = s0.n, N = s1.n;
  const int t = blockIdx.x * GTS_THREADS + threadIdx.x;
  if (t >= M + N) return;
  const int side = t >= M, k = side ? t - M : t;
  const SmSide& me = side ? s1 : s0;
  const SmSide& ot = side ? s0 : s1;
  const size_t g = (size_t)b * me.n + k;               // in the arrays of the caller
  const size_t w = (side ? side1 : 0) + g;             // in the workspace
  const size_t wo = (side ? 0 : side1) + (size_t)b * ot.n;  // the other side's rows of this pair in the workspace
  long long m = -2;
  const int seeds = w_count[w];
  if (seeds > 0) m = w_first[w];
  int p = -1;  // the distance positive
  if (has_pos) {
    const int a = w_arg[w];
    if (gt_mutual_positive(w_best[w] < pos2, w_arg + wo, a, k)) p = a;
  }
  if (m == -2 && p >= 0) m = p;
  const bool negative = has_neg && w_own[w] > neg2 && me.valid[g] != 0;
  if (m == -2 && negative) m = -1;
  (side ? m1_out : m0_out)[g] = m;
  w_state[w] = m == -2 ? SM_IGNORE : 0;
  unsigned char* masks = side ? masks1 : masks0;
  if (masks) {
    unsigned char* row = masks + (size_t)b * 4 * me.n + k;
    row[0] = seeds > 0;
    row[(size_t)me.n] = p >= 0;
    row[(size_t)2 * me.n] = negative;
    row[(size_t)3 * me.n] = 0;  // the epi kernel overwrites it when epi_th is set
  }
  if (side) return;
  w_pos0[g] = p;
  if (positive0) positive0[g] = p;
  if (extra_positives) {
    // |S u {p}| - 1: p is in S when the ids are equal and both points are valid 3D points
    int set = seeds;
    if (p >= 0) {
      const size_t q = (size_t)b * N + p;
      const bool in_s = me.ids && me.ids[g] == ot.ids[q] && sm_valid3d(me, g) && sm_valid3d(ot, q);
      set += in_s ? 0 : 1;
    }
    if (set > 1) atomicAdd(extra_positives + b, set - 1);
  }
}

// Step 6, gridded as the sweep: the minimum of the symmetric epipolar distance over ignore x ignore (the state the finish
// kernel left in the workspace, which this kernel does not change), never stored.
template <int SIDE>
__device__ __forceinline__ void sm_epi(const SmSide& own, const SmSide& oth, int blk, int b, float2* t_xy,
                                       unsigned char* t_ign, const unsigned char* __restrict__ st_own,
                                       const unsigned char* __restrict__ st_oth,
                                       const float* __restrict__ Fm, float epi_th, long long* __restrict__ m_out,
                                       unsigned char* __restrict__ masks) {
  const int tid = threadIdx.x, lane = tid % GTS_LANES;
  const int k = blk * GTS_OWN + tid / GTS_LANES;
  const bool live = k < own.n;
  const size_t g = (size_t)b * own.n + (live ? k : 0);
  const float mx = own.kp[2 * g], my = own.kp[2 * g + 1];
  const bool ign = live && (st_own[g] & SM_IGNORE);
  float Ff[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) Ff[q] = Fm[b * 9 + q];
  float best = INFINITY;
  for (int base = 0; base < oth.n; base += GTS_TILE) {
    const int cnt = min(GTS_TILE, oth.n - base);
    __syncthreads();
    if (tid < cnt) {
      const size_t q = (size_t)b * oth.n + base + tid;
      t_xy[tid] = make_float2(oth.kp[2 * q], oth.kp[2 * q + 1]);
      t_ign[tid] = st_oth[q] & SM_IGNORE;
    }
    __syncthreads();
    if (ign)
      for (int e = lane; e < cnt; e += GTS_LANES)
        if (t_ign[e]) {
          const float2 o = t_xy[e];
          best = fminf(best, SIDE == 0 ? gt_epi_dist(Ff, mx, my, o.x, o.y) : gt_epi_dist(Ff, o.x, o.y, mx, my));
        }
  }
#pragma unroll
  for (int o = GTS_LANES / 2; o > 0; o >>= 1) best = fminf(best, __shfl_xor(best, o, GTS_LANES));
  if (live && lane == 0) {
    const bool exclude = best > epi_th;
    if (masks) masks[(size_t)b * 4 * own.n + (size_t)3 * own.n + k] = exclude;
    if (exclude && ign && !own.valid[g]) m_out[g] = -1;
  }
}

__global__ __launch_bounds__(GTS_THREADS) void sm_epi_kernel(SmSide s0, SmSide s1, int row_blocks, size_t side1,
                                                            const unsigned char* __restrict__ w_state,
                                                            const float* __restrict__ Fm, float epi_th,
                                                            long long* __restrict__ m0_out,
                                                            long long* __restrict__ m1_out,
                                                            unsigned char* __restrict__ masks0,
                                                            unsigned char* __restrict__ masks1) {
  __shared__ float2 t_xy[GTS_TILE];  // one tile for both instantiations: 256 x (8 + 1) = 2304 bytes
  __shared__ unsigned char t_ign[GTS_TILE];
  const int b = blockIdx.y;
  if ((int)blockIdx.x < row_blocks)
    sm_epi<0>(s0, s1, blockIdx.x, b, t_xy, t_ign, w_state, w_state + side1, Fm, epi_th, m0_out, masks0);
  else
    sm_epi<1>(s1, s0, blockIdx.x - row_blocks, b, t_xy, t_ign, w_state + side1, w_state, Fm, epi_th, m1_out, masks1);
}

// Step 7: plain writes, one thread per element, blockIdx = (column block, row, pair).  epi_mode 0: no penalty;
// 1: epi > epi_val on the unmasked epi (neg_th); 2: epi +inf outside ignore x ignore of the state before step 6 (epi_th).
__global__ __launch_bounds__(GTS_THREADS) void sm_dense_kernel(SmSide s0, SmSide s1, size_t side1,
                                                              const unsigned char* __restrict__ w_state,
                                                              const int* __restrict__ w_pos0,
                                                              const float* __restrict__ Fm, float epi_val, int epi_mode,
                                                              int has_pos, float pos2,
                                                              unsigned char* __restrict__ assignment,
                                                              float* __restrict__ reward) {
  const int j = blockIdx.x * GTS_THREADS + threadIdx.x, i = blockIdx.y, b = blockIdx.z;
  const int M = s0.n, N = s1.n;
  if (j >= N) return;
  const size_t r = (size_t)b * M + i, c = (size_t)b * N + j;
  const size_t o = r * N + j;
  bool pos = w_pos0[r] == j;
  if (s0.ids)
    pos = pos || (s0.ids[r] == s1.ids[c] && sm_valid3d(s0, r) && sm_valid3d(s1, c));
  if (assignment) assignment[o] = pos;
  if (!reward) return;
  float gain = pos ? 1.f : 0.f;
  if (has_pos) {
    float d0, d1;
    gt_pair_dists(gt_coords(s0.kp, s0.proj, 0, r), gt_coords(s1.kp, s1.proj, 1, c), d0, d1);
    const bool vis = s0.visible[r] && s1.visible[c];
    const float d = vis ? fmaxf(d0, d1) : INFINITY;
    gain = fmaxf(d < pos2 ? 1.f : 0.f, gain);
  }
  float penalty = 0.f;
  if (epi_mode) {
    float Ff[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Ff[q] = Fm[b * 9 + q];
    float e = gt_epi_dist(Ff, s0.kp[2 * r], s0.kp[2 * r + 1], s1.kp[2 * c], s1.kp[2 * c + 1]);
    if (epi_mode == 2 && !((w_state[r] & SM_IGNORE) && (w_state[side1 + c] & SM_IGNORE))) e = INFINITY;
    penalty = e > epi_val ? 1.f : 0.f;
  }
  reward[o] = gain - penalty;
}

static bool sm_sizes_ok(int B, int M, int N) { return B > 0 && M >= 0 && N >= 0 && B <= 65535 && M <= 65535 && N <= 65535; }

extern "C" size_t gfc_gt_matches_sparse_map_workspace_bytes(int B, int M, int N) {
  if (!sm_sizes_ok(B, M, N) || M == 0 || N == 0) return 0;
  return sm_ws(B, M, N).total;
}

extern "C" int gfc_gt_matches_sparse_map(const float* kp0, const float* kp1, const float* proj_0to1,
                                         const float* proj_1to0, const uint8_t* visible0, const uint8_t* visible1,
                                         const uint8_t* valid0, const uint8_t* valid1, const int64_t* ids0,
                                         const int64_t* ids1, const uint8_t* valid3d0, const uint8_t* valid3d1,
                                         const float* F, int B, int M, int N, double pos_th, double neg_th, double epi_th,
                                         int64_t* matches0, int64_t* matches1, uint8_t* masks0, uint8_t* masks1,
                                         int32_t* positive0, int32_t* extra_positives, uint8_t* assignment,
                                         float* reward, void* workspace, size_t workspace_bytes, void* stream) {
  if (!sm_sizes_ok(B, M, N)) return GFC_ERR_INVALID;
  hipStream_t s = (hipStream_t)stream;
  if (M == 0 || N == 0)
    return gt_empty_side(B, M, N, matches0, matches1, positive0, nullptr, nullptr, masks0, masks1, extra_positives, s);
  if (!kp0 || !kp1 || !proj_0to1 || !proj_1to0 || !visible0 || !visible1 || !valid0 || !valid1 || !matches0 || !matches1)
    return GFC_ERR_INVALID;
  if ((ids0 == nullptr) != (ids1 == nullptr)) return GFC_ERR_INVALID;
  const int has_pos = pos_th >= 0.0, has_neg = neg_th >= 0.0, has_epi = epi_th >= 0.0;
  const int epi_mode = has_epi ? 2 : (has_neg ? 1 : 0);
  if ((has_epi || (reward && epi_mode)) && !F) return GFC_ERR_INVALID;
  const SmWs L = sm_ws(B, M, N);
  if (!workspace || workspace_bytes < L.total) return GFC_ERR_WORKSPACE;
  char* ws = (char*)workspace;
  const GtsOut w = gts_out(workspace, L.sweep);
  int* w_first = (int*)(ws + L.first);
  int* w_count = (int*)(ws + L.count);
  unsigned char* w_state = (unsigned char*)(ws + L.state);
  int* w_pos0 = (int*)(ws + L.pos0);
  const size_t side1 = (size_t)B * M;  // where the [B,N] part of a workspace array starts
  const SmSide s0{kp0, proj_0to1, visible0, valid0, (const long long*)ids0, ids0 ? valid3d0 : nullptr, M};
  const SmSide s1{kp1, proj_1to0, visible1, valid1, (const long long*)ids1, ids1 ? valid3d1 : nullptr, N};
  // the reference squares the Python double and compares the float32 tensor with it: the double square, rounded once
  const float pos2 = (float)(pos_th * pos_th), neg2 = (float)(neg_th * neg_th);
  const int row_blocks = gts_blocks(M), col_blocks = gts_blocks(N);
  if (extra_positives && hipMemsetAsync(extra_positives, 0, (size_t)B * sizeof(int32_t), s) != hipSuccess)
    return GFC_ERR_LAUNCH;
  hipLaunchKernelGGL(sm_sweep_kernel, dim3(row_blocks + col_blocks, B), dim3(GTS_THREADS), 0, s, s0, s1, row_blocks,
                     side1, w, w_first, w_count);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(sm_finish_kernel, dim3((M + N + GTS_THREADS - 1) / GTS_THREADS, B), dim3(GTS_THREADS), 0, s, s0, s1,
                     side1, w.best, w.arg, w.own, w_first, w_count, w_state, w_pos0, has_pos, pos2, has_neg, neg2,
                     (long long*)matches0, (long long*)matches1, masks0, masks1, positive0, extra_positives);
  GFC_LAUNCH_CHECK();
  if (has_epi) {
    hipLaunchKernelGGL(sm_epi_kernel, dim3(row_blocks + col_blocks, B), dim3(GTS_THREADS), 0, s, s0, s1, row_blocks,
                       side1, w_state, F, (float)epi_th, (long long*)matches0, (long long*)matches1, masks0, masks1);
    GFC_LAUNCH_CHECK();
  }
  if (assignment || reward) {
    hipLaunchKernelGGL(sm_dense_kernel, dim3((N + GTS_THREADS - 1) / GTS_THREADS, M, B), dim3(GTS_THREADS), 0, s, s0, s1,
                       side1, w_state, w_pos0, F, (float)(has_epi ? epi_th : neg_th), epi_mode, has_pos, pos2,
                       assignment, reward);
    GFC_LAUNCH_CHECK();
  }
  return GFC_OK;
}
