// Workgroup scan, order-preserving compaction, radix select and LDS sort: the integer tail every extractor and estimator
// ends in (sp_detect.hip, disk_detect.hip, sift.hip, lg_adaptive.hip, ransac.hip).  Device helpers only.
//
// Common contract of the gfc_block_* helpers: one-dimensional workgroups of WAVES * 64 (THREADS) threads, and EVERY
// thread of the workgroup calls the helper, in uniform control flow (they contain barriers).  Scratch is LDS.
//
//   gfc_order_bits / gfc_from_order_bits   float <-> unsigned, a < b <=> bits(a) < bits(b) (no NaNs reach the callers)
//   gfc_wave_count(keep)                   kept lanes of the calling wave.  No barrier; inactive lanes count as not kept.
//   gfc_wave_rank(keep, count)             kept lanes below this lane, count = gfc_wave_count(keep).  No barrier.
//   gfc_wave_scan_incl(v)                  inclusive prefix sum over the wave.  No barrier; all 64 lanes active.
//   gfc_block_scan_excl<WAVES>(v, wave_lds, total)
//       exclusive prefix sum of v over the workgroup in thread order, total = the workgroup's sum (uniform: it comes
//       back as a scalar).  wave_lds: int[WAVES], WAVES a power of two <= 16.
//       Barriers: one after the wave totals are written, one after every thread has read them -- so nothing a thread
//       does after the call can overtake another thread's work before the call, and the call may be repeated at once with
//       the same scratch.
//   gfc_block_rank<WAVES>(keep, wave_lds, total)
//       the same for a 0 / 1 value through one ballot: slot of this thread among the kept threads, total = how many.
//       Same scratch, same two barriers, same guarantees.  Callers keep their own running base across chunks.
//   gfc_block_radix_select<KEY, EARLY_STOP, THREADS>(load, n, want, hist, wave_lds, s_prefix, s_state)
//       the want-th largest (1 <= want <= n) of the keys load(0) .. load(n - 1), KEY = unsigned or unsigned long long,
//       MSB first, 8 bits per pass through a 256-bin histogram.  hist: int[256]; wave_lds: int[4]; s_prefix: KEY[1];
//       s_state: int[1], int[2] with EARLY_STOP.  THREADS >= 256.  Begins by initialising the scratch behind a barrier
//       (work of the caller before the call must be separated from earlier users of that scratch by the caller); every
//       pass is four barriers and the call ends in one, so the scratch is free on return.
//       EARLY_STOP: as soon as a bin holds exactly what is still wanted, all its keys are winners: the passes stop and the
//       result is the prefix with the lower bytes ZERO -- a lower bound of the want-th key that selects the same set with
//       `key >= result`, not the key itself.  Without it all sizeof(KEY) passes run and the result is the exact key.
//   gfc_block_bitonic_desc<THREADS>(keys, P)
//       sorts keys[0 .. P) in LDS descending, P a power of two.  The caller's barrier makes the keys visible before the
//       call; one barrier per compare-exchange step, the last of them closes the call (P < 2: no barrier at all).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned int gfc_order_bits(float f) {
  unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gfc_from_order_bits(unsigned int o) {
  unsigned int u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
  return __uint_as_float(u);
}

__device__ __forceinline__ int gfc_wave_count(bool keep) { return __popcll(__ballot(keep)); }
__device__ __forceinline__ int gfc_wave_rank(bool keep, int& count) {
  const unsigned long long bal = __ballot(keep);
  count = __popcll(bal);
  return __builtin_amdgcn_mbcnt_hi((unsigned int)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)bal, 0u));
}

// x + x of the lane a DPP control names, in the rows of 16 lanes that ROWS (a bit per row) enables; a lane that is not
// enabled or has no source adds 0.  0xB1 / 0x4E: quad_perm [1,0,3,2] / [2,3,0,1]; 0x110 + n: row_shr n; 0x120 + n:
// row_ror n; 0x142 / 0x143: row_bcast 15 / 31 (lane 15 of each row to the next row / lane 31 to rows 2 and 3).
// All 64 lanes must be active.
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ int gfc_dpp_add(int x) { return x + __builtin_amdgcn_update_dpp(0, x, CTRL, ROWS, 0xf, false); }

// inclusive prefix sum over the 64 lanes of the wave: inside each row (row_shr 1, 2, 4, 8), then the total of row 0 / 2
// into row 1 / 3, then the total of rows 0 and 1 into rows 2 and 3
__device__ __forceinline__ int gfc_wave_scan_incl(int v) {
  v = gfc_dpp_add<0x111>(v);
  v = gfc_dpp_add<0x112>(v);
  v = gfc_dpp_add<0x114>(v);
  v = gfc_dpp_add<0x118>(v);
  v = gfc_dpp_add<0x142, 0xa>(v);
  return gfc_dpp_add<0x143, 0xc>(v);
}

// base = sum of wave_lds[0 .. wave), total = sum of all, between the two barriers described above.  Every lane reads ONE
// wave total (lane l that of wave l mod WAVES: period WAVES inside each row of 16 lanes) and the sums run over the lanes
// of a row: one LDS read instead of WAVES per thread.
template <int WAVES>
__device__ __forceinline__ int gfc_block_wave_base(int* wave_lds, int& total) {
  static_assert(WAVES >= 1 && WAVES <= 16 && (WAVES & (WAVES - 1)) == 0, "gfc_block_wave_base");
  const int slot = threadIdx.x & (WAVES - 1), wave = threadIdx.x >> 6;
  __syncthreads();
  int tot = wave_lds[slot];
  __syncthreads();
  int base = slot < wave ? tot : 0;
  if constexpr (WAVES > 1) { base = gfc_dpp_add<0xB1>(base); tot = gfc_dpp_add<0xB1>(tot); }
  if constexpr (WAVES > 2) { base = gfc_dpp_add<0x4E>(base); tot = gfc_dpp_add<0x4E>(tot); }
  if constexpr (WAVES > 4) { base = gfc_dpp_add<0x124>(base); tot = gfc_dpp_add<0x124>(tot); }
  if constexpr (WAVES > 8) { base = gfc_dpp_add<0x128>(base); tot = gfc_dpp_add<0x128>(tot); }
  total = __builtin_amdgcn_readfirstlane(tot);  // the same in every lane: a scalar for the caller's loop bounds
  return base;
}

template <int WAVES>
__device__ __forceinline__ int gfc_block_scan_excl(int v, int* wave_lds, int& total) {
  const int inc = gfc_wave_scan_incl(v);
  if ((threadIdx.x & 63) == 63) wave_lds[threadIdx.x >> 6] = inc;
  return gfc_block_wave_base<WAVES>(wave_lds, total) + inc - v;
}

template <int WAVES>
__device__ __forceinline__ int gfc_block_rank(bool keep, int* wave_lds, int& total) {
  int count;
  const int before = gfc_wave_rank(keep, count);
  if ((threadIdx.x & 63) == 0) wave_lds[threadIdx.x >> 6] = count;
  return gfc_block_wave_base<WAVES>(wave_lds, total) + before;
}

template <typename KEY, bool EARLY_STOP, int THREADS, typename LOAD>
__device__ __forceinline__ KEY gfc_block_radix_select(LOAD&& load, unsigned int n, unsigned int want, int* hist,
                                                      int* wave_lds, KEY* s_prefix, int* s_state) {
  constexpr int TOP = 8 * ((int)sizeof(KEY) - 1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    *s_prefix = 0;
    s_state[0] = (int)want;
    if constexpr (EARLY_STOP) s_state[1] = 0;
  }
  __syncthreads();
  for (int shift = TOP; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    const KEY prefix = *s_prefix;
    const unsigned int rem = (unsigned int)s_state[0];
    __syncthreads();
    const KEY himask = shift == TOP ? (KEY)0 : (KEY)(~(KEY)0 << (shift + 8));
    for (unsigned int i = tid; i < n; i += THREADS) {
      const KEY key = load(i);
      if ((key & himask) == prefix) atomicAdd(&hist[(unsigned int)(key >> shift) & 0xFF], 1);
    }
    __syncthreads();
    // the bin that holds the wanted key, found by 256 threads: inclusive scan over the bins in descending order (a serial
    // walk by one thread costs a dependent LDS read per bin, ~10 k cycles per pass)
    unsigned int v = 0, inc = 0;
    if (tid < 256) {  // waves 0..3, whole waves
      v = (unsigned int)hist[255 - tid];
      inc = (unsigned int)gfc_wave_scan_incl((int)v);
      if (lane == 63) wave_lds[wave] = (int)inc;
    }
    __syncthreads();
    if (tid < 256) {
      for (int i = 0; i < wave; ++i) inc += (unsigned int)wave_lds[i];
      if (inc >= rem && inc - v < rem) {  // exactly one bin: the first (from the top) whose running count reaches rem
        *s_prefix = prefix | ((KEY)(255 - tid) << shift);
        s_state[0] = (int)(rem - (inc - v));
        if constexpr (EARLY_STOP) s_state[1] = inc == rem;
      }
    }
    __syncthreads();
    if constexpr (EARLY_STOP) {
      if (s_state[1]) break;  // uniform
    }
  }
  const KEY kth = *s_prefix;
  __syncthreads();
  return kth;
}

template <int THREADS>
__device__ __forceinline__ void gfc_block_bitonic_desc(unsigned long long* keys, unsigned int P) {
  for (unsigned int sz = 2; sz <= P; sz <<= 1)
    for (unsigned int st = sz >> 1; st > 0; st >>= 1) {
      for (unsigned int i = threadIdx.x; i < P / 2; i += THREADS) {
        const unsigned int lo = (i / st) * (st * 2) + (i % st), hi = lo + st;
        const bool desc = ((lo & sz) == 0);
        const unsigned long long a = keys[lo], c = keys[hi];
        if ((a < c) == desc) { keys[lo] = c; keys[hi] = a; }
      }
      __syncthreads();
    }
}
