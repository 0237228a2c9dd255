// What the robust estimators share (ransac.hip: homography; relpose.hip: relative pose): the counter-based sampler
// and the compaction of the matches.  One copy, so both draw the same stream and order their correspondences alike.
#pragma once
#include "eval_common.h"

#define RS_MAX_T 8
#define RS_LDS_CORR_BYTES (128 * 1024)
#define RS_GOLDEN 0x9E3779B97F4A7C15ull

// ---- sampler: splitmix64 finaliser as a counter-based generator ---------------------------------------------
__device__ __host__ __forceinline__ unsigned long long rs_mix64(unsigned long long z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
__device__ __host__ __forceinline__ unsigned long long rs_key(unsigned long long seed, unsigned long long stream) {
  return rs_mix64(rs_mix64(seed + RS_GOLDEN) ^ stream);
}

// K distinct indices in [0, n), n >= K: draw j of hypothesis h is u = mix64(key + GOLDEN (K h + j + 1)),
// r_j = ((u >> 32) (n - j)) >> 32, and the r_j index a partial Fisher-Yates over the virtual array a[p] = p ("take
// a[r_j], move the last live element a[n - 1 - j] into the hole"): a hole is looked up latest first.  K = 4 is the
// homography estimator's sampler (ransac.hip), K = 5 the relative-pose one's; eval_utils.ransac_sample_indices is the
// same function in integer numpy, and the GPU tests of both estimators check the kernels against it.
template <int K>
__device__ __host__ __forceinline__ void rs_sample_k(unsigned long long key, int h, int n, int* out) {
  int p[K], v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const unsigned long long u = rs_mix64(key + RS_GOLDEN * ((unsigned long long)K * (unsigned long long)h + (unsigned long long)(j + 1)));
    const int r = (int)(((u >> 32) * (unsigned long long)(n - j)) >> 32);
    const int l = n - 1 - j;
    int idx = r, val = l;
    bool fi = false, fv = false;
#pragma unroll
    for (int q = K - 1; q >= 0; --q) {
      if (q < j) {
        if (!fi && r == p[q]) { idx = v[q]; fi = true; }
        if (!fv && l == p[q]) { val = v[q]; fv = true; }
      }
    }
    out[j] = idx;
    p[j] = r;
    v[j] = val;
  }
}

// the matches (i, m0[i]) with 0 <= m0[i] < N in ascending i -> (x0, y0, x1, y1) records + their key-point-0 index + n
// (defined in ransac.hip)
__global__ __launch_bounds__(EM_THREADS) void ransac_compact_kernel(const float* __restrict__ kp0, const float* __restrict__ kp1,
                                      const long long* __restrict__ m0, int M, int N, float4* __restrict__ corr,
                                      int* __restrict__ cidx, int* __restrict__ cnt);
