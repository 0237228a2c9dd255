// Validation loss and matcher metrics of a batch of equal-sized pairs in one launch, one workgroup per pair.
//
// Replaces, for the forward-only validation pass, NLLLoss.forward / weight_loss (reference gluefactory/models/utils/
// losses.py:6-73), `row_norm` (models/matchers/lightglue.py:606) and matcher_metrics (models/utils/metrics.py:4-50).
// The (M+1) x (N+1) weight matrix of nll_loss is never built: the negatives are the last column / row of the log
// assignment read where gt_matches == -1, the positives la[i, j] where gt_assignment[i, j] is set (or, without a dense
// assignment, la[i, gt_matches0[i]] where that is > -1).  Only row_norm reads the whole matrix, once.
// Every sum is accumulated in fp64 and each output is rounded to fp32 once; exp is the fp32 expf (1 ulp).
// ranking_ap multiplies every recall increment by the LAST precision point, so it telescopes to
// p_last * (r_last - r_first), r_first that of the top-scoring key point: the lowest index among equal maxima here
// (torch.argsort is not stable; a tie of positive top scores is therefore unpinned in the reference itself).
#include "eval_common.h"
#include "../../include/gfc_amd_validation.h"

#define LV_OUT 10   // nll_pos, nll_neg, num_matchable, num_unmatchable, assignment_nll, row_norm, recall, precision,
                    // accuracy, average_precision
#define LV_SUMS 13
#define LV_THREADS 1024  // 16 waves on the one CU a pair occupies: the pass over the matrix is bound by load latency
#define LV_WAVES (LV_THREADS / 64)

// block-wide sum of NV doubles per thread in a fixed order; the result is valid in every thread
template <int NV>
__device__ __forceinline__ void lv_block_sum(double* v, double* lds /* [LV_WAVES][NV] */, int tid) {
  const int wave = tid >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const double t = wave_sum_f64(v[q]);
    if ((tid & 63) == 0) lds[wave * NV + q] = t;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double t = 0.0;
#pragma unroll 1  // (unrolled, the 16 x NV reads in flight spill the registers of a 1024-thread workgroup)
    for (int w = 0; w < LV_WAVES; ++w) t += lds[w * NV + q];
    v[q] = t;
  }
  __syncthreads();
}

__global__ __launch_bounds__(LV_THREADS) void lg_validation_kernel(
    const float* __restrict__ la, const long long* __restrict__ gt0, const long long* __restrict__ gt1,
    const unsigned char* __restrict__ gt_assignment, const long long* __restrict__ m0,
    const float* __restrict__ scores0, int M, int N, double balancing, float* __restrict__ out) {
  __shared__ double red[LV_WAVES * LV_SUMS];
  __shared__ float top_s[LV_WAVES];
  __shared__ int top_i[LV_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t ld = (size_t)N + 1;
  const float* L = la + (size_t)b * ((size_t)M + 1) * ld;
  const long long* g0 = gt0 + (size_t)b * M;
  const long long* g1 = gt1 + (size_t)b * N;
  const long long* mm = m0 + (size_t)b * M;
  const float* sc = scores0 + (size_t)b * M;
  // 0 row_norm sum, 1 / 2 positives (sum, count), 3 / 4 negatives of view 0, 5 / 6 of view 1,
  // 7 / 8 recall (hits, mask), 9 / 10 accuracy, 11 / 12 precision
  double s[LV_SUMS];
#pragma unroll
  for (int q = 0; q < LV_SUMS; ++q) s[q] = 0.0;
  // rows 0 .. M-1 with all N + 1 columns are the first M (N + 1) values of the pair; four loads in flight per thread
  {
    const size_t all = (size_t)M * ld, T = LV_THREADS;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    size_t e = tid;
    for (; e + 3 * T < all; e += 4 * T) {
      const float x0 = L[e], x1 = L[e + T], x2 = L[e + 2 * T], x3 = L[e + 3 * T];
      a0 += (double)expf(x0); a1 += (double)expf(x1); a2 += (double)expf(x2); a3 += (double)expf(x3);
    }
    for (; e < all; e += T) a0 += (double)expf(L[e]);
    s[0] = (a0 + a1) + (a2 + a3);
  }
  if (gt_assignment) {  // a wave per row, lanes along it
    const unsigned char* A = gt_assignment + (size_t)b * M * N;
    for (int i = tid >> 6; i < M; i += LV_WAVES)
      for (int j = tid & 63; j < N; j += 64)
        if (A[(size_t)i * N + j]) { s[1] += (double)L[(size_t)i * ld + j]; s[2] += 1.0; }
  }
  float best_s = -INFINITY;
  int best_i = 0x7fffffff;
  for (int i = tid; i < M; i += LV_THREADS) {
    const long long g = g0[i], m = mm[i];
    if (!gt_assignment && g > -1 && g < N) { s[1] += (double)L[(size_t)i * ld + g]; s[2] += 1.0; }
    if (g == -1) { s[3] += (double)L[(size_t)i * ld + N]; s[4] += 1.0; }
    const double hit = m == g ? 1.0 : 0.0;
    if (g > -1) { s[7] += hit; s[8] += 1.0; }
    if (g >= -1) { s[9] += hit; s[10] += 1.0; }
    if (m > -1 && g >= -1) { s[11] += hit; s[12] += 1.0; }
    const float v = sc[i];
    if (v > best_s) { best_s = v; best_i = i; }  // ascending i per thread: the first of equal maxima stays
  }
  for (int j = tid; j < N; j += LV_THREADS)
    if (g1[j] == -1) { s[5] += (double)L[(size_t)M * ld + j]; s[6] += 1.0; }
  lv_block_sum<LV_SUMS>(s, red, tid);
  // top score: the largest, the lowest index among equals
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(best_s, o, 64);
    const int oi = __shfl_xor(best_i, o, 64);
    if (os > best_s || (os == best_s && oi < best_i)) { best_s = os; best_i = oi; }
  }
  if ((tid & 63) == 0) { top_s[tid >> 6] = best_s; top_i[tid >> 6] = best_i; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < LV_WAVES; ++w)
      if (top_s[w] > best_s || (top_s[w] == best_s && top_i[w] < best_i)) { best_s = top_s[w]; best_i = top_i[w]; }
    float* o = out + (size_t)b * LV_OUT;
    const double num_pos = fmax(s[2], 1.0), num_neg0 = fmax(s[4], 1.0), num_neg1 = fmax(s[6], 1.0);
    const double nll_pos = -s[1] / num_pos, nll_neg = -(s[3] + s[5]) / (num_neg0 + num_neg1);
    o[0] = (float)nll_pos;
    o[1] = (float)nll_neg;
    o[2] = (float)num_pos;
    o[3] = (float)((num_neg0 + num_neg1) / 2.0);
    o[4] = (float)(balancing * nll_pos + (1.0 - balancing) * nll_neg);
    o[5] = (float)(s[0] / (double)M);  // mean over no rows is NaN, as in the reference
    // x / (1e-8 + count) in fp32: the counts are integers below 2^24, so 1e-8f + count is count (1e-8f for none), and
    // the quotient of two such integers rounded through fp64 is the correctly rounded fp32 quotient
    const float rec = (float)(s[7] / (s[8] > 0.0 ? s[8] : (double)1e-8f));
    const float acc = (float)(s[9] / (s[10] > 0.0 ? s[10] : (double)1e-8f));
    const float prec = (float)(s[11] / (s[12] > 0.0 ? s[12] : (double)1e-8f));
    o[6] = rec;
    o[7] = prec;
    o[8] = acc;
    float r_first = 0.f;
    if (M > 0 && best_i < M) {
      const long long g = g0[best_i];
      if (g > -1 && mm[best_i] == g) r_first = (float)(1.0 / s[8]);
    }
    o[9] = (float)((double)prec * ((double)rec - (double)r_first));
  }
}

extern "C" int gfc_lg_validation_metrics(const float* log_assignment, const int64_t* gt_matches0,
                                         const int64_t* gt_matches1, const uint8_t* gt_assignment,
                                         const int64_t* matches0, const float* matching_scores0, int B, int M, int N,
                                         float nll_balancing, float* out, void* stream) {
  if (!log_assignment || !out || B <= 0 || M < 0 || N < 0) return GFC_ERR_INVALID;
  if ((M > 0 && (!gt_matches0 || !matches0 || !matching_scores0)) || (N > 0 && !gt_matches1)) return GFC_ERR_INVALID;
  if (M > 0 && N > 0 && (size_t)M * N >= ((size_t)1 << 40)) return GFC_ERR_INVALID;
  hipLaunchKernelGGL(lg_validation_kernel, dim3(B), dim3(LV_THREADS), 0, (hipStream_t)stream, log_assignment,
                     (const long long*)gt_matches0, (const long long*)gt_matches1,
                     (M > 0 && N > 0) ? gt_assignment : nullptr, (const long long*)matches0, matching_scores0, M, N,
                     (double)nll_balancing, out);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
