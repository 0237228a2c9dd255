// Perspective warp on the GPU: the pair generator of the `homographies` dataset (reference
// gluefactory/datasets/homographies.py:37-44 `sample_homography` -> cv2.warpPerspective(img, H, size), twice per pair).
//
// The rule is a restatement of OpenCV's warpPerspective with INTER_LINEAR and BORDER_CONSTANT 0 (OpenCV is absent here ->
// parity UNPINNED; the pin is the float64 restatement of tests/warp_reference.py): per destination pixel the source
// position in fp64 with ONE divide (32 / W), rounded to nearest even onto a 1/32-pixel grid; the four bilinear weights are
// products of n/32 fractions and therefore exact in fp32; the four products are summed left to right in fp32.  The matrix
// is destination -> source; inverting the sampler's H_ is the host's job (float64).
//
// One thread per output pixel, x fastest: planar writes are coalesced, the taps of neighbouring lanes are neighbours in
// the source (L2 / L1 serve the overlap); the nine matrix entries and the source index are uniform per block.  HBM-bound
// like resize_kernel: B warps of one resident source read it once from HBM, B times from cache.  No workspace, no LDS.
#include "common.h"

enum { WP_F32_CHW = 0, WP_U8_HWC = 1 };

// One tap at WINDOW coordinates; outside the window is outside the image (0), even where the plane goes on.
// U8: numpy_image_to_torch's value / 255.  numpy divides in float64 and rounds to fp32; the correctly rounded fp32
// quotient is the same number (53 >= 2 * 24 + 2 bits: the double rounding of a quotient is innocuous).
template <bool U8>
__device__ __forceinline__ float warp_tap(const void* src, int H, int W, int C, int c, int left, int top, int cw, int ch,
                                          int y, int x) {
  if (x < 0 || y < 0 || x >= cw || y >= ch) return 0.f;
  const size_t yy = (size_t)(top + y), xx = (size_t)(left + x);
  if (U8) return (float)static_cast<const unsigned char*>(src)[(yy * W + xx) * C + c] / 255.f;
  return static_cast<const float*>(src)[((size_t)c * H + yy) * W + xx];
}

template <bool U8>
__global__ __launch_bounds__(256) void warp_perspective_kernel(const void* __restrict__ src, int S, int C, int H, int W,
                                                               int left, int top, int cw, int ch,
                                                               const int* __restrict__ src_index,
                                                               const double* __restrict__ M, int B, int gray,
                                                               float* __restrict__ dst, int OH, int OW) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y * blockDim.y + threadIdx.y;
  if (ox >= OW || oy >= OH) return;
  const int OC = gray ? 1 : C;
  const size_t plane = (size_t)OH * OW;
  const size_t src_stride = (size_t)C * H * W * (U8 ? 1 : 4);
  for (int b = blockIdx.z; b < B; b += gridDim.z) {
    float* db = dst + (size_t)b * OC * plane + (size_t)oy * OW + ox;
    const int s = src_index[b];
    if (s < 0 || s >= S) {  // device data the entry point cannot check: no read, zeros out
      for (int c = 0; c < OC; ++c) db[c * plane] = 0.f;
      continue;
    }
    const double* m = M + (size_t)b * 9;
    const double x = (double)ox, y = (double)oy;
    const double X = m[0] * x + (m[1] * y + m[2]);
    const double Y = m[3] * x + (m[4] * y + m[5]);
    double Wd = m[6] * x + (m[7] * y + m[8]);
    Wd = Wd != 0.0 ? 32.0 / Wd : 0.0;
    // saturate to int32, then round half to even (v_rndne_f64); the bounds are exact doubles
    const double fX = fmin(fmax(X * Wd, -2147483648.0), 2147483647.0);
    const double fY = fmin(fmax(Y * Wd, -2147483648.0), 2147483647.0);
    const int qx = (int)rint(fX), qy = (int)rint(fY);
    const int sx = qx >> 5, sy = qy >> 5;
    const float ax = (float)(qx & 31) * (1.f / 32.f), ay = (float)(qy & 31) * (1.f / 32.f);
    const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay), w10 = (1.f - ax) * ay, w11 = ax * ay;
    const char* sb = static_cast<const char*>(src) + (size_t)s * src_stride;
    float v[3];
    for (int c = 0; c < C; ++c) {
      const float t00 = warp_tap<U8>(sb, H, W, C, c, left, top, cw, ch, sy, sx);
      const float t01 = warp_tap<U8>(sb, H, W, C, c, left, top, cw, ch, sy, sx + 1);
      const float t10 = warp_tap<U8>(sb, H, W, C, c, left, top, cw, ch, sy + 1, sx);
      const float t11 = warp_tap<U8>(sb, H, W, C, c, left, top, cw, ch, sy + 1, sx + 1);
      v[c] = t00 * w00 + t01 * w01 + t10 * w10 + t11 * w11;
    }
    if (gray) {
      db[0] = 0.299f * v[0] + 0.587f * v[1] + 0.114f * v[2];  // (image * gs).sum(0) after the warp
    } else {
      for (int c = 0; c < C; ++c) db[c * plane] = v[c];
    }
  }
}

extern "C" int gfc_warp_perspective(const void* src, int src_kind, int S, int C, int H, int W, int left, int top, int cw,
                                    int ch, const int* src_index, const double* M, int B, int gray, float* dst, int OH,
                                    int OW, void* stream) {
  if (!src || !dst || !src_index || !M || S <= 0 || B <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return GFC_ERR_INVALID;
  if (src_kind != WP_F32_CHW && src_kind != WP_U8_HWC) return GFC_ERR_INVALID;
  if (C != 1 && C != 3) return GFC_ERR_INVALID;
  if (gray && C != 3) return GFC_ERR_INVALID;
  if (left < 0 || top < 0 || cw <= 0 || ch <= 0 || left > W - cw || top > H - ch) return GFC_ERR_INVALID;  // window leaves the plane
  const dim3 block(32, 8), grid((OW + 31) / 32, (OH + 7) / 8, B < 65535 ? B : 65535);
  if (src_kind == WP_U8_HWC)
    hipLaunchKernelGGL(warp_perspective_kernel<true>, grid, block, 0, (hipStream_t)stream, src, S, C, H, W, left, top, cw,
                       ch, src_index, M, B, gray, dst, OH, OW);
  else
    hipLaunchKernelGGL(warp_perspective_kernel<false>, grid, block, 0, (hipStream_t)stream, src, S, C, H, W, left, top, cw,
                       ch, src_index, M, B, gray, dst, OH, OW);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
