// The backward of one LightGlue FFN block with the projection in front of it, for R packed rows.  The closed form, the
// workspace and the refusals are stated in include/gfc_amd_ffn_backward.h.
//
// In launch order:
//   m = ctx Wout^T + bout, h = [x | m] W0^T + b0      gfc_linear, the forward's entry point
//   da = dy W3                                         hb_gemm_kernel (v_mfma_f32_32x32x2_f32, exact fp32)
//   (h, da) -> (dh, a) in place, chunk sums of dgamma, dbeta, db0     fb_ln_gelu_backward_kernel, a wave per row
//   dW3 = dy^T a, dW0 = dh^T [x | m] (split over rows), dm = dh W0[:, 256:], dx_in = dy + dh W0[:, :256]
//   dWout = dm^T ctx (split over rows), dctx = dm Wout
//   column sums db3, dbout per chunk of rows; the finishing launches add chunks and split-K parts in ascending order.
// Nothing is accumulated by atomics and no sum depends on the order in which workgroups run.
#include "lg_backward_common.h"
#include "../../include/gfc_amd_ffn_backward.h"

#define FB_H 512             // the FFN's hidden width: 2 d
#define FB_ROW_STRIDE 1536   // floats of one row-kernel chunk's record: 512 sums of du n | 512 of du | 512 of dh

// ---- workspace: one description, used by the *_workspace_bytes export and by the launcher ----------------------------
static inline bool fb_rows_ok(int R) { return R >= 1 && R <= HB_MAX_ROWS; }
struct FbLayout { size_t m, h, da, dm, wpart, cpart, rpart, total; };
static inline FbLayout fb_layout(int R) {
  const size_t r = (size_t)R, f = sizeof(float);
  gfc_slots s;
  return {s.take(r * HB_D * f), s.take(r * FB_H * f), s.take(r * FB_H * f), s.take(r * HB_D * f),
          s.take((size_t)hb_split(R).parts * FB_H * FB_H * f), s.take((size_t)hb_chunks(r) * HB_CS_STRIDE * f),
          s.take((size_t)hb_chunks(r) * FB_ROW_STRIDE * f), s.off};
}

// ---- LayerNorm(512) + GELU backward: a workgroup per chunk of HB_CS_ROWS rows, a wave per row ------------------------
// Lane l holds columns 4 l .. 4 l + 3 and 256 + 4 l .. 256 + 4 l + 3 of its row: two 16-byte loads per operand.  The
// statistics are two-pass (mean, then centred squares).  h is overwritten by dh and da by a: a lane writes only what it
// has read.  The wave's sums over its rows (ascending) meet the other three waves' in LDS and are added in wave order.
__global__ __launch_bounds__(256) void fb_ln_gelu_backward_kernel(float* h, float* da, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, size_t R,
                                                                  float* __restrict__ part) {
  __shared__ float red[4][FB_ROW_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t r_begin = (size_t)blockIdx.x * HB_CS_ROWS, r_end = min(R, r_begin + HB_CS_ROWS);
  float g[8], b[8], sg[8], sb[8], sh[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int col = (q >> 2) * 256 + 4 * lane + (q & 3);
    g[q] = gamma[col];
    b[q] = beta[col];
    sg[q] = sb[q] = sh[q] = 0.f;
  }
  const float inv = 1.f / FB_H;
  for (size_t row = r_begin + wave; row < r_end; row += 4) {
    float4* hp = reinterpret_cast<float4*>(h + row * FB_H) + lane;
    float4* ap = reinterpret_cast<float4*>(da + row * FB_H) + lane;
    const float4 h0 = hp[0], h1 = hp[64], d0 = ap[0], d1 = ap[64];
    float hv[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
    const float dv[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += hv[q];
    const float mu = wave_sum(s) * inv;
    s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      hv[q] -= mu;
      s += hv[q] * hv[q];
    }
    const float rstd = 1.f / sqrtf(wave_sum(s) * inv + 1e-5f);
    float nv[8], dn[8], av[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      nv[q] = hv[q] * rstd;
      const float u = nv[q] * g[q] + b[q];
      const float cdf = 0.5f * (1.f + gfc_gelu_erf(u * 0.70710678118654752440f));  // Phi(u), the forward's erf
      const float pdf = expf(-0.5f * (u * u)) * 0.39894228040143267794f;            // phi(u), exp of a value <= 0
      av[q] = gfc_gelu(u);
      const float du = dv[q] * (cdf + u * pdf);
      sg[q] += du * nv[q];
      sb[q] += du;
      dn[q] = du * g[q];
      s1 += dn[q];
      s2 += dn[q] * nv[q];
    }
    const float m1 = wave_sum(s1) * inv, m2 = wave_sum(s2) * inv;
    float o[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      o[q] = rstd * ((dn[q] - m1) - nv[q] * m2);
      sh[q] += o[q];
    }
    hp[0] = make_float4(o[0], o[1], o[2], o[3]);
    hp[64] = make_float4(o[4], o[5], o[6], o[7]);
    ap[0] = make_float4(av[0], av[1], av[2], av[3]);
    ap[64] = make_float4(av[4], av[5], av[6], av[7]);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int col = (q >> 2) * 256 + 4 * lane + (q & 3);
    red[wave][col] = sg[q];
    red[wave][FB_H + col] = sb[q];
    red[wave][2 * FB_H + col] = sh[q];
  }
  __syncthreads();
  float* out = part + (size_t)blockIdx.x * FB_ROW_STRIDE;
  for (int e = tid; e < FB_ROW_STRIDE; e += 256) out[e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

// the row kernel's chunk records [dgamma | dbeta | db0] in one launch, the same sums
__global__ __launch_bounds__(256) void fb_row_finish_kernel(const float* __restrict__ rec, int n,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            float* __restrict__ db0) {
  const int e = blockIdx.x * 256 + threadIdx.x;  // < FB_ROW_STRIDE: the grid is FB_ROW_STRIDE / 256 workgroups
  double s = 0.0;
#pragma unroll 8
  for (int p = 0; p < n; ++p) s += (double)rec[(size_t)p * FB_ROW_STRIDE + e];
  float* out = e < FB_H ? dgamma : e < 2 * FB_H ? dbeta : db0;
  out[e % FB_H] = (float)s;
}

// dx_in += dy
__global__ __launch_bounds__(256) void fb_residual_kernel(float* __restrict__ dx, const float* __restrict__ dy, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dx[i] = dy[i] + dx[i];
}

extern "C" size_t gfc_lg_ffn_backward_workspace_bytes(int R) { return fb_rows_ok(R) ? fb_layout(R).total : 0; }

extern "C" int gfc_lg_ffn_backward(const float* x, const float* ctx, const float* dy, const float* Wout,
                                   const float* bout, const float* W0, const float* b0, const float* gamma,
                                   const float* beta, const float* W3, int R, float* dWout, float* dbout, float* dW0,
                                   float* db0, float* dgamma, float* dbeta, float* dW3, float* db3, float* dx_in,
                                   float* dctx, void* ws, size_t ws_bytes, void* stream) {
  if (!fb_rows_ok(R)) return GFC_ERR_INVALID;
  if (!x || !ctx || !dy || !W0 || !b0 || !gamma || !beta || !W3 || !dW0 || !db0 || !dgamma || !dbeta || !dW3 || !db3)
    return GFC_ERR_INVALID;
  if ((Wout == nullptr) != (bout == nullptr) || (Wout == nullptr) != (dWout == nullptr) ||
      (Wout == nullptr) != (dbout == nullptr))
    return GFC_ERR_INVALID;
  const FbLayout L = fb_layout(R);
  if (!ws || ws_bytes < L.total || ((uintptr_t)ws & 15)) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  float* m = (float*)(base + L.m);
  float* h = (float*)(base + L.h);    // dh after the row kernel
  float* da = (float*)(base + L.da);  // a after the row kernel
  float* dm = (float*)(base + L.dm);
  float* wpart = (float*)(base + L.wpart);
  float* cpart = (float*)(base + L.cpart);
  float* rpart = (float*)(base + L.rpart);
  const size_t rows = (size_t)R;
  const int chunks = hb_chunks(rows);
  const HbSplit sp = hb_split(R);

  // the forward, with the forward's entry point
  const float* msg = ctx;
  if (Wout) {
    HB_TRY(gfc_linear(ctx, HB_D, HB_D, nullptr, 0, 0, Wout, HB_D, bout, nullptr, nullptr, 1.f, nullptr, nullptr, nullptr,
                      0, m, HB_D, R, HB_D, stream));
    msg = m;
  }
  HB_TRY(gfc_linear(x, HB_D, HB_D, msg, HB_D, HB_D, W0, FB_H, b0, nullptr, nullptr, 1.f, nullptr, nullptr, nullptr, 0, h,
                    FB_H, R, FB_H, stream));

  // da = dy W3
  HbGemm q{};
  q.alpha = 1.f;
  q.A = dy; q.a_m = HB_D; q.a_k = 1;
  q.B = W3; q.b_k = FB_H;
  q.C = da; q.c_m = FB_H;
  q.M = R; q.N = FB_H; q.K = HB_D; q.kchunk = HB_D;
  HB_TRY(hb_gemm(q, true, 1, 1, st));

  hipLaunchKernelGGL(fb_ln_gelu_backward_kernel, dim3(chunks), dim3(256), 0, st, h, da, gamma, beta, rows, rpart);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(fb_row_finish_kernel, dim3(FB_ROW_STRIDE / 256), dim3(256), 0, st, rpart, chunks, dgamma, dbeta, db0);
  GFC_LAUNCH_CHECK();

  // the weight gradients: A^T B over the rows, split over rows; the parts buffer is used by one of them at a time
  HbGemm w{};
  w.alpha = 1.f;
  w.a_m = 1; w.K = R; w.kchunk = sp.kchunk;
  // dW3 [256,512] = dy^T a
  w.A = dy; w.a_k = HB_D; w.B = da; w.b_k = FB_H; w.C = wpart; w.c_m = FB_H; w.c_p = (long long)HB_D * FB_H;
  w.M = HB_D; w.N = FB_H;
  HB_TRY(hb_gemm(w, false, sp.parts, 1, st));
  HB_TRY(hb_finish(wpart, sp.parts, (size_t)HB_D * FB_H, HB_D * FB_H, dW3, st));
  HB_TRY(hb_colsums(dy, nullptr, nullptr, nullptr, 0, rows, cpart, 1.f, db3, nullptr, nullptr, st));
  // dW0 [512,512] = dh^T [x | m], a half of the columns per launch
  w.A = h; w.a_k = FB_H; w.B = x; w.b_k = HB_D; w.C = wpart; w.c_m = FB_H; w.c_p = (long long)FB_H * FB_H;
  w.M = FB_H; w.N = HB_D;
  HB_TRY(hb_gemm(w, false, sp.parts, 1, st));
  w.B = msg; w.C = wpart + HB_D;
  HB_TRY(hb_gemm(w, false, sp.parts, 1, st));
  HB_TRY(hb_finish(wpart, sp.parts, (size_t)FB_H * FB_H, FB_H * FB_H, dW0, st));

  // dcat = dh W0: the second half is dm, the first one joins the residual
  HbGemm d{};
  d.alpha = 1.f;
  d.A = h; d.a_m = FB_H; d.a_k = 1;
  d.b_k = FB_H;
  d.c_m = HB_D;
  d.M = R; d.N = HB_D; d.K = FB_H; d.kchunk = FB_H;
  float* dmsg = Wout ? dm : dctx;  // without Wout the message is the context
  if (dmsg) {
    d.B = W0 + HB_D; d.C = dmsg;
    HB_TRY(hb_gemm(d, true, 1, 1, st));
  }
  if (dx_in) {
    d.B = W0; d.C = dx_in;
    HB_TRY(hb_gemm(d, true, 1, 1, st));
    const size_t n = rows * HB_D;
    hipLaunchKernelGGL(fb_residual_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dx_in, dy, n);
    GFC_LAUNCH_CHECK();
  }
  if (Wout) {
    // dWout [256,256] = dm^T ctx
    w.A = dm; w.a_k = HB_D; w.B = ctx; w.b_k = HB_D; w.C = wpart; w.c_m = HB_D; w.c_p = (long long)HB_D * HB_D;
    w.M = HB_D; w.N = HB_D;
    HB_TRY(hb_gemm(w, false, sp.parts, 1, st));
    HB_TRY(hb_finish(wpart, sp.parts, (size_t)HB_D * HB_D, HB_D * HB_D, dWout, st));
    HB_TRY(hb_colsums(dm, nullptr, nullptr, nullptr, 0, rows, cpart, 1.f, dbout, nullptr, nullptr, st));
    if (dctx) {
      d.A = dm; d.a_m = HB_D; d.K = HB_D; d.kchunk = HB_D;
      d.B = Wout; d.b_k = HB_D; d.C = dctx;
      HB_TRY(hb_gemm(d, true, 1, 1, st));
    }
  }
  return GFC_OK;
}
