// The opt-in fp16 matcher (gfc_lg_params.precision = GFC_LG_FP16): products in fp16, sums in fp32.
//
// Both kernels run on v_mfma_f32_32x32x16_f16 (fp16 operands, fp32 accumulation, 32 cycles per instruction: the
// bf16 rate, 16x the fp32 MFMA's).  Operand lane map (same as the bf16 form): lane l (r = l&31, h = l>>5) holds
// A[row r][k = 8h + j] and B[k = 8h + j][col r] in element j = 0..7; the accumulator keeps the fp32 maps of common.h
// (register i of lane l: row acc_row(i, h), column r).
//
// Every fp32 -> fp16 conversion is a plain C++ cast, i.e. v_cvt_f16_f32 under the default round-to-nearest-even mode:
// the same rounding as torch's tensor.half().  (The round-toward-zero packing instruction is never emitted here.)
#include "common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ uint4 f32x8_to_f16x8(float4 a, float4 b) {
  f16x8 h;
  h[0] = (_Float16)a.x; h[1] = (_Float16)a.y; h[2] = (_Float16)a.z; h[3] = (_Float16)a.w;
  h[4] = (_Float16)b.x; h[5] = (_Float16)b.y; h[6] = (_Float16)b.z; h[7] = (_Float16)b.w;
  return __builtin_bit_cast(uint4, h);
}

// ---------------------------------------------------------------------------------------------
// GEMM  Y[M,N] = epilogue( [A0 | A1][M,K0+K1] . W[N,K0+K1]^T )
// ---------------------------------------------------------------------------------------------
struct GemmF16Args {
  const void* A0;
  const void* A1;
  const _Float16* W;
  const float* bias;
  const float* residual;  // fp32, ld = ldy
  const float* rot_cos;   // [M,64] each value twice, or
  const float* rot_sin;
  const float* rot_cs;    // packed [M][32][cos, sin]
  void* Y;
  long long sA, sW, sY;   // batch strides (elements) of A0, W and Y: blockIdx.z
  int lda0, lda1, ldw, ldy, K0, K1, M, N, rot_cols;
  int a0_f16, a1_f16, y_f16;
  float alpha;
};

#define HB_M 128
#define HB_N 128
#define HB_K 32
#define HB_LD (HB_K + 8)  // halves per LDS row: 80 bytes, 16-byte aligned, rows spread over the banks

// 256 threads = 4 waves in 2 x 2, each wave a 64 x 64 patch (2 x 2 accumulators of 32 x 32).  A and W tiles go through
// LDS (double-buffered, registers prefetch the next K tile while the current one is multiplied); an fp32 A is
// converted to fp16 on its way into LDS.
__global__ __launch_bounds__(256, 2) void gemm_f16_kernel(GemmF16Args g) {
  __shared__ __attribute__((aligned(16))) _Float16 sa[2][HB_M * HB_LD];
  __shared__ __attribute__((aligned(16))) _Float16 sw[2][HB_N * HB_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * HB_M, n0 = blockIdx.x * HB_N;
  const int z = blockIdx.z;
  const int ktiles0 = g.K0 / HB_K, ktiles = ktiles0 + g.K1 / HB_K;
  // staging: thread -> row tid >> 1, 16 consecutive k at (tid & 1) * 16
  const int st_row = tid >> 1, st_k = (tid & 1) * 16;
  const int arow = min(m0 + st_row, g.M - 1);
  const int wrow = min(n0 + st_row, g.N - 1);
  const char* a0p = (const char*)g.A0 + (size_t)z * g.sA * (g.a0_f16 ? 2 : 4);
  const _Float16* wp = g.W + (size_t)z * g.sW + (size_t)wrow * g.ldw + st_k;

  // named prefetch registers (an array here was demoted to scratch)
  uint4 ra0, ra1, ra2, ra3, rw0, rw1;
  auto load = [&](int kt) {
    const bool second = kt >= ktiles0;
    const int k = (second ? kt - ktiles0 : kt) * HB_K + st_k;
    const bool f16 = second ? g.a1_f16 : g.a0_f16;
    const char* base = second ? (const char*)g.A1 : a0p;
    const int lda = second ? g.lda1 : g.lda0;
    if (f16) {
      const uint4* p = reinterpret_cast<const uint4*>((const _Float16*)base + (size_t)arow * lda + k);
      ra0 = p[0]; ra1 = p[1];
    } else {
      const uint4* p = reinterpret_cast<const uint4*>((const float*)base + (size_t)arow * lda + k);
      ra0 = p[0]; ra1 = p[1]; ra2 = p[2]; ra3 = p[3];
    }
    const uint4* q = reinterpret_cast<const uint4*>(wp + (second ? g.K0 + (kt - ktiles0) * HB_K : kt * HB_K));
    rw0 = q[0]; rw1 = q[1];
    return f16;
  };
  auto store = [&](int buf, bool f16) {
    uint4* da = reinterpret_cast<uint4*>(&sa[buf][st_row * HB_LD + st_k]);
    if (f16) {
      da[0] = ra0; da[1] = ra1;
    } else {
      da[0] = f32x8_to_f16x8(__builtin_bit_cast(float4, ra0), __builtin_bit_cast(float4, ra1));
      da[1] = f32x8_to_f16x8(__builtin_bit_cast(float4, ra2), __builtin_bit_cast(float4, ra3));
    }
    uint4* dw = reinterpret_cast<uint4*>(&sw[buf][st_row * HB_LD + st_k]);
    dw[0] = rw0; dw[1] = rw1;
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  store(0, load(0));
  __syncthreads();
  for (int kt = 0; kt < ktiles; ++kt) {
    const bool has_next = kt + 1 < ktiles;
    bool nf16 = false;
    if (has_next) nf16 = load(kt + 1);
    const int buf = kt & 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      f16x8 af[2], bf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        af[t] = *reinterpret_cast<const f16x8*>(&sa[buf][(wm * 64 + t * 32 + r) * HB_LD + ks * 16 + 8 * h]);
        bf[t] = *reinterpret_cast<const f16x8*>(&sw[buf][(wn * 64 + t * 32 + r) * HB_LD + ks * 16 + 8 * h]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(af[i], bf[j], acc[i][j]);
    }
    if (has_next) store(buf ^ 1, nf16);
    __syncthreads();
  }

  // epilogue straight from the accumulator layout: lane = column, register = row.  Order of the fp32 path:
  // bias, rotary, alpha, residual.
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wn * 64 + j * 32 + r;
    const bool rot = (g.rot_cs != nullptr || g.rot_cos != nullptr) && n0 + wn * 64 + j * 32 < g.rot_cols;  // wave-uniform
    const float bi = (g.bias != nullptr && col < g.N) ? g.bias[col] : 0.f;
    const int d = col & 63;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + i * 32 + acc_row(e, h);
        float v = acc[i][j][e] + bi;
        if (rot) {
          // out[d] = t[d] cos + rot(t)[d] sin, rot(t)[2f] = -t[2f+1], rot(t)[2f+1] = t[2f]; the partner column is the
          // neighbouring lane
          const float p = __shfl_xor(v, 1);
          const int rr = min(row, g.M - 1);
          float c, s;
          if (g.rot_cs) {
            c = g.rot_cs[(size_t)rr * 64 + (d & ~1)];
            s = g.rot_cs[(size_t)rr * 64 + (d | 1)];
          } else {
            c = g.rot_cos[(size_t)rr * 64 + d];
            s = g.rot_sin[(size_t)rr * 64 + d];
          }
          v = (d & 1) ? v * c + p * s : v * c + (-p) * s;
        }
        v *= g.alpha;
        if (row < g.M && col < g.N) {
          const size_t o = (size_t)z * g.sY + (size_t)row * g.ldy + col;
          if (g.residual) v = g.residual[o] + v;
          if (g.y_f16) ((_Float16*)g.Y)[o] = (_Float16)v;
          else ((float*)g.Y)[o] = v;
        }
      }
    }
  }
}

static int launch_gemm_f16(const GemmF16Args& g, int batch, hipStream_t st) {
  hipLaunchKernelGGL(gemm_f16_kernel, dim3((g.N + HB_N - 1) / HB_N, (g.M + HB_M - 1) / HB_M, batch), dim3(256), 0, st, g);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

extern "C" int gfc_linear_f16(const void* A0, int a0_f16, int lda0, int K0, const void* A1, int a1_f16, int lda1, int K1,
                              const void* W, int ldw, const float* bias, float alpha, const float* residual,
                              const float* rot_cs, const float* rot_cos, const float* rot_sin, int rot_cols, void* Y,
                              int y_f16, int ldy, int M, int N, void* stream) {
  if (!A0 || !W || !Y || M <= 0 || N <= 0 || K0 <= 0 || K0 % HB_K || K1 < 0 || K1 % HB_K) return GFC_ERR_INVALID;
  if ((K1 > 0) != (A1 != nullptr)) return GFC_ERR_INVALID;
  // 16-byte operand loads: rows of fp16 operands start on 8 elements, fp32 ones on 4
  if (lda0 % (a0_f16 ? 8 : 4) || lda0 < K0 || ldw % 8 || ldw < K0 + K1 || ldy < N) return GFC_ERR_INVALID;
  if (A1 && (lda1 % (a1_f16 ? 8 : 4) || lda1 < K1)) return GFC_ERR_INVALID;
  if ((rot_cos == nullptr) != (rot_sin == nullptr) || (rot_cs && rot_cos)) return GFC_ERR_INVALID;
  if ((rot_cs || rot_cos) && (rot_cols <= 0 || rot_cols % 64 || rot_cols > N)) return GFC_ERR_INVALID;
  GemmF16Args g{};
  g.A0 = A0; g.A1 = A1; g.W = (const _Float16*)W; g.bias = bias; g.residual = residual;
  g.rot_cs = rot_cs; g.rot_cos = rot_cos; g.rot_sin = rot_sin; g.Y = Y;
  g.lda0 = lda0; g.lda1 = lda1; g.ldw = ldw; g.ldy = ldy; g.K0 = K0; g.K1 = K1; g.M = M; g.N = N;
  g.rot_cols = (rot_cs || rot_cos) ? rot_cols : 0;
  g.a0_f16 = a0_f16 != 0; g.a1_f16 = a1_f16 != 0; g.y_f16 = y_f16 != 0; g.alpha = alpha;
  return launch_gemm_f16(g, 1, (hipStream_t)stream);
}

extern "C" int gfc_batched_nt_f16(const void* A, int lda, long long strideA, const void* Bm, int ldb, long long strideB,
                                  float* Y, int ldy, long long strideY, int M, int N, int K, int batch, void* stream) {
  if (!A || !Bm || !Y || M <= 0 || N <= 0 || K <= 0 || K % HB_K || batch <= 0) return GFC_ERR_INVALID;
  if (lda % 8 || ldb % 8 || lda < K || ldb < K || ldy < N || strideA % 8 || strideB % 8) return GFC_ERR_INVALID;
  GemmF16Args g{};
  g.A0 = A; g.W = (const _Float16*)Bm; g.Y = Y;
  g.sA = strideA; g.sW = strideB; g.sY = strideY;
  g.lda0 = lda; g.ldw = ldb; g.ldy = ldy; g.K0 = K; g.M = M; g.N = N;
  g.a0_f16 = 1; g.alpha = 1.f;
  return launch_gemm_f16(g, batch, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Attention, head dim 64
// ---------------------------------------------------------------------------------------------
// The structure of attention.hip on the fp16 MFMA: per 32-key chunk a wave computes
//     S^T[key][q] = K . Q^T         A = K rows (LDS), B = Q (registers, 4 k-steps of 16 channels)
// whose accumulator registers 8s..8s+7, rounded to fp16, are the B operand of k-step s of
//     O^T[d][q] += V^T[d][key] . P^T[key][q]
// with the k order of the accumulator: element j of lane half h is key 16s + 8(j>>2) + 4h + (j&3).  V is therefore
// staged TRANSPOSED into LDS with bits 2 and 3 of the key index swapped, so that those 8 keys are 8 consecutive
// halves of one row of V^T.  Scores and soft-max statistics stay fp32; scale * log2(e) is applied to the fp32 score
// (one fma per element in front of the exp) so that Q is used exactly as stored.
#define FK 64            // keys per LDS tile
#define FLD (64 + 8)     // halves per row of the K and V^T images: 144 bytes

__device__ __forceinline__ int vt_pos(int key) { return (key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1); }

__global__ __launch_bounds__(256, 2) void attention_f16_kernel(const _Float16* __restrict__ Q, int ldq,
                                                             const _Float16* __restrict__ Kp, int ldk,
                                                             const _Float16* __restrict__ V, int ldv,
                                                             _Float16* __restrict__ O, int ldo,
                                                             const int4* __restrict__ problems, float scale_log2e,
                                                             int ksplit, float* __restrict__ part, int max_nq) {
  __shared__ __attribute__((aligned(16))) _Float16 sk[2][FK * FLD];
  __shared__ __attribute__((aligned(16))) _Float16 sv[2][64 * FLD];
  unsigned bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  {  // XCD-aware order (common.h), as the fp32 kernel
    const unsigned per_z = gridDim.x * gridDim.y;
    unsigned t = gfc_xcd_chunk(bx + gridDim.x * (by + gridDim.y * bz), per_z * gridDim.z);
    bz = t / per_z;
    t -= bz * per_z;
    by = t / gridDim.x;
    bx = t - by * gridDim.x;
  }
  const int4 pb = problems[bz];
  const int q_row0 = pb.x, nq = pb.y, kv_row0 = pb.z, nk = pb.w;
  const int ks = bx % ksplit;
  const int qt0 = (bx / ksplit) * 128;
  if (qt0 >= nq) return;  // uniform
  const int head = by;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  const int q = qt0 + wave * 32 + r;
  f16x8 qf[4];
  {
    const _Float16* qp = Q + (size_t)(q_row0 + min(q, nq - 1)) * ldq + head * 64 + 8 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const f16x8*>(qp + 16 * s);
  }
  f32x16 o[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) { o[0][e] = 0.f; o[1][e] = 0.f; }
  float m_run = -INFINITY, l_run = 0.f;

  const int ntiles_all = (nk + FK - 1) / FK;
  const int tiles_per = (ntiles_all + ksplit - 1) / ksplit;
  const int kt0 = ks * tiles_per;
  const int kt1 = min(ntiles_all, kt0 + tiles_per);
  // staging: thread -> key tid >> 3 (+32), 8 channels at (tid & 7) * 8; K row-major, V transposed
  const int st_key = tid >> 3, st_c = (tid & 7) * 8;
  uint4 kr0, kr1, vr0, vr1;
  auto load = [&](int kt) {
    const size_t r0 = kv_row0 + min(kt * FK + st_key, nk - 1);
    const size_t r1 = kv_row0 + min(kt * FK + st_key + 32, nk - 1);
    kr0 = *reinterpret_cast<const uint4*>(Kp + r0 * ldk + head * 64 + st_c);
    kr1 = *reinterpret_cast<const uint4*>(Kp + r1 * ldk + head * 64 + st_c);
    vr0 = *reinterpret_cast<const uint4*>(V + r0 * ldv + head * 64 + st_c);
    vr1 = *reinterpret_cast<const uint4*>(V + r1 * ldv + head * 64 + st_c);
  };
  auto store = [&](int buf) {
    *reinterpret_cast<uint4*>(&sk[buf][st_key * FLD + st_c]) = kr0;
    *reinterpret_cast<uint4*>(&sk[buf][(st_key + 32) * FLD + st_c]) = kr1;
    const _Float16* v0 = reinterpret_cast<const _Float16*>(&vr0);
    const _Float16* v1 = reinterpret_cast<const _Float16*>(&vr1);
    const int p0 = vt_pos(st_key), p1 = vt_pos(st_key + 32);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      sv[buf][(st_c + c) * FLD + p0] = v0[c];
      sv[buf][(st_c + c) * FLD + p1] = v1[c];
    }
  };

  if (kt0 < kt1) {
    load(kt0);
    store(0);
  }
  __syncthreads();
  for (int kt = kt0; kt < kt1; ++kt) {
    const bool has_next = kt + 1 < kt1;
    if (has_next) load(kt + 1);
    const int buf = (kt - kt0) & 1;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int key0 = kt * FK + half * 32;
      if (key0 >= nk) break;  // uniform
      f32x16 s;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = 0.f;
      const _Float16* kp = &sk[buf][(half * 32 + r) * FLD + 8 * h];
#pragma unroll
      for (int st = 0; st < 4; ++st) s = mfma16(*reinterpret_cast<const f16x8*>(kp + 16 * st), qf[st], s);
      if (key0 + 32 > nk) {
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (key0 + acc_row(e, h) >= nk) s[e] = -INFINITY;
      }
      float mx = s[0];
#pragma unroll
      for (int e = 1; e < 16; ++e) mx = fmaxf(mx, s[e]);
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run, mx * scale_log2e);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      float rs = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        s[e] = __builtin_amdgcn_exp2f(fmaf(s[e], scale_log2e, -m_new));
        rs += s[e];
      }
      rs += __shfl_xor(rs, 32);
      l_run = l_run * alpha + rs;
      if (!__all(m_new == m_run)) {
#pragma unroll
        for (int e = 0; e < 16; ++e) { o[0][e] *= alpha; o[1][e] *= alpha; }
      }
      m_run = m_new;
      f16x8 pf[2];
#pragma unroll
      for (int e = 0; e < 16; ++e) pf[e >> 3][e & 7] = (_Float16)s[e];
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const f16x8 vf =
              *reinterpret_cast<const f16x8*>(&sv[buf][(dt * 32 + r) * FLD + half * 32 + 16 * st + 8 * h]);
          o[dt] = mfma16(vf, pf[st], o[dt]);
        }
    }
    if (has_next) store(buf ^ 1);
    __syncthreads();
  }

  // lane holds O[q][32 dt + 8 g + 4 h + (0..3)] in registers 4g..4g+3 of o[dt]
  if (q >= nq) return;
  if (part != nullptr) {
    float* pp = part + ((((size_t)bz * gridDim.y + head) * max_nq + q) * ksplit + ks) * GFC_ATT_PART;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float* dst = pp + dt * 32 + 8 * g + 4 * h;
        dst[0] = o[dt][4 * g]; dst[1] = o[dt][4 * g + 1]; dst[2] = o[dt][4 * g + 2]; dst[3] = o[dt][4 * g + 3];
      }
    if (h == 0) { pp[64] = m_run; pp[65] = l_run; }
    return;
  }
  const float inv = 1.f / l_run;
  _Float16* op = O + (size_t)(q_row0 + q) * ldo + head * 64 + 4 * h;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f16x4 v;
      v[0] = (_Float16)(o[dt][4 * g] * inv); v[1] = (_Float16)(o[dt][4 * g + 1] * inv);
      v[2] = (_Float16)(o[dt][4 * g + 2] * inv); v[3] = (_Float16)(o[dt][4 * g + 3] * inv);
      *reinterpret_cast<f16x4*>(op + dt * 32 + 8 * g) = v;
    }
}

// combine the key-split partials (layout of attention.hip): one wave per (query, head), lane = channel
__global__ __launch_bounds__(256) void attention_f16_merge_kernel(const float* __restrict__ part, _Float16* __restrict__ O,
                                                                  int ldo, const int4* __restrict__ problems, int ksplit,
                                                                  int max_nq) {
  const int4 pb = problems[blockIdx.z];
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), head = blockIdx.y, lane = threadIdx.x & 63;
  if (q >= pb.y) return;
  const float* pp = part + (((size_t)blockIdx.z * gridDim.y + head) * max_nq + q) * ksplit * GFC_ATT_PART;
  float m = -INFINITY;
  for (int s = 0; s < ksplit; ++s) m = fmaxf(m, pp[s * GFC_ATT_PART + 64]);
  float acc = 0.f, l = 0.f;
  for (int s = 0; s < ksplit; ++s) {
    const float ms = pp[s * GFC_ATT_PART + 64];
    const float w = (ms == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(ms - m);
    acc += w * pp[s * GFC_ATT_PART + lane];
    l += w * pp[s * GFC_ATT_PART + 65];
  }
  O[(size_t)(pb.x + q) * ldo + head * 64 + lane] = (_Float16)(acc / l);
}

extern "C" int gfc_attention_f16(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                                 const int32_t* problems, int n_problems, int max_nq, int heads, float scale, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!Q || !K || !V || !O || !problems || n_problems <= 0 || max_nq <= 0 || heads <= 0) return GFC_ERR_INVALID;
  if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4 || ldq < 64 * heads || ldk < 64 * heads || ldv < 64 * heads ||
      ldo < 64 * heads)
    return GFC_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int4* pt = reinterpret_cast<const int4*>(problems);
  const float sl2 = scale * 1.4426950408889634f;
  // the key split of gfc_attention (gfc_att_split), merged below
  const long long wgs = (long long)((max_nq + 127) / 128) * heads * n_problems;
  const int ksplit = ws != nullptr ? gfc_att_split(wgs, (size_t)n_problems * max_nq, heads, ws_bytes) : 1;
  float* part = ksplit > 1 ? (float*)ws : nullptr;
  hipLaunchKernelGGL(attention_f16_kernel, dim3(((max_nq + 127) / 128) * ksplit, heads, n_problems), dim3(256), 0, st,
                     (const _Float16*)Q, ldq, (const _Float16*)K, ldk, (const _Float16*)V, ldv, (_Float16*)O, ldo, pt, sl2,
                     ksplit, part, max_nq);
  GFC_LAUNCH_CHECK();
  if (ksplit > 1) {
    hipLaunchKernelGGL(attention_f16_merge_kernel, dim3((max_nq + 3) / 4, heads, n_problems), dim3(256), 0, st, part,
                       (_Float16*)O, ldo, pt, ksplit, max_nq);
    GFC_LAUNCH_CHECK();
  }
  return GFC_OK;
}
