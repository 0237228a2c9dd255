// Flash-style multi-head attention on fp32 MFMA (head_dim 64), score matrix never materialised.
//
// Replaces F.scaled_dot_product_attention in SelfBlock (reference
// gluefactory/models/matchers/lightglue.py:119-122,160-162) and the bidirectional cross attention
// of CrossBlock (lightglue.py:207-217: softmax over rows and over columns of the same similarity
// matrix), issued as two problems of one launch -- or, for large uniform batches, as one launch per direction with the
// raw score tiles handed from the first to the second (gfc_attention_cross_stored below).
//
// Layout: one workgroup = 4 waves = 128 query rows of one (problem, head); each wave owns 32
// queries.  Keys/values stream through LDS in tiles of 64.  Per 32-key half tile a wave computes
//     S^T[key][q] = K . Q^T            A = K rows (LDS, ds_read_b128), B = Q (registers)
// so that the accumulator holds, for lane (q = lane&31, half h), the 16 keys r -> (r&3)+8(r>>2)+4h.
// Softmax statistics are then lane-local (+ one exchange with lane^32), and the accumulator
// registers are *already* the B operand of
//     O^T[d][q] += V^T[d][key] . P^T[key][q]      A = V[key][d] (LDS, ds_read_b32), B = P register r
// -- no transpose, no LDS round trip for P.  O^T keeps q on the lane, so the running rescale is a
// per-lane scalar multiply.
#include <limits.h>
#include <stdlib.h>

#include "../../include/gfc_amd_cross_attention.h"
#include "common.h"

#define AK 64    // keys per LDS tile
#define AD 64    // head dim
#define AKLD (AD + 4)
#define AW 4     // waves per workgroup

#ifdef ATT_DIAG  // diagnostic build (tools/micro/attn_timeline.py): per-wave cycle accounting, 8 words per wave
__device__ unsigned long long* g_att_diag_dev = nullptr;
extern "C" void gfc_diag_set_attn_stamps(void* p) {
  unsigned long long* q = (unsigned long long*)p;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_att_diag_dev), &q, sizeof(q));
}
#define ATT_T(v_) const unsigned long long v_ = __builtin_readcyclecounter()
#else
#define ATT_T(v_) do {} while (0)
#endif

// QT = 32-query tiles per wave (1 or 2): a workgroup covers 128*QT queries.  With QT = 2 every K / V
// fragment read from LDS feeds two independent score tiles, the barrier count per query halves, and
// the MFMAs of one tile can issue while the softmax of the other runs on the VALU.
//
// SM: the hand-over of the cross block's score matrix between its two directions (gfc_attention_cross_stored).  Both
// directions multiply the same rows, sim[i][j] = qk0_i . qk1_j, and a score element is the same number in both: what
// lane (q = i) holds in register r for key j is what lane (q = j) of the other direction wants for key i.
//   ATT_PLAIN    nothing of it (gfc_attention)
//   ATT_STORE_S  first direction (queries i of image 0): additionally writes every raw score tile, before the soft-max
//                touches it, to Sg[(problem, head)][j][i], i contiguous, row pitch ldS -- per register the 32 lanes of a
//                half wave store 128 consecutive bytes.  Its own result is that of ATT_PLAIN bit for bit.
//   ATT_LOAD_S   second direction (queries j of image 1; problems[] is still the FIRST direction's table and is read
//                swapped): no Q fragments, no K tile, no K.Q^T; lane (j, h) loads its 16 scores of a half tile as four
//                float4 from Sg[..][j][key0 + 4h + 8g ..+3], which is the accumulator layout, one half tile ahead of the
//                P.V that consumes them.  Only V goes through LDS.
// Sg has s_rows = N rounded up to 32 rows of ldS = M rounded up to 32 floats per (problem, head), so that whole 32x32
// tiles are stored without a per-element guard; what lies beyond a problem's own (n, m) is never used by the reader
// (its key mask replaces those columns before any arithmetic, NaN or not).  ksplit must be 1 with either flag.
enum { ATT_PLAIN = 0, ATT_STORE_S = 1, ATT_LOAD_S = 2 };
template <int QT, int SM = ATT_PLAIN>
__global__ __launch_bounds__(64 * AW, 2) void attention_kernel(const float* __restrict__ Q, int ldq,
                                                           const float* __restrict__ Kp, int ldk,
                                                           const float* __restrict__ V, int ldv,
                                                           float* __restrict__ O, int ldo,
                                                           const int4* __restrict__ problems, float scale_log2e,
                                                           int ksplit, float* __restrict__ part, int max_nq, int xcd_remap,
                                                           float* __restrict__ Sg = nullptr, int ldS = 0, int s_rows = 0) {
  // double-buffered K / V tiles: [2][AK*AKLD] keys, then [2][AK*AD] values (67.6 KB -> 2 workgroups / CU); ATT_LOAD_S
  // stages no keys
  constexpr int KS = SM == ATT_LOAD_S ? 0 : 2 * AK * AKLD;  // floats of the K buffers
  __shared__ __attribute__((aligned(16))) float smem[KS + 2 * AK * AD];
  constexpr int AQ = 32 * AW * QT;
  constexpr int T = 64 * AW;
  constexpr int NLD = (AK * AD / 4) / T;  // float4 of K (and of V) per thread per tile

  // XCD-aware order (common.h): the query blocks (and key splits) of one (problem, head) run at the same time behind
  // one L2, so its K and V rows come from HBM once instead of once per query block
  unsigned bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (xcd_remap) {
    const unsigned per_z = gridDim.x * gridDim.y;
    unsigned t = gfc_xcd_chunk(bx + gridDim.x * (by + gridDim.y * bz), per_z * gridDim.z);
    bz = t / per_z;
    t -= bz * per_z;
    by = t / gridDim.x;
    bx = t - by * gridDim.x;
  }
  int4 pb = problems[bz];
  if (SM == ATT_LOAD_S) pb = make_int4(pb.z, pb.w, pb.x, pb.y);  // the other direction of the same pair
  // (with a score array: never more rows or columns than it holds)
  const int q_row0 = pb.x, nq = SM == ATT_PLAIN ? pb.y : min(pb.y, SM == ATT_STORE_S ? ldS : s_rows);
  const int kv_row0 = pb.z, nk = SM == ATT_PLAIN ? pb.w : min(pb.w, SM == ATT_STORE_S ? s_rows : ldS);
  // key split (small problems only): bx = q-block * ksplit + s; split s walks its share of the key
  // tiles and leaves an un-normalised partial (O, m, l) for attention_merge_kernel
  const int ks = bx % ksplit;
  const int qt0 = (bx / ksplit) * AQ;
  if (qt0 >= nq) return;  // uniform for the whole workgroup
  const int head = by;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
#ifdef ATT_DIAG
  unsigned long long d_bar = 0, d_store = 0;
#endif
  ATT_T(t_entry);

  // ---- Q fragments: lane (q, h) keeps Q[q][8g + 4h + s], g = 0..7, s = 0..3 ----
  int q[QT];
  float4 qf[QT][8];
  // score array of this (problem, head), and this lane's element offset in it: ATT_STORE_S writes row key0 + krow + 4h,
  // column q; ATT_LOAD_S reads row q, columns key0 + 4h + ...
  float* const Ss = SM == ATT_PLAIN ? nullptr : Sg + ((size_t)bz * gridDim.y + head) * s_rows * ldS;
  unsigned s_off[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    q[t] = qt0 + (wave * QT + t) * 32 + l31;
    const int qc = min(q[t], nq - 1);
    s_off[t] = SM == ATT_STORE_S ? (unsigned)(4 * h * ldS + q[t]) : (unsigned)(qc * ldS + 4 * h);
    if constexpr (SM != ATT_LOAD_S) {
    const float* qp = Q + (size_t)(q_row0 + qc) * ldq + head * AD + 4 * h;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      // scale * log2(e) folded into the query fragment once (round 5): the scores then come out of the matrix pipe in
      // the soft-max's own units and the per-element multiply in front of every v_exp_f32 is gone -- on this part every
      // VALU instruction costs the fp32 matrix pipe its issue cycles (tools/micro/mfma_valu_hybrid.hip)
      const float4 qv = *reinterpret_cast<const float4*>(qp + 8 * g);
      qf[t][g] = make_float4(qv.x * scale_log2e, qv.y * scale_log2e, qv.z * scale_log2e, qv.w * scale_log2e);
    }
    }
  }

  f32x16 o[QT][2];
  float m_run[QT], l_run[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[t][0][r] = 0.f; o[t][1][r] = 0.f; }
    m_run[t] = -INFINITY;
    l_run[t] = 0.f;
  }

  const int ntiles_all = (nk + AK - 1) / AK;
  const int tiles_per = (ntiles_all + ksplit - 1) / ksplit;
  const int kt0 = ks * tiles_per;
  const int kt1 = min(ntiles_all, kt0 + tiles_per);
  // staging: thread -> (key = tid>>4 (+16 i), 4 floats at c4); the next tile is prefetched into
  // registers while the current one is multiplied, then written to the other LDS buffer
  const int st_key = tid >> 4, st_c4 = (tid & 15) * 4;  // keys st_key + (T/16) * i
  const float* kbase = Kp + head * AD + st_c4;
  const float* vbase = V + head * AD + st_c4;
  // named prefetch registers (arrays were demoted to private memory by hipcc)
  float4 kr0, kr1, kr2, kr3, vr0, vr1, vr2, vr3;
  static_assert(NLD == 4, "staging layout");
#define ATT_LOAD(kt_)                                                                                                                                                                       \
  do {                                                                                                                                                                                      \
    const int kb_ = (kt_) * AK + st_key;                                                                                                                                                    \
    { const size_t r_ = kv_row0 + min(kb_ + (T / 16) * 0, nk - 1); if constexpr (SM != ATT_LOAD_S) kr0 = *reinterpret_cast<const float4*>(kbase + r_ * ldk); vr0 = *reinterpret_cast<const float4*>(vbase + r_ * ldv); }    \
    { const size_t r_ = kv_row0 + min(kb_ + (T / 16) * 1, nk - 1); if constexpr (SM != ATT_LOAD_S) kr1 = *reinterpret_cast<const float4*>(kbase + r_ * ldk); vr1 = *reinterpret_cast<const float4*>(vbase + r_ * ldv); }    \
    { const size_t r_ = kv_row0 + min(kb_ + (T / 16) * 2, nk - 1); if constexpr (SM != ATT_LOAD_S) kr2 = *reinterpret_cast<const float4*>(kbase + r_ * ldk); vr2 = *reinterpret_cast<const float4*>(vbase + r_ * ldv); }    \
    { const size_t r_ = kv_row0 + min(kb_ + (T / 16) * 3, nk - 1); if constexpr (SM != ATT_LOAD_S) kr3 = *reinterpret_cast<const float4*>(kbase + r_ * ldk); vr3 = *reinterpret_cast<const float4*>(vbase + r_ * ldv); }    \
  } while (0)
#define ATT_STORE(buf_)                                                                                                                                    \
  do {                                                                                                                                                     \
    float* kd_ = smem + (buf_) * AK * AKLD + st_c4;                                                                                                        \
    float* vd_ = smem + KS + (buf_) * AK * AD + st_c4;                                                                                         \
    { const int key_ = st_key + (T / 16) * 0; if constexpr (SM != ATT_LOAD_S) *reinterpret_cast<float4*>(kd_ + key_ * AKLD) = kr0; *reinterpret_cast<float4*>(vd_ + key_ * AD) = vr0; }    \
    { const int key_ = st_key + (T / 16) * 1; if constexpr (SM != ATT_LOAD_S) *reinterpret_cast<float4*>(kd_ + key_ * AKLD) = kr1; *reinterpret_cast<float4*>(vd_ + key_ * AD) = vr1; }    \
    { const int key_ = st_key + (T / 16) * 2; if constexpr (SM != ATT_LOAD_S) *reinterpret_cast<float4*>(kd_ + key_ * AKLD) = kr2; *reinterpret_cast<float4*>(vd_ + key_ * AD) = vr2; }    \
    { const int key_ = st_key + (T / 16) * 3; if constexpr (SM != ATT_LOAD_S) *reinterpret_cast<float4*>(kd_ + key_ * AKLD) = kr3; *reinterpret_cast<float4*>(vd_ + key_ * AD) = vr3; }    \
  } while (0)

  // ATT_LOAD_S: the 16 scores of this lane's queries for the 32 keys from key0_ on, as the accumulator holds them
  f32x16 sa[QT], sb[QT];
#define ATT_LOAD_SCORES(dst_, key0_)                                                        \
  do {                                                                                      \
    const float* sp_ = Ss + (key0_); /* uniform */                                          \
    _Pragma("unroll") for (int t_ = 0; t_ < QT; ++t_) _Pragma("unroll") for (int g_ = 0; g_ < 4; ++g_) { \
      const float4 x_ = *reinterpret_cast<const float4*>(sp_ + s_off[t_] + 8 * g_);         \
      dst_[t_][4 * g_] = x_.x; dst_[t_][4 * g_ + 1] = x_.y; dst_[t_][4 * g_ + 2] = x_.z; dst_[t_][4 * g_ + 3] = x_.w; \
    }                                                                                       \
  } while (0)
  // one 32-key half tile of the soft-max and of P.V for the QT query tiles of the wave: s_ holds the raw scores
  // S^T[key][q] (log2 units) on entry and P^T on exit; vp_ = this lane's first V element of the half tile in LDS
#define ATT_SOFTMAX_PV(s_, vp_, key0_)                                                                           \
  do {                                                                                                           \
    const bool tail = (key0_) + 32 > nk;                                                                         \
    _Pragma("unroll") for (int t = 0; t < QT; ++t) {                                                             \
      /* mask the tail keys, running max */                                                                      \
      if (tail) {                                                                                                \
        _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                           \
          if ((key0_) + acc_row(r, h) >= nk) s_[t][r] = -INFINITY;                                               \
      }                                                                                                          \
      float mx = -INFINITY;                                                                                      \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s_[t][r]);                                   \
      mx = fmaxf(mx, __shfl_xor(mx, 32));                                                                        \
      const float m_new = fmaxf(m_run[t], mx);                                                                   \
      const float alpha = __builtin_amdgcn_exp2f(m_run[t] - m_new);                                              \
      float rs = 0.f;                                                                                            \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                           \
        s_[t][r] = __builtin_amdgcn_exp2f(s_[t][r] - m_new); /* raw v_exp_f32 (scores already in log2 units) */  \
        rs += s_[t][r];                                                                                          \
      }                                                                                                          \
      rs += __shfl_xor(rs, 32);                                                                                  \
      l_run[t] = l_run[t] * alpha + rs;                                                                          \
      /* the running maximum rarely moves after the first tiles: skip the 32 rescale multiplies when */          \
      /* no lane of the wave needs them (alpha == 1 exactly -> bit-identical result) */                          \
      if (!__all(m_new == m_run[t])) {                                                                           \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) { o[t][0][r] *= alpha; o[t][1][r] *= alpha; }             \
      }                                                                                                          \
      m_run[t] = m_new;                                                                                          \
    }                                                                                                            \
    /* O^T += V^T P^T */                                                                                         \
    const float* vp = (vp_);                                                                                     \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                             \
      const int krow = (r & 3) + 8 * (r >> 2);                                                                   \
      const float v0 = vp[krow * AD];                                                                            \
      const float v1 = vp[krow * AD + 32];                                                                       \
      _Pragma("unroll") for (int t = 0; t < QT; ++t) {                                                           \
        o[t][0] = mfma32(v0, s_[t][r], o[t][0]);                                                                 \
        o[t][1] = mfma32(v1, s_[t][r], o[t][1]);                                                                 \
      }                                                                                                          \
    }                                                                                                            \
  } while (0)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  typedef __attribute__((address_space(1))) char att_gchar;  // global address space, spelled out: the asm hides it
  typedef __attribute__((address_space(1))) float att_gfloat;

  if (kt0 < kt1) {
    ATT_LOAD(kt0);
    if constexpr (SM == ATT_LOAD_S) ATT_LOAD_SCORES(sa, kt0 * AK);
    ATT_STORE(0);
  }
  __syncthreads();
  ATT_T(t_loop);
  for (int kt = kt0; kt < kt1; ++kt) {
    const bool has_next = kt + 1 < kt1;
    if (has_next) ATT_LOAD(kt + 1);
    const int buf = (kt - kt0) & 1;
    const float* Ks = smem + buf * AK * AKLD;
    const float* Vs = smem + KS + buf * AK * AD;

    if constexpr (SM == ATT_LOAD_S) {
      // the scores come from the first direction's array; sa holds this tile's first half (loaded one step ago), the
      // loads of the step after are in flight while the P.V of the present one runs
      const int key0 = kt * AK;
      const bool second = key0 + 32 < nk;  // uniform
      if (second) ATT_LOAD_SCORES(sb, key0 + 32);
      ATT_SOFTMAX_PV(sa, Vs + (4 * h) * AD + l31, key0);
      if (second) {
        if (has_next) ATT_LOAD_SCORES(sa, key0 + AK);
        ATT_SOFTMAX_PV(sb, Vs + (32 + 4 * h) * AD + l31, key0 + 32);
      }
    } else {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int key0 = kt * AK + half * 32;
      if (key0 >= nk) break;  // uniform
      f32x16 s[QT];
#pragma unroll
      for (int t = 0; t < QT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
      const float* kp = Ks + (half * 32 + l31) * AKLD + 4 * h;
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const float4 kf = *reinterpret_cast<const float4*>(kp + 8 * g);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
          s[t] = mfma32(kf.x, qf[t][g].x, s[t]);
          s[t] = mfma32(kf.y, qf[t][g].y, s[t]);
          s[t] = mfma32(kf.z, qf[t][g].z, s[t]);
          s[t] = mfma32(kf.w, qf[t][g].w, s[t]);
        }
      }
      if constexpr (SM == ATT_STORE_S) {
        // the wait for the prefetched K / V tile also waits for every score store issued before it (one counter, and
        // hipcc waits it down to 0 here), so the tile goes to LDS HERE, in front of the second half's stores: the
        // youngest stores it has to wait for are then the first half's, a soft-max, a P.V and a K.Q^T old, and the
        // second half's get a whole tile's time.  At the end of the step the stores just issued would stall it (4 us
        // of 286 per launch at 32 x 1024 x 1024).  The other buffer is free since the barrier of the step before.
        if (half == 1 && has_next) ATT_STORE(buf ^ 1);
        // hand the raw tile over: 16 stores of 128 B per half wave and query tile, one basic block per tile (the tile
        // test is uniform: a wave's 32 queries lie on one side of nq rounded up to 32 <= ldS)
#pragma unroll
        for (int t = 0; t < QT; ++t) {
          if (qt0 + (wave_u * QT + t) * 32 < nq) {
            // the row's address in scalar registers, the lane's byte offset in one VGPR: a store with a scalar base and
            // no vector arithmetic in front of it (the two empty asm keep hipcc from folding the lane offset into a
            // 64-bit vector address outside the loop that it then advances by one VALU instruction per store)
            unsigned lane_off = 4u * s_off[t];
            asm volatile("" : "+v"(lane_off));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              att_gchar* rowp = (att_gchar*)(Ss + (size_t)(key0 + (r & 3) + 8 * (r >> 2)) * ldS);  // uniform
              asm volatile("" : "+s"(rowp));
              *(att_gfloat*)(rowp + lane_off) = s[t][r];
            }
          }
        }
      }
      ATT_SOFTMAX_PV(s, Vs + (half * 32 + 4 * h) * AD + l31, key0);
    }
    }
#ifdef ATT_DIAG
    {
      ATT_T(t_s0);
      if (has_next) ATT_STORE(buf ^ 1);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      ATT_T(t_s1);
      __syncthreads();
      ATT_T(t_s2);
      d_store += t_s1 - t_s0;
      d_bar += t_s2 - t_s1;
    }
#else
    if (SM != ATT_STORE_S && has_next) ATT_STORE(buf ^ 1);
    __syncthreads();
#endif
  }
  ATT_T(t_end);

  // ---- key-split partials: [problem][head][q][split][64 O | m | l] ----
  if (part != nullptr) {
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      if (q[t] < nq) {
        float* pp = part + ((((size_t)bz * gridDim.y + head) * max_nq + q[t]) * ksplit + ks) * GFC_ATT_PART;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float* dst = pp + db * 32 + 8 * g + 4 * h;  // 8-byte aligned (GFC_ATT_PART is even)
            dst[0] = o[t][db][4 * g]; dst[1] = o[t][db][4 * g + 1];
            dst[2] = o[t][db][4 * g + 2]; dst[3] = o[t][db][4 * g + 3];
          }
        if (h == 0) { pp[64] = m_run[t]; pp[65] = l_run[t]; }
      }
    }
    return;
  }
  // ---- normalise and store: lane holds O[q][db*32 + 8*(r>>2) + 4h + (r&3)] ----
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    if (q[t] < nq) {
      const float inv = 1.f / l_run[t];
      float* op = O + (size_t)(q_row0 + q[t]) * ldo + head * AD + 4 * h;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float4 v = make_float4(o[t][db][4 * g] * inv, o[t][db][4 * g + 1] * inv, o[t][db][4 * g + 2] * inv,
                                 o[t][db][4 * g + 3] * inv);
          *reinterpret_cast<float4*>(op + db * 32 + 8 * g) = v;
        }
    }
  }
#ifdef ATT_DIAG
  if (g_att_diag_dev && lane == 0) {
    unsigned hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    unsigned long long* dd = g_att_diag_dev +
        ((size_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) * AW + wave) * 8;
    dd[0] = t_loop - t_entry; dd[1] = t_end - t_loop; dd[2] = d_bar; dd[3] = d_store;
    dd[4] = __builtin_readcyclecounter() - t_end; dd[5] = hw; dd[6] = t_entry;
  }
#endif
}

// combine the key-split partials: one wave per (query, head); lane = channel
__global__ __launch_bounds__(256) void attention_merge_kernel(const float* __restrict__ part, float* __restrict__ O,
                                                              int ldo, const int4* __restrict__ problems, int ksplit,
                                                              int max_nq, float scale_log2e) {
  const int4 pb = problems[blockIdx.z];
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), head = blockIdx.y, lane = threadIdx.x & 63;
  if (q >= pb.y) return;
  const float* pp = part + (((size_t)blockIdx.z * gridDim.y + head) * max_nq + q) * ksplit * GFC_ATT_PART;
  float m = -INFINITY;
  for (int s = 0; s < ksplit; ++s) m = fmaxf(m, pp[s * GFC_ATT_PART + 64]);
  float acc = 0.f, l = 0.f;
  for (int s = 0; s < ksplit; ++s) {
    const float ms = pp[s * GFC_ATT_PART + 64];
    const float w = (ms == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(ms - m);  // (partials carry the maximum in log2 units)
    acc += w * pp[s * GFC_ATT_PART + lane];
    l += w * pp[s * GFC_ATT_PART + 65];
  }
  O[(size_t)(pb.x + q) * ldo + head * AD + lane] = acc / l;
}

// Scratch for the key-split path (0 when the problem set is large enough not to need it).
extern "C" size_t gfc_attention_workspace_bytes(int n_problems, int max_nq, int heads) {
  if (n_problems <= 0 || max_nq <= 0 || heads <= 0) return 0;
  const long long wgs128 = (long long)((max_nq + 127) / 128) * heads * n_problems;
  if (wgs128 >= 256) return 0;
  return gfc_align(gfc_att_scratch_bytes((size_t)n_problems * max_nq, heads, GFC_ATT_MAX_SPLIT));
}

extern "C" int gfc_attention(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O,
                             int ldo, const int32_t* problems, int n_problems, int max_nq, int heads, float scale,
                             void* ws, size_t ws_bytes, void* stream) {
  if (!Q || !K || !V || !O || !problems || n_problems <= 0 || max_nq <= 0 || heads <= 0) return GFC_ERR_INVALID;
  if (ldq % 4 || ldk % 4 || ldv % 4 || ldo % 4) return GFC_ERR_INVALID;
  // tuning knob (tools/bench_kernels.py): GFC_ATTN_CFG = 1: 2 q-tiles/wave (256 queries / workgroup), 2: 1 q-tile/wave
  // (128); anything else = automatic
  const int forced = gfc_knobs().attn_cfg;
  auto wgs = [&](int aq) { return (long long)((max_nq + aq - 1) / aq) * heads * n_problems; };
  // the largest query block that still fills the chip twice over (256 CUs x 2 workgroups)
  const int cfg = (forced == 1 || forced == 2) ? forced : (wgs(256) >= 1024 ? 1 : 2);
  const float sl2 = scale * 1.4426950408889634f;
  hipStream_t st = (hipStream_t)stream;
  const int4* pt = reinterpret_cast<const int4*>(problems);
  // key split for small problem sets (batch 1..2, gfc_att_split); a tiny merge kernel combines the partial soft-maxes
  const int ksplit =
      cfg == 2 && ws != nullptr ? gfc_att_split(wgs(128), (size_t)n_problems * max_nq, heads, ws_bytes) : 1;
  if (cfg == 1) {
    hipLaunchKernelGGL(attention_kernel<2>, dim3((max_nq + 255) / 256, heads, n_problems), dim3(256), 0, st, Q, ldq, K,
                       ldk, V, ldv, O, ldo, pt, sl2, 1, (float*)nullptr, max_nq, 1);
  } else {
    float* part = ksplit > 1 ? (float*)ws : nullptr;
    hipLaunchKernelGGL(attention_kernel<1>, dim3(((max_nq + 127) / 128) * ksplit, heads, n_problems), dim3(256), 0, st,
                       Q, ldq, K, ldk, V, ldv, O, ldo, pt, sl2, ksplit, part, max_nq, 1);
    if (ksplit > 1)
      hipLaunchKernelGGL(attention_merge_kernel, dim3((max_nq + 3) / 4, heads, n_problems), dim3(256), 0, st, part, O,
                         ldo, pt, ksplit, max_nq, sl2);
  }
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}

// ---- cross attention with the score matrix evaluated once (ATT_STORE_S / ATT_LOAD_S above) ----
// per (pair, head): N rounded up to 32 rows of M rounded up to 32 floats; a lane's offset in it is a 32-bit byte offset
static inline int att_round32(int x) { return (x + 31) & ~31; }
static inline size_t att_sim_slab_bytes(int M, int N) { return (size_t)att_round32(N) * att_round32(M) * sizeof(float); }

extern "C" size_t gfc_attention_cross_stored_workspace_bytes(int n_pairs, int M, int N, int heads) {
  if (n_pairs <= 0 || M <= 0 || N <= 0 || heads <= 0) return 0;
  if (M > INT_MAX - 31 || N > INT_MAX - 31 || att_sim_slab_bytes(M, N) > 0xffffffffull) return 0;
  return gfc_align((size_t)n_pairs * heads * att_sim_slab_bytes(M, N));
}

extern "C" int gfc_attention_cross_stored(const float* qk, int ld, const float* v, int ldv, float* out, int ldo,
                                          const int32_t* pairs, int n_pairs, int M, int N, int heads, float scale,
                                          void* sim, size_t sim_bytes, void* stream) {
  if (!qk || !v || !out || !pairs || n_pairs <= 0 || M <= 0 || N <= 0 || heads <= 0) return GFC_ERR_INVALID;
  if (ld % 4 || ldv % 4 || ldo % 4) return GFC_ERR_INVALID;
  const size_t need = gfc_attention_cross_stored_workspace_bytes(n_pairs, M, N, heads);
  if (need == 0) return GFC_ERR_INVALID;
  if (!sim || sim_bytes < need) return GFC_ERR_WORKSPACE;
  const int forced = gfc_knobs().attn_cfg;
  // each direction is a launch of its own.  The first takes 256 queries per workgroup as soon as those fill the chip's
  // 2 x 256 workgroup slots once (at 32 x 1024 x 1024: 300 us against 314 with 128 queries, before the store addressing
  // was tuned); the second, with half the MFMAs per key tile, wants them filled twice over, as gfc_attention does (there:
  // 178-181 us with 128 queries against 182-192; profiles/cross_stored_sim.md)
  auto two_tiles = [&](int nq, int min_wgs) {
    if (forced == 1 || forced == 2) return forced == 1;
    return (long long)((nq + 255) / 256) * heads * n_pairs >= min_wgs;
  };
  const float sl2 = scale * 1.4426950408889634f;
  hipStream_t st = (hipStream_t)stream;
  const int4* pt = reinterpret_cast<const int4*>(pairs);
  float* S = (float*)sim;
  const int ldS = att_round32(M), s_rows = att_round32(N);
  // first direction: image-0 queries over image-1 keys, scores stored; second: image-1 queries read them back
  if (two_tiles(M, 512))
    hipLaunchKernelGGL((attention_kernel<2, ATT_STORE_S>), dim3((M + 255) / 256, heads, n_pairs), dim3(256), 0, st, qk, ld,
                       qk, ld, v, ldv, out, ldo, pt, sl2, 1, (float*)nullptr, M, 1, S, ldS, s_rows);
  else
    hipLaunchKernelGGL((attention_kernel<1, ATT_STORE_S>), dim3((M + 127) / 128, heads, n_pairs), dim3(256), 0, st, qk, ld,
                       qk, ld, v, ldv, out, ldo, pt, sl2, 1, (float*)nullptr, M, 1, S, ldS, s_rows);
  GFC_LAUNCH_CHECK();
  if (two_tiles(N, 1024))
    hipLaunchKernelGGL((attention_kernel<2, ATT_LOAD_S>), dim3((N + 255) / 256, heads, n_pairs), dim3(256), 0, st, qk, ld,
                       qk, ld, v, ldv, out, ldo, pt, sl2, 1, (float*)nullptr, N, 1, S, ldS, s_rows);
  else
    hipLaunchKernelGGL((attention_kernel<1, ATT_LOAD_S>), dim3((N + 127) / 128, heads, n_pairs), dim3(256), 0, st, qk, ld,
                       qk, ld, v, ldv, out, ldo, pt, sl2, 1, (float*)nullptr, N, 1, S, ldS, s_rows);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
