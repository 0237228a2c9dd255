// LightGlue adaptive depth / width: the step BETWEEN two layers (lightglue.py:500-521,555-580) for a batch of pairs,
// entirely on the device.  Four launches on the caller's stream:
//   decide  one wave per live row: token confidence and matchability from ONE read of the row (the arithmetic of
//           gfc_lg_rowdot, lg_rowdot.h) -> two flag bits per row
//   count   one workgroup per (pair, side) segment: kept rows and low-confidence rows
//   plan    one workgroup: per pair stop / emptied / live, the order of the output (live pairs first), the exclusive
//           scan of the 2B output counts, the problem tables of the next layer, the report the host reads
//   pack    stable compaction of every segment into the second set of row buffers + the prune counters
// Plain vector loads and stores only; every output element has exactly one writer, so nothing is atomic.
#include <climits>

#include "block_select.h"
#include "common.h"
#include "lg_rowdot.h"

namespace {

enum { FLAG_KEEP = 1, FLAG_LOW = 2 };

// a segment {row0, n} cut to the row buffer [0, rows): the tables are device data the host never sees, so every kernel
// bounds them itself
__device__ __forceinline__ void seg_load(const int32_t* __restrict__ seg, int s, int rows, int& row0, int& n) {
  row0 = seg[2 * s];
  n = seg[2 * s + 1];
  if (row0 < 0 || row0 > rows) { row0 = 0; n = 0; }
  n = max(0, min(n, rows - row0));
}

// tok = sigmoid(x . token_w + token_b), sc = sigmoid(x . matchability_w + matchability_b); FLAG_LOW = tok < thr
// (check_if_stop counts these), FLAG_KEEP = sc > keep_thr || tok <= thr (get_pruning_mask).  tw / mw NULL: that criterion
// is disabled.
__global__ __launch_bounds__(256) void adaptive_decide_kernel(const float* __restrict__ x, int rows,
                                                              const float* __restrict__ tw, const float* __restrict__ tb,
                                                              const float* __restrict__ mw, const float* __restrict__ mb,
                                                              float thr, float keep_thr, int32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float4 a = *reinterpret_cast<const float4*>(x + (size_t)row * 256 + lane * 4);
  int f = 0;
  bool keep = (mw == nullptr);
  if (tw) {
    const float tok = gfc_sigmoid(gfc_rowdot256_wave(a, tw, tb, lane));
    if (tok < thr) f |= FLAG_LOW;
    keep = keep || (tok <= thr);
  }
  if (mw) {
    const float sc = gfc_sigmoid(gfc_rowdot256_wave(a, mw, mb, lane));
    keep = keep || (sc > keep_thr);
  }
  if (keep) f |= FLAG_KEEP;
  if (lane == 0) flags[row] = f;
}

// segcnt[s] = {rows with FLAG_KEEP, rows with FLAG_LOW} of segment s
__global__ __launch_bounds__(256) void adaptive_count_kernel(const int32_t* __restrict__ seg, int rows,
                                                             const int32_t* __restrict__ flags,
                                                             int32_t* __restrict__ segcnt) {
  __shared__ int s_keep[4], s_low[4];
  const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  int row0, n;
  seg_load(seg, s, rows, row0, n);
  int keep = 0, low = 0;  // wave-uniform
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + t;
    const int f = i < n ? flags[row0 + i] : 0;
    keep += __popcll(__ballot(f & FLAG_KEEP));
    low += __popcll(__ballot(f & FLAG_LOW));
  }
  if (lane == 0) { s_keep[w] = keep; s_low[w] = low; }
  __syncthreads();
  if (t == 0) {
    *reinterpret_cast<int2*>(segcnt + 2 * s) =
        make_int2(s_keep[0] + s_keep[1] + s_keep[2] + s_keep[3], s_low[0] + s_low[1] + s_low[2] + s_low[3]);
  }
}

// one workgroup, thread t = pair t (B <= 128).  plan[t] = {first output row of side 0, of side 1, copy-all flag, 0}.
__global__ __launch_bounds__(256) void adaptive_plan_kernel(const int32_t* __restrict__ seg,
                                                            const int32_t* __restrict__ pairs, int B, int rows,
                                                            const int32_t* __restrict__ segcnt, double depth_confidence,
                                                            int do_stop, int do_prune, int32_t* __restrict__ report,
                                                            int32_t* __restrict__ plan, int32_t* __restrict__ seg_out,
                                                            int32_t* __restrict__ pairs_out, int32_t* __restrict__ self_p,
                                                            int32_t* __restrict__ cross_p) {
  __shared__ int s_wave[4];
  __shared__ int s_cnt[256];
  const int t = threadIdx.x;
  int state = GFC_LG_ADAPTIVE_LIVE, c0 = 0, c1 = 0, cnt = 0, live = 0;
  int2 pr = make_int2(0, 0);
  if (t < B) {
    int r, n0, n1;
    seg_load(seg, 2 * t, rows, r, n0);
    seg_load(seg, 2 * t + 1, rows, r, n1);
    const int4 sc = *reinterpret_cast<const int4*>(segcnt + 4 * t);  // {keep0, low0, keep1, low1}
    pr = *reinterpret_cast<const int2*>(pairs + 2 * t);              // {un-pruned m + n, slot}
    bool stop = false;
    if (do_stop) {
      // check_if_stop (lightglue.py:569-580) in the fp32 arithmetic of the torch expression, compared as a double
      cnt = sc.y + sc.w;
      const float ratio = 1.0f - (float)cnt / (float)pr.x;
      stop = (double)ratio > depth_confidence;
    }
    if (stop) {
      state = GFC_LG_ADAPTIVE_STOPPED;
      c0 = n0; c1 = n1;
    } else {
      c0 = do_prune ? sc.x : n0;
      c1 = do_prune ? sc.z : n1;
      if (c0 == 0 || c1 == 0) state = GFC_LG_ADAPTIVE_EMPTIED;
    }
    live = state == GFC_LG_ADAPTIVE_LIVE;
  }
  int n_live, n_rows;
  const int incl = gfc_block_scan_excl<4>(live, s_wave, n_live) + live;
  // live pairs keep their order in front, finished pairs keep theirs behind them
  const int pos = live ? incl - 1 : n_live + (t - incl);
  s_cnt[t] = 0;
  __syncthreads();
  if (t < B) { s_cnt[2 * pos] = c0; s_cnt[2 * pos + 1] = c1; }
  __syncthreads();
  const int mine = s_cnt[t];
  const int off = gfc_block_scan_excl<4>(mine, s_wave, n_rows);  // in output order
  s_cnt[t] = off;
  __syncthreads();
  if (t >= B) return;
  const int o0 = s_cnt[2 * pos], o1 = s_cnt[2 * pos + 1];
  *reinterpret_cast<int4*>(report + 4 * t) = make_int4(state, c0, c1, cnt);
  *reinterpret_cast<int4*>(plan + 4 * t) = make_int4(o0, o1, (state == GFC_LG_ADAPTIVE_STOPPED || !do_prune) ? 1 : 0, 0);
  *reinterpret_cast<int4*>(seg_out + 4 * pos) = make_int4(o0, c0, o1, c1);
  *reinterpret_cast<int2*>(pairs_out + 2 * pos) = pr;
  if (live) {
    *reinterpret_cast<int4*>(self_p + 8 * pos) = make_int4(o0, c0, o0, c0);
    *reinterpret_cast<int4*>(self_p + 8 * pos + 4) = make_int4(o1, c1, o1, c1);
    *reinterpret_cast<int4*>(cross_p + 8 * pos) = make_int4(o0, c0, o1, c1);
    *reinterpret_cast<int4*>(cross_p + 8 * pos + 4) = make_int4(o1, c1, o0, c0);
  }
}

// grid (chunks, 2B): workgroup (c, s) packs the 256-row chunks c, c + gridDim.x, ... of segment s.  Destination of a kept
// row = first output row of the segment + kept rows before it: the rank inside the chunk (block_select.h) and a running
// base over the part of the segment in front of the chunk.
__global__ __launch_bounds__(256) void adaptive_pack_kernel(
    const float* __restrict__ x, const float* __restrict__ cosb, const float* __restrict__ sinb,
    const int32_t* __restrict__ ind, int rows, const int32_t* __restrict__ seg, const int32_t* __restrict__ pairs,
    const int32_t* __restrict__ prune_off, const int32_t* __restrict__ plan, const int32_t* __restrict__ flags,
    int n_slots, float* __restrict__ x_out, float* __restrict__ cos_out, float* __restrict__ sin_out,
    int32_t* __restrict__ ind_out, int32_t* __restrict__ prune, int prune_len) {
  __shared__ int s_wave[4];
  __shared__ int s_src[256];  // kept rows of the chunk, dense, in order
  const int s = blockIdx.y, pair = s >> 1, side = s & 1;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int row0, n;
  seg_load(seg, s, rows, row0, n);
  const int dst0 = plan[4 * pair + side];
  const bool all = plan[4 * pair + 2] != 0;  // a pair that stopped, or no pruning: copied as it is, counters untouched
  const int slot = pairs[2 * pair + 1];
  const bool count = !all && prune != nullptr && slot >= 0 && slot < n_slots;
  const int poff = count ? prune_off[2 * slot + side] : 0;
  int base = 0, counted = 0;  // kept rows in [0, counted) of the segment
  for (int c0 = blockIdx.x * 256; c0 < n; c0 += gridDim.x * 256) {
    if (all) {
      base = c0;
    } else if (counted < c0) {
      int add = 0;  // wave-uniform
      for (int i0 = counted; i0 < c0; i0 += 256) {
        const int i = i0 + t;
        add += __popcll(__ballot(i < c0 && (flags[row0 + i] & FLAG_KEEP)));
      }
      if (lane == 0) s_wave[w] = add;
      __syncthreads();
      base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
      __syncthreads();
    }
    const int i = c0 + t;
    const bool k = i < n && (all || (flags[row0 + i] & FLAG_KEEP));
    // slot among the kept rows of the chunk.  The barriers inside the rank also put this chunk's writes of s_wave and
    // s_src behind every read of the chunk before, so the loop body needs no barrier at its end.
    int total;
    const int j = gfc_block_rank<4>(k, s_wave, total);
    // the output buffers hold `rows` rows: a consistent table never asks for more (kept <= live), an inconsistent one is cut
    total = max(0, min(total, rows - (dst0 + base)));
    if (k && j < total) {
      s_src[j] = t;
      const int id = ind[row0 + i];
      ind_out[dst0 + base + j] = id;
      if (count) {
        const long long p = (long long)poff + id;
        if (p >= 0 && p < prune_len) prune[p] += 1;  // one writer: a point is one row of one segment
      }
    }
    __syncthreads();
    // one wave moves one 1 KB row of x as float4 (+ the 256 B rows of cos and sin on its first 32 lanes)
#pragma unroll 4
    for (int j = w; j < total; j += 4) {
      const size_t src = (size_t)row0 + c0 + s_src[j], dst = (size_t)dst0 + base + j;
      const float4 v = *reinterpret_cast<const float4*>(x + src * 256 + lane * 4);
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lane < 16)
        r = *reinterpret_cast<const float4*>(cosb + src * 64 + lane * 4);
      else if (lane < 32)
        r = *reinterpret_cast<const float4*>(sinb + src * 64 + (lane - 16) * 4);
      *reinterpret_cast<float4*>(x_out + dst * 256 + lane * 4) = v;
      if (lane < 16)
        *reinterpret_cast<float4*>(cos_out + dst * 64 + lane * 4) = r;
      else if (lane < 32)
        *reinterpret_cast<float4*>(sin_out + dst * 64 + (lane - 16) * 4) = r;
    }
    base += total;
    counted = c0 + 256;
  }
}

// flags [rows] | segcnt [2B][2] | plan [B][4]
struct step_layout { size_t flags, segcnt, plan, total; };
step_layout step_plan(int B, int rows) {
  gfc_slots s;
  return {s.take((size_t)rows * 4), s.take((size_t)B * 4 * 4), s.take((size_t)B * 4 * 4), s.off};
}

}  // namespace

extern "C" size_t gfc_lg_adaptive_step_workspace_bytes(int B, int rows) {
  if (B <= 0 || B > GFC_LG_MAX_RAGGED_PAIRS || rows <= 0 || rows > INT_MAX / 768) return 0;
  return step_plan(B, rows).total;
}

extern "C" int gfc_lg_adaptive_step(const gfc_lg_params* p, int layer, const float* x, const float* cos_tab,
                                    const float* sin_tab, const int32_t* ind, int rows, const int32_t* seg,
                                    const int32_t* pairs, const int32_t* prune_off, int n_slots, int B, int max_n,
                                    float thr, float keep_thr, double depth_confidence, int do_stop, int do_prune,
                                    float* x_out, float* cos_out, float* sin_out, int32_t* ind_out, int32_t* prune,
                                    int prune_len,
                                    int32_t* self_problems, int32_t* cross_problems, int32_t* seg_out,
                                    int32_t* pairs_out, int32_t* report, void* ws, size_t ws_bytes, void* stream) {
  if (!p || !x || !cos_tab || !sin_tab || !ind || !seg || !pairs || !x_out || !cos_out || !sin_out || !ind_out ||
      !self_problems || !cross_problems || !seg_out || !pairs_out || !report || !ws)
    return GFC_ERR_INVALID;
  if (B <= 0 || B > GFC_LG_MAX_RAGGED_PAIRS || rows <= 0 || rows > INT_MAX / 768 || max_n <= 0) return GFC_ERR_INVALID;
  if (!do_stop && !do_prune) return GFC_ERR_INVALID;
  // the decision after the last layer does not exist (lightglue.py:513): no token head there
  if (layer < 0 || layer >= p->n_layers - 1) return GFC_ERR_INVALID;
  if (do_stop && (!p->token_w[layer] || !p->token_b[layer])) return GFC_ERR_INVALID;
  if (do_prune && (!p->matchability_w[layer] || !p->matchability_b[layer])) return GFC_ERR_INVALID;
  if (do_prune && (!prune || !prune_off || prune_len <= 0 || n_slots <= 0)) return GFC_ERR_INVALID;
  // the tables are read and written as int4 / int2
  for (const void* t : {(const void*)seg, (const void*)pairs, (const void*)self_problems, (const void*)cross_problems,
                        (const void*)seg_out, (const void*)pairs_out, (const void*)report, (const void*)x, (const void*)cos_tab,
                        (const void*)sin_tab, (const void*)x_out, (const void*)cos_out, (const void*)sin_out, (const void*)ws})
    if ((uintptr_t)t % 16) return GFC_ERR_INVALID;
  // the re-pack is a copy between two sets of buffers, and pack reads the tables plan has replaced
  if (x_out == x || cos_out == cos_tab || sin_out == sin_tab || ind_out == ind || seg_out == seg || pairs_out == pairs)
    return GFC_ERR_INVALID;
  const step_layout L = step_plan(B, rows);
  if (ws_bytes < L.total) return GFC_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int32_t* flags = (int32_t*)((char*)ws + L.flags);
  int32_t* segcnt = (int32_t*)((char*)ws + L.segcnt);
  int32_t* plan = (int32_t*)((char*)ws + L.plan);
  hipLaunchKernelGGL(adaptive_decide_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, rows,
                     do_stop ? p->token_w[layer] : nullptr, do_stop ? p->token_b[layer] : nullptr,
                     do_prune ? p->matchability_w[layer] : nullptr, do_prune ? p->matchability_b[layer] : nullptr, thr,
                     keep_thr, flags);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(adaptive_count_kernel, dim3(2 * B), dim3(256), 0, st, seg, rows, flags, segcnt);
  GFC_LAUNCH_CHECK();
  hipLaunchKernelGGL(adaptive_plan_kernel, dim3(1), dim3(256), 0, st, seg, pairs, B, rows, segcnt, depth_confidence,
                     do_stop, do_prune, report, plan, seg_out, pairs_out, self_problems, cross_problems);
  GFC_LAUNCH_CHECK();
  const int chunks = (int)(((long long)min(max_n, rows) + 255) / 256);
  hipLaunchKernelGGL(adaptive_pack_kernel, dim3(chunks, 2 * B), dim3(256), 0, st, x, cos_tab, sin_tab, ind, rows, seg,
                     pairs, do_prune ? prune_off : nullptr, plan, flags, n_slots, x_out, cos_out, sin_out, ind_out,
                     do_prune ? prune : nullptr, prune_len);
  GFC_LAUNCH_CHECK();
  return GFC_OK;
}
