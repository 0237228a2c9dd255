// Process-wide, thread-safe host state of the library (all of it read-only after its first use):
//  * the tuning knobs ($GFC_GEMM_TILE, $GFC_ATTN_CFG, ...) are read ONCE, by one std::call_once, for every
//    translation unit -- host threads that drive their own HIP streams (export_predictions(workers=N)) all see
//    the same values;
//  * per-device facts (CU count) and per-(kernel, device) attributes (dynamic LDS above 64 KB) are keyed by the
//    current HIP device, so one process may drive several GPUs.
// The knobs are for tests and tuning: GFC_GEMM_TILE, GFC_ATTN_CFG and GFC_NMS_MODE force a variant that the automatic
// choice also takes at some problem size, so that tests can cover it on small inputs; GFC_STEM_F43 = 0 selects the
// F(2x2,3x3) stem, the fallback for the F(4x4,3x3) numerics; GFC_CROSS_STORED = 0 keeps the cross block of large uniform
// LightGlue batches in one launch (tests/test_gpu_cross_stored_sim.py runs a batch both ways).  The variants are held to the same parity tests
// (tests/test_gpu_primitives.py::test_gemm_tile_variants_via_knob etc.).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

struct GfcKnobs {
  int gemm_tile;     // GFC_GEMM_TILE: 0 = by problem size, 3 = 64x64 tiles everywhere, 4 = 128x128 tiles everywhere
  int attn_cfg;      // GFC_ATTN_CFG: 0 / anything else = by problem size, 1 = 256 queries per workgroup, 2 = 128 queries
  int nms_mode;      // GFC_NMS_MODE: 0 (default) = by problem size, 1 = LDS-image kernel, 2 = streaming kernel (waves walk column bands, rings in registers)
  int stem_f43;      // GFC_STEM_F43: 1 (default) = Winograd F(4x4,3x3) stem when its filters are supplied, 0 = F(2x2,3x3) stem
  int cross_stored;  // GFC_CROSS_STORED: 1 (default) = large uniform batches evaluate the cross block's sim once (gfc_attention_cross_stored), 0 = never (tests: the same batch both ways)
};
const GfcKnobs& gfc_knobs();

// number of compute units of the CURRENT device (cached per device)
int gfc_device_cus();

// hipFuncAttributeMaxDynamicSharedMemorySize, applied once per (kernel instantiation, device).
// `done` is one word per kernel instantiation (bit d = device d configured); safe from any thread.  `bytes` is the
// largest dynamic size the kernel is ever launched with.  false: the runtime refused (asked again at the next call).
inline bool gfc_allow_dynamic_lds(const void* kernel, size_t bytes, std::atomic<unsigned long long>& done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) dev = 0;
  const unsigned long long bit = 1ull << dev;
  if (done.load(std::memory_order_acquire) & bit) return true;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
  done.fetch_or(bit, std::memory_order_release);
  return true;
}
