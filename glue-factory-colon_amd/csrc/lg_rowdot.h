// The 256-wide row dot product and the sigmoid behind gfc_lg_rowdot, as device functions: rowdot256_kernel
// (lg_misc.hip), sigmoid_inplace_kernel (api.hip) and the adaptive step (lg_adaptive.hip) all take their bits from
// here, so a stop / prune decision made inside the step is the decision the host would take on gfc_lg_rowdot's output.
#pragma once
#include "common.h"

// x[row,:256] . w + bias[0] on one wave: lane l holds channels 4l..4l+3 of the row in `a`.  Every lane returns the sum.
__device__ __forceinline__ float gfc_rowdot256_wave(const float4 a, const float* __restrict__ w,
                                                    const float* __restrict__ bias, int lane) {
  const float4 b = *reinterpret_cast<const float4*>(w + lane * 4);
  const float s = wave_sum(a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w);
  return s + bias[0];
}

__device__ __forceinline__ float gfc_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
