/* Cross attention with the score matrix evaluated once: the C entries of csrc/attention.hip behind the cross block of
 * large uniform LightGlue batches, exported by libgfc_amd.so and written in the grammar of gfc_amd.h
 * (glue-factory-colon_amd/_native.py parses all five headers).  A header of its own because the suite pins the function
 * lists of the other four; it declares functions only and takes its types from gfc_amd.h. */
#ifndef GFC_AMD_CROSS_ATTENTION_H
#define GFC_AMD_CROSS_ATTENTION_H

#include "gfc_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The bidirectional cross attention of lightglue.py:207-217 with sim = qk0 . qk1^T evaluated once.  Q and K of both
 * directions are the rows of qk (row pitch ld), the values those of v.  pairs[p] = {row0_0, m, row0_1, n} (int32 x4,
 * device; m <= M, n <= N): the m rows of image 0 from row0_0 on attend to the n rows of image 1 from row0_1 on and the
 * other way round, out has the rows of qk.  Two launches on `stream`: the first direction is gfc_attention's result bit
 * for bit and also stores its raw score tiles into `sim`; the second direction reads them back instead of multiplying
 * (its scores carry the scale on the other operand: one rounding apart from gfc_attention's).  `sim` needs
 * gfc_attention_cross_stored_workspace_bytes(n_pairs, M, N, heads) bytes (n_pairs x heads x N x M floats, N and M
 * rounded up to 32; 0 = shape not supported) and may hold anything on entry; GFC_ERR_WORKSPACE if it is smaller. */
int gfc_attention_cross_stored(const float* qk, int ld, const float* v, int ldv, float* out, int ldo,
                               const int32_t* pairs, int n_pairs, int M, int N, int heads, float scale, void* sim,
                               size_t sim_bytes, void* stream);
size_t gfc_attention_cross_stored_workspace_bytes(int n_pairs, int M, int N, int heads);

#ifdef __cplusplus
}
#endif

#endif /* GFC_AMD_CROSS_ATTENTION_H */
