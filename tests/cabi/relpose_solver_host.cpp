// csrc/relpose_solver.h compiled for the HOST: the entry points tests/test_relpose_reference_host.py compares with the
// float64 numpy restatement (tests/relpose_reference.py), value for value.  No GPU, no HIP.
#include "relpose_solver.h"

extern "C" void five_point_many(const double* rec, int K, double* Es, unsigned char* ok) {
  double work[200 + 121];
  for (int i = 0; i < K; ++i) {
    bool o[RP_MAX_SOL] = {false};
    double E[RP_MAX_SOL * 9] = {0.0};
    const int ns = rp_five_point(rec + 20 * i, work, E, o);
    for (int k = 0; k < RP_MAX_SOL; ++k) {
      ok[i * RP_MAX_SOL + k] = (k < ns && o[k]) ? 1 : 0;
      for (int e = 0; e < 9; ++e) Es[(i * RP_MAX_SOL + k) * 9 + e] = ok[i * RP_MAX_SOL + k] ? E[k * 9 + e] : 0.0;
    }
  }
}

extern "C" void decompose(const double* E, double* Rt) { rp_decompose(E, Rt); }

// one Gauss-Newton round over the inliers of [t]x R, sums in record order; returns rp_gn_update's verdict
extern "C" int gn_step(const double* rec, int n, double t2, double* R, double* t) {
  double E[9], b3[3], b4[3], acc[20] = {0.0};
  rp_essential(R, t, E);
  rp_tangent(t, b3, b4);
  for (int c = 0; c < n; ++c) {
    const double* q = rec + 4 * c;
    if (rp_sampson2(E, q[0], q[1], q[2], q[3]) < t2) rp_gn_accumulate(acc, R, t, E, b3, b4, q[0], q[1], q[2], q[3]);
  }
  return rp_gn_update(acc, b3, b4, R, t) ? 1 : 0;
}

extern "C" void cheiral(const double* R, const double* t, const double* rec, int n, unsigned char* out) {
  for (int c = 0; c < n; ++c) out[c] = rp_cheiral(R, t, rec[4 * c], rec[4 * c + 1], rec[4 * c + 2], rec[4 * c + 3]) ? 1 : 0;
}

extern "C" void pose_error(const double* R, const double* t, const double* Rg, const double* tg, double thr, double* out) {
  rp_pose_error(R, t, Rg, tg, thr, out[0], out[1]);
}
