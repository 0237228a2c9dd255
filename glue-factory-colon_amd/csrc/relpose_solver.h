// The arithmetic of the relative-pose estimator (relpose.hip; DESIGN.md "Robust relative pose"), fp64, one thread:
// five-point minimal solve (null space -> ten cubic constraints -> 10x20 elimination -> degree-10 polynomial in z ->
// Sturm bracketing, bisection, Newton polish), Sampson distance, the decomposition of E and the pieces of the
// Gauss-Newton step.  Plain C++ without device intrinsics, so the same text also compiles for the host.
// Convention: X1 = R X0 + t, E = [t]x R, q1^T E q0 = 0 with q = (u, v, 1).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RP_HD __host__ __device__ __forceinline__
#define RP_HD_NOINLINE __host__ __device__ __noinline__
#else
#define RP_HD inline
#define RP_HD_NOINLINE inline
#endif

#define RP_MAX_SOL 10
#define RP_PIVOT_EPS 1e-12     // null space (entries of q1 (x) q0 are O(1))
#define RP_ELIM_EPS 1e-14      // 10x20 elimination
#define RP_BISECT_ITERS 52
#define RP_NEWTON_ITERS 4
#define RP_JACOBI_SWEEPS 12

RP_HD bool rp_finite(double v) { return v - v == 0.0; }

// ---- null space of the 5x9 matrix of rows q1 (x) q0 -----------------------------------------------------------------
// Gauss-Jordan with full pivoting (largest |entry| of the live block, first in row-major order on a tie); basis vector j
// has a 1 at free column j and minus the reduced entries at the pivot columns.  basis [4][9] = X, Y, Z, W.
RP_HD bool rp_nullspace(const double* rec /* [5][4] u0 v0 u1 v1 */, double* basis) {
  double A[5][9];
  int perm[9];
  for (int r = 0; r < 5; ++r) {
    const double u0 = rec[r * 4], v0 = rec[r * 4 + 1], u1 = rec[r * 4 + 2], v1 = rec[r * 4 + 3];
    A[r][0] = u1 * u0; A[r][1] = u1 * v0; A[r][2] = u1;
    A[r][3] = v1 * u0; A[r][4] = v1 * v0; A[r][5] = v1;
    A[r][6] = u0;      A[r][7] = v0;      A[r][8] = 1.0;
  }
  for (int c = 0; c < 9; ++c) perm[c] = c;
  for (int r = 0; r < 5; ++r) {
    double best = -1.0;
    int pr = r, pc = r;
    for (int i = r; i < 5; ++i)
      for (int j = r; j < 9; ++j) {
        const double a = fabs(A[i][j]);
        if (a > best) { best = a; pr = i; pc = j; }
      }
    if (!(best > RP_PIVOT_EPS) || !rp_finite(best)) return false;
    for (int j = 0; j < 9; ++j) { const double t = A[r][j]; A[r][j] = A[pr][j]; A[pr][j] = t; }
    for (int i = 0; i < 5; ++i) { const double t = A[i][r]; A[i][r] = A[i][pc]; A[i][pc] = t; }
    { const int t = perm[r]; perm[r] = perm[pc]; perm[pc] = t; }
    const double inv = 1.0 / A[r][r];
    for (int j = 0; j < 9; ++j) A[r][j] *= inv;
    for (int i = 0; i < 5; ++i) {
      if (i == r) continue;
      const double f = A[i][r];
      for (int j = 0; j < 9; ++j) A[i][j] -= f * A[r][j];
    }
  }
  for (int k = 0; k < 4; ++k) {
    for (int c = 0; c < 9; ++c) basis[k * 9 + c] = 0.0;
    basis[k * 9 + perm[5 + k]] = 1.0;
    for (int i = 0; i < 5; ++i) basis[k * 9 + perm[i]] = -A[i][5 + k];
  }
  return true;
}

// ---- polynomials in (x, y, z) ------------------------------------------------------------------------------------------
// linear: x y z 1;  quadratic: xx xy xz x yy yz y zz z 1;  cubic: the 20 sorted triples in lexicographic order.
RP_HD void rp_mul11(const double* a, const double* b, double s, double* out /* [10] += s a b */) {
  const int Q[16] = {0, 1, 2, 3, 1, 4, 5, 6, 2, 5, 7, 8, 3, 6, 8, 9};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) out[Q[i * 4 + j]] += s * (a[i] * b[j]);
}
RP_HD void rp_mul21(const double* q, const double* l, double* out /* [20] += q l */) {
  const int C[40] = {0, 1, 2, 3, 1, 4, 5, 6, 2, 5, 7, 8, 3, 6, 8, 9, 4, 10, 11, 12, 5, 11, 13, 14,
                     6, 12, 14, 15, 7, 13, 16, 17, 8, 14, 17, 18, 9, 15, 18, 19};
  for (int a = 0; a < 10; ++a)
    for (int b = 0; b < 4; ++b) out[C[a * 4 + b]] += q[a] * l[b];
}

// The ten cubic constraints on E = xX + yY + zZ + W as a 10x20 matrix, columns in Nister's order
//   x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1
// rows 0..8: (E E^T - tr(E E^T)/2 I) E = 0, entry (i, j) at row 3 i + j; row 9: det E = 0.
RP_HD void rp_constraints(const double* basis, double* Mx /* [10][20] */) {
  const int PERM[20] = {0, 10, 1, 4, 2, 3, 11, 12, 5, 6, 7, 8, 9, 13, 14, 15, 16, 17, 18, 19};
  double E[9][4];
  for (int e = 0; e < 9; ++e)
    for (int k = 0; k < 4; ++k) E[e][k] = basis[k * 9 + e];
  double L[6][10];  // E E^T - tr/2 I, upper triangle 00 01 02 11 12 22
  const int LI[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
  int q = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      for (int m = 0; m < 10; ++m) L[q][m] = 0.0;
      for (int k = 0; k < 3; ++k) rp_mul11(E[i * 3 + k], E[j * 3 + k], 1.0, L[q]);
      ++q;
    }
  for (int m = 0; m < 10; ++m) {
    const double half_tr = 0.5 * ((L[0][m] + L[3][m]) + L[5][m]);
    L[0][m] -= half_tr; L[3][m] -= half_tr; L[5][m] -= half_tr;
  }
  double row[20];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      for (int m = 0; m < 20; ++m) row[m] = 0.0;
      for (int k = 0; k < 3; ++k) rp_mul21(L[LI[i * 3 + k]], E[k * 3 + j], row);
      for (int m = 0; m < 20; ++m) Mx[(i * 3 + j) * 20 + m] = row[PERM[m]];
    }
  // det E = E20 (E01 E12 - E02 E11) + E21 (E02 E10 - E00 E12) + E22 (E00 E11 - E01 E10)
  for (int m = 0; m < 20; ++m) row[m] = 0.0;
  const int D[3][5] = {{1, 5, 2, 4, 6}, {2, 3, 0, 5, 7}, {0, 4, 1, 3, 8}};
  for (int k = 0; k < 3; ++k) {
    double m2[10];
    for (int m = 0; m < 10; ++m) m2[m] = 0.0;
    rp_mul11(E[D[k][0]], E[D[k][1]], 1.0, m2);
    rp_mul11(E[D[k][2]], E[D[k][3]], -1.0, m2);
    rp_mul21(m2, E[D[k][4]], row);
  }
  for (int m = 0; m < 20; ++m) Mx[9 * 20 + m] = row[PERM[m]];
}

// Forward elimination of the first ten columns with partial pivoting (largest |entry| of the column, the first on a
// tie), then back substitution into rows 4..9 only (x2z, x2, y2z, y2, xyz, xy: the rows Nister's construction uses).
RP_HD bool rp_eliminate(double* Mx) {
  for (int c = 0; c < 10; ++c) {
    double best = -1.0;
    int pr = c;
    for (int r = c; r < 10; ++r) {
      const double a = fabs(Mx[r * 20 + c]);
      if (a > best) { best = a; pr = r; }
    }
    if (!(best > RP_ELIM_EPS) || !rp_finite(best)) return false;
    if (pr != c)
      for (int k = c; k < 20; ++k) { const double t = Mx[c * 20 + k]; Mx[c * 20 + k] = Mx[pr * 20 + k]; Mx[pr * 20 + k] = t; }
    const double inv = 1.0 / Mx[c * 20 + c];
    for (int k = c; k < 20; ++k) Mx[c * 20 + k] *= inv;
    for (int r = c + 1; r < 10; ++r) {
      const double f = Mx[r * 20 + c];
      for (int k = c; k < 20; ++k) Mx[r * 20 + k] -= f * Mx[c * 20 + k];
    }
  }
  for (int c = 9; c > 4; --c)
    for (int r = 4; r < c; ++r) {
      const double f = Mx[r * 20 + c];
      for (int k = 10; k < 20; ++k) Mx[r * 20 + k] -= f * Mx[c * 20 + k];
    }
  return true;
}

// B(z) [x y 1]^T = 0: rows <x2z> - z <x2>, <y2z> - z <y2>, <xyz> - z <xy>; entries in ascending powers of z:
// Bz[r][0..3] (x, degree 3), Bz[r][4..7] (y, degree 3), Bz[r][8..12] (1, degree 4).
RP_HD void rp_hidden_variable(const double* Mx, double* Bz /* [3][13] */) {
  for (int r = 0; r < 3; ++r) {
    const double* e = Mx + (4 + 2 * r) * 20 + 10;
    const double* f = Mx + (5 + 2 * r) * 20 + 10;
    double* b = Bz + r * 13;
    b[0] = e[2]; b[1] = e[1] - f[2]; b[2] = e[0] - f[1]; b[3] = -f[0];
    b[4] = e[5]; b[5] = e[4] - f[5]; b[6] = e[3] - f[4]; b[7] = -f[3];
    b[8] = e[9]; b[9] = e[8] - f[9]; b[10] = e[7] - f[8]; b[11] = e[6] - f[7]; b[12] = -f[6];
  }
}

// det B(z), degree 10, ascending powers, divided by its largest |coefficient|
RP_HD bool rp_det_poly(const double* Bz, double* c /* [11] */) {
  for (int k = 0; k < 11; ++k) c[k] = 0.0;
  const int RA[3] = {1, 2, 0}, RB[3] = {2, 0, 1};  // cofactor of (r, col 2): rows RA, RB of columns x, y (cyclic: sign +)
  for (int r = 0; r < 3; ++r) {
    const double* a = Bz + RA[r] * 13;
    const double* b = Bz + RB[r] * 13;
    double cof[7];
    for (int k = 0; k < 7; ++k) cof[k] = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) cof[i + j] += a[i] * b[4 + j] - a[4 + i] * b[j];
    const double* w = Bz + r * 13 + 8;
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 7; ++j) c[i + j] += w[i] * cof[j];
  }
  double mx = 0.0;
  for (int k = 0; k < 11; ++k) mx = fabs(c[k]) > mx ? fabs(c[k]) : mx;
  if (!(mx > 0.0) || !rp_finite(mx)) return false;
  const double inv = 1.0 / mx;
  for (int k = 0; k < 11; ++k) c[k] *= inv;
  return true;
}

// ---- real roots ------------------------------------------------------------------------------------------------------
// Sturm chain s[0] = p, s[1] = p', s[i] = -rem(s[i-2], s[i-1]) times 1 / max|coefficient| (a positive factor); s[i] has
// degree 10 - i and lives at s + 11 i.
RP_HD void rp_sturm_chain(const double* c, double* s /* [11][11] */) {
  for (int k = 0; k < 11; ++k) s[k] = c[k];
  for (int k = 0; k < 10; ++k) s[11 + k] = (double)(k + 1) * c[k + 1];
  s[11 + 10] = 0.0;
  for (int i = 2; i <= 10; ++i) {
    const double* a = s + 11 * (i - 2);
    const double* b = s + 11 * (i - 1);
    const int da = 12 - i, db = 11 - i;
    double r[11];
    for (int k = 0; k <= da; ++k) r[k] = a[k];
    const double q1 = r[da] / b[db];
    for (int k = 0; k <= db; ++k) r[k + 1] -= q1 * b[k];
    const double q0 = r[da - 1] / b[db];
    for (int k = 0; k <= db; ++k) r[k] -= q0 * b[k];
    double mx = 0.0;
    for (int k = 0; k < db; ++k) mx = fabs(r[k]) > mx ? fabs(r[k]) : mx;
    const double sc = (mx > 0.0 && rp_finite(mx)) ? 1.0 / mx : 1.0;
    double* o = s + 11 * i;
    for (int k = 0; k < 11; ++k) o[k] = (k < db) ? -(r[k] * sc) : 0.0;
  }
}

RP_HD double rp_horner(const double* c, int deg, double x) {
  double v = c[deg];
  for (int k = deg - 1; k >= 0; --k) v = v * x + c[k];
  return v;
}

// sign changes of the chain at x (zeros and NaNs are passed over)
RP_HD int rp_sturm_count(const double* s, double x) {
  int changes = 0, last = 0;
  for (int i = 0; i <= 10; ++i) {
    const double v = rp_horner(s + 11 * i, 10 - i, x);
    const int sg = v > 0.0 ? 1 : (v < 0.0 ? -1 : 0);
    if (sg != 0) {
      if (last != 0 && sg != last) ++changes;
      last = sg;
    }
  }
  return changes;
}

// x = s / (1 - |s|) maps (-1, 1) onto the real line: bisecting s needs no root bound and resolves a root near x to
// about (1 + |x|)^2 times the resolution in s
RP_HD double rp_unit_to_line(double s) { return s / (1.0 - fabs(s)); }

// The real roots of c (degree 10) in ascending order, those beyond |x| = 2^40 left out: per root a bisection on the
// Sturm count in s over [-S, S], S = 1 - 2^-40 (the k-th root is the least x with count(x(-S)) - count(x) >= k + 1),
// then Newton steps kept only inside the bracket.
RP_HD int rp_real_roots(const double* c, double* s /* scratch [121] */, double* roots /* [10] */) {
  const double S = 1.0 - 9.094947017729282e-13;  // 1 - 2^-40
  rp_sturm_chain(c, s);
  const int v_lo = rp_sturm_count(s, rp_unit_to_line(-S));
  int nr = v_lo - rp_sturm_count(s, rp_unit_to_line(S));
  nr = nr < 0 ? 0 : (nr > RP_MAX_SOL ? RP_MAX_SOL : nr);
  for (int k = 0; k < nr; ++k) {
    double lo = -S, hi = S;
    for (int it = 0; it < RP_BISECT_ITERS; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (v_lo - rp_sturm_count(s, rp_unit_to_line(mid)) >= k + 1) hi = mid; else lo = mid;
    }
    const double xlo = rp_unit_to_line(lo), xhi = rp_unit_to_line(hi);
    double z = rp_unit_to_line(0.5 * (lo + hi));
    for (int it = 0; it < RP_NEWTON_ITERS; ++it) {
      const double zn = z - rp_horner(s, 10, z) / rp_horner(s + 11, 9, z);
      if (!(zn >= xlo && zn <= xhi)) break;
      z = zn;
    }
    roots[k] = z;
  }
  return nr;
}

// x, y from the null vector of B(z) (the cross product of two rows with the largest |third component|, the first on a
// tie), then E = xX + yY + zZ + W scaled to unit Frobenius norm.  false: a non-finite entry.
RP_HD bool rp_model_at_root(const double* Bz, const double* basis, double z, double* E) {
  double b[3][3];
  for (int r = 0; r < 3; ++r) {
    b[r][0] = rp_horner(Bz + r * 13, 3, z);
    b[r][1] = rp_horner(Bz + r * 13 + 4, 3, z);
    b[r][2] = rp_horner(Bz + r * 13 + 8, 4, z);
  }
  const int PA[3] = {0, 0, 1}, PB[3] = {1, 2, 2};
  double bx = 0.0, by = 0.0, bw = 0.0;
  for (int p = 0; p < 3; ++p) {
    const double* u = b[PA[p]];
    const double* v = b[PB[p]];
    const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cw = u[0] * v[1] - u[1] * v[0];
    if (p == 0 || fabs(cw) > fabs(bw)) { bx = cx; by = cy; bw = cw; }
  }
  const double x = bx / bw, y = by / bw;
  double n2 = 0.0;
  for (int e = 0; e < 9; ++e) {
    E[e] = ((x * basis[e] + y * basis[9 + e]) + z * basis[18 + e]) + basis[27 + e];
    n2 += E[e] * E[e];
  }
  const double inv = 1.0 / sqrt(n2);
  bool ok = true;
  for (int e = 0; e < 9; ++e) { E[e] *= inv; ok = ok && rp_finite(E[e]); }
  return ok;
}

// Five correspondences -> up to ten essential matrices Es [10][9] (slot k = k-th real root), ok[k]; returns the number
// of slots (0: the sample is skipped).  work: [200 + 121] doubles.
RP_HD_NOINLINE int rp_five_point(const double* rec /* [5][4] */, double* work, double* Es, bool* ok) {
  double basis[36], Bz[39], c[11], roots[RP_MAX_SOL];
  for (int k = 0; k < 20; ++k)
    if (!rp_finite(rec[k])) return 0;
  if (!rp_nullspace(rec, basis)) return 0;
  rp_constraints(basis, work);
  if (!rp_eliminate(work)) return 0;
  rp_hidden_variable(work, Bz);
  if (!rp_det_poly(Bz, c)) return 0;
  const int nr = rp_real_roots(c, work + 200, roots);
  bool any = false;
  for (int k = 0; k < nr; ++k) { ok[k] = rp_model_at_root(Bz, basis, roots[k], Es + 9 * k); any = any || ok[k]; }
  return any ? nr : 0;
}

// ---- residual -------------------------------------------------------------------------------------------------------
// squared Sampson distance of (u0, v0) <-> (u1, v1) under E; a zero denominator gives inf or NaN, which no threshold
// accepts (the MSAC sum then takes t^2)
RP_HD double rp_sampson2(const double* E, double u0, double v0, double u1, double v1) {
  const double a0 = (E[0] * u0 + E[1] * v0) + E[2];
  const double a1 = (E[3] * u0 + E[4] * v0) + E[5];
  const double a2 = (E[6] * u0 + E[7] * v0) + E[8];
  const double b0 = (E[0] * u1 + E[3] * v1) + E[6];
  const double b1 = (E[1] * u1 + E[4] * v1) + E[7];
  const double r = (u1 * a0 + v1 * a1) + a2;
  const double den = (a0 * a0 + a1 * a1) + (b0 * b0 + b1 * b1);
  return (r * r) / den;
}

RP_HD void rp_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
RP_HD double rp_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RP_HD void rp_normalise(double* a) {
  const double inv = 1.0 / sqrt(rp_dot(a, a));
  a[0] *= inv; a[1] *= inv; a[2] *= inv;
}

// E = [t]x R
RP_HD void rp_essential(const double* R, const double* t, double* E) {
  for (int c = 0; c < 3; ++c) {
    E[c] = t[1] * R[6 + c] - t[2] * R[3 + c];
    E[3 + c] = t[2] * R[c] - t[0] * R[6 + c];
    E[6 + c] = t[0] * R[3 + c] - t[1] * R[c];
  }
}

// ---- decomposition ---------------------------------------------------------------------------------------------------
// SVD of E through a cyclic Jacobi on E^T E: v1, v2 the eigenvectors of the two largest eigenvalues (the lower index
// first on a tie), v3 = v1 x v2; u1 = E v1 / |.|, u2 = E v2 made orthogonal to u1 / |.|, u3 = u1 x u2 (det U = det V = +1).
// The four candidates in order: (U W V^T, +u3), (U W V^T, -u3), (U W^T V^T, +u3), (U W^T V^T, -u3).  Rt [4][12] = R, t.
RP_HD void rp_decompose(const double* E, double* Rt) {
  double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i * 3 + j] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
  for (int sweep = 0; sweep < RP_JACOBI_SWEEPS; ++sweep)
    for (int p = 0; p < 2; ++p)
      for (int r = p + 1; r < 3; ++r) {
        const double apq = A[p * 3 + r];
        if (!(fabs(apq) > 1e-300)) continue;
        const double theta = (A[r * 3 + r] - A[p * 3 + p]) / (2.0 * apq);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k * 3 + p], akr = A[k * 3 + r];
          A[k * 3 + p] = c * akp - s * akr;
          A[k * 3 + r] = s * akp + c * akr;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p * 3 + k], ark = A[r * 3 + k];
          A[p * 3 + k] = c * apk - s * ark;
          A[r * 3 + k] = s * apk + c * ark;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k * 3 + p], vkr = V[k * 3 + r];
          V[k * 3 + p] = c * vkp - s * vkr;
          V[k * 3 + r] = s * vkp + c * vkr;
        }
      }
  int i1 = 0;
  for (int k = 1; k < 3; ++k)
    if (A[k * 4] > A[i1 * 4]) i1 = k;
  int i2 = -1;
  for (int k = 0; k < 3; ++k)
    if (k != i1 && (i2 < 0 || A[k * 4] > A[i2 * 4])) i2 = k;
  double v1[3] = {V[i1], V[3 + i1], V[6 + i1]}, v2[3] = {V[i2], V[3 + i2], V[6 + i2]}, v3[3];
  rp_normalise(v1);
  const double d12 = rp_dot(v1, v2);
  for (int k = 0; k < 3; ++k) v2[k] -= d12 * v1[k];
  rp_normalise(v2);
  rp_cross(v1, v2, v3);
  double u1[3], u2[3], u3[3];
  for (int k = 0; k < 3; ++k) {
    u1[k] = rp_dot(E + 3 * k, v1);
    u2[k] = rp_dot(E + 3 * k, v2);
  }
  rp_normalise(u1);
  const double du = rp_dot(u1, u2);
  for (int k = 0; k < 3; ++k) u2[k] -= du * u1[k];
  rp_normalise(u2);
  rp_cross(u1, u2, u3);
  for (int cnd = 0; cnd < 4; ++cnd) {
    const double sw = cnd < 2 ? 1.0 : -1.0, st = (cnd & 1) ? -1.0 : 1.0;
    double* o = Rt + 12 * cnd;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) o[i * 3 + j] = sw * (u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j];
    for (int i = 0; i < 3; ++i) o[9 + i] = st * u3[i];
  }
}

// closed-form two-ray triangulation X1 = d0 R q0 + t = d1 q1: both depths positive (the common positive denominator
// |R q0 x q1|^2 is left out)
RP_HD bool rp_cheiral(const double* R, const double* t, double u0, double v0, double u1, double v1) {
  const double p[3] = {(R[0] * u0 + R[1] * v0) + R[2], (R[3] * u0 + R[4] * v0) + R[5], (R[6] * u0 + R[7] * v0) + R[8]};
  const double q1[3] = {u1, v1, 1.0};
  double pxq[3], txq[3], txp[3];
  rp_cross(p, q1, pxq);
  rp_cross(t, q1, txq);
  rp_cross(t, p, txp);
  const double n0 = -rp_dot(txq, pxq);  // d0 |p x q1|^2
  const double n1 = -rp_dot(txp, pxq);  // d1 |p x q1|^2
  return n0 > 0.0 && n1 > 0.0;
}

// ---- local optimisation ----------------------------------------------------------------------------------------------
// tangent basis of the unit t: b3 = normalise(t x e_j), e_j the axis of smallest |t_j| (the lowest j on a tie), b4 = t x b3
RP_HD void rp_tangent(const double* t, double* b3, double* b4) {
  int j = 0;
  for (int k = 1; k < 3; ++k)
    if (fabs(t[k]) < fabs(t[j])) j = k;
  const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
  rp_cross(t, e, b3);
  rp_normalise(b3);
  rp_cross(t, b3, b4);
}

// One correspondence of the Gauss-Newton step on rho = w q1^T E q0, w the Sampson weight of the current model (frozen):
// J = w [p x (q1 x t), q1.(b3 x p), q1.(b4 x p)], p = R q0.  acc [20] += the upper triangle of J^T J (15), J^T rho (5).
RP_HD void rp_gn_accumulate(double* acc, const double* R, const double* t, const double* E, const double* b3,
                            const double* b4, double u0, double v0, double u1, double v1) {
  const double a0 = (E[0] * u0 + E[1] * v0) + E[2];
  const double a1 = (E[3] * u0 + E[4] * v0) + E[5];
  const double a2 = (E[6] * u0 + E[7] * v0) + E[8];
  const double e0 = (E[0] * u1 + E[3] * v1) + E[6];
  const double e1 = (E[1] * u1 + E[4] * v1) + E[7];
  const double r = (u1 * a0 + v1 * a1) + a2;
  const double w = 1.0 / sqrt((a0 * a0 + a1 * a1) + (e0 * e0 + e1 * e1));
  const double p[3] = {(R[0] * u0 + R[1] * v0) + R[2], (R[3] * u0 + R[4] * v0) + R[5], (R[6] * u0 + R[7] * v0) + R[8]};
  const double q1[3] = {u1, v1, 1.0};
  double c[3], jw[3], b3p[3], b4p[3];
  rp_cross(q1, t, c);
  rp_cross(p, c, jw);
  rp_cross(b3, p, b3p);
  rp_cross(b4, p, b4p);
  const double J[5] = {w * jw[0], w * jw[1], w * jw[2], w * rp_dot(q1, b3p), w * rp_dot(q1, b4p)};
  const double rho = w * r;
  int q = 0;
  for (int i = 0; i < 5; ++i)
    for (int j = i; j < 5; ++j) acc[q++] += J[i] * J[j];
  for (int i = 0; i < 5; ++i) acc[15 + i] += J[i] * rho;
}

// (J^T J) d = -J^T rho by Cholesky; then R <- exp([w]x) R (Rodrigues), t <- normalise(t + d3 b3 + d4 b4).
// false: a pivot <= 0 or not finite, or a non-finite result.
RP_HD bool rp_gn_update(const double* acc, const double* b3, const double* b4, double* R, double* t) {
  double Lm[25], d[5];
  int q = 0;
  for (int i = 0; i < 5; ++i)
    for (int j = i; j < 5; ++j) { Lm[j * 5 + i] = acc[q]; ++q; }  // lower triangle holds the symmetric matrix
  for (int j = 0; j < 5; ++j) {
    double s = Lm[j * 5 + j];
    for (int k = 0; k < j; ++k) s -= Lm[j * 5 + k] * Lm[j * 5 + k];
    if (!(s > 0.0) || !rp_finite(s)) return false;
    const double dj = sqrt(s);
    Lm[j * 5 + j] = dj;
    for (int i = j + 1; i < 5; ++i) {
      double v = Lm[i * 5 + j];
      for (int k = 0; k < j; ++k) v -= Lm[i * 5 + k] * Lm[j * 5 + k];
      Lm[i * 5 + j] = v / dj;
    }
  }
  for (int i = 0; i < 5; ++i) {
    double v = -acc[15 + i];
    for (int k = 0; k < i; ++k) v -= Lm[i * 5 + k] * d[k];
    d[i] = v / Lm[i * 5 + i];
  }
  for (int i = 4; i >= 0; --i) {
    double v = d[i];
    for (int k = i + 1; k < 5; ++k) v -= Lm[k * 5 + i] * d[k];
    d[i] = v / Lm[i * 5 + i];
  }
  const double th2 = rp_dot(d, d), th = sqrt(th2);
  // sin(th)/th and (1 - cos th)/th^2, by their series below 1e-4 (the next terms are below 1e-17 relative)
  const double A = th < 1e-4 ? 1.0 - th2 / 6.0 : sin(th) / th;
  const double B = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / th2;
  const double K[9] = {0, -d[2], d[1], d[2], 0, -d[0], -d[1], d[0], 0};
  double X[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double k2 = (K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j]) + K[i * 3 + 2] * K[6 + j];
      X[i * 3 + j] = ((i == j ? 1.0 : 0.0) + A * K[i * 3 + j]) + B * k2;
    }
  double Rn[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = (X[i * 3] * R[j] + X[i * 3 + 1] * R[3 + j]) + X[i * 3 + 2] * R[6 + j];
  double tn[3];
  for (int k = 0; k < 3; ++k) tn[k] = (t[k] + d[3] * b3[k]) + d[4] * b4[k];
  rp_normalise(tn);
  bool ok = true;
  for (int k = 0; k < 9; ++k) ok = ok && rp_finite(Rn[k]);
  for (int k = 0; k < 3; ++k) ok = ok && rp_finite(tn[k]);
  if (!ok) return false;
  for (int k = 0; k < 9; ++k) R[k] = Rn[k];
  for (int k = 0; k < 3; ++k) t[k] = tn[k];
  return true;
}

// eval_utils.relative_pose_error in fp64: t up to sign, both angles as atan2(sine, cosine), degrees
RP_HD void rp_pose_error(const double* R, const double* t, const double* Rg, const double* tg, double ignore_gt_t_thr,
                         double& r_err, double& t_err) {
  const double RAD = 57.29577951308232;
  double cx[3];
  rp_cross(t, tg, cx);
  double te = atan2(sqrt(rp_dot(cx, cx)), rp_dot(t, tg)) * RAD;
  te = te < 180.0 - te ? te : 180.0 - te;
  if (sqrt(rp_dot(tg, tg)) < ignore_gt_t_thr) te = 0.0;
  double D[9];  // R^T R_gt
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) D[i * 3 + j] = (R[i] * Rg[j] + R[3 + i] * Rg[3 + j]) + R[6 + i] * Rg[6 + j];
  const double ax[3] = {D[7] - D[5], D[2] - D[6], D[3] - D[1]};
  r_err = atan2(sqrt(rp_dot(ax, ax)) / 2.0, (((D[0] + D[4]) + D[8]) - 1.0) / 2.0) * RAD;
  t_err = te;
}
