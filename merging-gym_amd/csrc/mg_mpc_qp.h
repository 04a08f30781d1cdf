// mg_mpc_qp.h -- mpc_qp_constants: mpc_1d's equality step in quadprog's operation order (host only).
// A part of the one translation unit merging_hip.hip (see its head comment).
#pragma once

#include "mg_common.h"

namespace {

// The constants of mpc_1d's equality step (helper.py:152-191) in the operation order of quadprog
// 0.1.11's qpgen2 (Goldfarb-Idnani; helper.py:182 -> qpsolvers 1.8.0 -> quadprog.solve_qp with
// G = P, C = -A[1]', b = -B, meq = 1), file compiled without contraction:
//   n = A[1] = (dt, ..., dt), dt = t / 10 (the velocity row of [a^9 b, ..., b]);
//   P = D'D + 0.01 I, D the 9 x 10 first-difference operator (integer sums, then + 0.01);
//   dpofa: P = R'R, column by column, s accumulating t*t before a(j,j) - s;
//   dpori: J = R^-1 in place (a(k,k) = 1 / a(k,k), column k scaled by -a(k,k), then
//          a(1:k, j) += a(k, j) a(1:k, k) for j > k);
//   d = J'n (d_i = sum_j J(j,i) n_j), z = J d (z_i = sum_j J(i,j) d_j, accumulated in j order),
//   z'n (sum in index order).
// The residual's sign only negates n, d, z and the step exactly, so u0 = (b / z'n) z0 for either
// sign of b = vt - v0. Restated from the published algorithm (LINPACK dpofa / dpori and
// Goldfarb & Idnani 1983 as coded in Turlach's solve.QP.f); quadprog is not in this image.
void mpc_qp_constants(double t, double* nz_out, double* z0_out, double* vsmall_out) {
  constexpr int kT = 10;
  const double dt = t / kT;
  double n[kT], a[kT][kT] = {}, d[kT], z[kT];  // a[i][j] = LINPACK's a(i+1, j+1)
  for (int i = 0; i < kT; ++i) n[i] = 0.0 * 0.0 + 1.0 * dt;  // row [0 1] of a^k times b
  for (int i = 0; i + 1 < kT; ++i) {
    a[i][i] += 1.0;
    a[i + 1][i + 1] += 1.0;
    a[i][i + 1] -= 1.0;
    a[i + 1][i] -= 1.0;
  }
  for (int i = 0; i < kT; ++i) a[i][i] += 0.01;
  for (int j = 0; j < kT; ++j) {  // dpofa (upper triangle)
    double s = 0.0;
    for (int k = 0; k < j; ++k) {
      double dot = 0.0;
      for (int l = 0; l < k; ++l) dot = dot + a[l][k] * a[l][j];
      double tk = a[k][j] - dot;
      tk = tk / a[k][k];
      a[k][j] = tk;
      s = s + tk * tk;
    }
    s = a[j][j] - s;
    a[j][j] = std::sqrt(s);
  }
  for (int k = 0; k < kT; ++k) {  // dpori
    a[k][k] = 1.0 / a[k][k];
    const double tk = -a[k][k];
    for (int i = 0; i < k; ++i) a[i][k] = tk * a[i][k];
    for (int j = k + 1; j < kT; ++j) {
      const double tj = a[k][j];
      a[k][j] = 0.0;
      if (tj == 0.0) continue;  // daxpy returns early for a zero multiplier
      for (int i = 0; i <= k; ++i) a[i][j] = a[i][j] + tj * a[i][k];
    }
  }
  for (int i = 0; i < kT; ++i) {  // d = J'n (J is upper triangular: a[j][i] = 0 for j > i)
    double s = 0.0;
    for (int j = 0; j < kT; ++j) s = s + (j <= i ? a[j][i] : 0.0) * n[j];
    d[i] = s;
  }
  for (int i = 0; i < kT; ++i) z[i] = 0.0;
  for (int j = 0; j < kT; ++j)  // z = J d
    for (int i = 0; i < kT; ++i) z[i] = z[i] + (i <= j ? a[i][j] : 0.0) * d[j];
  double nz = 0.0;
  for (int i = 0; i < kT; ++i) nz = nz + z[i] * n[i];
  // qpgen2's machine-precision probe: a constraint residual below vsmall is set to 0
  volatile double vs = 1e-60;
  for (;;) {
    vs = vs + vs;
    const double ta = vs * 0.1 + 1.0, tb = vs * 0.2 + 1.0;
    if (ta > 1.0 && tb > 1.0) break;
  }
  *nz_out = nz;
  *z0_out = z[0];
  *vsmall_out = vs;
}

}  // namespace
