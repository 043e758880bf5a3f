// gel_host_lgr.hip -- the extended-precision generators: LGR nodes and differentiation matrix, barycentric weights and Lagrange rows,
// the matrices of the collocation error estimate.  Host arithmetic only: no HIP call, no handle.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "gel_host_internal.h"

namespace gelhost {

// ---------------------------------------------------------------------------
// LGR nodes / differentiation matrix.
// What: lib/PSfunctions.py:149-168 (flipped LGR nodes, ending at +1) and :182-208
// (D[k][i] = l_i'(tau_x[k+1]) on tau_x = [-1, tau]).  How: the flipped LGR points
// are the negated roots of P_{n-1}(x) + P_n(x) (Legendre), found by Newton in
// extended precision from the classic -cos(2 pi k/(2n-1)) guesses; D comes from
// barycentric weights in O(n^2) instead of the reference's O(n^4) products.
// ---------------------------------------------------------------------------
static void legendre_pair(int n, ld x, ld& Pn, ld& Pn1) {  // P_n, P_{n-1}
  ld p0 = 1.0L, p1 = x;
  if (n == 0) { Pn = 1.0L; Pn1 = 0.0L; return; }
  for (int k = 2; k <= n; k++) {
    const ld p2 = ((2 * k - 1) * x * p1 - (k - 1) * p0) / k;
    p0 = p1; p1 = p2;
  }
  Pn = p1; Pn1 = p0;
}

int lgr_nodes_ld(int n, std::vector<ld>& tau) {
  if (n < 2) return -1;
  std::vector<ld> xs(n);
  xs[0] = -1.0L;  // the Radau end point of the un-flipped set
  const ld pi = 3.141592653589793238462643383279502884L;
  for (int k = 1; k < n; k++) {
    ld x = -cosl(2.0L * pi * k / (2 * n - 1));
    for (int it = 0; it < 100; it++) {
      ld Pn, Pn1;
      legendre_pair(n, x, Pn, Pn1);  // P_n, P_{n-1}
      ld Pm, Pm1;
      legendre_pair(n - 1, x, Pm, Pm1);  // P_{n-1}, P_{n-2}
      const ld f = Pn1 + Pn;
      // P_k'(x) = k (x P_k - P_{k-1}) / (x^2 - 1)
      const ld dPn = n * (x * Pn - Pn1) / (x * x - 1.0L);
      const ld dPn1 = (n - 1) * (x * Pm - Pm1) / (x * x - 1.0L);
      // deflate the known root at -1: g = f/(1+x)
      const ld gval = f / (1.0L + x);
      const ld dg = (dPn + dPn1) / (1.0L + x) - f / ((1.0L + x) * (1.0L + x));
      const ld step = gval / dg;
      x -= step;
      if (fabsl(step) < 1e-19L) break;
    }
    xs[k] = x;
  }
  tau.resize(n);
  for (int k = 0; k < n; k++) tau[k] = -xs[k];
  std::sort(tau.begin(), tau.end());
  tau[n - 1] = 1.0L;
  return 0;
}

int lgr_diffmat_ld(int n, std::vector<double>& D, std::vector<double>& tau_out) {
  std::vector<ld> tau;
  if (lgr_nodes_ld(n, tau)) return -1;
  std::vector<ld> t(n + 1), w(n + 1);
  t[0] = -1.0L;
  for (int k = 0; k < n; k++) t[k + 1] = tau[k];
  for (int i = 0; i <= n; i++) {
    ld p = 1.0L;
    for (int m = 0; m <= n; m++)
      if (m != i) p *= (t[i] - t[m]);
    w[i] = 1.0L / p;
  }
  D.assign((size_t)n * (n + 1), 0.0);
  for (int k = 0; k < n; k++) {
    ld diag = 0.0L;
    for (int i = 0; i <= n; i++) {
      if (i == k + 1) continue;
      const ld v = (w[i] / w[k + 1]) / (t[k + 1] - t[i]);
      D[(size_t)k * (n + 1) + i] = (double)v;
      diag -= v;
    }
    D[(size_t)k * (n + 1) + k + 1] = (double)diag;
  }
  tau_out.resize(n);
  for (int k = 0; k < n; k++) tau_out[k] = (double)tau[k];
  return 0;
}

// ---------------------------------------------------------------------------
// Collocation error estimate (gel_mesh_*): per phase of n nodes, on the fine grid sigma = the flipped LGR points
// of n + 1 (sigma_0 = -1), the Lagrange bases of the phase's support tau_x = [-1, tau] (Lx) and of its collocation points tau
// (Lu) at sigma_1 .. sigma_{n+1}, and the fine grid's Radau integration matrix I = (D^[:, 1:])^-1, D^ = lgr_diffmat(n + 1):
// barycentric weights and Gauss-Jordan elimination in extended precision, rounded once.
// ---------------------------------------------------------------------------
std::vector<ld> bary_weights(const std::vector<ld>& t) {
  std::vector<ld> w(t.size());
  for (size_t i = 0; i < t.size(); i++) {
    ld p = 1.0L;
    for (size_t m = 0; m < t.size(); m++)
      if (m != i) p *= (t[i] - t[m]);
    w[i] = 1.0L / p;
  }
  return w;
}
// the Lagrange basis of support t (weights w) at z, second barycentric form; exactly 1 / 0 at a support point
void lagrange_row(const std::vector<ld>& t, const std::vector<ld>& w, ld z, ld* out) {
  for (size_t i = 0; i < t.size(); i++)
    if (z == t[i]) {
      for (size_t k = 0; k < t.size(); k++) out[k] = (k == i) ? 1.0L : 0.0L;
      return;
    }
  ld sum = 0.0L;
  for (size_t i = 0; i < t.size(); i++) { out[i] = w[i] / (z - t[i]); sum += out[i]; }
  for (size_t i = 0; i < t.size(); i++) out[i] /= sum;
}
// sigma [P], Lx [P][n+1], Lu [P][n], I [P][P] (row-major, P = n + 1) of a phase whose collocation points are tau [n]
int mesh_matrices_ld(const std::vector<double>& tau, std::vector<double>& out) {
  const int n = (int)tau.size(), P = n + 1;
  std::vector<ld> sg;
  if (lgr_nodes_ld(P, sg)) return -1;
  std::vector<ld> tx(P), tc(n);
  tx[0] = -1.0L;
  for (int k = 0; k < n; k++) tx[k + 1] = tc[k] = (ld)tau[k];
  const std::vector<ld> wx = bary_weights(tx), wc = bary_weights(tc);
  // D^ on the fine support s = [-1, sigma]: D^[k][i] = l_i'(s[k+1]); A = its columns 1 .. P, inverted in place
  std::vector<ld> sup(P + 1);
  sup[0] = -1.0L;
  for (int k = 0; k < P; k++) sup[k + 1] = sg[k];
  const std::vector<ld> ws = bary_weights(sup);
  std::vector<ld> A((size_t)P * P), Inv((size_t)P * P, 0.0L);
  for (int k = 0; k < P; k++) {
    ld diag = 0.0L;
    for (int i = 0; i <= P; i++) {
      if (i == k + 1) continue;
      const ld v = (ws[i] / ws[k + 1]) / (sup[k + 1] - sup[i]);
      if (i > 0) A[(size_t)k * P + i - 1] = v;
      diag -= v;
    }
    A[(size_t)k * P + k] = diag;
    Inv[(size_t)k * P + k] = 1.0L;
  }
  for (int c = 0; c < P; c++) {   // Gauss-Jordan, partial pivoting
    int piv = c;
    for (int r = c + 1; r < P; r++)
      if (fabsl(A[(size_t)r * P + c]) > fabsl(A[(size_t)piv * P + c])) piv = r;
    if (!(fabsl(A[(size_t)piv * P + c]) > 0.0L)) return -1;
    if (piv != c)
      for (int k = 0; k < P; k++) { std::swap(A[(size_t)c * P + k], A[(size_t)piv * P + k]); std::swap(Inv[(size_t)c * P + k], Inv[(size_t)piv * P + k]); }
    const ld ip = 1.0L / A[(size_t)c * P + c];
    for (int k = 0; k < P; k++) { A[(size_t)c * P + k] *= ip; Inv[(size_t)c * P + k] *= ip; }
    for (int r = 0; r < P; r++) {
      if (r == c) continue;
      const ld f = A[(size_t)r * P + c];
      if (f == 0.0L) continue;
      for (int k = 0; k < P; k++) { A[(size_t)r * P + k] -= f * A[(size_t)c * P + k]; Inv[(size_t)r * P + k] -= f * Inv[(size_t)c * P + k]; }
    }
  }
  out.clear();
  out.reserve((size_t)P * (1 + P + n + P));
  for (int l = 0; l < P; l++) out.push_back((double)sg[l]);
  std::vector<ld> row(P);
  for (int l = 0; l < P; l++) {
    lagrange_row(tx, wx, sg[l], row.data());
    for (int i = 0; i < P; i++) out.push_back((double)row[i]);
  }
  for (int l = 0; l < P; l++) {
    lagrange_row(tc, wc, sg[l], row.data());
    for (int j = 0; j < n; j++) out.push_back((double)row[j]);
  }
  for (size_t k = 0; k < (size_t)P * P; k++) out.push_back((double)Inv[k]);
  return 0;
}

}  // namespace gelhost

using namespace gelhost;

extern "C" {

int gel_lgr_nodes(int32_t n, double* tau) {
  std::vector<ld> t;
  if (!tau || lgr_nodes_ld(n, t)) return fail(GEL_ERR_ARG, "gel_lgr_nodes: n >= 2 required");
  for (int k = 0; k < n; k++) tau[k] = (double)t[k];
  return GEL_OK;
}

int gel_lgr_diffmat(int32_t n, double* D) {
  std::vector<double> d, t;
  if (!D || lgr_diffmat_ld(n, d, t)) return fail(GEL_ERR_ARG, "gel_lgr_diffmat: n >= 2 required");
  std::memcpy(D, d.data(), d.size() * 8);
  return GEL_OK;
}

}  // extern "C"
