// gel_wind_rows.h -- the last link of the wind-profile sensitivities: from the interpolated wind to the rows of
// the table.  With the altitudes x fixed, the lookup of wind_ned2_centre is linear in the table's values W [Kw][2]; along a seed
// dW it is the same lookup applied to the seed, on the piece the VALUE lookup took (xl < h <= xu; piece -1: h <= x[0]; piece -2:
// h > x[Kw - 1]).
//
// THE EXPRESSION (fp64; the tangent kernel, the adjoint kernel and the tests' host restatement use exactly this):
//   inside the table, piece = i:  th = (h - x[i]) / (x[i + 1] - x[i])            one division per stage, nothing staged
//       tangent:  fma(th, dW[i + 1] - dW[i], dW[i])
//       adjoint:  cell(i) = fma(1.0 - th, m, cell(i)), then cell(i + 1) = fma(th, m, cell(i + 1))
//   clamped ends:  i0 = i1 = 0 (piece -1) or Kw - 1 (piece -2), th = 0.0
//       tangent:  dW[i0]         adjoint:  cell(i0) = cell(i0) + m
// The rows are SELECTED with clamps to 0 .. Kw - 1 from piece (which wind_ned2_centre returns in {-2, -1, 0 .. Kw - 2}): no address
// is formed by arithmetic on an unchecked value.
#pragma once
#include "gel_physics.h"

namespace gel {

struct WindRows {
  int i0, i1;   // the two rows of the piece; the end row twice in a clamped end
  double th;    // the weight of row i1 (row i0: 1 - th); 0 in a clamped end
};

GEL_DEV WindRows wind_rows(double h, int piece, const double* tab, int Kw) {
  const int last = Kw - 1;
  const bool in = piece >= 0;
  WindRows r;
  r.i0 = min(max(in ? piece : (piece == -1 ? 0 : last), 0), last);
  r.i1 = min(max(in ? piece + 1 : r.i0, 0), last);
  const double xl = tab[3 * r.i0], xu = tab[3 * r.i1];
  const double den = in ? xu - xl : 1.0;
  r.th = in ? (h - xl) / den : 0.0;
  return r;
}

// the seed's component c (0 north, 1 east) on the rows of r; dw [Kw][2]
GEL_DEV double wind_rows_seed(const WindRows& r, const double* dw, int c) {
  const double a = dw[2 * r.i0 + c], b = dw[2 * r.i1 + c];
  return (r.i1 != r.i0) ? __builtin_fma(r.th, b - a, a) : a;
}

}  // namespace gel
