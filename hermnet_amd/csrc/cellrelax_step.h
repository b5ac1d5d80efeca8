// The arithmetic of the device-resident cell relaxation (cellrelax_kernels.hip): ONE text for the device kernels, their host
// twins (hermnet_host_cellrelax_advance / _finish) and -- transcribed operation by operation -- the numpy float64 reference of
// tests/cellrelax_reference.py.  The model is ASE's UnitCellFilter under ASE's FIRE, independently per graph.  Only IEEE +,
// -, x, / and comparisons on doubles, one rounding each (contraction off), in the order written.  3x3 matrices are row-major
// [9]; the rows of a cell are the lattice vectors.
//
// Per graph, with C0 the float64 cell at construction and cf = cell_factor:
//   the deformation gradient F starts as I, the cell is C = C0 F^T;
//   generalised coordinates: q_i = x_i F^-T (the reference-frame coordinates: the STATE) and three cell rows G = cf F;
//   generalised forces:      fq_i = f_i F (0 for an atom that is held) and fG = proj(S F^-T) / cf with S = sym(W) - p V I,
//                            W the step's float32 virial widened, V = |det C|, p the external pressure;
//   proj, in ASE's order: hydrostatic_strain (replace by (tr / 3) I), x mask entry-wise, constant_volume (subtract tr / 3
//   from the diagonal);  the objective is the enthalpy E + p V.
// FIRE is relax_step.h's relax_graph_update / relax_velocity_atom / relax_graph_scale, unchanged, on all n + 3 rows.
//
// THE SUM ORDER (part of the contract: the sums steer the trajectory).  P = sum fq.vq, ff = sum fq.fq, vv = sum vq.vq and
// the clamp's s = sum v.v are the ATOMS' canonical sums of resident_step.h first (a term is (t0 + t1) + t2); the three cell
// rows' terms are then added to that result in row order 0, 1, 2: ((atoms + row0) + row1) + row2.  fm2 is the maximum over
// atoms and cell rows (the atoms' canonical maximum, then the rows 0, 1, 2), so `fmax` is one threshold on generalised forces.
#ifndef HERMNET_CELLRELAX_STEP_H
#define HERMNET_CELLRELAX_STEP_H

#include "npt_step.h"
#include "relax_step.h"

// From the cell rows G: F = G / cf, C = C0 F^T, cell32 = float(C), det F and F^-1 = adj(F) / det F (npt_inverse3).
HN_HD inline void cellrelax_cell(const double G[9], double cf, const double C0[9], double F[9], double Finv[9], double C[9],
                                 float cell32[9], double* det_f) {
#pragma clang fp contract(off)
  for (int k = 0; k < 9; ++k) F[k] = G[k] / cf;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (C0[3 * i] * F[3 * j] + C0[3 * i + 1] * F[3 * j + 1]) + C0[3 * i + 2] * F[3 * j + 2];
  for (int k = 0; k < 9; ++k) cell32[k] = (float)C[k];
  *det_f = npt_det3(F);
  npt_inverse3(F, Finv);
}

// x = q F^T (a row vector).
HN_HD inline void cellrelax_to_cart(const double q[3], const double F[9], double x[3]) {
#pragma clang fp contract(off)
  for (int j = 0; j < 3; ++j) x[j] = (q[0] * F[3 * j] + q[1] * F[3 * j + 1]) + q[2] * F[3 * j + 2];
}

// fq = f F (f: relax_force's, already zero for an atom that is held).
HN_HD inline void cellrelax_atom_force(const double f[3], const double F[9], double fq[3]) {
#pragma clang fp contract(off)
  for (int j = 0; j < 3; ++j) fq[j] = (f[0] * F[j] + f[1] * F[3 + j]) + f[2] * F[6 + j];
}

// The cell rows' generalised force fG [9] of one graph, and what the evaluation says about the cell: *volume = |det C|,
// *pressure = tr W / 3V, stress [9] = -sym(W) / V.  mask [9]: the entry-wise factors.
HN_HD inline void cellrelax_cell_force(const float w[9], const double C[9], const double Finv[9], double cf, double p,
                                       const double mask[9], int flags, double fG[9], double* volume, double* pressure,
                                       double stress[9]) {
#pragma clang fp contract(off)
  const double det = npt_det3(C);
  const double vol = det < 0.0 ? -det : det;
  double sw[9], s[9], a[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) sw[3 * i + j] = 0.5 * ((double)w[3 * i + j] + (double)w[3 * j + i]);
  const double pv = p * vol;
  for (int k = 0; k < 9; ++k) {
    s[k] = (k % 4 == 0) ? sw[k] - pv : sw[k];
    stress[k] = -sw[k] / vol;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) a[3 * i + j] = (s[3 * i] * Finv[3 * j] + s[3 * i + 1] * Finv[3 * j + 1]) + s[3 * i + 2] * Finv[3 * j + 2];
  if (flags & HN_CELLRELAX_HYDROSTATIC) {
    const double t = ((a[0] + a[4]) + a[8]) / 3.0;
    for (int k = 0; k < 9; ++k) a[k] = (k % 4 == 0) ? t : 0.0;
  }
  for (int k = 0; k < 9; ++k) a[k] = a[k] * mask[k];
  if (flags & HN_CELLRELAX_CONSTANT_VOLUME) {
    const double t = ((a[0] + a[4]) + a[8]) / 3.0;
    for (int k = 0; k < 3; ++k) a[4 * k] = a[4 * k] - t;
  }
  for (int k = 0; k < 9; ++k) fG[k] = a[k] / cf;
  *volume = vol;
  *pressure = (((sw[0] + sw[4]) + sw[8]) / 3.0) / vol;
}

// The three cell rows' terms of the four sums, added to the atoms' results in row order (the header's note).
HN_HD inline void cellrelax_add_rows(const double fG[9], const double vG[9], double s[4]) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; ++r) {
    const double f2 = relax_dot3(fG + 3 * r, fG + 3 * r);
    s[0] = s[0] + relax_dot3(fG + 3 * r, vG + 3 * r);
    s[1] = s[1] + f2;
    s[2] = s[2] + relax_dot3(vG + 3 * r, vG + 3 * r);
    s[3] = f2 > s[3] ? f2 : s[3];
  }
}

// The cell rows' new velocities; returns the clamp's sum with their terms added in row order.
HN_HD inline double cellrelax_rows_velocity(double vG[9], const double fG[9], const RelaxCoef& c, double s) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; ++r) {
    relax_velocity_atom(vG + 3 * r, fG + 3 * r, c, 0);
    s = s + relax_dot3(vG + 3 * r, vG + 3 * r);
  }
  return s;
}

// What makes a step void beside resident_step.h's causes: a virial entry that is not finite, or det F <= 0 (NaN too).
HN_HD inline int cellrelax_bad_graph(const float w[9], double det_f) {
  int bad = !(det_f > 0.0);
  for (int k = 0; k < 9; ++k) bad |= hn_not_finite(w[k]);
  return bad;
}

#endif  // HERMNET_CELLRELAX_STEP_H
