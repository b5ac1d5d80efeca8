// The per-graph arithmetic of the device-resident Berendsen barostat (md_kernels.hip: hermnet_md_finish_npt): ONE text for
// the device kernels, their host twin (hermnet_host_md_finish_npt) and -- transcribed operation by operation -- the numpy
// float64 reference of tests/npt_reference.py.  Only IEEE +, -, x, / and comparisons on doubles, one rounding each
// (contraction off), in the order written: device, host and numpy agree bit for bit.  3x3 matrices are row-major [9]; the
// rows of a cell are the lattice vectors, so a coordinate scales as the row vector x mu.  Behind the arithmetic: the
// barostat's argument struct, its check and what one graph and one atom of a committed step do (md_finish.h's skeleton
// around them is the finish).
#ifndef HERMNET_NPT_STEP_H
#define HERMNET_NPT_STEP_H

#include "md_finish.h"

// The six entries of a symmetric 3x3 tensor, in the order the kinetic sums are taken.
#define HN_NPT_XX 0
#define HN_NPT_YY 1
#define HN_NPT_ZZ 2
#define HN_NPT_XY 3
#define HN_NPT_XZ 4
#define HN_NPT_YZ 5

// Atom i's terms of K_ab = sum m v_a v_b (m = 2 half_mass: exact; 0 for an atom that is held), added to the lane's partials.
HN_HD inline void npt_kinetic_terms(const double v[3], double half_mass, double s[6]) {
#pragma clang fp contract(off)
  const double m = 2.0 * half_mass;
  const double mx = m * v[0], my = m * v[1], mz = m * v[2];
  s[HN_NPT_XX] = s[HN_NPT_XX] + mx * v[0];
  s[HN_NPT_YY] = s[HN_NPT_YY] + my * v[1];
  s[HN_NPT_ZZ] = s[HN_NPT_ZZ] + mz * v[2];
  s[HN_NPT_XY] = s[HN_NPT_XY] + mx * v[1];
  s[HN_NPT_XZ] = s[HN_NPT_XZ] + mx * v[2];
  s[HN_NPT_YZ] = s[HN_NPT_YZ] + my * v[2];
}

HN_HD inline double npt_det3(const double c[9]) {
#pragma clang fp contract(off)
  return (c[0] * (c[4] * c[8] - c[5] * c[7]) + c[1] * (c[5] * c[6] - c[3] * c[8])) + c[2] * (c[3] * c[7] - c[4] * c[6]);
}

// inv = adj(c) / det(c).
HN_HD inline void npt_inverse3(const double c[9], double inv[9]) {
#pragma clang fp contract(off)
  const double det = npt_det3(c);
  inv[0] = (c[4] * c[8] - c[5] * c[7]) / det;
  inv[1] = (c[2] * c[7] - c[1] * c[8]) / det;
  inv[2] = (c[1] * c[5] - c[2] * c[4]) / det;
  inv[3] = (c[5] * c[6] - c[3] * c[8]) / det;
  inv[4] = (c[0] * c[8] - c[2] * c[6]) / det;
  inv[5] = (c[2] * c[3] - c[0] * c[5]) / det;
  inv[6] = (c[3] * c[7] - c[4] * c[6]) / det;
  inv[7] = (c[1] * c[6] - c[0] * c[7]) / det;
  inv[8] = (c[0] * c[4] - c[1] * c[3]) / det;
}

HN_HD inline int npt_not_finite(double a) { return !(a - a == 0.0); }

// One entry of mu - I asked for: -c (P0 delta_ab - P_ab), clamped to +-max_strain; *clamped is set where the clamp acted.
HN_HD inline double npt_strain(double c, double target, double p, double max_strain, int* clamped) {
#pragma clang fp contract(off)
  const double e = c * (target - p);
  if (e > max_strain) {
    *clamped = 1;
    return max_strain;
  }
  if (e < -max_strain) {
    *clamped = 1;
    return -max_strain;
  }
  return e;
}

// The barostat of one graph.  kin[6]: the kinetic tensor's sums; w[9]: the step's float32 virial; cell[9]: the float64 cell
// (the truth), replaced by cell mu.  Out: mu[9], cell32[9] = float(cell), inv[9] = the float64 inverse of the WIDENED
// float32 cell (what the search sees is what the next wrap uses), *e_kin = tr K / 2, *pressure = tr P / 3, *volume = |det
// cell| before the scaling.  Returns 1 where the clamp acted or the pressure was not finite (then mu = I), else 0.
HN_HD inline int npt_graph(const double kin[6], const float w[9], double c, double p0, int coupling, int mask, double max_strain,
                           double cell[9], double mu[9], float cell32[9], double inv[9], double* e_kin, double* pressure,
                           double* volume) {
#pragma clang fp contract(off)
  const double det = npt_det3(cell);
  const double vol = det < 0.0 ? -det : det;
  double p[9];
  p[0] = (kin[HN_NPT_XX] + 0.5 * ((double)w[0] + (double)w[0])) / vol;
  p[4] = (kin[HN_NPT_YY] + 0.5 * ((double)w[4] + (double)w[4])) / vol;
  p[8] = (kin[HN_NPT_ZZ] + 0.5 * ((double)w[8] + (double)w[8])) / vol;
  p[1] = p[3] = (kin[HN_NPT_XY] + 0.5 * ((double)w[1] + (double)w[3])) / vol;
  p[2] = p[6] = (kin[HN_NPT_XZ] + 0.5 * ((double)w[2] + (double)w[6])) / vol;
  p[5] = p[7] = (kin[HN_NPT_YZ] + 0.5 * ((double)w[5] + (double)w[7])) / vol;
  const double ptr3 = ((p[0] + p[4]) + p[8]) / 3.0;
  *e_kin = 0.5 * ((kin[HN_NPT_XX] + kin[HN_NPT_YY]) + kin[HN_NPT_ZZ]);
  *pressure = ptr3;
  *volume = vol;
  int bad = 0, clamped = 0;
  for (int k = 0; k < 9; ++k) bad |= npt_not_finite(p[k]);
  for (int k = 0; k < 9; ++k) mu[k] = (k % 4 == 0) ? 1.0 : 0.0;
  if (!bad) {
    if (coupling == HN_MD_BARO_ISOTROPIC) {
      const double e = npt_strain(c, p0, ptr3, max_strain, &clamped);
      for (int k = 0; k < 3; ++k) mu[4 * k] = 1.0 - e;
    } else if (coupling == HN_MD_BARO_AXES) {
      for (int k = 0; k < 3; ++k)
        if (mask & (1 << k)) mu[4 * k] = 1.0 - npt_strain(c, p0, p[4 * k], max_strain, &clamped);
    } else {
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          const double e = npt_strain(c, a == b ? p0 : 0.0, p[3 * a + b], max_strain, &clamped);
          mu[3 * a + b] = (a == b ? 1.0 : 0.0) - e;
        }
    }
  }
  double scaled[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      scaled[3 * i + j] = (cell[3 * i] * mu[j] + cell[3 * i + 1] * mu[3 + j]) + cell[3 * i + 2] * mu[6 + j];
  double wide[9];
  for (int k = 0; k < 9; ++k) {
    cell[k] = scaled[k];
    cell32[k] = (float)scaled[k];
    wide[k] = (double)cell32[k];
  }
  npt_inverse3(wide, inv);
  return bad | clamped;
}

// x <- x mu (a row vector).
HN_HD inline void npt_scale_atom(double x[3], const double mu[9]) {
#pragma clang fp contract(off)
  const double x0 = x[0], x1 = x[1], x2 = x[2];
  for (int j = 0; j < 3; ++j) x[j] = (x0 * mu[j] + x1 * mu[3 + j]) + x2 * mu[6 + j];
}

// ---- the barostat's part of hermnet_md_finish_npt: its arguments, and what one graph and one atom do -------------------------
namespace {

struct NptArgs {
  MdFinishArgs m;
  const long* batch;
  const float* virial;
  const double *pressure, *coupling_c;
  double* cell64;
  float* cell32;
  double *inv_cell, *mu;
  long* clamped;
  int coupling, mask;
  double max_strain;
};

inline bool npt_args_ok(const NptArgs& a) {
  if (!md_finish_args_ok(a.m)) return false;
  if (a.coupling != HN_MD_BARO_ISOTROPIC && a.coupling != HN_MD_BARO_AXES && a.coupling != HN_MD_BARO_FULL) return false;
  if ((a.mask & ~7) || !(a.max_strain > 0.0)) return false;
  return a.virial && a.pressure && a.coupling_c && a.cell64 && a.cell32 && a.inv_cell && a.mu && a.clamped;
}

// Graph g of a committed step, from its six kinetic sums: mu, the new cell in its three forms and the log row of width 5
// (E_pot, E_kin, edges found, the pressure mu was made from, the volume before the scaling).
HN_HD inline void npt_graph_one(const NptArgs& a, long step, int g, const double kin[6]) {
  float w[9], cell32[9];
  double cell[9], mu[9], inv[9], e_kin, pressure, volume;
  for (int k = 0; k < 9; ++k) {
    w[k] = a.virial[9 * (size_t)g + k];
    cell[k] = a.cell64[9 * (size_t)g + k];
  }
  const int acted = npt_graph(kin, w, a.coupling_c[g], a.pressure[g], a.coupling, a.mask, a.max_strain, cell, mu, cell32, inv,
                              &e_kin, &pressure, &volume);
  for (int k = 0; k < 9; ++k) {
    a.cell64[9 * (size_t)g + k] = cell[k];
    a.cell32[9 * (size_t)g + k] = cell32[k];
    a.inv_cell[9 * (size_t)g + k] = inv[k];
    a.mu[9 * (size_t)g + k] = mu[k];
  }
  if (acted) a.clamped[g] = a.clamped[g] + 1;
  double* row = hn_log_row(a.m.log, step, a.m.log_steps, a.m.num_graphs, g, 5);
  row[0] = (double)a.m.energy[g];
  row[1] = e_kin;
  row[2] = (double)a.m.total[0];
  row[3] = pressure;
  row[4] = volume;
}

HN_HD inline void npt_kinetic_of(const NptArgs& a, int i, double* s) {
  double v[3];
  for (int k = 0; k < 3; ++k) v[k] = a.m.v[3 * (size_t)i + k];
  npt_kinetic_terms(v, a.m.half_mass[i], s);
}

// Atom i of a committed step (held atoms too): x <- x mu of its graph, pos32 = float(x).
HN_HD inline void npt_scale_one(const NptArgs& a, int i) {
  const long g = hn_graph_of(a.batch, i, a.m.num_graphs);
  double mu[9], x[3];
  for (int k = 0; k < 9; ++k) mu[k] = a.mu[9 * g + k];
  for (int k = 0; k < 3; ++k) x[k] = a.m.x[3 * (size_t)i + k];
  npt_scale_atom(x, mu);
  for (int k = 0; k < 3; ++k) {
    a.m.x[3 * (size_t)i + k] = x[k];
    a.m.pos32[3 * (size_t)i + k] = (float)x[k];
  }
}

}  // namespace

#endif  // HERMNET_NPT_STEP_H
