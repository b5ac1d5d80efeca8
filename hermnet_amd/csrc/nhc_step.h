// Nose-Hoover chain NVT inside the replayed MD step (nhc_kernels.hip; hermnet_amd/nhc.py: DeviceNHC): ONE text for the device
// kernels, the host twins (hermnet_host_nhc_advance / _finish) and -- transcribed operation by operation --
// tests/nhc_reference.py.  Contraction is off inside every function: only IEEE +, x, floor, ldexp and the library's own exp
// (metad_step.h: mt_exp) on doubles, one rounding each, in the order written; every division is made on the host.
//
// A time step:  NHC(dt/2) . kick(dt/2) . drift(dt) . [forces] . kick(dt/2) . NHC(dt/2)  -- kick, drift, wrap, the void step's
// restore and the commit are md_step.h's and md_finish.h's, unchanged.  A chain couples to its graph through ONE number, the
// kinetic energy, and acts on it through ONE factor:
//
// NHC(Delta) of graph g (Martyna, Tuckerman, Tobias, Klein, Mol. Phys. 87, 1117 (1996)), chain of M thermostats (xi_j, v_j)
// with masses Q_1 = dof kB T tau^2, Q_j = kB T tau^2; K2 = 2 E_kin, s = 1; for each of `substeps` substeps and each of the
// `order` Suzuki-Yoshida weights w, with d = delta[w] = w Delta / substeps made on the host, d2 = 0.5 d, d4 = 0.25 d:
//   1  v_M = v_M + G_M d2
//   2  j = M-1 ... 1:  e = mt_exp(-(d4 v_{j+1}));  v_j = (v_j e + G_j d2) e
//   3  a = mt_exp(-(d v_1));  s = s a;  K2 = (K2 a) a
//   4  xi_j = xi_j + d v_j  for every j
//   5  j = 1 ... M-1:  e = mt_exp(-(d4 v_{j+1}));  v_j = (v_j e + G_j d2) e
//   6  v_M = v_M + G_M d2
// G_1 = (K2 - dof_kt) inv_q_1,  G_j = (q_{j-1} (v_{j-1} v_{j-1}) - kt) inv_q_j,  always from the current values (M = 1: the
// loops are empty and G_M is G_1).  The velocities of the graph are multiplied by s.  tau = inf: q = inv_q = 0 and v = 0, so
// every G is 0, every factor mt_exp(+-0) = 1.0 exactly and the step is hermnet_md_advance's / _finish's NVE bit for bit.
//
// The conserved quantity is E_pot + E_kin + E_nhc,  E_nhc = dof_kt xi_1 + kt sum_{j>=2} xi_j + sum_j 0.5 (q_j (v_j v_j)),
// added in that order from the first term.
//
// Launches.  advance: nhc_open_kernel (a workgroup per graph: E_kin from v and half_mass in the canonical order -- NOT a number
// the last finish left, so velocities written from outside need no bookkeeping --; lane 0 backs the chain up, runs NHC(dt/2)
// and writes scale[g][0]), nhc_advance_kernel (a lane per atom: md_advance_one with v scale[g][0] in front of the first kick;
// the backup v0 is the unscaled v).  finish: md_finish_atoms_kernel<> (unchanged), nhc_close_kernel (a workgroup per graph: on
// a step that commits the canonical E_kin, NHC(dt/2), scale[g][1] and the log row (E_pot, (K s) s, edges, E_nhc); on a void
// step the chain's restore), nhc_scale_kernel (a lane per atom: v scale[g][1] on a step that commits), md_commit_kernel<>
// (unchanged: the single writer of `state`).  No atomics; no workgroup reads what another of the same launch writes.
#ifndef HERMNET_NHC_STEP_H
#define HERMNET_NHC_STEP_H

#include "md_finish.h"
#include "metad_step.h"

#define HN_NHC_MAX_CHAIN 8
#define HN_NHC_LOG_WIDTH 4

namespace {

// The chains of the B graphs: constants made on the host, the state and its backup.
struct NhcChains {
  int chain, order, substeps;        // M, Suzuki-Yoshida weights, substeps
  const double* delta;               // [order]: w (dt / 2) / substeps
  const double *kt, *dof_kt;         // [B]: kB T, dof kB T
  const double *q, *inv_q;           // [B,M]; tau = inf: both 0
  double *xi, *v_xi, *xi0, *v_xi0;   // [B,M]; the backups: nhc_open
  double* scale;                     // [B,2]: the last opening and closing factor
};

struct NhcAdvanceArgs {
  MdAdvanceArgs m;                   // hermnet_md_advance's, without a Langevin thermostat
  const int* graph_ptr;
  const double* half_mass;
  NhcChains c;
};

struct NhcFinishArgs {
  MdFinishArgs m;
  const long* batch;
  NhcChains c;
};

inline bool nhc_chains_ok(const NhcChains& c) {
  if (c.chain < 1 || c.chain > HN_NHC_MAX_CHAIN || c.substeps < 1) return false;
  if (c.order != 1 && c.order != 3 && c.order != 5) return false;
  return c.delta && c.kt && c.dof_kt && c.q && c.inv_q && c.xi && c.v_xi && c.xi0 && c.v_xi0 && c.scale;
}

inline bool nhc_advance_args_ok(const NhcAdvanceArgs& a) {
  if (!md_advance_args_ok(a.m) || (a.m.flags & HN_MD_LANGEVIN) || !a.m.state || !a.graph_ptr) return false;
  return nhc_chains_ok(a.c) && (a.m.n == 0 || a.half_mass);
}

inline bool nhc_finish_args_ok(const NhcFinishArgs& a) { return md_finish_args_ok(a.m) && nhc_chains_ok(a.c); }

// G_j (j counts from 0) from the current values.
HN_HD inline double nhc_force(int j, double k2, const double* v, double kt, double dof_kt, const double* q, const double* inv_q) {
#pragma clang fp contract(off)
  if (j == 0) return (k2 - dof_kt) * inv_q[0];
  return (q[j - 1] * (v[j - 1] * v[j - 1]) - kt) * inv_q[j];
}

// NHC(Delta) of graph g on the caller's copies xi, v [M] and *k2; returns s.
HN_HD inline double nhc_half_step(const NhcChains& c, int g, double* xi, double* v, double* k2_io) {
#pragma clang fp contract(off)
  const int M = c.chain;
  const double kt = c.kt[g], dof_kt = c.dof_kt[g];
  const double *q = c.q + (size_t)g * M, *inv_q = c.inv_q + (size_t)g * M;
  double k2 = *k2_io, s = 1.0;
  for (int n = 0; n < c.substeps; ++n)
    for (int w = 0; w < c.order; ++w) {
      const double d = c.delta[w], d2 = 0.5 * d, d4 = 0.25 * d;
      v[M - 1] = v[M - 1] + nhc_force(M - 1, k2, v, kt, dof_kt, q, inv_q) * d2;
      for (int j = M - 2; j >= 0; --j) {
        const double e = mt_exp(-(d4 * v[j + 1]));
        v[j] = (v[j] * e + nhc_force(j, k2, v, kt, dof_kt, q, inv_q) * d2) * e;
      }
      const double a = mt_exp(-(d * v[0]));
      s = s * a;
      k2 = (k2 * a) * a;
      for (int j = 0; j < M; ++j) xi[j] = xi[j] + d * v[j];
      for (int j = 0; j < M - 1; ++j) {
        const double e = mt_exp(-(d4 * v[j + 1]));
        v[j] = (v[j] * e + nhc_force(j, k2, v, kt, dof_kt, q, inv_q) * d2) * e;
      }
      v[M - 1] = v[M - 1] + nhc_force(M - 1, k2, v, kt, dof_kt, q, inv_q) * d2;
    }
  *k2_io = k2;
  return s;
}

// E_nhc of graph g's chain.
HN_HD inline double nhc_energy(const NhcChains& c, int g, const double* xi, const double* v) {
#pragma clang fp contract(off)
  const int M = c.chain;
  const double* q = c.q + (size_t)g * M;
  double e = c.dof_kt[g] * xi[0];
  for (int j = 1; j < M; ++j) e = e + c.kt[g] * xi[j];
  for (int j = 0; j < M; ++j) e = e + 0.5 * (q[j] * (v[j] * v[j]));
  return e;
}

// Graph g's E_kin from v and half_mass in the canonical order (the 256 lanes of g's workgroup together; the host walks them).
HN_HD inline double nhc_kinetic_sum(const NhcAdvanceArgs& a, int g, double (*part)[256]) {
#pragma clang fp contract(off)
  const int lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.m.n);
  const double* v = a.m.v;
  hn_canonical_sums<1, -1>(lo, hi, part, [&](int i, double* s) {
    const double v0 = v[3 * (size_t)i], v1 = v[3 * (size_t)i + 1], v2 = v[3 * (size_t)i + 2];
    s[0] = s[0] + a.half_mass[i] * ((v0 * v0 + v1 * v1) + v2 * v2);
  });
  return part[0][0];
}

// The half step of graph g's chain with K2 = 2 e_kin; slot 0: the opening one (the chain is backed up first), 1: the closing
// one.  Returns what the chain left of K2.
HN_HD inline double nhc_graph_one(const NhcChains& c, int g, double e_kin, int slot) {
#pragma clang fp contract(off)
  const int M = c.chain;
  double xi[HN_NHC_MAX_CHAIN], v[HN_NHC_MAX_CHAIN];
  for (int j = 0; j < M; ++j) {
    xi[j] = c.xi[(size_t)g * M + j];
    v[j] = c.v_xi[(size_t)g * M + j];
    if (slot == 0) {
      c.xi0[(size_t)g * M + j] = xi[j];
      c.v_xi0[(size_t)g * M + j] = v[j];
    }
  }
  double k2 = 2.0 * e_kin;
  c.scale[2 * (size_t)g + slot] = nhc_half_step(c, g, xi, v, &k2);
  for (int j = 0; j < M; ++j) {
    c.xi[(size_t)g * M + j] = xi[j];
    c.v_xi[(size_t)g * M + j] = v[j];
  }
  return k2;
}

// The closing half step of a step that commits, and the log row: E_kin behind the closing factor, (K s) s.
HN_HD inline void nhc_close_one(const NhcFinishArgs& a, long step, int g, double e_kin) {
#pragma clang fp contract(off)
  nhc_graph_one(a.c, g, e_kin, 1);
  const double s = a.c.scale[2 * (size_t)g + 1];
  double* row = hn_log_row(a.m.log, step, a.m.log_steps, a.m.num_graphs, g, HN_NHC_LOG_WIDTH);
  row[0] = (double)a.m.energy[g];
  row[1] = (e_kin * s) * s;
  row[2] = (double)a.m.total[0];
  row[3] = nhc_energy(a.c, g, a.c.xi + (size_t)g * a.c.chain, a.c.v_xi + (size_t)g * a.c.chain);
}

// A void step: graph g's chain returns to where the step began.
HN_HD inline void nhc_restore_one(const NhcChains& c, int g) {
  for (int j = 0; j < c.chain; ++j) {
    c.xi[(size_t)g * c.chain + j] = c.xi0[(size_t)g * c.chain + j];
    c.v_xi[(size_t)g * c.chain + j] = c.v_xi0[(size_t)g * c.chain + j];
  }
}

// md_advance_one (md_step.h) of a step without noise, with v scale[g][0] in front of the first kick.
HN_HD inline void nhc_advance_one(const NhcAdvanceArgs& a, int i, long mode) {
#pragma clang fp contract(off)
  const MdAdvanceArgs& m = a.m;
  double x[3], v[3];
  for (int k = 0; k < 3; ++k) x[k] = m.x[3 * (size_t)i + k];
  if (mode == 0) {
    int image[3];
    float f[3];
    for (int k = 0; k < 3; ++k) {
      v[k] = m.v[3 * (size_t)i + k];
      image[k] = m.image[3 * (size_t)i + k];
      f[k] = m.f_prev[3 * (size_t)i + k];
      m.x0[3 * (size_t)i + k] = x[k];
      m.v0[3 * (size_t)i + k] = v[k];
      m.image0[3 * (size_t)i + k] = image[k];
    }
    const long g = hn_graph_of(m.batch, i, m.num_graphs);
    const double s = a.c.scale[2 * (size_t)g], none[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k) v[k] = v[k] * s;
    md_advance_atom(x, v, f, m.kick[i], m.dt, 0, 0.0, 0.0, none);
    if (m.flags & HN_MD_WRAP) {
      double cell[9], inv[9];
      hn_load_cell(m.cell, m.inv_cell, g, cell, inv);
      md_wrap_atom(x, image, cell, inv);
    }
    for (int k = 0; k < 3; ++k) {
      m.x[3 * (size_t)i + k] = x[k];
      m.v[3 * (size_t)i + k] = v[k];
      m.image[3 * (size_t)i + k] = image[k];
    }
  }
  for (int k = 0; k < 3; ++k) m.pos32[3 * (size_t)i + k] = (float)x[k];
}

// The closing factor on atom i's velocity (a step that commits).
HN_HD inline void nhc_scale_one(const NhcFinishArgs& a, int i) {
#pragma clang fp contract(off)
  const double s = a.c.scale[2 * (size_t)hn_graph_of(a.batch, i, a.m.num_graphs) + 1];
  for (int k = 0; k < 3; ++k) a.m.v[3 * (size_t)i + k] = a.m.v[3 * (size_t)i + k] * s;
}

}  // namespace

#endif  // HERMNET_NHC_STEP_H
