// The arithmetic of the device-resident FIRE relaxation (relax_kernels.hip; the finish that strings it together, for the
// cell relaxation too: relax_driver.h): ONE text for the device kernels, their host twins (hermnet_host_relax_advance /
// _finish) and -- transcribed operation by operation -- the numpy float64 reference of tests/relax_reference.py.  FIRE as
// ASE's optimize/fire.py steps it (Bitzek et al., PRL 97, 170201), independently per graph.  Per-atom work is IEEE + and x
// on doubles, one rounding each (contraction off), in the order written; `/` and sqrt appear in the two per-graph scalar
// functions alone (relax_graph_update, relax_graph_scale), where they are the correctly rounded IEEE operations on the
// device as on the host (no fast-math).
//
// The per-graph sums that steer the trajectory take the canonical order of resident_step.h; an atom's term is (t0 + t1) + t2.
#ifndef HERMNET_RELAX_STEP_H
#define HERMNET_RELAX_STEP_H

#include "resident_step.h"

// ASE's defaults; the time step, its ceiling, the longest step and the force threshold are arguments.
#define HN_RELAX_NMIN 5
#define HN_RELAX_FINC 1.1
#define HN_RELAX_FDEC 0.5
#define HN_RELAX_ASTART 0.1
#define HN_RELAX_FA 0.99

// What a graph's scalar decision asks of its atoms' velocities, before v += dt f.
#define HN_RELAX_KEEP 0      // the first step of a run: v as it is
#define HN_RELAX_MIX 1       // downhill: v = keep v + cf f
#define HN_RELAX_STOP 2      // uphill: v = 0
#define HN_RELAX_FREEZE 3    // converged: v = 0 and no kick

// A graph's state.  In memory: gf [B,5] float64 = (dt, a, scale, fnorm, energy), gi [B,4] int64 = (nsteps, fresh, converged,
// conv_step).  scale: what the next advance multiplies v with (dt, shortened where dt |v| > maxstep; 0 until the first
// evaluation and once converged).  fnorm, energy: max |f_i| and E_pot of the graph's last evaluation while it was moving.
struct RelaxGraph {
  double dt, a, scale, fnorm, energy;
  long long nsteps, fresh, converged, conv_step;
};

struct RelaxCoef {
  int mode;
  double keep, cf, dt;
};

HN_HD inline RelaxGraph relax_graph_load(const double* gf, const long* gi, int g) {
  RelaxGraph G;
  G.dt = gf[5 * (size_t)g], G.a = gf[5 * (size_t)g + 1], G.scale = gf[5 * (size_t)g + 2];
  G.fnorm = gf[5 * (size_t)g + 3], G.energy = gf[5 * (size_t)g + 4];
  G.nsteps = gi[4 * (size_t)g], G.fresh = gi[4 * (size_t)g + 1];
  G.converged = gi[4 * (size_t)g + 2], G.conv_step = gi[4 * (size_t)g + 3];
  return G;
}

HN_HD inline void relax_graph_store(const RelaxGraph& G, double* gf, long* gi, int g) {
  gf[5 * (size_t)g] = G.dt, gf[5 * (size_t)g + 1] = G.a, gf[5 * (size_t)g + 2] = G.scale;
  gf[5 * (size_t)g + 3] = G.fnorm, gf[5 * (size_t)g + 4] = G.energy;
  gi[4 * (size_t)g] = (long)G.nsteps, gi[4 * (size_t)g + 1] = (long)G.fresh;
  gi[4 * (size_t)g + 2] = (long)G.converged, gi[4 * (size_t)g + 3] = (long)G.conv_step;
}

HN_HD inline double relax_dot3(const double p[3], const double q[3]) {
#pragma clang fp contract(off)
  return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2];
}

// An atom's forces as the optimiser sees them: float32 widened, zero for an atom that is held.
HN_HD inline void relax_force(const float* forces, const unsigned char* fixed, int i, double f[3]) {
  const int held = fixed && fixed[i];
  for (int k = 0; k < 3; ++k) f[k] = held ? 0.0 : (double)forces[3 * (size_t)i + k];
}

// The move in front of the search: x += scale v, then the wrap.
HN_HD inline void relax_advance_atom(double x[3], int image[3], const double v[3], double scale, const double* cell,
                                     const double* inv) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; ++k) x[k] = x[k] + scale * v[k];
  if (cell) md_wrap_atom(x, image, cell, inv);
}

// ASE's FIRE.step up to the velocity update, on the graph's four sums P = sum f.v, ff = sum f.f, vv = sum v.v and
// fm2 = max |f_i|^2.  `step`: the evaluation's index, `dt0`: the time step a fresh run starts with.
HN_HD inline RelaxCoef relax_graph_update(double P, double ff, double vv, double fm2, double fmax, double dt0, double dtmax,
                                          long long step, RelaxGraph& G) {
#pragma clang fp contract(off)
  RelaxCoef c = {HN_RELAX_KEEP, 0.0, 0.0, 0.0};
  G.fnorm = sqrt(fm2);
  if (fm2 < fmax * fmax) {
    G.converged = 1, G.conv_step = step, G.scale = 0.0;
    c.mode = HN_RELAX_FREEZE;
    return c;
  }
  if (G.fresh) {
    G.fresh = 0, G.dt = dt0, G.a = HN_RELAX_ASTART, G.nsteps = 0;
  } else if (P > 0.0) {
    c.mode = HN_RELAX_MIX;
    c.keep = 1.0 - G.a;
    c.cf = ff > 0.0 ? (G.a / sqrt(ff)) * sqrt(vv) : 0.0;
    if (G.nsteps > HN_RELAX_NMIN) {
      const double grown = G.dt * HN_RELAX_FINC;
      G.dt = grown < dtmax ? grown : dtmax;
      G.a = G.a * HN_RELAX_FA;
    }
    G.nsteps += 1;
  } else {
    c.mode = HN_RELAX_STOP;
    G.a = HN_RELAX_ASTART;
    G.dt = G.dt * HN_RELAX_FDEC;
    G.nsteps = 0;
  }
  c.dt = G.dt;
  return c;
}

// The velocity update of one atom (f: relax_force's); an atom that is held keeps v = 0.
HN_HD inline void relax_velocity_atom(double v[3], const double f[3], const RelaxCoef& c, int held) {
#pragma clang fp contract(off)
  if (held || c.mode == HN_RELAX_FREEZE) {
    for (int k = 0; k < 3; ++k) v[k] = 0.0;
    return;
  }
  if (c.mode == HN_RELAX_MIX)
    for (int k = 0; k < 3; ++k) v[k] = c.keep * v[k] + c.cf * f[k];
  else if (c.mode == HN_RELAX_STOP)
    for (int k = 0; k < 3; ++k) v[k] = 0.0;
  for (int k = 0; k < 3; ++k) v[k] = v[k] + c.dt * f[k];
}

// The step clamp on s = sum v.v of the new velocities: the next move is scale v, no longer than maxstep.
HN_HD inline double relax_graph_scale(double s, double dt, double maxstep) {
#pragma clang fp contract(off)
  const double nd = dt * sqrt(s);
  return nd > maxstep ? dt * (maxstep / nd) : dt;
}

#endif  // HERMNET_RELAX_STEP_H
