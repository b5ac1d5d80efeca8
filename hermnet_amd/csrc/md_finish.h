// The finish skeleton of the MD drivers (md_kernels.hip: hermnet_md_finish / _npt; remd_kernels.hip: hermnet_remd_finish;
// pimd_kernels.hip: hermnet_pimd_finish; swapmc_kernels.hip: hermnet_swapmc_finish; nhc_kernels.hip: hermnet_nhc_finish),
// stated once as relax_driver.h states
// the relaxations': the arguments of the per-atom half of a finish, that half itself (the second kick, a void step's restore, a prime's copy), the test every
// kernel behind it makes (md_committed), E_kin in the canonical order, the log row, the commit -- the single writer of
// `state` --, the two kernels every driver launches unchanged, and the host twins' skeleton (md_host_finish) around the
// part that is a driver's own.  ONE text for the kernels and the host twins.
//
// Everything is in the unnamed namespace of the source that includes this: the kernels' argument types keep the names the
// launch records in profiles/ show.
#ifndef HERMNET_MD_FINISH_H
#define HERMNET_MD_FINISH_H

#include "md_step.h"

namespace {

struct MdFinishArgs {
  int n, num_graphs;
  double *x, *v;
  const double *x0, *v0;
  int* image;
  const int* image0;
  float* f_prev;
  const float *forces, *energy;
  const long* total;
  long capacity;
  const double *kick, *half_mass;
  const int* graph_ptr;
  float* pos32;
  double *ke_atom, *log;
  long log_steps;
  long* state;
};

HN_HD inline void md_finish_one(const MdFinishArgs& a, int i, long code, long mode) {
#pragma clang fp contract(off)
  if (mode != 0) {
    if (code == 0)
      for (int k = 0; k < 3; ++k) a.f_prev[3 * (size_t)i + k] = a.forces[3 * (size_t)i + k];
    return;
  }
  if (code != 0) {        // the step is void: back to the state it began with
    hn_restore_atom(i, a.x, a.x0, a.image, a.image0, a.pos32);
    for (int k = 0; k < 3; ++k) a.v[3 * (size_t)i + k] = a.v0[3 * (size_t)i + k];
    return;
  }
  double v[3];
  float f[3];
  for (int k = 0; k < 3; ++k) {
    v[k] = a.v[3 * (size_t)i + k];
    f[k] = a.forces[3 * (size_t)i + k];
  }
  a.ke_atom[i] = md_finish_atom(v, f, a.kick[i], a.half_mass[i]);
  for (int k = 0; k < 3; ++k) {
    a.v[3 * (size_t)i + k] = v[k];
    a.f_prev[3 * (size_t)i + k] = f[k];
  }
}

// The single writer of `state`: a void step records its halt, a completed one is counted; a prime clears its mode.
HN_HD inline void md_commit(long* state, long step, long code, long mode) {
  if (!hn_commit_halt(state, step, code) && mode == 0) state[HN_STATE_STEP] = step + 1;
  if (mode != 0) state[HN_STATE_MODE] = 0;
}

inline bool md_finish_args_ok(const MdFinishArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || a.log_steps < 1 || a.capacity < 0) return false;
  if (!a.state || !a.energy || !a.total || !a.graph_ptr || !a.log) return false;
  if (a.n == 0) return true;
  return a.x && a.v && a.x0 && a.v0 && a.image && a.image0 && a.f_prev && a.forces && a.kick && a.half_mass && a.pos32 &&
         a.ke_atom;
}

// True only on a step that commits -- not halted, not a prime, halt code 0 --, and *step is its index: what every kernel
// between the per-atom half and the commit asks first (observe_step.h's obs_due is the observers' counterpart).  On the
// device every lane of the workgroup calls it (hn_step_code ends in a barrier); the two words in front of that barrier are
// the same for every lane, so a workgroup returns as one.
HN_HD inline bool md_committed(const MdFinishArgs& m, long* step) {
  *step = m.state[HN_STATE_STEP];
  if (m.state[HN_STATE_CODE] != 0 || m.state[HN_STATE_MODE] != 0) return false;
  return hn_step_code(m.energy, m.num_graphs, m.total, m.capacity) == 0;
}

// Graph g's E_kin: its atoms' ke_atom in the canonical order (the 256 lanes of g's workgroup together; the host walks them).
HN_HD inline double md_kinetic_sum(const MdFinishArgs& m, int g, double (*part)[256]) {
#pragma clang fp contract(off)
  const int lo = hn_graph_lo(m.graph_ptr, g), hi = hn_graph_hi(m.graph_ptr, g, m.n);
  hn_canonical_sums<1, -1>(lo, hi, part, [&](int i, double* s) { s[0] = s[0] + m.ke_atom[i]; });
  return part[0][0];
}

HN_HD inline void md_log_row(const MdFinishArgs& a, long step, int g, double e_kin) {
  double* row = hn_log_row(a.log, step, a.log_steps, a.num_graphs, g, 3);
  row[0] = (double)a.energy[g];
  row[1] = e_kin;
  row[2] = (double)a.total[0];
}

// A host twin's finish behind its argument check: the per-atom half, `committed(step)` -- the loops that the driver's own
// launches are -- on a step that commits, then `commit(step, code, mode)` (without one: md_commit).
template <class Committed, class Commit>
inline void md_host_finish(const MdFinishArgs& m, Committed committed, Commit commit) {
  const long step = m.state[HN_STATE_STEP], mode = m.state[HN_STATE_MODE];
  if (m.state[HN_STATE_CODE] != 0) return;
  const long code = hn_step_code(m.energy, m.num_graphs, m.total, m.capacity);
  for (int i = 0; i < m.n; ++i) md_finish_one(m, i, code, mode);
  if (code == 0 && mode == 0) committed(step);
  commit(step, code, mode);
}

template <class Committed>
inline void md_host_finish(const MdFinishArgs& m, Committed committed) {
  md_host_finish(m, committed, [&](long step, long code, long mode) { md_commit(m.state, step, code, mode); });
}

#if defined(__HIPCC__)
// The first and the last launch of a finish: one lane per atom, 256-lane workgroups; one workgroup of 64.  Templates
// (Args = MdFinishArgs: launch them as md_finish_atoms_kernel<>, md_commit_kernel<>) only so that a source carries the
// kernels it launches and no dead copy of the other: remd_kernels.hip has a commit of its own, and cellrelax_kernels.hip,
// which comes here through npt_step.h's inverse, launches neither.
template <class Args = MdFinishArgs>
__global__ __launch_bounds__(256) void md_finish_atoms_kernel(Args a) {
  const long halted = a.state[HN_STATE_CODE], mode = a.state[HN_STATE_MODE];
  if (halted != 0) return;
  const long code = hn_step_code(a.energy, a.num_graphs, a.total, a.capacity);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) md_finish_one(a, i, code, mode);
}

template <class Args = MdFinishArgs>
__global__ __launch_bounds__(64) void md_commit_kernel(Args a) {
  const long step = a.state[HN_STATE_STEP], halted = a.state[HN_STATE_CODE], mode = a.state[HN_STATE_MODE];
  if (halted != 0) return;
  const long code = hn_step_code(a.energy, a.num_graphs, a.total, a.capacity);
  if (threadIdx.x == 0) md_commit(a.state, step, code, mode);
}
#endif

}  // namespace

#endif  // HERMNET_MD_FINISH_H
