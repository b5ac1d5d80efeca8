// What the finishes of the MD drivers share (md_kernels.hip: hermnet_md_finish / _npt; remd_kernels.hip:
// hermnet_remd_finish): the arguments of the per-atom half of a finish, that half itself (the second kick, a void step's
// restore, a prime's copy) and the commit, the single writer of `state`.  ONE text for the kernels and the host twins.
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

}  // namespace

#endif  // HERMNET_MD_FINISH_H
