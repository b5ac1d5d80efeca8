// The step protocol of the device-resident drivers (md_kernels.hip, relax_kernels.hip, cellrelax_kernels.hip), stated once:
// ONE text for the device kernels and their host twins, transcribed operation by operation in tests/md_reference.py,
// tests/relax_reference.py and tests/cellrelax_reference.py.  Contraction is off inside every function, so device, host and
// numpy agree bit for bit.  hn_lead_lane and hn_barrier let a driver write a workgroup's body and its host loop as one text
// too (relax_driver.h: the FIRE finish of both relaxations).
//
// A driver brackets the captured step with an advance in front of the neighbour search and a finish behind the force
// backward.  Finish derives the step's halt code from what the evaluation left behind (hn_step_code); every workgroup derives
// the same code for itself.  Code != 0: the step is VOID -- every atom returns to where the step began (hn_restore_atom), no
// log row is written, (code, step) is recorded (hn_commit_halt), and while the code is set every kernel returns at once.  The
// words the kernels branch on are written by the LAST, single-workgroup kernel of finish alone, so every workgroup of a step
// reads the words the step began with, whatever the order they are scheduled in.
#ifndef HERMNET_RESIDENT_STEP_H
#define HERMNET_RESIDENT_STEP_H

#include <math.h>
#include <stdint.h>
#include "../../include/hermnet_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HN_HD __host__ __device__
#else
#define HN_HD
#endif

// state [4] int64 = (step, halt code, step at which it halted, the driver's own word).
#define HN_STATE_STEP 0
#define HN_STATE_CODE 1
#define HN_STATE_HALT_STEP 2
#define HN_STATE_MODE 3  // MD: 1 = prime (evaluate the forces of the coordinates as they are)
#define HN_STATE_DONE 3  // relaxation: every graph has converged

// The bits of a halt code: the neighbour list's flags, more pairs than columns, an energy that is not finite.
#define HN_HALT_LIST_FLAGS 255
#define HN_HALT_CAPACITY 4
#define HN_HALT_NONFINITE HN_MD_HALT_NONFINITE

// Halt code of a step from what the force evaluation left behind: the list's flags (+ the capacity bit where only the count
// says so) in the low bits, HN_HALT_NONFINITE for an energy that is not finite (the stale-weight guard answers with NaN).
HN_HD inline long long md_step_code(long long found, long long flags, long long capacity, int nonfinite) {
  long long code = flags & HN_HALT_LIST_FLAGS;
  if (found > capacity) code |= HN_HALT_CAPACITY;
  if (nonfinite) code |= HN_HALT_NONFINITE;
  return code;
}

HN_HD inline int hn_not_finite(float e) { return !(e - e == 0.0f); }

// The step's halt code from the B energies and the list's (found, flags).  On the device every lane of the workgroup
// calls it (B energies from the cache: nothing to what a launch costs) and every lane gets the code; on the host one call.
HN_HD inline long hn_step_code(const float* energy, int num_graphs, const long* total, long capacity) {
  int bad = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  for (int g = threadIdx.x; g < num_graphs; g += blockDim.x) bad |= hn_not_finite(energy[g]);
  bad = __syncthreads_or(bad);
#else
  for (int g = 0; g < num_graphs; ++g) bad |= hn_not_finite(energy[g]);
#endif
  return md_step_code(total[0], total[1], capacity, bad);
}

// For a text that a workgroup and a host loop both run (relax_driver.h): the lane that does a graph's scalar work, and the
// workgroup's barrier.  The host is that lane, and has nobody to wait for.
HN_HD inline bool hn_lead_lane() {
#if defined(__HIP_DEVICE_COMPILE__)
  return threadIdx.x == 0;
#else
  return true;
#endif
}

HN_HD inline void hn_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}

// The halt half of the commit (the single writer of `state`): true where the step was void.
HN_HD inline bool hn_commit_halt(long* state, long step, long code) {
  if (code == 0) return false;
  state[HN_STATE_CODE] = code;
  state[HN_STATE_HALT_STEP] = step;
  return true;
}

// Triclinic wrap: s = x cell^-1 (rows of `cell` are the lattice vectors), x -= floor(s) cell, image += floor(s).  A
// coordinate that is not finite, or 2^30 cells away, is left alone (the cast below would be undefined).
HN_HD inline void md_wrap_atom(double x[3], int image[3], const double cell[9], const double inv[9]) {
#pragma clang fp contract(off)
  double n[3];
  for (int k = 0; k < 3; ++k) {
    const double s = (x[0] * inv[k] + x[1] * inv[3 + k]) + x[2] * inv[6 + k];
    const double fl = floor(s);
    n[k] = (fl >= -1073741824.0 && fl <= 1073741824.0) ? fl : 0.0;
  }
  for (int j = 0; j < 3; ++j) x[j] = x[j] - ((n[0] * cell[j] + n[1] * cell[3 + j]) + n[2] * cell[6 + j]);
  for (int k = 0; k < 3; ++k) image[k] += (int)n[k];
}

// The graph of atom i (a broken `batch` must not read out of bounds).
HN_HD inline long hn_graph_of(const long* batch, int i, int num_graphs) {
  const long g = batch ? batch[i] : 0;
  return g < 0 ? 0 : (g >= num_graphs ? num_graphs - 1 : g);
}

// Graph g's cell (the float32 tensor the search reads, widened) and its float64 inverse.
HN_HD inline void hn_load_cell(const float* cell32, const double* inv_cell, long g, double cell[9], double inv[9]) {
  for (int k = 0; k < 9; ++k) {
    cell[k] = (double)cell32[9 * g + k];
    inv[k] = inv_cell[9 * g + k];
  }
}

// Graph g's atoms [lo, hi), clamped to the n atoms there are.
HN_HD inline int hn_graph_lo(const int* graph_ptr, int g) { return graph_ptr[g] < 0 ? 0 : graph_ptr[g]; }
HN_HD inline int hn_graph_hi(const int* graph_ptr, int g, int n) { return graph_ptr[g + 1] > n ? n : graph_ptr[g + 1]; }

// A void step: the atom returns to where the step began (a driver that backs velocities up restores them beside this).
HN_HD inline void hn_restore_atom(int i, double* x, const double* x0, int* image, const int* image0, float* pos32) {
  for (int k = 0; k < 3; ++k) {
    const double xk = x0[3 * (size_t)i + k];
    x[3 * (size_t)i + k] = xk;
    image[3 * (size_t)i + k] = image0[3 * (size_t)i + k];
    pos32[3 * (size_t)i + k] = (float)xk;
  }
}

// Graph g's row of the log ring [log_steps, B, width] for `step`.
HN_HD inline double* hn_log_row(double* log, long step, long log_steps, int num_graphs, int g, int width) {
  return log + ((size_t)(step % log_steps) * num_graphs + g) * width;
}

// COUNT (1..6) per-graph sums over the atoms lo..hi-1 in the CANONICAL ORDER (the sums steer a trajectory, so their order is
// part of the contract): lane l of 256 adds the terms of atoms lo+l, lo+l+256, ... in ascending order starting from 0.0 --
// term(i, s) adds atom i's to the lane's partials s[0..COUNT) --; the 256 partials are then folded part[l] += part[l+m] for
// m = 128, 64, ..., 1; the sum at MAX_AT (-1: none) is a maximum and takes the same tree.  No atomics.  Results: part[k][0].
// On the device the 256 lanes of the workgroup call it together (`part` in LDS; it ends behind a barrier); on the host one
// call walks the lanes in turn.
template <int COUNT, int MAX_AT, class Term>
HN_HD inline void hn_canonical_sums(int lo, int hi, double (*part)[256], Term term) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
  const int first = threadIdx.x, last = first + 1;
#else
  const int first = 0, last = 256;
#endif
  for (int l = first; l < last; ++l) {
    double s[COUNT];
    for (int k = 0; k < COUNT; ++k) s[k] = 0.0;
    for (int i = lo + l; i < hi; i += 256) term(i, s);
    for (int k = 0; k < COUNT; ++k) part[k][l] = s[k];
  }
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
  for (int m = 128; m >= 1; m >>= 1) {
    for (int l = first; l < last && l < m; ++l)
      for (int k = 0; k < COUNT; ++k)
        part[k][l] = k == MAX_AT ? (part[k][l + m] > part[k][l] ? part[k][l + m] : part[k][l]) : part[k][l] + part[k][l + m];
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
  }
}

#endif  // HERMNET_RESIDENT_STEP_H
