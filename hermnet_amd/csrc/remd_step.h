// Temperature replica exchange at the end of a replayed Langevin step (remd_kernels.hip; hermnet_amd/remd.py: DeviceREMD):
// ONE text for the device kernels, the host twin (hermnet_host_remd_finish) and -- transcribed operation by operation --
// tests/remd_reference.py.  Contraction is off inside every function, as in md_step.h.
//
// One ladder of R = B replicas of one system.  rung[g] is the rung replica g holds, replica_at[r] its inverse; both start as
// the identity.  Replicas stay where they are in the batch: temperatures travel.  The committed step with 0-based index
// `step` ends with an attempt when (step + 1) % interval == 0; the attempt's index a = (step + 1) / interval - 1 picks the
// pairs (r, r + 1) with r % 2 == a % 2 and r + 1 < R, which are disjoint.  A void step, a prime and a parked or halted
// replay attempt nothing.  Pair r, with ga = replica_at[r], gb = replica_at[r + 1]:
//   delta = (beta[r] - beta[r + 1]) * ((double)E[ga] - (double)E[gb]);   accept iff delta >= 0.0 || log(u) < delta,
//   u = (md_u53(w0, w1) + 1) 2^-53 in (0, 1], w = Philox4x32-10 of the noise's key and the counter (r, step low, step high, 2)
// -- streams 0 and 1 are the atoms' noise --, so a decision is a function of (seed, step, r, energies, assignment) alone.
// beta = 1 / (kB T), up[r] = sqrt(T[r+1] / T[r]), down[r] = sqrt(T[r] / T[r+1]) and sigma_table [R, n_rep] come from the
// host in float64: the kernels only subtract, multiply, compare and take that one log.  On acceptance the two replicas swap
// rungs, every velocity of ga is multiplied by up[r], every one of gb by down[r], and each atom's sigma becomes its new
// rung's row of sigma_table.
//
// The three launches behind the per-atom finish (remd_decide, remd_apply_replica, remd_commit) keep resident_step.h's
// protocol: decide writes scratch alone (rung_new, vscale, outcome); apply reads it, one workgroup per replica, and writes
// that replica's atoms and log row; the commit alone writes what a kernel of the NEXT replay branches on -- rung, replica_at,
// the counters, state.  No atomics; no workgroup reads what another workgroup of the same launch writes.
#ifndef HERMNET_REMD_STEP_H
#define HERMNET_REMD_STEP_H

#include "md_finish.h"

namespace {

struct RemdArgs {
  MdFinishArgs m;
  int n_rep;                                       // atoms of one replica: n / num_graphs
  long interval;
  uint64_t seed;
  const double *beta;                              // [R]
  const double *up, *down;                         // [R-1]
  const double* sigma_table;                       // [R, n_rep]
  double* sigma;                                   // [N]: advance reads it; remd_apply_replica
  long *rung, *replica_at;                         // [B], [R]; the commit
  long* rung_new;                                  // scratch [B]: the rung behind this step's exchange; remd_decide
  double* vscale;                                  // scratch [B]: 1.0 where nothing changes; remd_decide
  long* outcome;                                   // scratch [R-1]: 0 not tried, 1 rejected, 2 accepted; remd_decide
  long *attempts, *accepts;                        // [R-1]; the commit
};

inline bool remd_args_ok(const RemdArgs& a) {
  if (!md_finish_args_ok(a.m) || a.m.num_graphs < 2 || a.interval < 1) return false;
  if (a.m.n % a.m.num_graphs != 0 || a.n_rep != a.m.n / a.m.num_graphs) return false;
  if (!a.beta || !a.up || !a.down || !a.rung || !a.replica_at || !a.rung_new || !a.vscale || !a.outcome || !a.attempts ||
      !a.accepts)
    return false;
  return a.m.n == 0 || (a.sigma_table && a.sigma);
}

// The attempt's index at the end of the committed step `step`, -1 where none is made.
HN_HD inline long remd_attempt_of(long step, long interval) {
  return (step + 1) % interval == 0 ? (step + 1) / interval - 1 : -1;
}

// The four words of pair r's uniform: the noise's key, counter (r, step low, step high, 2).
HN_HD inline void remd_words(uint64_t seed, uint64_t step, uint32_t r, uint32_t w[4]) {
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  const uint32_t ctr[4] = {r, (uint32_t)step, (uint32_t)(step >> 32), 2u};
  md_philox4x32_10(ctr, key, w);
}

HN_HD inline double remd_uniform(const uint32_t w[4]) {
#pragma clang fp contract(off)
  return (md_u53(w[0], w[1]) + 1.0) * (1.0 / 9007199254740992.0);
}

HN_HD inline double remd_delta(double beta_lo, double beta_hi, float e_lo, float e_hi) {
#pragma clang fp contract(off)
  return (beta_lo - beta_hi) * ((double)e_lo - (double)e_hi);
}

HN_HD inline int remd_accept(double delta, double u) { return delta >= 0.0 || log(u) < delta; }

// Launch 2, one workgroup (host: first = 0, stride = 1) of a committed step: every replica keeps its rung and its
// velocities unless a pair of this step's attempt says otherwise.  rung / replica_at are read as the step began.
HN_HD inline void remd_decide(const RemdArgs& a, long step, int first, int stride) {
  const int R = a.m.num_graphs;
  for (int g = first; g < R; g += stride) {
    a.rung_new[g] = a.rung[g];
    a.vscale[g] = 1.0;
  }
  for (int r = first; r + 1 < R; r += stride) a.outcome[r] = 0;
  hn_barrier();
  const long attempt = remd_attempt_of(step, a.interval);
  if (attempt < 0) return;
  for (int r = first; r + 1 < R; r += stride) {
    if ((r & 1) != (int)(attempt & 1)) continue;
    const long ga = a.replica_at[r], gb = a.replica_at[r + 1];
    if (ga < 0 || ga >= R || gb < 0 || gb >= R || ga == gb) continue;      // (a broken replica_at must not index out of bounds)
    uint32_t w[4];
    remd_words(a.seed, (uint64_t)step, (uint32_t)r, w);
    const double delta = remd_delta(a.beta[r], a.beta[r + 1], a.m.energy[ga], a.m.energy[gb]);
    const int yes = remd_accept(delta, remd_uniform(w));
    a.outcome[r] = yes ? 2 : 1;
    if (yes) {
      a.rung_new[ga] = r + 1;
      a.rung_new[gb] = r;
      a.vscale[ga] = a.up[r];
      a.vscale[gb] = a.down[r];
    }
  }
}

// Launch 3, replica g's workgroup (256 lanes; the host walks them) of a committed step: E_kin in the canonical order -- of
// ke_atom, that is, before any rescaling --, the log row (E_pot, E_kin, edges found, rung held during the step, rung held
// behind its exchange), and where the rung changed its atoms' v *= vscale[g], sigma = the new rung's row.
HN_HD inline void remd_apply_replica(const RemdArgs& a, long step, int g, double (*part)[256]) {
#pragma clang fp contract(off)
  const int lo = hn_graph_lo(a.m.graph_ptr, g), hi = hn_graph_hi(a.m.graph_ptr, g, a.m.n);
  const double e_kin = md_kinetic_sum(a.m, g, part);
  const long was = a.rung[g], now = a.rung_new[g];
  if (hn_lead_lane()) {
    double* row = hn_log_row(a.m.log, step, a.m.log_steps, a.m.num_graphs, g, 5);
    row[0] = (double)a.m.energy[g];
    row[1] = e_kin;
    row[2] = (double)a.m.total[0];
    row[3] = (double)was;
    row[4] = (double)now;
  }
  if (now == was || now < 0 || now >= a.m.num_graphs) return;
  const double s = a.vscale[g];
  const double* table = a.sigma_table + (size_t)now * a.n_rep;
#if defined(__HIP_DEVICE_COMPILE__)
  const int first = threadIdx.x, stride = 256;
#else
  const int first = 0, stride = 1;
#endif
  for (int i = lo + first; i < hi && i - lo < a.n_rep; i += stride) {
    for (int k = 0; k < 3; ++k) a.m.v[3 * (size_t)i + k] = a.m.v[3 * (size_t)i + k] * s;
    a.sigma[i] = table[i - lo];
  }
}

// Launch 4, one workgroup (host: first = 0, stride = 1): rung <- rung_new with its inverse and the counters on a committed
// step, then md_commit by the lead lane.  (Every lane has read `state` in front of hn_step_code's barrier by then.)
HN_HD inline void remd_commit(const RemdArgs& a, long step, long code, long mode, int first, int stride) {
  const int R = a.m.num_graphs;
  if (code == 0 && mode == 0) {
    for (int g = first; g < R; g += stride) {
      const long now = a.rung_new[g];
      a.rung[g] = now;
      if (now >= 0 && now < R) a.replica_at[now] = g;
    }
    for (int r = first; r + 1 < R; r += stride) {
      const long o = a.outcome[r];
      if (o != 0) a.attempts[r] = a.attempts[r] + 1;
      if (o == 2) a.accepts[r] = a.accepts[r] + 1;
    }
  }
  if (hn_lead_lane()) md_commit(a.m.state, step, code, mode);
}

}  // namespace

#endif  // HERMNET_REMD_STEP_H
