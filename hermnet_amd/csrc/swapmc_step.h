// Species-swap Monte Carlo between the steps of a replayed MD run (swapmc_kernels.hip; hermnet_amd/swapmc.py: DeviceSwapMD):
// ONE text for the device kernels, the host twins (hermnet_host_swapmc_advance / _finish) and -- transcribed operation by
// operation -- tests/swapmc_reference.py.  Contraction is off inside every function, as in md_step.h.
//
// In a fixed composition, exchanging the species of atoms i and j is exchanging their coordinates: z, masses, velocities and
// every per-atom table stay with their rows, and the captured step is untouched.  The kernels branch on `state` and on
// mc [2] int64 = (t, left): t trials committed so far, left trials still due in this block.  A replay is a PRIME where
// state[MODE] == 1, else a TRIAL where left > 0, else an MD step (md_step.h / md_finish.h, unchanged).  The commit sets
// left = swaps behind the committed MD step that makes step % interval == 0, and left -= 1, t += 1 behind a committed trial;
// a prime leaves both alone, so a block that a halt interrupted continues where it stopped.
//
// Trial t of graph g: w = Philox4x32-10 of the noise's key and the counter (g, t low, t high, 3) -- streams 0 and 1 are the
// atoms' noise, stream 2 is the replica exchange's.  The candidates are the atoms of finite mass, listed per graph in
// cand (sorted by species, then atom) with cand_ptr [B, S+1] the absolute offsets of each species' range.  With m the
// graph's candidates and mulhi(w, m) = ((uint64)w * m) >> 32:  i = cand[ptr[0] + mulhi(w0, m)], s its species, m_s its count,
// k = mulhi(w1, m - m_s), q = k < ptr[s] - ptr[0] ? k : k + m_s, j = cand[ptr[0] + q] -- a uniform first atom and a uniform
// partner among the candidates of every OTHER species (the multiply-shift is biased by at most m / 2^32).  m - m_s == 0 (one
// species, or no candidate at all): the graph is NOT TRIED.  The proposal reads no coordinate, so it is symmetric.
//
// The advance of a trial exchanges x and image of (i, j) and writes their two pos32 rows; nothing else moves, and nothing is
// backed up: exchanging twice is the identity, bit for bit.  Behind the force backward
//   d = (double)energy[g] - e_ref[g];  delta = -beta[g] * d;  accept iff delta >= 0.0 || log(u) < delta  (remd_accept),
//   u = (md_u53(w2, w3) + 1) 2^-53,
// with beta = 1 / (kB T) from the host and e_ref [B] the energy of the current configuration (written by a prime, by every
// committed MD step and by an accepted trial of that graph).  Accepted: f_prev of g's atoms and e_ref[g] take the new
// evaluation.  Rejected: (i, j) are exchanged back.  Halt code != 0: the trial is VOID -- every graph is exchanged back, the
// halt is recorded, t and left stay, so the resumed run repeats the same trial.  A trial kicks nobody, draws no atom's
// noise, writes no MD log row and does not advance state[STEP].
//
// The launches keep resident_step.h's protocol: swapmc_decide writes scratch alone (pair, dval, outcome); the per-atom
// launch reads it; the commit alone writes what a kernel of the NEXT replay branches on -- e_ref, the counters, the
// swap_log row, mc, state.  No atomics; no workgroup reads what another workgroup of the same launch writes.
#ifndef HERMNET_SWAPMC_STEP_H
#define HERMNET_SWAPMC_STEP_H

#include "remd_step.h"

#define HN_MC_TRIALS 0
#define HN_MC_LEFT 1

namespace {

// The candidate tables and what bounds them (both entry points carry one).
struct SwapTables {
  const int* graph_ptr;                            // [B+1]
  const int* cand;                                 // [num_cand]
  const int* cand_ptr;                             // [B, S+1] absolute offsets into cand
  int num_species, num_cand;
  const long* mc;                                  // (t, left): read here, written by the commit
};

struct SwapAdvanceArgs {
  MdAdvanceArgs m;
  SwapTables s;
};

struct SwapFinishArgs {
  MdFinishArgs m;
  SwapTables s;
  const long* batch;                               // [N] or NULL: one graph
  long interval, swaps;
  uint64_t seed;
  const double* beta;                              // [B]
  double* e_ref;                                   // [B]; the commit
  long* mc_out;                                    // = s.mc; the commit
  int* pair;                                       // scratch [B,2]: (i, j), (-1, -1) where not tried; swapmc_decide
  double* dval;                                    // scratch [B]: d; swapmc_decide
  long* outcome;                                   // scratch [B]: 0 not tried, 1 rejected (or void), 2 accepted; swapmc_decide
  long *attempts, *accepts;                        // [B]; the commit
  double* swap_log;                                // [swap_rows, B, 4] = (i, j, d, outcome) at row t % swap_rows; the commit
  long swap_rows;
};

inline bool swapmc_tables_ok(const SwapTables& s) {
  return s.graph_ptr && s.cand_ptr && s.mc && s.num_species >= 1 && s.num_cand >= 0 && (s.num_cand == 0 || s.cand);
}

inline bool swapmc_advance_args_ok(const SwapAdvanceArgs& a) { return md_advance_args_ok(a.m) && swapmc_tables_ok(a.s); }

inline bool swapmc_finish_args_ok(const SwapFinishArgs& a) {
  if (!md_finish_args_ok(a.m) || !swapmc_tables_ok(a.s) || a.interval < 1 || a.swaps < 0 || a.swap_rows < 1) return false;
  return a.beta && a.e_ref && a.mc_out && a.pair && a.dval && a.outcome && a.attempts && a.accepts && a.swap_log;
}

// What the host twins can check and the device entry points cannot (their pointers are the device's): every graph's
// species ranges ascend inside cand, and every candidate is an atom of its graph, ascending within its species.
inline bool swapmc_host_tables_ok(const SwapTables& s, int n, int num_graphs) {
  if (s.mc[HN_MC_TRIALS] < 0 || s.mc[HN_MC_LEFT] < 0) return false;
  for (int g = 0; g < num_graphs; ++g) {
    const int* ptr = s.cand_ptr + (size_t)g * (s.num_species + 1);
    const int lo = s.graph_ptr[g], hi = s.graph_ptr[g + 1];
    if (lo < 0 || hi < lo || hi > n || ptr[0] < 0 || ptr[s.num_species] > s.num_cand) return false;
    for (int k = 0; k < s.num_species; ++k) {
      if (ptr[k + 1] < ptr[k]) return false;
      for (int c = ptr[k]; c < ptr[k + 1]; ++c)
        if (s.cand[c] < lo || s.cand[c] >= hi || (c > ptr[k] && s.cand[c] <= s.cand[c - 1])) return false;
    }
  }
  return true;
}

HN_HD inline uint32_t swapmc_mulhi(uint32_t w, uint32_t m) { return (uint32_t)(((uint64_t)w * m) >> 32); }

// The four words of graph g's trial t: the noise's key, counter (g, t low, t high, 3).
HN_HD inline void swapmc_words(uint64_t seed, uint64_t t, uint32_t g, uint32_t w[4]) {
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  const uint32_t ctr[4] = {g, (uint32_t)t, (uint32_t)(t >> 32), 3u};
  md_philox4x32_10(ctr, key, w);
}

// The pair of graph g from the words w; false: not tried.  (Broken tables must not index out of bounds: a range outside
// cand or a candidate outside the graph's atoms is "not tried" too.)
HN_HD inline bool swapmc_pick(const SwapTables& s, int n, int g, const uint32_t w[4], int* i, int* j) {
  const int S = s.num_species;
  const int* ptr = s.cand_ptr + (size_t)g * (S + 1);
  const int base = ptr[0], m = ptr[S] - base;
  if (base < 0 || m <= 0 || ptr[S] > s.num_cand) return false;
  const int at = (int)swapmc_mulhi(w[0], (uint32_t)m);
  int sp = 0;
  while (sp + 1 < S && ptr[sp + 1] - base <= at) ++sp;
  const int before = ptr[sp] - base, m_s = ptr[sp + 1] - ptr[sp], rest = m - m_s;
  if (before < 0 || before > at || m_s <= 0 || rest <= 0) return false;
  const int k = (int)swapmc_mulhi(w[1], (uint32_t)rest);
  const int q = k < before ? k : k + m_s;
  const int a = s.cand[base + at], b = s.cand[base + q];
  const int lo = hn_graph_lo(s.graph_ptr, g), hi = hn_graph_hi(s.graph_ptr, g, n);
  if (a < lo || a >= hi || b < lo || b >= hi || a == b) return false;
  *i = a;
  *j = b;
  return true;
}

// Atoms i and j exchange coordinates and images; their two pos32 rows follow.  Twice is the identity.
HN_HD inline void swapmc_exchange(int i, int j, double* x, int* image, float* pos32) {
  for (int k = 0; k < 3; ++k) {
    const double xi = x[3 * (size_t)i + k], xj = x[3 * (size_t)j + k];
    const int ni = image[3 * (size_t)i + k], nj = image[3 * (size_t)j + k];
    x[3 * (size_t)i + k] = xj;
    x[3 * (size_t)j + k] = xi;
    image[3 * (size_t)i + k] = nj;
    image[3 * (size_t)j + k] = ni;
    pos32[3 * (size_t)i + k] = (float)xj;
    pos32[3 * (size_t)j + k] = (float)xi;
  }
}

// True where this replay is a trial (the words as the replay began).
HN_HD inline bool swapmc_is_trial(long mode, long left) { return mode == 0 && left > 0; }

// ---- the advance: one lane per atom (an MD step, a prime: md_advance_one) or per graph (a trial: the move) ----------------
HN_HD inline void swapmc_advance_one(const SwapAdvanceArgs& a, int idx, long step, long mode, long t, long left) {
  if (!swapmc_is_trial(mode, left)) {
    if (idx < a.m.n) md_advance_one(a.m, idx, step, mode);
    return;
  }
  if (idx >= a.m.num_graphs) return;
  uint32_t w[4];
  int i, j;
  swapmc_words(a.m.seed, (uint64_t)t, (uint32_t)idx, w);
  if (swapmc_pick(a.s, a.m.n, idx, w, &i, &j)) swapmc_exchange(i, j, a.m.x, a.m.image, a.m.pos32);
}

// ---- the finish of a trial ---------------------------------------------------------------------------------------------------
// Launch 1, one workgroup (host: first = 0, stride = 1): graph g's pair again, and its decision.  A void trial (code != 0)
// decides nothing: every pair is marked for the exchange back.
HN_HD inline void swapmc_decide(const SwapFinishArgs& a, long t, long code, int first, int stride) {
#pragma clang fp contract(off)
  for (int g = first; g < a.m.num_graphs; g += stride) {
    uint32_t w[4];
    int i = -1, j = -1;
    swapmc_words(a.seed, (uint64_t)t, (uint32_t)g, w);
    const bool tried = swapmc_pick(a.s, a.m.n, g, w, &i, &j);
    double d = 0.0;
    long o = tried ? 1 : 0;
    if (tried && code == 0) {
      d = (double)a.m.energy[g] - a.e_ref[g];
      const double delta = -a.beta[g] * d;
      o = remd_accept(delta, remd_uniform(w + 2)) ? 2 : 1;
    }
    a.pair[2 * g] = tried ? i : -1;
    a.pair[2 * g + 1] = tried ? j : -1;
    a.dval[g] = d;
    a.outcome[g] = o;
  }
}

// Launch 2, lane g < B: a rejected pair, and on a void trial every pair, goes back.
HN_HD inline void swapmc_undo_graph(const SwapFinishArgs& a, int g, long code) {
  const int i = a.pair[2 * g], j = a.pair[2 * g + 1];
  if (i < 0 || j < 0 || i >= a.m.n || j >= a.m.n) return;
  if (code != 0 || a.outcome[g] == 1) swapmc_exchange(i, j, a.m.x, a.m.image, a.m.pos32);
}

// Launch 2, lane i < N of a trial that is not void: the atoms of an accepted graph take the new forces.
HN_HD inline void swapmc_keep_atom(const SwapFinishArgs& a, int i) {
  if (a.outcome[hn_graph_of(a.batch, i, a.m.num_graphs)] != 2) return;
  for (int k = 0; k < 3; ++k) a.m.f_prev[3 * (size_t)i + k] = a.m.forces[3 * (size_t)i + k];
}

// The per-atom launch of every kind of replay, lane idx of max(N, B).
HN_HD inline void swapmc_finish_one(const SwapFinishArgs& a, int idx, long code, long mode, long left) {
  if (!swapmc_is_trial(mode, left)) {
    if (idx < a.m.n) md_finish_one(a.m, idx, code, mode);
    return;
  }
  if (idx < a.m.num_graphs) swapmc_undo_graph(a, idx, code);
  if (idx < a.m.n && code == 0) swapmc_keep_atom(a, idx);
}

// The last launch, one workgroup (host: first = 0, stride = 1): the single writer of e_ref, the counters, the swap_log row,
// mc and state.  step, mode, t, left: the words as the replay began (every lane has read them in front of hn_step_code's
// barrier).
HN_HD inline void swapmc_commit(const SwapFinishArgs& a, long step, long code, long mode, long t, long left, int first,
                                int stride) {
  const bool trial = swapmc_is_trial(mode, left);
  const int B = a.m.num_graphs;
  if (code == 0) {
    for (int g = first; g < B; g += stride) {
      if (!trial) {
        a.e_ref[g] = (double)a.m.energy[g];
        continue;
      }
      const long o = a.outcome[g];
      const long slot = t % a.swap_rows;           // (a broken t must not write in front of the ring)
      double* row = a.swap_log + ((size_t)(slot < 0 ? 0 : slot) * B + g) * 4;
      row[0] = (double)a.pair[2 * g];
      row[1] = (double)a.pair[2 * g + 1];
      row[2] = a.dval[g];
      row[3] = (double)o;
      if (o != 0) a.attempts[g] = a.attempts[g] + 1;
      if (o == 2) {
        a.accepts[g] = a.accepts[g] + 1;
        a.e_ref[g] = (double)a.m.energy[g];
      }
    }
  }
  if (!hn_lead_lane()) return;
  if (trial) {
    if (!hn_commit_halt(a.m.state, step, code)) {
      a.mc_out[HN_MC_TRIALS] = t + 1;
      a.mc_out[HN_MC_LEFT] = left - 1;
    }
    return;
  }
  md_commit(a.m.state, step, code, mode);
  if (code == 0 && mode == 0 && (step + 1) % a.interval == 0) a.mc_out[HN_MC_LEFT] = a.swaps;
}

}  // namespace

#endif  // HERMNET_SWAPMC_STEP_H
