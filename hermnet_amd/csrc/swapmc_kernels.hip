// gfx950: species-swap Monte Carlo inside the replayed MD step (hermnet_amd/swapmc.py: DeviceSwapMD).  hermnet_swapmc_advance
// takes the place of hermnet_md_advance in front of the search and hermnet_swapmc_finish that of hermnet_md_finish behind the
// force backward.  A replay is a prime, a trial or an MD step, as `state` and mc = (t, left) say when it begins: an MD step
// and a prime run md_step.h's and md_finish.h's per-atom text unchanged; a trial exchanges one pair of coordinates per graph
// in the advance and keeps the new forces or exchanges the pair back in the finish.
//
// The definition and the text of the launches are swapmc_step.h's, shared with the host twins at the end of this file.
//   advance  1. swapmc_advance_kernel       a lane per atom (MD step, prime) or per graph (trial: the move)
//   finish   1. swapmc_decide_kernel        one workgroup, a lane per graph of a trial: pair, d, outcome (scratch)
//            2. swapmc_finish_atoms_kernel  a lane per atom: md_finish_one; on a trial f_prev of the accepted graphs, and a
//                                           lane per graph the exchange back of a rejected (void trial: every) pair
//            3. swapmc_log_kernel           one workgroup per graph of a committed MD step: E_kin, the MD log row
//            4. swapmc_commit_kernel        one workgroup: e_ref, counters, the swap_log row, then mc and state -- the single
//                                           writer
// Every kernel returns at once while a halt code is set.  Contraction is off for the whole file; no atomics.
#include <hip/hip_runtime.h>
#include "swapmc_step.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void swapmc_advance_kernel(SwapAdvanceArgs a) {
  const long step = a.m.state[HN_STATE_STEP], code = a.m.state[HN_STATE_CODE], mode = a.m.state[HN_STATE_MODE];
  if (code != 0) return;
  swapmc_advance_one(a, blockIdx.x * 256 + threadIdx.x, step, mode, a.s.mc[HN_MC_TRIALS], a.s.mc[HN_MC_LEFT]);
}

__global__ __launch_bounds__(256) void swapmc_decide_kernel(SwapFinishArgs a) {
  const long halted = a.m.state[HN_STATE_CODE], mode = a.m.state[HN_STATE_MODE];
  const long t = a.s.mc[HN_MC_TRIALS], left = a.s.mc[HN_MC_LEFT];
  if (halted != 0 || !swapmc_is_trial(mode, left)) return;
  const long code = hn_step_code(a.m.energy, a.m.num_graphs, a.m.total, a.m.capacity);
  swapmc_decide(a, t, code, threadIdx.x, 256);
}

__global__ __launch_bounds__(256) void swapmc_finish_atoms_kernel(SwapFinishArgs a) {
  const long halted = a.m.state[HN_STATE_CODE], mode = a.m.state[HN_STATE_MODE], left = a.s.mc[HN_MC_LEFT];
  if (halted != 0) return;
  const long code = hn_step_code(a.m.energy, a.m.num_graphs, a.m.total, a.m.capacity);
  swapmc_finish_one(a, blockIdx.x * 256 + threadIdx.x, code, mode, left);
}

__global__ __launch_bounds__(256) void swapmc_log_kernel(SwapFinishArgs a) {
  __shared__ double part[1][256];
  long step;
  if (a.s.mc[HN_MC_LEFT] > 0) return;
  if (!md_committed(a.m, &step)) return;
  const double e_kin = md_kinetic_sum(a.m, blockIdx.x, part);
  if (threadIdx.x == 0) md_log_row(a.m, step, blockIdx.x, e_kin);
}

__global__ __launch_bounds__(256) void swapmc_commit_kernel(SwapFinishArgs a) {
  const long step = a.m.state[HN_STATE_STEP], halted = a.m.state[HN_STATE_CODE], mode = a.m.state[HN_STATE_MODE];
  const long t = a.s.mc[HN_MC_TRIALS], left = a.s.mc[HN_MC_LEFT];
  if (halted != 0) return;
  const long code = hn_step_code(a.m.energy, a.m.num_graphs, a.m.total, a.m.capacity);
  swapmc_commit(a, step, code, mode, t, left, threadIdx.x, 256);
}

unsigned swapmc_atom_blocks(int num_atoms, int num_graphs) {
  const int lanes = num_atoms > num_graphs ? num_atoms : num_graphs;
  return (unsigned)((lanes + 255) / 256);
}

}  // namespace

extern "C" int hermnet_swapmc_advance(int num_atoms, int num_graphs, int flags, double dt, unsigned long seed, double* x, double* v,
                                      double* x0, double* v0, int* image, int* image0, const float* f_prev, const double* kick,
                                      const double* c1, const double* sigma, const long* batch, const float* cell,
                                      const double* inv_cell, float* pos32, const long* state, const long* mc,
                                      const int* graph_ptr, const int* cand, const int* cand_ptr, int num_species, int num_cand,
                                      void* stream) {
  const SwapAdvanceArgs a = {{num_atoms, num_graphs, flags, x, v, x0, v0, image, image0, f_prev, kick, c1, sigma, batch, cell,
                              inv_cell, pos32, state, dt, (uint64_t)seed},
                             {graph_ptr, cand, cand_ptr, num_species, num_cand, mc}};
  if (!swapmc_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  if (num_atoms == 0) return HN_OK;
  hipLaunchKernelGGL(swapmc_advance_kernel, dim3(swapmc_atom_blocks(num_atoms, num_graphs)), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_swapmc_finish(int num_atoms, int num_graphs, const int* graph_ptr, const long* batch, const float* forces,
                                     const float* energy, const long* total, long capacity, long swap_interval, long swaps,
                                     unsigned long seed, double* x, double* v, const double* x0, const double* v0, int* image,
                                     const int* image0, float* f_prev, const double* kick, const double* half_mass, float* pos32,
                                     double* ke_atom, const double* beta, double* e_ref, long* mc, const int* cand,
                                     const int* cand_ptr, int num_species, int num_cand, int* pair, double* dval, long* outcome,
                                     long* attempts, long* accepts, double* swap_log, long swap_rows, double* log, long log_steps,
                                     long* state, void* stream) {
  const SwapFinishArgs a = {{num_atoms, num_graphs, x, v, x0, v0, image, image0, f_prev, forces, energy, total, capacity, kick,
                             half_mass, graph_ptr, pos32, ke_atom, log, log_steps, state},
                            {graph_ptr, cand, cand_ptr, num_species, num_cand, mc},
                            batch, swap_interval, swaps, (uint64_t)seed, beta, e_ref, mc, pair, dval, outcome, attempts, accepts,
                            swap_log, swap_rows};
  if (!swapmc_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(swapmc_decide_kernel, dim3(1), dim3(256), 0, s, a);
  hipLaunchKernelGGL(swapmc_finish_atoms_kernel, dim3(swapmc_atom_blocks(num_atoms, num_graphs)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(swapmc_log_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(swapmc_commit_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twins: the same functions in a CPU loop (all pointers HOST pointers) -----------------------------------------------
extern "C" int hermnet_host_swapmc_advance(int num_atoms, int num_graphs, int flags, double dt, unsigned long seed, double* x_host,
                                           double* v_host, double* x0_host, double* v0_host, int* image_host, int* image0_host,
                                           const float* f_prev_host, const double* kick_host, const double* c1_host,
                                           const double* sigma_host, const long* batch_host, const float* cell_host,
                                           const double* inv_cell_host, float* pos32_host, const long* state_host,
                                           const long* mc_host, const int* graph_ptr_host, const int* cand_host,
                                           const int* cand_ptr_host, int num_species, int num_cand) {
  const SwapAdvanceArgs a = {{num_atoms, num_graphs, flags, x_host, v_host, x0_host, v0_host, image_host, image0_host, f_prev_host,
                              kick_host, c1_host, sigma_host, batch_host, cell_host, inv_cell_host, pos32_host, state_host, dt,
                              (uint64_t)seed},
                             {graph_ptr_host, cand_host, cand_ptr_host, num_species, num_cand, mc_host}};
  if (!swapmc_advance_args_ok(a) || !swapmc_host_tables_ok(a.s, num_atoms, num_graphs)) return HN_ERR_BAD_ARG;
  if (num_atoms == 0 || state_host[HN_STATE_CODE] != 0) return HN_OK;
  const int lanes = num_atoms > num_graphs ? num_atoms : num_graphs;
  for (int idx = 0; idx < lanes; ++idx)
    swapmc_advance_one(a, idx, state_host[HN_STATE_STEP], state_host[HN_STATE_MODE], mc_host[HN_MC_TRIALS], mc_host[HN_MC_LEFT]);
  return HN_OK;
}

// E_kin takes the canonical order of the device (hermnet_host_md_finish's sequential sum is not used).
extern "C" int hermnet_host_swapmc_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const long* batch_host,
                                          const float* forces_host, const float* energy_host, const long* total_host,
                                          long capacity, long swap_interval, long swaps, unsigned long seed, double* x_host,
                                          double* v_host, const double* x0_host, const double* v0_host, int* image_host,
                                          const int* image0_host, float* f_prev_host, const double* kick_host,
                                          const double* half_mass_host, float* pos32_host, double* ke_atom_host,
                                          const double* beta_host, double* e_ref_host, long* mc_host, const int* cand_host,
                                          const int* cand_ptr_host, int num_species, int num_cand, int* pair_host,
                                          double* dval_host, long* outcome_host, long* attempts_host, long* accepts_host,
                                          double* swap_log_host, long swap_rows, double* log_host, long log_steps,
                                          long* state_host) {
  const SwapFinishArgs a = {{num_atoms, num_graphs, x_host, v_host, x0_host, v0_host, image_host, image0_host, f_prev_host,
                             forces_host, energy_host, total_host, capacity, kick_host, half_mass_host, graph_ptr_host, pos32_host,
                             ke_atom_host, log_host, log_steps, state_host},
                            {graph_ptr_host, cand_host, cand_ptr_host, num_species, num_cand, mc_host},
                            batch_host, swap_interval, swaps, (uint64_t)seed, beta_host, e_ref_host, mc_host, pair_host, dval_host,
                            outcome_host, attempts_host, accepts_host, swap_log_host, swap_rows};
  if (!swapmc_finish_args_ok(a) || !swapmc_host_tables_ok(a.s, num_atoms, num_graphs)) return HN_ERR_BAD_ARG;
  const long step = state_host[HN_STATE_STEP], mode = state_host[HN_STATE_MODE];
  const long t = mc_host[HN_MC_TRIALS], left = mc_host[HN_MC_LEFT];
  if (state_host[HN_STATE_CODE] != 0) return HN_OK;
  const long code = hn_step_code(energy_host, num_graphs, total_host, capacity);
  if (swapmc_is_trial(mode, left)) swapmc_decide(a, t, code, 0, 1);
  const int lanes = num_atoms > num_graphs ? num_atoms : num_graphs;
  for (int idx = 0; idx < lanes; ++idx) swapmc_finish_one(a, idx, code, mode, left);
  if (code == 0 && mode == 0 && left <= 0) {
    double part[1][256];
    for (int g = 0; g < num_graphs; ++g) md_log_row(a.m, step, g, md_kinetic_sum(a.m, g, part));
  }
  swapmc_commit(a, step, code, mode, t, left, 0, 1);
  return HN_OK;
}
