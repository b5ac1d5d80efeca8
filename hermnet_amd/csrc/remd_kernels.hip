// gfx950: temperature replica exchange inside the replayed MD step (hermnet_amd/remd.py: DeviceREMD).  The front of the
// replay is DeviceMD's, unchanged: hermnet_md_advance reads sigma[i] as it always did.  hermnet_remd_finish takes the place
// of hermnet_md_finish behind the force backward: the Langevin step's second half and, at every exchange_interval-th
// committed step, one attempt of the ladder -- the decisions, the velocity rescaling and the new thermostat coefficients
// never leave the device.
//
// The arithmetic and the text of the launches are remd_step.h's, around md_finish.h's skeleton (the per-atom half and its
// kernel, md_committed, E_kin), shared with the host twin at the end of this file.  The replicas are COUPLED -- a decision
// needs two replicas' energies -- so, as in neb_kernels.hip, what one workgroup needs of another's work it reads in the NEXT
// launch:
//   1. md_finish_atoms_kernel     md_finish.h's, unchanged: second kick, ke_atom; restore on a void step; a prime's copy
//   2. remd_decide_kernel         one workgroup, a lane per pair: rung_new, vscale, outcome (scratch) from rung / replica_at
//   3. remd_apply_kernel          one workgroup per replica: E_kin, the log row; where its rung changed, v and sigma
//   4. remd_commit_kernel         one workgroup: rung, replica_at, attempts, accepts, then state -- the single writer
// Contraction is off for the whole file; no atomics.
#include <hip/hip_runtime.h>
#include "remd_step.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void remd_decide_kernel(RemdArgs a) {
  long step;
  if (!md_committed(a.m, &step)) return;
  remd_decide(a, step, threadIdx.x, 256);
}

__global__ __launch_bounds__(256) void remd_apply_kernel(RemdArgs a) {
  __shared__ double part[1][256];
  long step;
  if (!md_committed(a.m, &step)) return;
  remd_apply_replica(a, step, blockIdx.x, part);
}

__global__ __launch_bounds__(256) void remd_commit_kernel(RemdArgs a) {
  const long step = a.m.state[HN_STATE_STEP], halted = a.m.state[HN_STATE_CODE], mode = a.m.state[HN_STATE_MODE];
  if (halted != 0) return;
  const long code = hn_step_code(a.m.energy, a.m.num_graphs, a.m.total, a.m.capacity);
  remd_commit(a, step, code, mode, threadIdx.x, 256);
}

// What the host twin can check and the device entry point cannot (its pointers are the device's): the replicas tile the
// atoms in equal ranges, rung is a permutation of the rungs and replica_at its inverse.
bool remd_host_layout_ok(const RemdArgs& a) {
  const int R = a.m.num_graphs;
  for (int g = 0; g <= R; ++g)
    if (a.m.graph_ptr[g] != g * a.n_rep) return false;
  for (int g = 0; g < R; ++g)
    if (a.rung[g] < 0 || a.rung[g] >= R || a.replica_at[a.rung[g]] != g) return false;
  return true;
}

}  // namespace

extern "C" int hermnet_remd_finish(int num_atoms, int num_graphs, const int* graph_ptr, const float* forces, const float* energy,
                                   const long* total, long capacity, long exchange_interval, unsigned long seed, double* x,
                                   double* v, const double* x0, const double* v0, int* image, const int* image0, float* f_prev,
                                   const double* kick, const double* half_mass, float* pos32, double* ke_atom,
                                   const double* beta, const double* up, const double* down, const double* sigma_table,
                                   double* sigma, long* rung, long* replica_at, long* rung_new, double* vscale, long* outcome,
                                   long* attempts, long* accepts, double* log, long log_steps, long* state, void* stream) {
  const RemdArgs a = {{num_atoms, num_graphs, x, v, x0, v0, image, image0, f_prev, forces, energy, total, capacity, kick,
                       half_mass, graph_ptr, pos32, ke_atom, log, log_steps, state},
                      num_graphs > 0 ? num_atoms / num_graphs : 0, exchange_interval, (uint64_t)seed, beta, up, down, sigma_table,
                      sigma, rung, replica_at, rung_new, vscale, outcome, attempts, accepts};
  if (!remd_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (num_atoms > 0)
    hipLaunchKernelGGL(md_finish_atoms_kernel<>, dim3((unsigned)((num_atoms + 255) / 256)), dim3(256), 0, s, a.m);
  hipLaunchKernelGGL(remd_decide_kernel, dim3(1), dim3(256), 0, s, a);
  hipLaunchKernelGGL(remd_apply_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(remd_commit_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twin: the same functions in a CPU loop (all pointers HOST pointers) -----------------------------------------------
// E_kin takes the canonical order of the device (hermnet_host_md_finish's sequential sum is not used).
extern "C" int hermnet_host_remd_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const float* forces_host,
                                        const float* energy_host, const long* total_host, long capacity, long exchange_interval,
                                        unsigned long seed, double* x_host, double* v_host, const double* x0_host,
                                        const double* v0_host, int* image_host, const int* image0_host, float* f_prev_host,
                                        const double* kick_host, const double* half_mass_host, float* pos32_host,
                                        double* ke_atom_host, const double* beta_host, const double* up_host,
                                        const double* down_host, const double* sigma_table_host, double* sigma_host,
                                        long* rung_host, long* replica_at_host, long* rung_new_host, double* vscale_host,
                                        long* outcome_host, long* attempts_host, long* accepts_host, double* log_host,
                                        long log_steps, long* state_host) {
  const RemdArgs a = {{num_atoms, num_graphs, x_host, v_host, x0_host, v0_host, image_host, image0_host, f_prev_host, forces_host,
                       energy_host, total_host, capacity, kick_host, half_mass_host, graph_ptr_host, pos32_host, ke_atom_host,
                       log_host, log_steps, state_host},
                      num_graphs > 0 ? num_atoms / num_graphs : 0, exchange_interval, (uint64_t)seed, beta_host, up_host,
                      down_host, sigma_table_host, sigma_host, rung_host, replica_at_host, rung_new_host, vscale_host,
                      outcome_host, attempts_host, accepts_host};
  if (!remd_args_ok(a) || !remd_host_layout_ok(a)) return HN_ERR_BAD_ARG;
  md_host_finish(
      a.m,
      [&](long step) {
        double part[1][256];
        remd_decide(a, step, 0, 1);
        for (int g = 0; g < num_graphs; ++g) remd_apply_replica(a, step, g, part);
      },
      [&](long step, long code, long mode) { remd_commit(a, step, code, mode, 0, 1); });
  return HN_OK;
}
