// gfx950: Nose-Hoover chain NVT inside the replayed MD step (hermnet_amd/nhc.py: DeviceNHC).  hermnet_nhc_advance takes the
// place of hermnet_md_advance in front of the search and hermnet_nhc_finish that of hermnet_md_finish behind the force
// backward.  A chain reads one number of its graph, the kinetic energy, and acts through one factor on its velocities, so
// the per-atom text is md_step.h's and md_finish.h's with one multiplication added at either end of the step.
//
// The definition and the text of the launches are nhc_step.h's, shared with the host twins at the end of this file.
//   advance  1. nhc_open_kernel          one workgroup per graph: E_kin from v in the canonical order; lane 0: the chain's
//                                        backup, NHC(dt/2), scale[g][0]
//            2. nhc_advance_kernel       a lane per atom: md_advance_one with v scale[g][0] in front of the first kick
//   finish   1. md_finish_atoms_kernel<> unchanged: the second kick and ke_atom; a void step's restore; a prime's copy
//            2. nhc_close_kernel         one workgroup per graph: the canonical E_kin; lane 0: NHC(dt/2), scale[g][1], the log
//                                        row -- or, on a void step, the chain's restore
//            3. nhc_scale_kernel         a lane per atom: v scale[g][1] on a step that commits
//            4. md_commit_kernel<>       unchanged: the single writer of `state`
// Every kernel returns at once while a halt code is set; a prime leaves the chain alone.  Lane 0's chain is serial: a few
// dozen dependent mt_exp per half step, beside which a launch's own latency is the larger part.  Contraction is off for
// the whole file; no atomics.
#include <hip/hip_runtime.h>
#include "nhc_step.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void nhc_open_kernel(NhcAdvanceArgs a) {
  __shared__ double part[1][256];
  if (a.m.state[HN_STATE_CODE] != 0 || a.m.state[HN_STATE_MODE] != 0) return;
  const double e_kin = nhc_kinetic_sum(a, blockIdx.x, part);
  if (threadIdx.x == 0) nhc_graph_one(a.c, blockIdx.x, e_kin, 0);
}

__global__ __launch_bounds__(256) void nhc_advance_kernel(NhcAdvanceArgs a) {
  const long code = a.m.state[HN_STATE_CODE], mode = a.m.state[HN_STATE_MODE];
  if (code != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.m.n) nhc_advance_one(a, i, mode);
}

__global__ __launch_bounds__(256) void nhc_close_kernel(NhcFinishArgs a) {
  __shared__ double part[1][256];
  const long step = a.m.state[HN_STATE_STEP];
  if (a.m.state[HN_STATE_CODE] != 0 || a.m.state[HN_STATE_MODE] != 0) return;
  const long code = hn_step_code(a.m.energy, a.m.num_graphs, a.m.total, a.m.capacity);
  if (code != 0) {
    if (threadIdx.x == 0) nhc_restore_one(a.c, blockIdx.x);
    return;
  }
  const double e_kin = md_kinetic_sum(a.m, blockIdx.x, part);
  if (threadIdx.x == 0) nhc_close_one(a, step, blockIdx.x, e_kin);
}

__global__ __launch_bounds__(256) void nhc_scale_kernel(NhcFinishArgs a) {
  long step;
  if (!md_committed(a.m, &step)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.m.n) nhc_scale_one(a, i);
}

}  // namespace

extern "C" int hermnet_nhc_advance(int num_atoms, int num_graphs, int flags, double dt, double* x, double* v, double* x0,
                                   double* v0, int* image, int* image0, const float* f_prev, const double* kick,
                                   const long* batch, const float* cell, const double* inv_cell, float* pos32,
                                   const long* state, const int* graph_ptr, const double* half_mass, int chain, int order,
                                   int substeps, const double* delta, const double* kt, const double* dof_kt, const double* q,
                                   const double* inv_q, double* xi, double* v_xi, double* xi0, double* v_xi0, double* scale,
                                   void* stream) {
  const NhcAdvanceArgs a = {{num_atoms, num_graphs, flags, x, v, x0, v0, image, image0, f_prev, kick, nullptr, nullptr, batch,
                             cell, inv_cell, pos32, state, dt, 0},
                            graph_ptr, half_mass,
                            {chain, order, substeps, delta, kt, dof_kt, q, inv_q, xi, v_xi, xi0, v_xi0, scale}};
  if (!nhc_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nhc_open_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  if (num_atoms > 0) hipLaunchKernelGGL(nhc_advance_kernel, dim3((unsigned)((num_atoms + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_nhc_finish(int num_atoms, int num_graphs, const int* graph_ptr, const long* batch, const float* forces,
                                  const float* energy, const long* total, long capacity, double* x, double* v,
                                  const double* x0, const double* v0, int* image, const int* image0, float* f_prev,
                                  const double* kick, const double* half_mass, float* pos32, double* ke_atom, int chain,
                                  int order, int substeps, const double* delta, const double* kt, const double* dof_kt,
                                  const double* q, const double* inv_q, double* xi, double* v_xi, double* xi0, double* v_xi0,
                                  double* scale, double* log, long log_steps, long* state, void* stream) {
  const NhcFinishArgs a = {{num_atoms, num_graphs, x, v, x0, v0, image, image0, f_prev, forces, energy, total, capacity, kick,
                            half_mass, graph_ptr, pos32, ke_atom, log, log_steps, state},
                           batch,
                           {chain, order, substeps, delta, kt, dof_kt, q, inv_q, xi, v_xi, xi0, v_xi0, scale}};
  if (!nhc_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  const dim3 atoms((unsigned)((num_atoms + 255) / 256));
  if (num_atoms > 0) hipLaunchKernelGGL(md_finish_atoms_kernel<>, atoms, dim3(256), 0, s, a.m);
  hipLaunchKernelGGL(nhc_close_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  if (num_atoms > 0) hipLaunchKernelGGL(nhc_scale_kernel, atoms, dim3(256), 0, s, a);
  hipLaunchKernelGGL(md_commit_kernel<>, dim3(1), dim3(64), 0, s, a.m);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twins: the same functions in a CPU loop (all pointers HOST pointers) -----------------------------------------------
extern "C" int hermnet_host_nhc_advance(int num_atoms, int num_graphs, int flags, double dt, double* x_host, double* v_host,
                                        double* x0_host, double* v0_host, int* image_host, int* image0_host,
                                        const float* f_prev_host, const double* kick_host, const long* batch_host,
                                        const float* cell_host, const double* inv_cell_host, float* pos32_host,
                                        const long* state_host, const int* graph_ptr_host, const double* half_mass_host,
                                        int chain, int order, int substeps, const double* delta_host, const double* kt_host,
                                        const double* dof_kt_host, const double* q_host, const double* inv_q_host,
                                        double* xi_host, double* v_xi_host, double* xi0_host, double* v_xi0_host,
                                        double* scale_host) {
  const NhcAdvanceArgs a = {{num_atoms, num_graphs, flags, x_host, v_host, x0_host, v0_host, image_host, image0_host,
                             f_prev_host, kick_host, nullptr, nullptr, batch_host, cell_host, inv_cell_host, pos32_host,
                             state_host, dt, 0},
                            graph_ptr_host, half_mass_host,
                            {chain, order, substeps, delta_host, kt_host, dof_kt_host, q_host, inv_q_host, xi_host, v_xi_host,
                             xi0_host, v_xi0_host, scale_host}};
  if (!nhc_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  if (state_host[HN_STATE_CODE] != 0) return HN_OK;
  const long mode = state_host[HN_STATE_MODE];
  if (mode == 0) {
    double part[1][256];
    for (int g = 0; g < num_graphs; ++g) nhc_graph_one(a.c, g, nhc_kinetic_sum(a, g, part), 0);
  }
  for (int i = 0; i < num_atoms; ++i) nhc_advance_one(a, i, mode);
  return HN_OK;
}

// E_kin takes the canonical order of the device (hermnet_host_md_finish's sequential sum is not used).
extern "C" int hermnet_host_nhc_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const long* batch_host,
                                       const float* forces_host, const float* energy_host, const long* total_host,
                                       long capacity, double* x_host, double* v_host, const double* x0_host,
                                       const double* v0_host, int* image_host, const int* image0_host, float* f_prev_host,
                                       const double* kick_host, const double* half_mass_host, float* pos32_host,
                                       double* ke_atom_host, int chain, int order, int substeps, const double* delta_host,
                                       const double* kt_host, const double* dof_kt_host, const double* q_host,
                                       const double* inv_q_host, double* xi_host, double* v_xi_host, double* xi0_host,
                                       double* v_xi0_host, double* scale_host, double* log_host, long log_steps,
                                       long* state_host) {
  const NhcFinishArgs a = {{num_atoms, num_graphs, x_host, v_host, x0_host, v0_host, image_host, image0_host, f_prev_host,
                            forces_host, energy_host, total_host, capacity, kick_host, half_mass_host, graph_ptr_host,
                            pos32_host, ke_atom_host, log_host, log_steps, state_host},
                           batch_host,
                           {chain, order, substeps, delta_host, kt_host, dof_kt_host, q_host, inv_q_host, xi_host, v_xi_host,
                            xi0_host, v_xi0_host, scale_host}};
  if (!nhc_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  md_host_finish(
      a.m,
      [&](long step) {
        double part[1][256];
        for (int g = 0; g < num_graphs; ++g) nhc_close_one(a, step, g, md_kinetic_sum(a.m, g, part));
        for (int i = 0; i < num_atoms; ++i) nhc_scale_one(a, i);
      },
      [&](long step, long code, long mode) {
        if (code != 0 && mode == 0)
          for (int g = 0; g < num_graphs; ++g) nhc_restore_one(a.c, g);
        md_commit(a.m.state, step, code, mode);
      });
  return HN_OK;
}
