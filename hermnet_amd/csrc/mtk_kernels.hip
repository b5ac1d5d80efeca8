// gfx950: Nose-Hoover (MTK) barostat NPT inside the replayed MD step (hermnet_amd/mtk.py: DeviceMTK).  hermnet_mtk_advance
// takes the place of hermnet_md_advance in front of the search -- it moves the cell BEFORE the search reads it --, and
// hermnet_mtk_finish that of hermnet_md_finish_npt behind the force backward and the virial.
//
// The definition and the text of the launches are mtk_step.h's, shared with the host twins at the end of this file.
//   advance  1. mtk_open_kernel          one workgroup per graph: E_kin and sum m v_a v_a in the canonical order; lane 0: the
//                                        backups, NHC_baro, NHC_particles, the barostat's half kick, the twelve factors, the
//                                        flag, the new cell in its three forms
//            2. mtk_advance_kernel       a lane per atom: the scaled kick, the scaled drift, the wrap in the new cell, pos32
//   finish   1. mtk_finish_atoms_kernel  a lane per atom: the second scaled kick and ke_atom; a void step's restore; a prime's
//                                        copy (md_finish_one's structure)
//            2. mtk_close_kernel         one workgroup per graph: the canonical sums; lane 0: the barostat's second half kick,
//                                        NHC_particles, NHC_baro, the log row, w_prev -- or a void step's restores, or a
//                                        prime's w_prev; and e_code[g]
//            3. mtk_scale_kernel         a lane per atom: v scale[g][1] on a step that commits
//            4. md_commit_kernel<>       unchanged: the single writer of `state`; it reads e_code for the energies
// Every kernel returns at once while a halt code is set.  Lane 0's two chains are serial, as in nhc_kernels.hip.  Contraction
// is off for the whole file; no atomics; no workgroup reads what another of the same launch writes.
#include <hip/hip_runtime.h>
#include "mtk_step.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void mtk_open_kernel(MtkAdvanceArgs a) {
  __shared__ double part[4][256];
  if (a.m.state[HN_STATE_CODE] != 0 || a.m.state[HN_STATE_MODE] != 0) return;
  double e_kin, kaa[3];
  mtk_kinetic_sums(a.graph_ptr, a.m.n, blockIdx.x, a.m.v, a.half_mass, nullptr, part, &e_kin, kaa);
  if (threadIdx.x == 0) mtk_open_one(a, blockIdx.x, e_kin, kaa);
}

__global__ __launch_bounds__(256) void mtk_advance_kernel(MtkAdvanceArgs a) {
  const long code = a.m.state[HN_STATE_CODE], mode = a.m.state[HN_STATE_MODE];
  if (code != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.m.n) mtk_advance_one(a, i, mode);
}

__global__ __launch_bounds__(256) void mtk_finish_atoms_kernel(MtkFinishArgs a) {
  const long halted = a.m.state[HN_STATE_CODE], mode = a.m.state[HN_STATE_MODE];
  if (halted != 0) return;
  int extra;
  const long code = mtk_code(a, mode, &extra);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.m.n) mtk_finish_one(a, i, code, mode);
}

__global__ __launch_bounds__(256) void mtk_close_kernel(MtkFinishArgs a) {
  __shared__ double part[4][256];
  const long step = a.m.state[HN_STATE_STEP], mode = a.m.state[HN_STATE_MODE];
  if (a.m.state[HN_STATE_CODE] != 0) return;
  const int g = blockIdx.x;
  int extra;
  const long code = mtk_code(a, mode, &extra);
  if (threadIdx.x == 0) mtk_code_word(a, g, extra);
  if (mode != 0) {
    if (code == 0 && threadIdx.x == 0) mtk_prime_one(a, g);
    return;
  }
  if (code != 0) {
    if (threadIdx.x == 0) mtk_restore_one(a, g);
    return;
  }
  double e_kin, kaa[3];
  mtk_kinetic_sums(a.m.graph_ptr, a.m.n, g, a.m.v, a.m.half_mass, a.m.ke_atom, part, &e_kin, kaa);
  if (threadIdx.x == 0) mtk_close_one(a, step, g, e_kin, kaa);
}

__global__ __launch_bounds__(256) void mtk_scale_kernel(MtkFinishArgs a) {
  const long mode = a.m.state[HN_STATE_MODE];
  if (a.m.state[HN_STATE_CODE] != 0 || mode != 0) return;
  int extra;
  if (mtk_code(a, mode, &extra) != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.m.n) mtk_scale_one(a, i);
}

// The arguments as the two structs, device and host alike.
inline MtkBaro mtk_baro(int coupling, int mask, double max_strain, const double* par, const double* dof_kt_b, const double* q_b,
                        const double* inv_q_b, double* xi_b, double* v_xi_b, double* scale_b, double* v_cell, double* cell64,
                        float* cell32, double* inv_cell, float* w_prev, double* factors, double* backup, long* flag,
                        long* refused, float* e_code) {
  const MtkBaro b = {coupling, mask,  max_strain, par,      dof_kt_b, q_b,     inv_q_b, xi_b, v_xi_b,  scale_b,
                     v_cell,   cell64, cell32,     inv_cell, w_prev,   factors, backup,  flag, refused, e_code};
  return b;
}

}  // namespace

#define MTK_CHAIN_PARAMS                                                                                                       \
  int chain, int order, int substeps, const double *delta, const double *kt, const double *dof_kt, const double *q,           \
      const double *inv_q, double *xi, double *v_xi, double *xi0, double *v_xi0, double *scale
#define MTK_CHAIN_ARGS {chain, order, substeps, delta, kt, dof_kt, q, inv_q, xi, v_xi, xi0, v_xi0, scale}
#define MTK_BARO_PARAMS                                                                                                        \
  int coupling, int mask, double max_strain, const double *par, const double *dof_kt_b, const double *q_b,                    \
      const double *inv_q_b, double *xi_b, double *v_xi_b, double *scale_b, double *v_cell, double *cell64, float *cell32,    \
      double *inv_cell, float *w_prev, double *factors, double *backup, long *flag, long *refused, float *e_code
#define MTK_BARO_ARGS                                                                                                          \
  mtk_baro(coupling, mask, max_strain, par, dof_kt_b, q_b, inv_q_b, xi_b, v_xi_b, scale_b, v_cell, cell64, cell32, inv_cell,  \
           w_prev, factors, backup, flag, refused, e_code)

extern "C" int hermnet_mtk_advance(int num_atoms, int num_graphs, int flags, double dt, double* x, double* v, double* x0,
                                   double* v0, int* image, int* image0, const float* f_prev, const double* kick,
                                   const long* batch, float* pos32, const long* state, const int* graph_ptr,
                                   const double* half_mass, MTK_CHAIN_PARAMS, MTK_BARO_PARAMS, void* stream) {
  const MtkAdvanceArgs a = {{num_atoms, num_graphs, flags, x, v, x0, v0, image, image0, f_prev, kick, nullptr, nullptr, batch,
                             cell32, inv_cell, pos32, state, dt, 0},
                            graph_ptr, half_mass, MTK_CHAIN_ARGS, MTK_BARO_ARGS};
  if (!mtk_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mtk_open_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  if (num_atoms > 0) hipLaunchKernelGGL(mtk_advance_kernel, dim3((unsigned)((num_atoms + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_mtk_finish(int num_atoms, int num_graphs, const int* graph_ptr, const long* batch, const float* forces,
                                  const float* energy, const float* virial, const long* total, long capacity, double dt,
                                  double* x, double* v, const double* x0, const double* v0, int* image, const int* image0,
                                  float* f_prev, const double* kick, const double* half_mass, float* pos32, double* ke_atom,
                                  MTK_CHAIN_PARAMS, MTK_BARO_PARAMS, double* log, long log_steps, long* state, void* stream) {
  const MtkFinishArgs a = {{num_atoms, num_graphs, x, v, x0, v0, image, image0, f_prev, forces, energy, total, capacity, kick,
                            half_mass, graph_ptr, pos32, ke_atom, log, log_steps, state},
                           batch, virial, dt, MTK_CHAIN_ARGS, MTK_BARO_ARGS};
  if (!mtk_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  MdFinishArgs commit = a.m;
  commit.energy = e_code;              // energy[g], or NaN where the barostat voids the step: mtk_close_kernel
  hipStream_t s = (hipStream_t)stream;
  const dim3 atoms((unsigned)((num_atoms + 255) / 256));
  if (num_atoms > 0) hipLaunchKernelGGL(mtk_finish_atoms_kernel, atoms, dim3(256), 0, s, a);
  hipLaunchKernelGGL(mtk_close_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  if (num_atoms > 0) hipLaunchKernelGGL(mtk_scale_kernel, atoms, dim3(256), 0, s, a);
  hipLaunchKernelGGL(md_commit_kernel<>, dim3(1), dim3(64), 0, s, commit);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twins: the same functions in a CPU loop (all pointers HOST pointers) -----------------------------------------------
extern "C" int hermnet_host_mtk_advance(int num_atoms, int num_graphs, int flags, double dt, double* x, double* v, double* x0,
                                        double* v0, int* image, int* image0, const float* f_prev, const double* kick,
                                        const long* batch, float* pos32, const long* state, const int* graph_ptr,
                                        const double* half_mass, MTK_CHAIN_PARAMS, MTK_BARO_PARAMS) {
  const MtkAdvanceArgs a = {{num_atoms, num_graphs, flags, x, v, x0, v0, image, image0, f_prev, kick, nullptr, nullptr, batch,
                             cell32, inv_cell, pos32, state, dt, 0},
                            graph_ptr, half_mass, MTK_CHAIN_ARGS, MTK_BARO_ARGS};
  if (!mtk_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  if (state[HN_STATE_CODE] != 0) return HN_OK;
  const long mode = state[HN_STATE_MODE];
  if (mode == 0) {
    double part[4][256], e_kin, kaa[3];
    for (int g = 0; g < num_graphs; ++g) {
      mtk_kinetic_sums(graph_ptr, num_atoms, g, v, half_mass, nullptr, part, &e_kin, kaa);
      mtk_open_one(a, g, e_kin, kaa);
    }
  }
  for (int i = 0; i < num_atoms; ++i) mtk_advance_one(a, i, mode);
  return HN_OK;
}

extern "C" int hermnet_host_mtk_finish(int num_atoms, int num_graphs, const int* graph_ptr, const long* batch,
                                       const float* forces, const float* energy, const float* virial, const long* total,
                                       long capacity, double dt, double* x, double* v, const double* x0, const double* v0,
                                       int* image, const int* image0, float* f_prev, const double* kick,
                                       const double* half_mass, float* pos32, double* ke_atom, MTK_CHAIN_PARAMS,
                                       MTK_BARO_PARAMS, double* log, long log_steps, long* state) {
  const MtkFinishArgs a = {{num_atoms, num_graphs, x, v, x0, v0, image, image0, f_prev, forces, energy, total, capacity, kick,
                            half_mass, graph_ptr, pos32, ke_atom, log, log_steps, state},
                           batch, virial, dt, MTK_CHAIN_ARGS, MTK_BARO_ARGS};
  if (!mtk_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  const long step = state[HN_STATE_STEP], mode = state[HN_STATE_MODE];
  if (state[HN_STATE_CODE] != 0) return HN_OK;
  int extra;
  const long code = mtk_code(a, mode, &extra);
  for (int i = 0; i < num_atoms; ++i) mtk_finish_one(a, i, code, mode);
  double part[4][256], e_kin, kaa[3];
  for (int g = 0; g < num_graphs; ++g) {
    mtk_code_word(a, g, extra);
    if (mode != 0) {
      if (code == 0) mtk_prime_one(a, g);
    } else if (code != 0) {
      mtk_restore_one(a, g);
    } else {
      mtk_kinetic_sums(graph_ptr, num_atoms, g, v, half_mass, ke_atom, part, &e_kin, kaa);
      mtk_close_one(a, step, g, e_kin, kaa);
    }
  }
  if (code == 0 && mode == 0)
    for (int i = 0; i < num_atoms; ++i) mtk_scale_one(a, i);
  md_commit(state, step, code, mode);
  return HN_OK;
}
