// gfx950: ring-polymer path-integral MD inside the replayed MD step (hermnet_amd/pimd.py: DevicePIMD).  The mirror image of
// remd_kernels.hip: there the advance stayed and the finish was replaced; here hermnet_pimd_advance takes the place of
// hermnet_md_advance in front of the search -- the beads of a ring are coupled by harmonic springs, which it integrates
// exactly in normal modes --, and hermnet_pimd_finish is hermnet_md_finish with a wider log row: md_finish.h's per-atom half
// and commit, kernels included (md_finish_atoms_kernel, md_commit_kernel), around a per-bead kernel that takes E_kin, the
// spring energy and the centroid-virial sum in the canonical order.  A replay has as many launches as DeviceMD's: one in
// front, three behind.
//
// The arithmetic, the phases of a tile and the LDS layout are pimd_step.h's, shared with the host twins at the end of this
// file.  One workgroup of 256 lanes holds a tile of 256 / P atoms x P lanes; the beads of an atom never leave their tile, so
// no workgroup reads what another of the same launch writes.  Contraction is off for the whole file; no atomics.
#include <hip/hip_runtime.h>
#include "pimd_step.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void pimd_advance_kernel(PimdAdvanceArgs a) {
  __shared__ double sb[6][256], sm[6][256];
  const long step = a.state[HN_STATE_STEP], code = a.state[HN_STATE_CODE], mode = a.state[HN_STATE_MODE];
  if (code != 0) return;
  const int first = blockIdx.x * pimd_tile_atoms(a.beads), l = threadIdx.x;
  if (mode != 0) {
    pimd_prime_lane(a, first, l);
    return;
  }
  pimd_bead_in(a, first, l, sb);
  __syncthreads();
  pimd_mode(a, step, first, l, sb, sm);
  __syncthreads();
  pimd_bead_out(a, first, l, sm, sb);
  __syncthreads();
  pimd_centroid(a, first, l, sb, sm);          // (sm is free again: n of the atom in its rows 0..2)
  __syncthreads();
  pimd_store(a, first, l, sb, sm);
}

__global__ __launch_bounds__(256) void pimd_log_kernel(PimdFinishArgs a) {
  __shared__ double part[3][256];
  long step;
  if (!md_committed(a.m, &step)) return;
  pimd_log_bead(a, step, blockIdx.x, part);
}

// What the host twins can check and the device entry points cannot: the beads tile the atoms in equal ranges.
bool pimd_host_layout_ok(const int* graph_ptr, int beads, int n_rep) {
  for (int g = 0; g <= beads; ++g)
    if (graph_ptr[g] != g * n_rep) return false;
  return true;
}

}  // namespace

extern "C" int hermnet_pimd_advance(int num_atoms, int num_graphs, int flags, unsigned long seed, double inv_beads, double* x,
                                    double* v, double* x0, double* v0, int* image, int* image0, const float* f_prev,
                                    const double* kick, const double* cmat, const double* cs, const double* sw, const double* ws,
                                    const double* c1, const double* sigma, const float* cell, const double* inv_cell,
                                    float* pos32, double* centroid, const long* state, void* stream) {
  const PimdAdvanceArgs a = {num_atoms, num_graphs, num_graphs > 0 ? num_atoms / num_graphs : 0, flags, x, v, x0, v0, image, image0,
                             f_prev, kick, cmat, cs, sw, ws, c1, sigma, inv_beads, cell, inv_cell, pos32, centroid, state,
                             (uint64_t)seed};
  if (!pimd_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  if (num_atoms == 0) return HN_OK;
  const int tile = pimd_tile_atoms(a.beads);
  hipLaunchKernelGGL(pimd_advance_kernel, dim3((unsigned)((a.n_rep + tile - 1) / tile)), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_pimd_finish(int num_atoms, int num_graphs, const int* graph_ptr, const float* forces, const float* energy,
                                   const long* total, long capacity, double* x, double* v, const double* x0, const double* v0,
                                   int* image, const int* image0, float* f_prev, const double* kick, const double* half_mass,
                                   float* pos32, double* ke_atom, const double* spring_c, const double* centroid, double* log,
                                   long log_steps, long* state, void* stream) {
  const PimdFinishArgs a = {{num_atoms, num_graphs, x, v, x0, v0, image, image0, f_prev, forces, energy, total, capacity, kick,
                             half_mass, graph_ptr, pos32, ke_atom, log, log_steps, state},
                            num_graphs > 0 ? num_atoms / num_graphs : 0, spring_c, centroid};
  if (!pimd_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (num_atoms > 0)
    hipLaunchKernelGGL(md_finish_atoms_kernel<>, dim3((unsigned)((num_atoms + 255) / 256)), dim3(256), 0, s, a.m);
  hipLaunchKernelGGL(pimd_log_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(md_commit_kernel<>, dim3(1), dim3(64), 0, s, a.m);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twins: the same functions in a CPU loop (all pointers HOST pointers) ----------------------------------------------
extern "C" int hermnet_host_pimd_advance(int num_atoms, int num_graphs, int flags, unsigned long seed, double inv_beads,
                                         double* x_host, double* v_host, double* x0_host, double* v0_host, int* image_host,
                                         int* image0_host, const float* f_prev_host, const double* kick_host,
                                         const double* cmat_host, const double* cs_host, const double* sw_host,
                                         const double* ws_host, const double* c1_host, const double* sigma_host,
                                         const float* cell_host, const double* inv_cell_host, float* pos32_host,
                                         double* centroid_host, const long* state_host) {
  const PimdAdvanceArgs a = {num_atoms, num_graphs, num_graphs > 0 ? num_atoms / num_graphs : 0, flags, x_host, v_host, x0_host,
                             v0_host, image_host, image0_host, f_prev_host, kick_host, cmat_host, cs_host, sw_host, ws_host,
                             c1_host, sigma_host, inv_beads, cell_host, inv_cell_host, pos32_host, centroid_host, state_host,
                             (uint64_t)seed};
  if (!pimd_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  if (num_atoms == 0 || state_host[HN_STATE_CODE] != 0) return HN_OK;
  const long step = state_host[HN_STATE_STEP], mode = state_host[HN_STATE_MODE];
  const int tile = pimd_tile_atoms(a.beads);
  double sb[6][256], sm[6][256];
  for (int first = 0; first < a.n_rep; first += tile) {
    if (mode != 0) {
      for (int l = 0; l < 256; ++l) pimd_prime_lane(a, first, l);
      continue;
    }
    for (int l = 0; l < 256; ++l) pimd_bead_in(a, first, l, sb);
    for (int l = 0; l < 256; ++l) pimd_mode(a, step, first, l, sb, sm);
    for (int l = 0; l < 256; ++l) pimd_bead_out(a, first, l, sm, sb);
    for (int l = 0; l < 256; ++l) pimd_centroid(a, first, l, sb, sm);
    for (int l = 0; l < 256; ++l) pimd_store(a, first, l, sb, sm);
  }
  return HN_OK;
}

extern "C" int hermnet_host_pimd_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const float* forces_host,
                                        const float* energy_host, const long* total_host, long capacity, double* x_host,
                                        double* v_host, const double* x0_host, const double* v0_host, int* image_host,
                                        const int* image0_host, float* f_prev_host, const double* kick_host,
                                        const double* half_mass_host, float* pos32_host, double* ke_atom_host,
                                        const double* spring_c_host, const double* centroid_host, double* log_host,
                                        long log_steps, long* state_host) {
  const PimdFinishArgs a = {{num_atoms, num_graphs, x_host, v_host, x0_host, v0_host, image_host, image0_host, f_prev_host,
                             forces_host, energy_host, total_host, capacity, kick_host, half_mass_host, graph_ptr_host, pos32_host,
                             ke_atom_host, log_host, log_steps, state_host},
                            num_graphs > 0 ? num_atoms / num_graphs : 0, spring_c_host, centroid_host};
  if (!pimd_finish_args_ok(a) || !pimd_host_layout_ok(graph_ptr_host, num_graphs, a.n_rep)) return HN_ERR_BAD_ARG;
  md_host_finish(a.m, [&](long step) {
    double part[3][256];
    for (int j = 0; j < num_graphs; ++j) pimd_log_bead(a, step, j, part);
  });
  return HN_OK;
}
