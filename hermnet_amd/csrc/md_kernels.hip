// gfx950: the device-resident MD integrator (hermnet_amd/md.py: DeviceMD).  Two entry points bracket the captured step --
// hermnet_md_advance in front of the neighbour search, hermnet_md_finish behind the force backward -- so that a replay of the
// hipGraph IS a time step: coordinates, velocities, thermostat noise, halt logic and the observables log never leave the
// device.  Plain streaming passes (one thread per atom, 256-lane workgroups, 48 B of float64 state per atom and pass).
//
// This file holds the kernels, the entry points and the host twins.  The text they run is the headers': md_step.h (the
// arithmetic, the advance and the noise of one atom), md_finish.h (the finish skeleton every MD driver shares, with the two
// kernels at its ends) and npt_step.h (the barostat).  Contraction is off for the whole file, so device, host twin and a
// numpy float64 transcription agree bit for bit.
//
// The step protocol (state words, halt code, void step, single writer) is resident_step.h's.  What MD adds: velocities are
// backed up and restored with the coordinates, and the fourth state word is a mode -- 1 ("prime"): advance only rewrites the
// float32 input, finish only copies the forces to f_prev and clears the mode (the first evaluation, and a recapture's).
//
// hermnet_md_finish_npt is hermnet_md_finish with a Berendsen barostat behind the second kick (hermnet_amd/md.py: DeviceNPT;
// the arithmetic is npt_step.h's): a committed step scales the cell and the coordinates by mu, made from the step's own
// virial and the kinetic tensor, and writes the float32 cell the NEXT replay's search reads.  A void step, a prime and a
// parked replay never scale, so the cell needs no backup.
#include <hip/hip_runtime.h>
#include "md_finish.h"
#include "npt_step.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void md_advance_kernel(MdAdvanceArgs a) {
  const long step = a.state[HN_STATE_STEP], code = a.state[HN_STATE_CODE], mode = a.state[HN_STATE_MODE];
  if (code != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) md_advance_one(a, i, step, mode);
}

// One workgroup per graph: its atoms' kinetic energies in the canonical order, and the graph's log row.
__global__ __launch_bounds__(256) void md_log_kernel(MdFinishArgs a) {
  __shared__ double part[1][256];
  long step;
  if (!md_committed(a, &step)) return;
  const double e_kin = md_kinetic_sum(a, blockIdx.x, part);
  if (threadIdx.x == 0) md_log_row(a, step, blockIdx.x, e_kin);
}

__global__ __launch_bounds__(256) void md_noise_kernel(uint64_t seed, uint64_t step, int n, uint32_t* words, double* gauss) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) md_noise_one(seed, step, i, words, gauss);
}

// ---- the barostat (hermnet_md_finish_npt) -----------------------------------------------------------------------------------
// One workgroup per graph: the kinetic tensor's six sums in the canonical order, then lane 0 makes the graph's barostat.
__global__ __launch_bounds__(256) void npt_graph_kernel(NptArgs a) {
  __shared__ double part[6][256];
  long step;
  if (!md_committed(a.m, &step)) return;
  const int g = blockIdx.x, lo = hn_graph_lo(a.m.graph_ptr, g), hi = hn_graph_hi(a.m.graph_ptr, g, a.m.n);
  hn_canonical_sums<6, -1>(lo, hi, part, [&](int i, double* s) { npt_kinetic_of(a, i, s); });
  if (threadIdx.x == 0) {
    double kin[6];
    for (int k = 0; k < 6; ++k) kin[k] = part[k][0];
    npt_graph_one(a, step, g, kin);
  }
}

__global__ __launch_bounds__(256) void npt_scale_kernel(NptArgs a) {
  long step;
  if (!md_committed(a.m, &step)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.m.n) npt_scale_one(a, i);
}

}  // namespace

extern "C" int hermnet_md_advance(int num_atoms, int num_graphs, int flags, double dt, unsigned long seed, double* x, double* v, double* x0,
                                  double* v0, int* image, int* image0, const float* f_prev, const double* kick,
                                  const double* c1, const double* sigma, const long* batch, const float* cell,
                                  const double* inv_cell, float* pos32, const long* state, void* stream) {
  const MdAdvanceArgs a = {num_atoms, num_graphs, flags, x, v, x0, v0, image, image0, f_prev, kick, c1, sigma, batch, cell, inv_cell, pos32,
                           state, dt, (uint64_t)seed};
  if (!md_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  if (num_atoms == 0) return HN_OK;
  hipLaunchKernelGGL(md_advance_kernel, dim3((unsigned)((num_atoms + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_md_finish(int num_atoms, int num_graphs, const int* graph_ptr, const float* forces, const float* energy,
                                 const long* total, long capacity, double* x, double* v, const double* x0, const double* v0,
                                 int* image, const int* image0, float* f_prev, const double* kick, const double* half_mass,
                                 float* pos32, double* ke_atom, double* log, long log_steps, long* state, void* stream) {
  const MdFinishArgs a = {num_atoms, num_graphs, x, v, x0, v0, image, image0, f_prev, forces, energy, total, capacity, kick,
                          half_mass, graph_ptr, pos32, ke_atom, log, log_steps, state};
  if (!md_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (num_atoms > 0)
    hipLaunchKernelGGL(md_finish_atoms_kernel<>, dim3((unsigned)((num_atoms + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(md_log_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(md_commit_kernel<>, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_md_finish_npt(int num_atoms, int num_graphs, const int* graph_ptr, const long* batch, const float* forces,
                                     const float* energy, const float* virial, const long* total, long capacity, int coupling,
                                     int mask, double max_strain, const double* pressure, const double* coupling_c, double* x,
                                     double* v, const double* x0, const double* v0, int* image, const int* image0,
                                     float* f_prev, const double* kick, const double* half_mass, float* pos32, double* ke_atom,
                                     double* cell64, float* cell32, double* inv_cell, double* mu, long* clamped, double* log,
                                     long log_steps, long* state, void* stream) {
  const NptArgs a = {{num_atoms, num_graphs, x, v, x0, v0, image, image0, f_prev, forces, energy, total, capacity, kick,
                      half_mass, graph_ptr, pos32, ke_atom, log, log_steps, state},
                     batch, virial, pressure, coupling_c, cell64, cell32, inv_cell, mu, clamped, coupling, mask, max_strain};
  if (!npt_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  const dim3 atoms((unsigned)((num_atoms + 255) / 256));
  if (num_atoms > 0) hipLaunchKernelGGL(md_finish_atoms_kernel<>, atoms, dim3(256), 0, s, a.m);
  hipLaunchKernelGGL(npt_graph_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  if (num_atoms > 0) hipLaunchKernelGGL(npt_scale_kernel, atoms, dim3(256), 0, s, a);
  hipLaunchKernelGGL(md_commit_kernel<>, dim3(1), dim3(64), 0, s, a.m);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_md_noise(unsigned long seed, unsigned long step, int n, unsigned* out_words, double* out_gauss,
                                void* stream) {
  if (n < 0 || (!out_words && !out_gauss)) return HN_ERR_BAD_ARG;
  if (n == 0) return HN_OK;
  hipLaunchKernelGGL(md_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint64_t)seed,
                     (uint64_t)step, n, out_words, out_gauss);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twins: the same functions in a CPU loop (all pointers HOST pointers) ----------------------------------------------
extern "C" int hermnet_host_md_noise(unsigned long seed, unsigned long step, int n, unsigned* out_words_host,
                                     double* out_gauss_host) {
  if (n < 0 || (!out_words_host && !out_gauss_host)) return HN_ERR_BAD_ARG;
  for (int i = 0; i < n; ++i) md_noise_one((uint64_t)seed, (uint64_t)step, i, out_words_host, out_gauss_host);
  return HN_OK;
}

extern "C" int hermnet_host_md_advance(int num_atoms, int num_graphs, int flags, double dt, unsigned long seed, double* x_host, double* v_host,
                                       double* x0_host, double* v0_host, int* image_host, int* image0_host,
                                       const float* f_prev_host, const double* kick_host, const double* c1_host,
                                       const double* sigma_host, const long* batch_host, const float* cell_host,
                                       const double* inv_cell_host, float* pos32_host, const long* state_host) {
  const MdAdvanceArgs a = {num_atoms, num_graphs, flags, x_host, v_host, x0_host, v0_host, image_host, image0_host, f_prev_host, kick_host,
                           c1_host, sigma_host, batch_host, cell_host, inv_cell_host, pos32_host, state_host, dt, (uint64_t)seed};
  if (!md_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  if (num_atoms == 0 || state_host[HN_STATE_CODE] != 0) return HN_OK;
  for (int i = 0; i < num_atoms; ++i) md_advance_one(a, i, state_host[HN_STATE_STEP], state_host[HN_STATE_MODE]);
  return HN_OK;
}

extern "C" int hermnet_host_md_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const float* forces_host,
                                      const float* energy_host, const long* total_host, long capacity, double* x_host,
                                      double* v_host, const double* x0_host, const double* v0_host, int* image_host,
                                      const int* image0_host, float* f_prev_host, const double* kick_host,
                                      const double* half_mass_host, float* pos32_host, double* ke_atom_host, double* log_host,
                                      long log_steps, long* state_host) {
  const MdFinishArgs a = {num_atoms, num_graphs, x_host, v_host, x0_host, v0_host, image_host, image0_host, f_prev_host,
                          forces_host, energy_host, total_host, capacity, kick_host, half_mass_host, graph_ptr_host, pos32_host,
                          ke_atom_host, log_host, log_steps, state_host};
  if (!md_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  md_host_finish(a, [&](long step) {
    for (int g = 0; g < num_graphs; ++g) {
      const int lo = hn_graph_lo(graph_ptr_host, g), hi = hn_graph_hi(graph_ptr_host, g, num_atoms);
      double s = 0.0;      // sequential, NOT the canonical order the device takes: frozen with ABI v13
      for (int i = lo; i < hi; ++i) s = s + ke_atom_host[i];
      md_log_row(a, step, g, s);
    }
  });
  return HN_OK;
}

// The kinetic sums here take the canonical order of the device (hermnet_host_md_finish's sequential sum is not used).
extern "C" int hermnet_host_md_finish_npt(int num_atoms, int num_graphs, const int* graph_ptr_host, const long* batch_host,
                                          const float* forces_host, const float* energy_host, const float* virial_host,
                                          const long* total_host, long capacity, int coupling, int mask, double max_strain,
                                          const double* pressure_host, const double* coupling_c_host, double* x_host,
                                          double* v_host, const double* x0_host, const double* v0_host, int* image_host,
                                          const int* image0_host, float* f_prev_host, const double* kick_host,
                                          const double* half_mass_host, float* pos32_host, double* ke_atom_host,
                                          double* cell64_host, float* cell32_host, double* inv_cell_host, double* mu_host,
                                          long* clamped_host, double* log_host, long log_steps, long* state_host) {
  const NptArgs a = {{num_atoms, num_graphs, x_host, v_host, x0_host, v0_host, image_host, image0_host, f_prev_host, forces_host,
                      energy_host, total_host, capacity, kick_host, half_mass_host, graph_ptr_host, pos32_host, ke_atom_host,
                      log_host, log_steps, state_host},
                     batch_host, virial_host, pressure_host, coupling_c_host, cell64_host, cell32_host, inv_cell_host, mu_host,
                     clamped_host, coupling, mask, max_strain};
  if (!npt_args_ok(a)) return HN_ERR_BAD_ARG;
  md_host_finish(a.m, [&](long step) {
    double part[6][256];
    for (int g = 0; g < num_graphs; ++g) {
      const int lo = hn_graph_lo(graph_ptr_host, g), hi = hn_graph_hi(graph_ptr_host, g, num_atoms);
      hn_canonical_sums<6, -1>(lo, hi, part, [&](int i, double* s) { npt_kinetic_of(a, i, s); });
      double kin[6];
      for (int k = 0; k < 6; ++k) kin[k] = part[k][0];
      npt_graph_one(a, step, g, kin);
    }
    for (int i = 0; i < num_atoms; ++i) npt_scale_one(a, i);
  });
  return HN_OK;
}
