// gfx950: the device-resident MD integrator (hermnet_amd/md.py: DeviceMD).  Two entry points bracket the captured step --
// hermnet_md_advance in front of the neighbour search, hermnet_md_finish behind the force backward -- so that a replay of the
// hipGraph IS a time step: coordinates, velocities, thermostat noise, halt logic and the observables log never leave the
// device.  Plain streaming passes (one thread per atom, 256-lane workgroups, 48 B of float64 state per atom and pass).
//
// The arithmetic is md_step.h's, shared with the host twins at the end of this file; contraction is off for the whole
// file, so device, host twin and a numpy float64 transcription agree bit for bit.
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

struct MdAdvanceArgs {
  int n, num_graphs, flags;
  double *x, *v, *x0, *v0;
  int *image, *image0;
  const float* f_prev;
  const double *kick, *c1, *sigma;
  const long* batch;
  const float* cell;
  const double* inv_cell;
  float* pos32;
  const long* state;
  double dt;
  uint64_t seed;
};

__host__ __device__ inline void md_advance_one(const MdAdvanceArgs& a, int i, long step, long mode) {
  double x[3], v[3];
  for (int k = 0; k < 3; ++k) x[k] = a.x[3 * (size_t)i + k];
  if (mode == 0) {
    int image[3];
    float f[3];
    for (int k = 0; k < 3; ++k) {
      v[k] = a.v[3 * (size_t)i + k];
      image[k] = a.image[3 * (size_t)i + k];
      f[k] = a.f_prev[3 * (size_t)i + k];
      a.x0[3 * (size_t)i + k] = x[k];
      a.v0[3 * (size_t)i + k] = v[k];
      a.image0[3 * (size_t)i + k] = image[k];
    }
    const long g = hn_graph_of(a.batch, i, a.num_graphs);
    const int langevin = a.flags & HN_MD_LANGEVIN;
    double xi[3] = {0.0, 0.0, 0.0};
    if (langevin) {
      uint32_t w[8];
      md_noise_words(a.seed, (uint64_t)step, (uint32_t)i, w);
      md_gaussians(w, xi);
    }
    md_advance_atom(x, v, f, a.kick[i], a.dt, langevin, langevin ? a.c1[g] : 0.0, langevin ? a.sigma[i] : 0.0, xi);
    if (a.flags & HN_MD_WRAP) {
      double cell[9], inv[9];
      hn_load_cell(a.cell, a.inv_cell, g, cell, inv);
      md_wrap_atom(x, image, cell, inv);
    }
    for (int k = 0; k < 3; ++k) {
      a.x[3 * (size_t)i + k] = x[k];
      a.v[3 * (size_t)i + k] = v[k];
      a.image[3 * (size_t)i + k] = image[k];
    }
  }
  for (int k = 0; k < 3; ++k) a.pos32[3 * (size_t)i + k] = (float)x[k];
}

__host__ __device__ inline void md_log_row(const MdFinishArgs& a, long step, int g, double e_kin) {
  double* row = hn_log_row(a.log, step, a.log_steps, a.num_graphs, g, 3);
  row[0] = (double)a.energy[g];
  row[1] = e_kin;
  row[2] = (double)a.total[0];
}

__global__ __launch_bounds__(256) void md_advance_kernel(MdAdvanceArgs a) {
  const long step = a.state[HN_STATE_STEP], code = a.state[HN_STATE_CODE], mode = a.state[HN_STATE_MODE];
  if (code != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) md_advance_one(a, i, step, mode);
}

__global__ __launch_bounds__(256) void md_finish_atoms_kernel(MdFinishArgs a) {
  const long halted = a.state[HN_STATE_CODE], mode = a.state[HN_STATE_MODE];
  if (halted != 0) return;
  const long code = hn_step_code(a.energy, a.num_graphs, a.total, a.capacity);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) md_finish_one(a, i, code, mode);
}

// One workgroup per graph: its atoms' kinetic energies in the canonical order, and the graph's log row.
__global__ __launch_bounds__(256) void md_log_kernel(MdFinishArgs a) {
  __shared__ double part[1][256];
  const long step = a.state[HN_STATE_STEP], halted = a.state[HN_STATE_CODE], mode = a.state[HN_STATE_MODE];
  if (halted != 0 || mode != 0) return;
  if (hn_step_code(a.energy, a.num_graphs, a.total, a.capacity) != 0) return;
  const int g = blockIdx.x, lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.n);
  hn_canonical_sums<1, -1>(lo, hi, part, [&](int i, double* s) { s[0] = s[0] + a.ke_atom[i]; });
  if (threadIdx.x == 0) md_log_row(a, step, g, part[0][0]);
}

__global__ __launch_bounds__(64) void md_commit_kernel(MdFinishArgs a) {
  const long step = a.state[HN_STATE_STEP], halted = a.state[HN_STATE_CODE], mode = a.state[HN_STATE_MODE];
  if (halted != 0) return;
  const long code = hn_step_code(a.energy, a.num_graphs, a.total, a.capacity);
  if (threadIdx.x == 0) md_commit(a.state, step, code, mode);
}

// Atom i's eight words and three Gaussians of (seed, step) into the caller's arrays (either may be null).
__host__ __device__ inline void md_noise_one(uint64_t seed, uint64_t step, int i, uint32_t* words, double* gauss) {
  uint32_t w[8];
  double xi[3];
  md_noise_words(seed, step, (uint32_t)i, w);
  md_gaussians(w, xi);
  if (words)
    for (int k = 0; k < 8; ++k) words[8 * (size_t)i + k] = w[k];
  if (gauss)
    for (int k = 0; k < 3; ++k) gauss[3 * (size_t)i + k] = xi[k];
}

__global__ __launch_bounds__(256) void md_noise_kernel(uint64_t seed, uint64_t step, int n, uint32_t* words, double* gauss) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) md_noise_one(seed, step, i, words, gauss);
}

// ---- the barostat (hermnet_md_finish_npt) -----------------------------------------------------------------------------------
struct NptArgs {
  MdFinishArgs m;
  const long* batch;
  const float* virial;
  const double *pressure, *coupling_c;
  double* cell64;
  float* cell32;
  double *inv_cell, *mu;
  long* clamped;
  int coupling, mask;
  double max_strain;
};

// Graph g of a committed step, from its six kinetic sums: mu, the new cell in its three forms and the log row of width 5
// (E_pot, E_kin, edges found, the pressure mu was made from, the volume before the scaling).
__host__ __device__ inline void npt_graph_one(const NptArgs& a, long step, int g, const double kin[6]) {
  float w[9], cell32[9];
  double cell[9], mu[9], inv[9], e_kin, pressure, volume;
  for (int k = 0; k < 9; ++k) {
    w[k] = a.virial[9 * (size_t)g + k];
    cell[k] = a.cell64[9 * (size_t)g + k];
  }
  const int acted = npt_graph(kin, w, a.coupling_c[g], a.pressure[g], a.coupling, a.mask, a.max_strain, cell, mu, cell32, inv,
                              &e_kin, &pressure, &volume);
  for (int k = 0; k < 9; ++k) {
    a.cell64[9 * (size_t)g + k] = cell[k];
    a.cell32[9 * (size_t)g + k] = cell32[k];
    a.inv_cell[9 * (size_t)g + k] = inv[k];
    a.mu[9 * (size_t)g + k] = mu[k];
  }
  if (acted) a.clamped[g] = a.clamped[g] + 1;
  double* row = hn_log_row(a.m.log, step, a.m.log_steps, a.m.num_graphs, g, 5);
  row[0] = (double)a.m.energy[g];
  row[1] = e_kin;
  row[2] = (double)a.m.total[0];
  row[3] = pressure;
  row[4] = volume;
}

__host__ __device__ inline void npt_kinetic_of(const NptArgs& a, int i, double* s) {
  double v[3];
  for (int k = 0; k < 3; ++k) v[k] = a.m.v[3 * (size_t)i + k];
  npt_kinetic_terms(v, a.m.half_mass[i], s);
}

// Atom i of a committed step (held atoms too): x <- x mu of its graph, pos32 = float(x).
__host__ __device__ inline void npt_scale_one(const NptArgs& a, int i) {
  const long g = hn_graph_of(a.batch, i, a.m.num_graphs);
  double mu[9], x[3];
  for (int k = 0; k < 9; ++k) mu[k] = a.mu[9 * g + k];
  for (int k = 0; k < 3; ++k) x[k] = a.m.x[3 * (size_t)i + k];
  npt_scale_atom(x, mu);
  for (int k = 0; k < 3; ++k) {
    a.m.x[3 * (size_t)i + k] = x[k];
    a.m.pos32[3 * (size_t)i + k] = (float)x[k];
  }
}

// One workgroup per graph: the kinetic tensor's six sums in the canonical order, then lane 0 makes the graph's barostat.
__global__ __launch_bounds__(256) void npt_graph_kernel(NptArgs a) {
  __shared__ double part[6][256];
  const long step = a.m.state[HN_STATE_STEP], halted = a.m.state[HN_STATE_CODE], mode = a.m.state[HN_STATE_MODE];
  if (halted != 0 || mode != 0) return;
  if (hn_step_code(a.m.energy, a.m.num_graphs, a.m.total, a.m.capacity) != 0) return;
  const int g = blockIdx.x, lo = hn_graph_lo(a.m.graph_ptr, g), hi = hn_graph_hi(a.m.graph_ptr, g, a.m.n);
  hn_canonical_sums<6, -1>(lo, hi, part, [&](int i, double* s) { npt_kinetic_of(a, i, s); });
  if (threadIdx.x == 0) {
    double kin[6];
    for (int k = 0; k < 6; ++k) kin[k] = part[k][0];
    npt_graph_one(a, step, g, kin);
  }
}

__global__ __launch_bounds__(256) void npt_scale_kernel(NptArgs a) {
  const long halted = a.m.state[HN_STATE_CODE], mode = a.m.state[HN_STATE_MODE];
  if (halted != 0 || mode != 0) return;
  if (hn_step_code(a.m.energy, a.m.num_graphs, a.m.total, a.m.capacity) != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.m.n) npt_scale_one(a, i);
}

bool md_advance_args_ok(const MdAdvanceArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || (a.flags & ~(HN_MD_LANGEVIN | HN_MD_WRAP))) return false;
  if (a.n == 0) return true;
  if (!a.x || !a.v || !a.x0 || !a.v0 || !a.image || !a.image0 || !a.f_prev || !a.kick || !a.pos32 || !a.state) return false;
  if ((a.flags & HN_MD_LANGEVIN) && (!a.c1 || !a.sigma)) return false;
  if ((a.flags & HN_MD_WRAP) && (!a.cell || !a.inv_cell)) return false;
  return true;
}

bool npt_args_ok(const NptArgs& a) {
  if (!md_finish_args_ok(a.m)) return false;
  if (a.coupling != HN_MD_BARO_ISOTROPIC && a.coupling != HN_MD_BARO_AXES && a.coupling != HN_MD_BARO_FULL) return false;
  if ((a.mask & ~7) || !(a.max_strain > 0.0)) return false;
  return a.virial && a.pressure && a.coupling_c && a.cell64 && a.cell32 && a.inv_cell && a.mu && a.clamped;
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
    hipLaunchKernelGGL(md_finish_atoms_kernel, dim3((unsigned)((num_atoms + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(md_log_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(md_commit_kernel, dim3(1), dim3(64), 0, s, a);
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
  if (num_atoms > 0) hipLaunchKernelGGL(md_finish_atoms_kernel, atoms, dim3(256), 0, s, a.m);
  hipLaunchKernelGGL(npt_graph_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  if (num_atoms > 0) hipLaunchKernelGGL(npt_scale_kernel, atoms, dim3(256), 0, s, a);
  hipLaunchKernelGGL(md_commit_kernel, dim3(1), dim3(64), 0, s, a.m);
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
  const long step = state_host[HN_STATE_STEP], mode = state_host[HN_STATE_MODE];
  if (state_host[HN_STATE_CODE] != 0) return HN_OK;
  const long code = hn_step_code(energy_host, num_graphs, total_host, capacity);
  for (int i = 0; i < num_atoms; ++i) md_finish_one(a, i, code, mode);
  if (code == 0 && mode == 0)
    for (int g = 0; g < num_graphs; ++g) {
      const int lo = hn_graph_lo(graph_ptr_host, g), hi = hn_graph_hi(graph_ptr_host, g, num_atoms);
      double s = 0.0;      // sequential, NOT the canonical order the device takes: frozen with ABI v13
      for (int i = lo; i < hi; ++i) s = s + ke_atom_host[i];
      md_log_row(a, step, g, s);
    }
  md_commit(state_host, step, code, mode);
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
  const long step = state_host[HN_STATE_STEP], mode = state_host[HN_STATE_MODE];
  if (state_host[HN_STATE_CODE] != 0) return HN_OK;
  const long code = hn_step_code(energy_host, num_graphs, total_host, capacity);
  for (int i = 0; i < num_atoms; ++i) md_finish_one(a.m, i, code, mode);
  if (code == 0 && mode == 0) {
    double part[6][256];
    for (int g = 0; g < num_graphs; ++g) {
      const int lo = hn_graph_lo(graph_ptr_host, g), hi = hn_graph_hi(graph_ptr_host, g, num_atoms);
      hn_canonical_sums<6, -1>(lo, hi, part, [&](int i, double* s) { npt_kinetic_of(a, i, s); });
      double kin[6];
      for (int k = 0; k < 6; ++k) kin[k] = part[k][0];
      npt_graph_one(a, step, g, kin);
    }
    for (int i = 0; i < num_atoms; ++i) npt_scale_one(a, i);
  }
  md_commit(state_host, step, code, mode);
  return HN_OK;
}
