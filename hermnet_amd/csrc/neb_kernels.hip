// gfx950: the device-resident nudged elastic band (hermnet_amd/neb.py: DeviceNEB).  The captured step is bracketed like
// the relaxation's: hermnet_relax_advance, unchanged and without the wrap, in front of the neighbour search, and
// hermnet_neb_finish behind the force backward, so that a replay of the hipGraph IS one force evaluation of every image of
// every band, the NEB projection and one step of FIRE on each whole band.
//
// The arithmetic and the text of the three launches are neb_step.h's, shared with the host twin at the end of this file.
// The graphs are COUPLED here -- an image's force needs its neighbours' coordinates and energies, FIRE's sums run over the
// band -- which is why the finish is three launches where the relaxation's is two: what one image's workgroup needs of
// another's work it reads in the NEXT launch.
//   1. neb_force_kernel     one workgroup per image: restore on a void step; else tangent, scalars, g, the image's partials
//   2. neb_velocity_kernel  one workgroup per image: the band's sums, FIRE's decision, velocities, the clamp's partial
//   3. neb_commit_kernel    one workgroup: scale, the band's state into gf / gi, log rows, step count, done or the halt
// Contraction is off for the whole file; no atomics.
#include <hip/hip_runtime.h>
#include "neb_step.h"

#pragma clang fp contract(off)

namespace {

__host__ __device__ inline long neb_code(const NebFinishArgs& a) { return hn_step_code(a.energy, a.num_graphs, a.total, a.capacity); }

__global__ __launch_bounds__(256) void neb_force_kernel(NebFinishArgs a) {
  __shared__ double part[4][256];
  __shared__ NebScalars sc;
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return;
  neb_image_force(a, blockIdx.x, neb_code(a), part, &sc);
}

__global__ __launch_bounds__(256) void neb_velocity_kernel(NebFinishArgs a) {
  __shared__ double part[4][256];
  __shared__ RelaxCoef coef;
  const long step = a.state[HN_STATE_STEP];
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return;
  neb_image_velocity(a, blockIdx.x, step, neb_code(a), part, &coef);
}

__global__ __launch_bounds__(256) void neb_commit_kernel(NebFinishArgs a) {
  const long step = a.state[HN_STATE_STEP];
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return;
  neb_commit(a, step, neb_code(a), threadIdx.x, blockDim.x);
}

// What the host twin can check and the device entry point cannot (its pointers are the device's): the bands tile the graphs,
// each has three images or more, of one atom count, and band_of says so; k and fmax are positive.
bool neb_host_layout_ok(const NebFinishArgs& a) {
  if (a.band_ptr[0] != 0 || a.band_ptr[a.num_bands] != a.num_graphs) return false;
  if (a.graph_ptr[0] != 0 || a.graph_ptr[a.num_graphs] != a.n) return false;
  for (int g = 0; g < a.num_graphs; ++g)
    if (a.graph_ptr[g + 1] < a.graph_ptr[g]) return false;
  for (int k = 0; k < a.num_bands; ++k) {
    const int blo = a.band_ptr[k], bhi = a.band_ptr[k + 1];
    if (bhi - blo < 3 || blo < 0 || bhi > a.num_graphs) return false;
    if (!(a.k_band[k] >= 0.0) || !(a.fmax_band[k] > 0.0)) return false;
    const int count = a.graph_ptr[blo + 1] - a.graph_ptr[blo];
    for (int g = blo; g < bhi; ++g)
      if (a.band_of[g] != k || a.graph_ptr[g + 1] - a.graph_ptr[g] != count) return false;
  }
  return true;
}

}  // namespace

extern "C" int hermnet_neb_finish(int num_atoms, int num_graphs, int num_bands, int climb, const int* graph_ptr, const int* band_ptr,
                                  const int* band_of, const float* forces, const float* energy, const long* total, long capacity,
                                  double dt, double dtmax, double maxstep, const double* k_band, const double* fmax_band, double* x,
                                  double* v, const double* x0, int* image, const int* image0, float* f_prev,
                                  const unsigned char* fixed, float* pos32, double* gf, long* gi, double* obs, long* climber,
                                  double* g, double* isum, double* csum, double* bf_new, long* bi_new, long* climber_new,
                                  double* log, long log_steps, long* state, void* stream) {
  const NebFinishArgs a = {num_atoms, num_graphs, num_bands, climb, graph_ptr, band_ptr, band_of, forces, energy, total, capacity,
                           dt, dtmax, maxstep, k_band, fmax_band, x, v, x0, image, image0, f_prev, fixed, pos32, gf, gi, obs, climber,
                           g, isum, csum, bf_new, bi_new, climber_new, log, log_steps, state};
  if (!neb_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(neb_force_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(neb_velocity_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(neb_commit_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twin: the same functions in a CPU loop (all pointers HOST pointers) -----------------------------------------------
extern "C" int hermnet_host_neb_finish(int num_atoms, int num_graphs, int num_bands, int climb, const int* graph_ptr_host,
                                       const int* band_ptr_host, const int* band_of_host, const float* forces_host,
                                       const float* energy_host, const long* total_host, long capacity, double dt, double dtmax,
                                       double maxstep, const double* k_band_host, const double* fmax_band_host, double* x_host,
                                       double* v_host, const double* x0_host, int* image_host, const int* image0_host,
                                       float* f_prev_host, const unsigned char* fixed_host, float* pos32_host, double* gf_host,
                                       long* gi_host, double* obs_host, long* climber_host, double* g_host, double* isum_host,
                                       double* csum_host, double* bf_new_host, long* bi_new_host, long* climber_new_host,
                                       double* log_host, long log_steps, long* state_host) {
  const NebFinishArgs a = {num_atoms, num_graphs, num_bands, climb, graph_ptr_host, band_ptr_host, band_of_host, forces_host,
                           energy_host, total_host, capacity, dt, dtmax, maxstep, k_band_host, fmax_band_host, x_host, v_host,
                           x0_host, image_host, image0_host, f_prev_host, fixed_host, pos32_host, gf_host, gi_host, obs_host,
                           climber_host, g_host, isum_host, csum_host, bf_new_host, bi_new_host, climber_new_host, log_host,
                           log_steps, state_host};
  if (!neb_finish_args_ok(a) || !neb_host_layout_ok(a)) return HN_ERR_BAD_ARG;
  const long step = a.state[HN_STATE_STEP];
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return HN_OK;
  const long code = neb_code(a);
  double part[4][256];
  NebScalars sc;
  RelaxCoef coef;
  for (int g = 0; g < num_graphs; ++g) neb_image_force(a, g, code, part, &sc);
  for (int g = 0; g < num_graphs; ++g) neb_image_velocity(a, g, step, code, part, &coef);
  neb_commit(a, step, code, 0, 1);
  return HN_OK;
}
