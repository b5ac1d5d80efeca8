// gfx950: the device-resident FIRE relaxation (hermnet_amd/relax.py: DeviceRelax).  Like md_kernels.hip, two entry points
// bracket the captured step -- hermnet_relax_advance in front of the neighbour search, hermnet_relax_finish behind the force
// backward -- so that a replay of the hipGraph IS one force evaluation of the optimiser, for every structure of a batch on
// its own: a structure that has converged freezes while the others keep going.
//
// The arithmetic is relax_step.h's; the finish -- the per-graph step and the commit -- is relax_driver.h's, shared with the
// cell relaxation and with the host twins at the end of this file: what this file adds to it is PlainFilter, the atoms'
// forces as they are.  Contraction is off for the whole file, and the per-graph sums take resident_step.h's canonical order,
// so device, host twin and a numpy float64 transcription agree bit for bit.  No float atomics.
//
// The step protocol (state words, halt code, void step, single writer) is resident_step.h's.  What the relaxation adds: the
// fourth state word is `done` (every graph has converged), a void step leaves the velocities and a converged graph alone, and
// the single writer also owns gf / gi: it copies them from the scratch gf_new / gi_new the per-graph kernel filled.
#include <hip/hip_runtime.h>
#include "relax_driver.h"

#pragma clang fp contract(off)

namespace {

__host__ __device__ inline void relax_advance_one(const RelaxAdvanceArgs& a, int i) {
  const long g = hn_graph_of(a.batch, i, a.num_graphs);
  double x[3];
  for (int k = 0; k < 3; ++k) x[k] = a.x[3 * (size_t)i + k];
  if (!a.gi[4 * (size_t)g + 2]) {                                   // a converged graph is never touched again
    int image[3];
    for (int k = 0; k < 3; ++k) {
      image[k] = a.image[3 * (size_t)i + k];
      a.x0[3 * (size_t)i + k] = x[k];
      a.image0[3 * (size_t)i + k] = image[k];
    }
    if (!(a.fixed && a.fixed[i])) {
      double v[3], cell[9], inv[9];
      for (int k = 0; k < 3; ++k) v[k] = a.v[3 * (size_t)i + k];
      const int wrap = a.flags & HN_MD_WRAP;
      if (wrap) hn_load_cell(a.cell, a.inv_cell, g, cell, inv);
      relax_advance_atom(x, image, v, a.gf[5 * (size_t)g + 2], wrap ? cell : nullptr, inv);
      for (int k = 0; k < 3; ++k) {
        a.x[3 * (size_t)i + k] = x[k];
        a.image[3 * (size_t)i + k] = image[k];
      }
    }
  }
  for (int k = 0; k < 3; ++k) a.pos32[3 * (size_t)i + k] = (float)x[k];
}

// relax_driver.h's filter of the plain relaxation: the atoms' forces as they are, and nothing of the graph's own.
struct PlainFilter {
  typedef RelaxFinishArgs Args;
  struct Context {};
  static HN_HD const RelaxFinishArgs& base(const Args& a) { return a; }
  static HN_HD long code(const Args& a) { return hn_step_code(a.energy, a.num_graphs, a.total, a.capacity); }
  static HN_HD void restore_atom(const Args&, int) {}
  static HN_HD void restore_graph(const Args&, int) {}
  static HN_HD void load(const Args&, int, Context&) {}
  static HN_HD void force(const Args& a, const Context&, int i, double f[3]) { relax_force(a.forces, a.fixed, i, f); }
  static HN_HD void graph_terms(const Args& a, int g, double*, RelaxGraph& G, Context&) { G.energy = (double)a.energy[g]; }
  static HN_HD double clamp_sum(const Args&, int, const RelaxCoef&, double s, const Context&) { return s; }
  static HN_HD void log_row(const Args& a, long step, int g, const RelaxGraph& G) { relax_log_row(a, step, g, G, 4); }
};

__global__ __launch_bounds__(256) void relax_advance_kernel(RelaxAdvanceArgs a) {
  if (a.state[HN_STATE_CODE] != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) relax_advance_one(a, i);
}

// One workgroup per graph: relax_driver.h's step.
__global__ __launch_bounds__(256) void relax_graph_kernel(RelaxFinishArgs a) {
  __shared__ double part[4][256];
  __shared__ RelaxCoef coef;
  const long step = a.state[HN_STATE_STEP];
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return;
  relax_graph_step<PlainFilter>(a, blockIdx.x, step, PlainFilter::code(a), part, &coef);
}

// One workgroup: relax_driver.h's commit.
__global__ __launch_bounds__(256) void relax_commit_kernel(RelaxFinishArgs a) {
  const long step = a.state[HN_STATE_STEP];
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return;
  relax_commit(a, step, PlainFilter::code(a), threadIdx.x, blockDim.x);
}

bool plain_advance_args_ok(const RelaxAdvanceArgs& a) {
  if (!relax_advance_args_ok(a)) return false;
  return a.n == 0 || !(a.flags & HN_MD_WRAP) || (a.cell && a.inv_cell);
}

}  // namespace

extern "C" int hermnet_relax_advance(int num_atoms, int num_graphs, int flags, double* x, double* x0, const double* v, int* image,
                                     int* image0, const unsigned char* fixed, const long* batch, const float* cell,
                                     const double* inv_cell, float* pos32, const long* state, const double* gf, const long* gi,
                                     void* stream) {
  const RelaxAdvanceArgs a = {num_atoms, num_graphs, flags, x, x0, v, image, image0, fixed, batch, cell, inv_cell, pos32, state, gf, gi};
  if (!plain_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  if (num_atoms == 0) return HN_OK;
  hipLaunchKernelGGL(relax_advance_kernel, dim3((unsigned)((num_atoms + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_relax_finish(int num_atoms, int num_graphs, const int* graph_ptr, const float* forces, const float* energy,
                                    const long* total, long capacity, double dt, double dtmax, double maxstep, double fmax,
                                    const double* fmax_graph, double* x, double* v, const double* x0, int* image,
                                    const int* image0, float* f_prev, const unsigned char* fixed, float* pos32, double* gf,
                                    long* gi, double* gf_new, long* gi_new, double* log, long log_steps, long* state,
                                    void* stream) {
  const RelaxFinishArgs a = {num_atoms, num_graphs, graph_ptr, forces, energy, total, capacity, dt, dtmax, maxstep, fmax, fmax_graph,
                             x, v, x0, image, image0, f_prev, fixed, pos32, gf, gi, gf_new, gi_new, log, log_steps, state};
  if (!relax_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(relax_graph_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(relax_commit_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twins: the same functions in a CPU loop (all pointers HOST pointers) ----------------------------------------------
extern "C" int hermnet_host_relax_advance(int num_atoms, int num_graphs, int flags, double* x_host, double* x0_host,
                                          const double* v_host, int* image_host, int* image0_host,
                                          const unsigned char* fixed_host, const long* batch_host, const float* cell_host,
                                          const double* inv_cell_host, float* pos32_host, const long* state_host,
                                          const double* gf_host, const long* gi_host) {
  const RelaxAdvanceArgs a = {num_atoms, num_graphs, flags, x_host, x0_host, v_host, image_host, image0_host, fixed_host, batch_host,
                              cell_host, inv_cell_host, pos32_host, state_host, gf_host, gi_host};
  if (!plain_advance_args_ok(a)) return HN_ERR_BAD_ARG;
  if (num_atoms == 0 || state_host[HN_STATE_CODE] != 0) return HN_OK;
  for (int i = 0; i < num_atoms; ++i) relax_advance_one(a, i);
  return HN_OK;
}

extern "C" int hermnet_host_relax_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const float* forces_host,
                                         const float* energy_host, const long* total_host, long capacity, double dt,
                                         double dtmax, double maxstep, double fmax, const double* fmax_graph_host, double* x_host,
                                         double* v_host, const double* x0_host, int* image_host, const int* image0_host,
                                         float* f_prev_host, const unsigned char* fixed_host, float* pos32_host, double* gf_host,
                                         long* gi_host, double* gf_new_host, long* gi_new_host, double* log_host, long log_steps,
                                         long* state_host) {
  const RelaxFinishArgs a = {num_atoms, num_graphs, graph_ptr_host, forces_host, energy_host, total_host, capacity, dt, dtmax, maxstep,
                             fmax, fmax_graph_host, x_host, v_host, x0_host, image_host, image0_host, f_prev_host, fixed_host,
                             pos32_host, gf_host, gi_host, gf_new_host, gi_new_host, log_host, log_steps, state_host};
  if (!relax_finish_args_ok(a)) return HN_ERR_BAD_ARG;
  relax_host_finish<PlainFilter>(a);
  return HN_OK;
}
