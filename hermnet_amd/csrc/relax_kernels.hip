// gfx950: the device-resident FIRE relaxation (hermnet_amd/relax.py: DeviceRelax).  Like md_kernels.hip, two entry points
// bracket the captured step -- hermnet_relax_advance in front of the neighbour search, hermnet_relax_finish behind the force
// backward -- so that a replay of the hipGraph IS one force evaluation of the optimiser, for every structure of a batch on
// its own: a structure that has converged freezes while the others keep going.
//
// The arithmetic is relax_step.h's, shared with the host twins at the end of this file; contraction is off for the whole
// file, and the per-graph sums take resident_step.h's canonical order, so device, host twin and a numpy float64
// transcription agree bit for bit.  No float atomics.
//
// The step protocol (state words, halt code, void step, single writer) is resident_step.h's.  What the relaxation adds: the
// fourth state word is `done` (every graph has converged), a void step leaves the velocities and a converged graph alone, and
// the single writer also owns gf / gi: it copies them from the scratch gf_new / gi_new the per-graph kernel filled.
#include <hip/hip_runtime.h>
#include "relax_step.h"

#pragma clang fp contract(off)

namespace {

struct RelaxAdvanceArgs {
  int n, num_graphs, flags;
  double *x, *x0;
  const double* v;
  int *image, *image0;
  const unsigned char* fixed;
  const long* batch;
  const float* cell;
  const double* inv_cell;
  float* pos32;
  const long* state;
  const double* gf;
  const long* gi;
};

struct RelaxFinishArgs {
  int n, num_graphs;
  const int* graph_ptr;
  const float *forces, *energy;
  const long* total;
  long capacity;
  double dt, dtmax, maxstep, fmax;
  const double* fmax_graph;
  double *x, *v;
  const double* x0;
  int* image;
  const int* image0;
  float* f_prev;
  const unsigned char* fixed;
  float* pos32;
  double* gf;
  long* gi;
  double* gf_new;
  long* gi_new;
  double* log;
  long log_steps;
  long* state;
};

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

// An atom's terms of the four sums, added to the lane's partials.
__host__ __device__ inline void relax_sums_one(const RelaxFinishArgs& a, int i, double s[4]) {
  double f[3], v[3];
  relax_force(a.forces, a.fixed, i, f);
  for (int k = 0; k < 3; ++k) v[k] = a.v[3 * (size_t)i + k];
  const double f2 = relax_dot3(f, f);
  s[0] = s[0] + relax_dot3(f, v);
  s[1] = s[1] + f2;
  s[2] = s[2] + relax_dot3(v, v);
  s[3] = f2 > s[3] ? f2 : s[3];
}

// The atom's new velocity and its accepted forces; returns its term of the clamp's sum.
__host__ __device__ inline double relax_velocity_one(const RelaxFinishArgs& a, int i, const RelaxCoef& c) {
  double f[3], v[3];
  relax_force(a.forces, a.fixed, i, f);
  for (int k = 0; k < 3; ++k) v[k] = a.v[3 * (size_t)i + k];
  relax_velocity_atom(v, f, c, a.fixed && a.fixed[i]);
  for (int k = 0; k < 3; ++k) {
    a.v[3 * (size_t)i + k] = v[k];
    a.f_prev[3 * (size_t)i + k] = a.forces[3 * (size_t)i + k];
  }
  return relax_dot3(v, v);
}

__host__ __device__ inline void relax_log_row(const RelaxFinishArgs& a, long step, int g, const RelaxGraph& G) {
  double* row = hn_log_row(a.log, step, a.log_steps, a.num_graphs, g, 4);
  row[0] = G.energy;
  row[1] = G.fnorm;
  row[2] = G.dt;
  row[3] = (double)a.total[0];
}

// The single writer's last words: a void step records its halt, a completed one is counted and may be the last.
__host__ __device__ inline void relax_commit(long* state, long step, long code, int all) {
  if (hn_commit_halt(state, step, code)) return;
  state[HN_STATE_STEP] = step + 1;
  if (all) state[HN_STATE_DONE] = 1;
}

__global__ __launch_bounds__(256) void relax_advance_kernel(RelaxAdvanceArgs a) {
  if (a.state[HN_STATE_CODE] != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) relax_advance_one(a, i);
}

// One workgroup per graph: the four sums in the canonical order, the graph's decision, its atoms' new velocities, the
// clamp's sum over them, the new state into the scratch copy and the graph's log row.
__global__ __launch_bounds__(256) void relax_graph_kernel(RelaxFinishArgs a) {
  __shared__ double part[4][256];
  __shared__ RelaxCoef coef;
  const long step = a.state[HN_STATE_STEP];
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return;
  const long code = hn_step_code(a.energy, a.num_graphs, a.total, a.capacity);
  const int g = blockIdx.x, t = threadIdx.x, lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.n);
  RelaxGraph G = relax_graph_load(a.gf, a.gi, g);
  if (code != 0) {
    if (!G.converged)
      for (int i = lo + t; i < hi; i += 256) hn_restore_atom(i, a.x, a.x0, a.image, a.image0, a.pos32);
    return;
  }
  if (G.converged) {
    if (t == 0) {
      relax_graph_store(G, a.gf_new, a.gi_new, g);
      relax_log_row(a, step, g, G);
    }
    return;
  }
  hn_canonical_sums<4, 3>(lo, hi, part, [&](int i, double* s) { relax_sums_one(a, i, s); });
  if (t == 0) {
    G.energy = (double)a.energy[g];
    coef = relax_graph_update(part[0][0], part[1][0], part[2][0], part[3][0], a.fmax_graph ? a.fmax_graph[g] : a.fmax, a.dt,
                              a.dtmax, step, G);
  }
  __syncthreads();
  const RelaxCoef c = coef;
  hn_canonical_sums<1, -1>(lo, hi, part, [&](int i, double* s) { s[0] = s[0] + relax_velocity_one(a, i, c); });
  if (t == 0) {
    if (!G.converged) G.scale = relax_graph_scale(part[0][0], G.dt, a.maxstep);
    relax_graph_store(G, a.gf_new, a.gi_new, g);
    relax_log_row(a, step, g, G);
  }
}

// One workgroup: the scratch copy becomes the state, the step is counted, `done` is set once every graph has converged.
__global__ __launch_bounds__(256) void relax_commit_kernel(RelaxFinishArgs a) {
  const long step = a.state[HN_STATE_STEP];
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return;
  const long code = hn_step_code(a.energy, a.num_graphs, a.total, a.capacity);
  int all = 1;
  if (code == 0)
    for (int g = threadIdx.x; g < a.num_graphs; g += blockDim.x) {
      for (int k = 0; k < 5; ++k) a.gf[5 * (size_t)g + k] = a.gf_new[5 * (size_t)g + k];
      for (int k = 0; k < 4; ++k) a.gi[4 * (size_t)g + k] = a.gi_new[4 * (size_t)g + k];
      all &= a.gi_new[4 * (size_t)g + 2] != 0;
    }
  all = __syncthreads_and(all);
  if (threadIdx.x == 0) relax_commit(a.state, step, code, all);
}

bool relax_advance_args_ok(const RelaxAdvanceArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || (a.flags & ~HN_MD_WRAP)) return false;
  if (!a.state || !a.gf || !a.gi) return false;
  if (a.n == 0) return true;
  if (!a.x || !a.x0 || !a.v || !a.image || !a.image0 || !a.pos32) return false;
  if ((a.flags & HN_MD_WRAP) && (!a.cell || !a.inv_cell)) return false;
  return true;
}

bool relax_finish_args_ok(const RelaxFinishArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || a.log_steps < 1 || a.capacity < 0) return false;
  if (!(a.dt > 0.0) || !(a.dtmax > 0.0) || !(a.maxstep > 0.0) || !(a.fmax > 0.0)) return false;
  if (!a.state || !a.gf || !a.gi || !a.gf_new || !a.gi_new || !a.energy || !a.total || !a.graph_ptr || !a.log) return false;
  if (a.n == 0) return true;
  return a.x && a.v && a.x0 && a.image && a.image0 && a.f_prev && a.forces && a.pos32;
}

}  // namespace

extern "C" int hermnet_relax_advance(int num_atoms, int num_graphs, int flags, double* x, double* x0, const double* v, int* image,
                                     int* image0, const unsigned char* fixed, const long* batch, const float* cell,
                                     const double* inv_cell, float* pos32, const long* state, const double* gf, const long* gi,
                                     void* stream) {
  const RelaxAdvanceArgs a = {num_atoms, num_graphs, flags, x, x0, v, image, image0, fixed, batch, cell, inv_cell, pos32, state, gf, gi};
  if (!relax_advance_args_ok(a)) return HN_ERR_BAD_ARG;
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
  if (!relax_advance_args_ok(a)) return HN_ERR_BAD_ARG;
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
  const long step = state_host[HN_STATE_STEP];
  if (state_host[HN_STATE_CODE] != 0 || state_host[HN_STATE_DONE] != 0) return HN_OK;
  const long code = hn_step_code(energy_host, num_graphs, total_host, capacity);
  int all = 1;
  double part[4][256];
  for (int g = 0; g < num_graphs; ++g) {
    const int lo = hn_graph_lo(graph_ptr_host, g), hi = hn_graph_hi(graph_ptr_host, g, num_atoms);
    RelaxGraph G = relax_graph_load(gf_host, gi_host, g);
    if (code != 0) {
      if (!G.converged)
        for (int i = lo; i < hi; ++i) hn_restore_atom(i, x_host, x0_host, image_host, image0_host, pos32_host);
      continue;
    }
    if (!G.converged) {
      hn_canonical_sums<4, 3>(lo, hi, part, [&](int i, double* s) { relax_sums_one(a, i, s); });
      G.energy = (double)energy_host[g];
      const RelaxCoef c = relax_graph_update(part[0][0], part[1][0], part[2][0], part[3][0], fmax_graph_host ? fmax_graph_host[g] : fmax, dt, dtmax, step, G);
      hn_canonical_sums<1, -1>(lo, hi, part, [&](int i, double* s) { s[0] = s[0] + relax_velocity_one(a, i, c); });
      if (!G.converged) G.scale = relax_graph_scale(part[0][0], G.dt, maxstep);
    }
    relax_graph_store(G, gf_new_host, gi_new_host, g);
    relax_log_row(a, step, g, G);
    all &= G.converged != 0;
  }
  for (int g = 0; g < num_graphs && code == 0; ++g) {
    for (int k = 0; k < 5; ++k) gf_host[5 * (size_t)g + k] = gf_new_host[5 * (size_t)g + k];
    for (int k = 0; k < 4; ++k) gi_host[4 * (size_t)g + k] = gi_new_host[4 * (size_t)g + k];
  }
  relax_commit(state_host, step, code, all);
  return HN_OK;
}
