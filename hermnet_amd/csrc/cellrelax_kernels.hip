// gfx950: the device-resident cell relaxation (hermnet_amd/relax.py: DeviceCellRelax) -- ASE's UnitCellFilter under ASE's
// FIRE inside the replayed step.  As relax_kernels.hip: hermnet_cellrelax_advance in front of the neighbour search moves the
// atoms AND the cell (the search, the edge geometry and the virial kernels read the float32 cell it writes),
// hermnet_cellrelax_finish behind the force backward takes forces and virial, so that a replay of the hipGraph IS one force-
// and-stress evaluation of the optimiser for every structure of a batch on its own.
//
// The arithmetic is cellrelax_step.h's (FIRE itself: relax_step.h's, unchanged), shared with the host twins at the end of
// this file; contraction is off for the whole file; the per-graph sums take resident_step.h's canonical order over the atoms
// and then the three cell rows in row order.  No float atomics.
//
// One cell per step: the advance's FIRST kernel (a lane per graph) makes F, F^-1, C, the float32 cell and det F from the
// moved rows G; its second (a lane per atom) reads that F.  The step protocol is resident_step.h's; what this driver adds:
// the cell moves BEFORE the evaluation, so a void step takes it back too (G from its backup, the rest made of it again by
// the same function), and a step is also void on a virial that is not finite or det F <= 0.  The halt code is derived from
// arrays no kernel of finish writes (energy, virial, total, det_f), so every workgroup derives the same code.
#include <hip/hip_runtime.h>
#include "cellrelax_step.h"

#pragma clang fp contract(off)

namespace {

// Per-graph cell state, shared by both entry points.
struct CellState {
  const double *cell0, *inv_cell0, *cell_factor;   // [B,9], [B,9], [B]: constant
  double *rows, *rows0, *rows_v;                   // G, its start-of-step backup, the rows' velocities [B,9]
  double *deform, *deform_inv, *det_f, *cell64;    // F, F^-1 [B,9], det F [B] (of the last advance), C [B,9]
  float* cell32;                                   // the step's cell tensor [B,9]
};

struct CellAdvanceArgs {
  int n, num_graphs, flags;
  double *q, *q0, *x, *x0;
  const double* v;
  int *image, *image0;
  const unsigned char* fixed;
  const long* batch;
  CellState c;
  float* pos32;
  const long* state;
  const double* gf;
  const long* gi;
};

struct CellFinishArgs {
  int n, num_graphs, flags;
  const int* graph_ptr;
  const float *forces, *energy, *virial;
  const long* total;
  long capacity;
  double dt, dtmax, maxstep, fmax;
  const double *fmax_graph, *pressure;
  double mask[9];                                  // the entry-wise factors of proj: by value, from a HOST array
  double *q, *x, *v;
  const double *q0, *x0;
  int* image;
  const int* image0;
  float* f_prev;
  const unsigned char* fixed;
  float* pos32;
  CellState c;
  double* obs;
  double* gf;
  long* gi;
  double* gf_new;
  long* gi_new;
  double* log;
  long log_steps;
  long* state;
};

// Graph g's cell from its rows G: everything the step reads of it, made in one place.
__host__ __device__ inline void cell_from_rows(const CellState& c, int g) {
  double F[9], Finv[9], C[9], det;
  float c32[9];
  cellrelax_cell(c.rows + 9 * (size_t)g, c.cell_factor[g], c.cell0 + 9 * (size_t)g, F, Finv, C, c32, &det);
  for (int k = 0; k < 9; ++k) {
    c.deform[9 * (size_t)g + k] = F[k];
    c.deform_inv[9 * (size_t)g + k] = Finv[k];
    c.cell64[9 * (size_t)g + k] = C[k];
    c.cell32[9 * (size_t)g + k] = c32[k];
  }
  c.det_f[g] = det;
}

__host__ __device__ inline void cell_advance_graph(const CellAdvanceArgs& a, int g) {
  if (a.gi[4 * (size_t)g + 2]) return;                               // a converged graph is never touched again
  const double scale = a.gf[5 * (size_t)g + 2];
  for (int k = 0; k < 9; ++k) {
    const double r = a.c.rows[9 * (size_t)g + k];
    a.c.rows0[9 * (size_t)g + k] = r;
    a.c.rows[9 * (size_t)g + k] = r + scale * a.c.rows_v[9 * (size_t)g + k];
  }
  cell_from_rows(a.c, g);
}

__host__ __device__ inline void cell_advance_one(const CellAdvanceArgs& a, int i) {
  const long g = hn_graph_of(a.batch, i, a.num_graphs);
  double x[3];
  for (int k = 0; k < 3; ++k) x[k] = a.x[3 * (size_t)i + k];
  if (!a.gi[4 * (size_t)g + 2]) {
    double q[3], F[9];
    int image[3];
    for (int k = 0; k < 3; ++k) {
      q[k] = a.q[3 * (size_t)i + k];
      image[k] = a.image[3 * (size_t)i + k];
      a.q0[3 * (size_t)i + k] = q[k];
      a.x0[3 * (size_t)i + k] = x[k];
      a.image0[3 * (size_t)i + k] = image[k];
    }
    if (!(a.fixed && a.fixed[i])) {                                  // an atom that is held keeps q: it rides the cell
      double v[3];
      for (int k = 0; k < 3; ++k) v[k] = a.v[3 * (size_t)i + k];
      const int wrap = a.flags & HN_MD_WRAP;
      relax_advance_atom(q, image, v, a.gf[5 * (size_t)g + 2], wrap ? a.c.cell0 + 9 * g : nullptr, a.c.inv_cell0 + 9 * g);
      for (int k = 0; k < 3; ++k) {
        a.q[3 * (size_t)i + k] = q[k];
        a.image[3 * (size_t)i + k] = image[k];
      }
    }
    for (int k = 0; k < 9; ++k) F[k] = a.c.deform[9 * g + k];
    cellrelax_to_cart(q, F, x);
    for (int k = 0; k < 3; ++k) a.x[3 * (size_t)i + k] = x[k];
  }
  for (int k = 0; k < 3; ++k) a.pos32[3 * (size_t)i + k] = (float)x[k];
}

// The step's halt code: resident_step.h's, and HN_HALT_NONFINITE for a virial that is not finite or det F <= 0.  As
// hn_step_code: on the device every lane of the workgroup calls it and every lane gets the code.
__host__ __device__ inline long cell_step_code(const CellFinishArgs& a) {
  int bad = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  for (int g = threadIdx.x; g < a.num_graphs; g += blockDim.x) bad |= cellrelax_bad_graph(a.virial + 9 * (size_t)g, a.c.det_f[g]);
  bad = __syncthreads_or(bad);
#else
  for (int g = 0; g < a.num_graphs; ++g) bad |= cellrelax_bad_graph(a.virial + 9 * (size_t)g, a.c.det_f[g]);
#endif
  const long code = hn_step_code(a.energy, a.num_graphs, a.total, a.capacity);
  return bad ? (code | HN_HALT_NONFINITE) : code;
}

// A void step, graph g's atoms and cell back to the start of the step.
__host__ __device__ inline void cell_restore_atom(const CellFinishArgs& a, int i) {
  hn_restore_atom(i, a.x, a.x0, a.image, a.image0, a.pos32);
  for (int k = 0; k < 3; ++k) a.q[3 * (size_t)i + k] = a.q0[3 * (size_t)i + k];
}

__host__ __device__ inline void cell_restore_graph(const CellFinishArgs& a, int g) {
  for (int k = 0; k < 9; ++k) a.c.rows[9 * (size_t)g + k] = a.c.rows0[9 * (size_t)g + k];
  const double det = a.c.det_f[g];
  cell_from_rows(a.c, g);
  a.c.det_f[g] = det;                                                // what the halt code was derived from stays
}

__host__ __device__ inline void cell_atom_force(const CellFinishArgs& a, int i, const double F[9], double fq[3]) {
  double f[3];
  relax_force(a.forces, a.fixed, i, f);
  cellrelax_atom_force(f, F, fq);
}

__host__ __device__ inline void cell_sums_one(const CellFinishArgs& a, int i, const double F[9], double s[4]) {
  double f[3], v[3];
  cell_atom_force(a, i, F, f);
  for (int k = 0; k < 3; ++k) v[k] = a.v[3 * (size_t)i + k];
  const double f2 = relax_dot3(f, f);
  s[0] = s[0] + relax_dot3(f, v);
  s[1] = s[1] + f2;
  s[2] = s[2] + relax_dot3(v, v);
  s[3] = f2 > s[3] ? f2 : s[3];
}

__host__ __device__ inline double cell_velocity_one(const CellFinishArgs& a, int i, const double F[9], const RelaxCoef& c) {
  double f[3], v[3];
  cell_atom_force(a, i, F, f);
  for (int k = 0; k < 3; ++k) v[k] = a.v[3 * (size_t)i + k];
  relax_velocity_atom(v, f, c, a.fixed && a.fixed[i]);
  for (int k = 0; k < 3; ++k) {
    a.v[3 * (size_t)i + k] = v[k];
    a.f_prev[3 * (size_t)i + k] = a.forces[3 * (size_t)i + k];
  }
  return relax_dot3(v, v);
}

// Graph g's decision from the atoms' four sums s: the cell rows' force, their terms, FIRE's update; obs = (volume, pressure,
// stress [9]) of this evaluation.  fG: the rows' force for cell_rows_finish.
__host__ __device__ inline RelaxCoef cell_graph_decide(const CellFinishArgs& a, long step, int g, double s[4], RelaxGraph& G,
                                                       double fG[9]) {
  double vol, pr, stress[9];
  const double p = a.pressure[g];
  cellrelax_cell_force(a.virial + 9 * (size_t)g, a.c.cell64 + 9 * (size_t)g, a.c.deform_inv + 9 * (size_t)g, a.c.cell_factor[g], p,
                       a.mask, a.flags, fG, &vol, &pr, stress);
  cellrelax_add_rows(fG, a.c.rows_v + 9 * (size_t)g, s);
  G.energy = (double)a.energy[g] + p * vol;
  double* obs = a.obs + 11 * (size_t)g;
  obs[0] = vol;
  obs[1] = pr;
  for (int k = 0; k < 9; ++k) obs[2 + k] = stress[k];
  return relax_graph_update(s[0], s[1], s[2], s[3], a.fmax_graph ? a.fmax_graph[g] : a.fmax, a.dt, a.dtmax, step, G);
}

// ... and behind the atoms' new velocities (s: the clamp's sum over them): the rows' velocities and the next move's scale.
__host__ __device__ inline void cell_rows_finish(const CellFinishArgs& a, int g, const RelaxCoef& c, const double fG[9], double s,
                                                 RelaxGraph& G) {
  s = cellrelax_rows_velocity(a.c.rows_v + 9 * (size_t)g, fG, c, s);
  if (!G.converged) G.scale = relax_graph_scale(s, G.dt, a.maxstep);
}

__host__ __device__ inline void cell_log_row(const CellFinishArgs& a, long step, int g, const RelaxGraph& G) {
  double* row = hn_log_row(a.log, step, a.log_steps, a.num_graphs, g, 6);
  row[0] = G.energy;
  row[1] = G.fnorm;
  row[2] = G.dt;
  row[3] = (double)a.total[0];
  row[4] = a.obs[11 * (size_t)g];
  row[5] = a.obs[11 * (size_t)g + 1];
}

__host__ __device__ inline void cell_commit(long* state, long step, long code, int all) {
  if (hn_commit_halt(state, step, code)) return;
  state[HN_STATE_STEP] = step + 1;
  if (all) state[HN_STATE_DONE] = 1;
}

__global__ __launch_bounds__(256) void cellrelax_advance_graphs_kernel(CellAdvanceArgs a) {
  if (a.state[HN_STATE_CODE] != 0) return;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g < a.num_graphs) cell_advance_graph(a, g);
}

__global__ __launch_bounds__(256) void cellrelax_advance_atoms_kernel(CellAdvanceArgs a) {
  if (a.state[HN_STATE_CODE] != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) cell_advance_one(a, i);
}

// One workgroup per graph: the atoms' four sums in the canonical order, the cell rows' terms, the graph's decision, the
// new velocities of atoms and rows, the clamp, the new state into the scratch copy and the graph's log row.
__global__ __launch_bounds__(256) void cellrelax_graph_kernel(CellFinishArgs a) {
  __shared__ double part[4][256];
  __shared__ RelaxCoef coef;
  const long step = a.state[HN_STATE_STEP];
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return;
  const long code = cell_step_code(a);
  const int g = blockIdx.x, t = threadIdx.x, lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.n);
  RelaxGraph G = relax_graph_load(a.gf, a.gi, g);
  if (code != 0) {
    if (!G.converged) {
      for (int i = lo + t; i < hi; i += 256) cell_restore_atom(a, i);
      if (t == 0) cell_restore_graph(a, g);
    }
    return;
  }
  if (G.converged) {
    if (t == 0) {
      relax_graph_store(G, a.gf_new, a.gi_new, g);
      cell_log_row(a, step, g, G);
    }
    return;
  }
  double F[9], fG[9];
  for (int k = 0; k < 9; ++k) F[k] = a.c.deform[9 * (size_t)g + k];
  hn_canonical_sums<4, 3>(lo, hi, part, [&](int i, double* s) { cell_sums_one(a, i, F, s); });
  if (t == 0) {
    double s[4] = {part[0][0], part[1][0], part[2][0], part[3][0]};
    coef = cell_graph_decide(a, step, g, s, G, fG);
  }
  __syncthreads();
  const RelaxCoef c = coef;
  hn_canonical_sums<1, -1>(lo, hi, part, [&](int i, double* s) { s[0] = s[0] + cell_velocity_one(a, i, F, c); });
  if (t == 0) {
    cell_rows_finish(a, g, c, fG, part[0][0], G);
    relax_graph_store(G, a.gf_new, a.gi_new, g);
    cell_log_row(a, step, g, G);
  }
}

// One workgroup: the scratch copy becomes the state, the step is counted, `done` is set once every graph has converged.
__global__ __launch_bounds__(256) void cellrelax_commit_kernel(CellFinishArgs a) {
  const long step = a.state[HN_STATE_STEP];
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return;
  const long code = cell_step_code(a);
  int all = 1;
  if (code == 0)
    for (int g = threadIdx.x; g < a.num_graphs; g += blockDim.x) {
      for (int k = 0; k < 5; ++k) a.gf[5 * (size_t)g + k] = a.gf_new[5 * (size_t)g + k];
      for (int k = 0; k < 4; ++k) a.gi[4 * (size_t)g + k] = a.gi_new[4 * (size_t)g + k];
      all &= a.gi_new[4 * (size_t)g + 2] != 0;
    }
  all = __syncthreads_and(all);
  if (threadIdx.x == 0) cell_commit(a.state, step, code, all);
}

bool cell_state_ok(const CellState& c, int num_graphs, bool host) {
  if (!c.cell0 || !c.inv_cell0 || !c.cell_factor || !c.rows || !c.rows0 || !c.rows_v || !c.deform || !c.deform_inv || !c.det_f ||
      !c.cell64 || !c.cell32)
    return false;
  if (host)                                                          // (device pointers cannot be read here)
    for (int g = 0; g < num_graphs; ++g)
      if (!(c.cell_factor[g] > 0.0) || npt_not_finite(c.cell_factor[g])) return false;
  return true;
}

bool cell_advance_args_ok(const CellAdvanceArgs& a, bool host) {
  if (a.n < 0 || a.num_graphs < 1 || (a.flags & ~HN_MD_WRAP)) return false;
  if (!a.state || !a.gf || !a.gi || !cell_state_ok(a.c, a.num_graphs, host)) return false;
  if (a.n == 0) return true;
  return a.q && a.q0 && a.x && a.x0 && a.v && a.image && a.image0 && a.pos32;
}

bool cell_finish_args_ok(const CellFinishArgs& a, bool host) {
  if (a.n < 0 || a.num_graphs < 1 || a.log_steps < 1 || a.capacity < 0) return false;
  if (a.flags & ~(HN_CELLRELAX_HYDROSTATIC | HN_CELLRELAX_CONSTANT_VOLUME)) return false;
  if (!(a.dt > 0.0) || !(a.dtmax > 0.0) || !(a.maxstep > 0.0) || !(a.fmax > 0.0)) return false;
  if (!a.state || !a.gf || !a.gi || !a.gf_new || !a.gi_new || !a.energy || !a.virial || !a.total || !a.graph_ptr || !a.log ||
      !a.pressure || !a.obs || !cell_state_ok(a.c, a.num_graphs, host))
    return false;
  if (a.n == 0) return true;
  return a.q && a.q0 && a.x && a.x0 && a.v && a.image && a.image0 && a.f_prev && a.forces && a.pos32;
}

// The mask is read on the HOST by every entry point (it travels to the kernels by value): an entry that is not finite is
// refused without a GPU.  cell_factor <= 0 is refused where it can be read: by the host twins (the device entry points get a
// device pointer; hermnet_amd/relax.py refuses it at construction).
bool cell_mask_ok(const double* mask_host) {
  if (!mask_host) return false;
  for (int k = 0; k < 9; ++k)
    if (npt_not_finite(mask_host[k])) return false;
  return true;
}

CellFinishArgs with_mask(CellFinishArgs a, const double* mask_host) {
  for (int k = 0; k < 9; ++k) a.mask[k] = mask_host[k];
  return a;
}

}  // namespace

extern "C" int hermnet_cellrelax_advance(int num_atoms, int num_graphs, int flags, double* q, double* q0, double* x, double* x0,
                                         const double* v, int* image, int* image0, const unsigned char* fixed, const long* batch,
                                         const double* cell0, const double* inv_cell0, const double* cell_factor,
                                         double* rows, double* rows0, const double* rows_v,
                                         double* deform, double* deform_inv, double* det_f, double* cell64, float* cell32,
                                         float* pos32, const long* state, const double* gf, const long* gi, void* stream) {
  const CellAdvanceArgs a = {num_atoms, num_graphs, flags, q, q0, x, x0, v, image, image0, fixed, batch,
                             {cell0, inv_cell0, cell_factor, rows, rows0, const_cast<double*>(rows_v), deform, deform_inv, det_f,
                              cell64, cell32},
                             pos32, state, gf, gi};
  if (!cell_advance_args_ok(a, false)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cellrelax_advance_graphs_kernel, dim3((unsigned)((num_graphs + 255) / 256)), dim3(256), 0, s, a);
  if (num_atoms > 0)
    hipLaunchKernelGGL(cellrelax_advance_atoms_kernel, dim3((unsigned)((num_atoms + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_cellrelax_finish(int num_atoms, int num_graphs, int flags, const int* graph_ptr, const float* forces,
                                        const float* energy, const float* virial, const long* total, long capacity, double dt,
                                        double dtmax, double maxstep, double fmax, const double* fmax_graph,
                                        const double* pressure, const double* mask_host, const double* cell0,
                                        const double* inv_cell0, const double* cell_factor, double* q, const double* q0, double* x,
                                        const double* x0, double* v, int* image, const int* image0, float* f_prev,
                                        const unsigned char* fixed, float* pos32, double* rows, const double* rows0,
                                        double* rows_v, double* deform, double* deform_inv, double* det_f, double* cell64,
                                        float* cell32, double* obs, double* gf, long* gi, double* gf_new, long* gi_new,
                                        double* log, long log_steps, long* state, void* stream) {
  if (!cell_mask_ok(mask_host)) return HN_ERR_BAD_ARG;
  const CellFinishArgs a = with_mask({num_atoms, num_graphs, flags, graph_ptr, forces, energy, virial, total, capacity, dt, dtmax, maxstep, fmax,
                            fmax_graph, pressure, {0.0}, q, x, v, q0, x0, image, image0, f_prev, fixed, pos32,
                            {cell0, inv_cell0, cell_factor, rows, const_cast<double*>(rows0), rows_v, deform, deform_inv, det_f,
                             cell64, cell32},
                            obs, gf, gi, gf_new, gi_new, log, log_steps, state}, mask_host);
  if (!cell_finish_args_ok(a, false)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cellrelax_graph_kernel, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cellrelax_commit_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twins: the same functions in a CPU loop (all pointers HOST pointers) ----------------------------------------------
extern "C" int hermnet_host_cellrelax_advance(int num_atoms, int num_graphs, int flags, double* q_host, double* q0_host,
                                              double* x_host, double* x0_host, const double* v_host, int* image_host,
                                              int* image0_host, const unsigned char* fixed_host, const long* batch_host,
                                              const double* cell0_host, const double* inv_cell0_host,
                                              const double* cell_factor_host, double* rows_host, double* rows0_host,
                                              const double* rows_v_host, double* deform_host, double* deform_inv_host,
                                              double* det_f_host, double* cell64_host, float* cell32_host, float* pos32_host,
                                              const long* state_host, const double* gf_host, const long* gi_host) {
  const CellAdvanceArgs a = {num_atoms, num_graphs, flags, q_host, q0_host, x_host, x0_host, v_host, image_host, image0_host,
                             fixed_host, batch_host,
                             {cell0_host, inv_cell0_host, cell_factor_host, rows_host, rows0_host, const_cast<double*>(rows_v_host),
                              deform_host, deform_inv_host, det_f_host, cell64_host, cell32_host},
                             pos32_host, state_host, gf_host, gi_host};
  if (!cell_advance_args_ok(a, true)) return HN_ERR_BAD_ARG;
  if (state_host[HN_STATE_CODE] != 0) return HN_OK;
  for (int g = 0; g < num_graphs; ++g) cell_advance_graph(a, g);
  for (int i = 0; i < num_atoms; ++i) cell_advance_one(a, i);
  return HN_OK;
}

extern "C" int hermnet_host_cellrelax_finish(int num_atoms, int num_graphs, int flags, const int* graph_ptr_host,
                                             const float* forces_host, const float* energy_host, const float* virial_host,
                                             const long* total_host, long capacity, double dt, double dtmax, double maxstep,
                                             double fmax, const double* fmax_graph_host, const double* pressure_host,
                                             const double* mask_host, const double* cell0_host, const double* inv_cell0_host,
                                             const double* cell_factor_host, double* q_host, const double* q0_host,
                                             double* x_host, const double* x0_host, double* v_host, int* image_host,
                                             const int* image0_host, float* f_prev_host, const unsigned char* fixed_host,
                                             float* pos32_host, double* rows_host, const double* rows0_host, double* rows_v_host,
                                             double* deform_host, double* deform_inv_host, double* det_f_host,
                                             double* cell64_host, float* cell32_host, double* obs_host, double* gf_host,
                                             long* gi_host, double* gf_new_host, long* gi_new_host, double* log_host,
                                             long log_steps, long* state_host) {
  if (!cell_mask_ok(mask_host)) return HN_ERR_BAD_ARG;
  const CellFinishArgs a = with_mask({num_atoms, num_graphs, flags, graph_ptr_host, forces_host, energy_host, virial_host, total_host, capacity,
                            dt, dtmax, maxstep, fmax, fmax_graph_host, pressure_host, {0.0}, q_host, x_host, v_host, q0_host,
                            x0_host, image_host, image0_host, f_prev_host, fixed_host, pos32_host,
                            {cell0_host, inv_cell0_host, cell_factor_host, rows_host, const_cast<double*>(rows0_host), rows_v_host,
                             deform_host, deform_inv_host, det_f_host, cell64_host, cell32_host},
                            obs_host, gf_host, gi_host, gf_new_host, gi_new_host, log_host, log_steps, state_host}, mask_host);
  if (!cell_finish_args_ok(a, true)) return HN_ERR_BAD_ARG;
  const long step = state_host[HN_STATE_STEP];
  if (state_host[HN_STATE_CODE] != 0 || state_host[HN_STATE_DONE] != 0) return HN_OK;
  const long code = cell_step_code(a);
  int all = 1;
  double part[4][256];
  for (int g = 0; g < num_graphs; ++g) {
    const int lo = hn_graph_lo(graph_ptr_host, g), hi = hn_graph_hi(graph_ptr_host, g, num_atoms);
    RelaxGraph G = relax_graph_load(gf_host, gi_host, g);
    if (code != 0) {
      if (!G.converged) {
        for (int i = lo; i < hi; ++i) cell_restore_atom(a, i);
        cell_restore_graph(a, g);
      }
      continue;
    }
    if (!G.converged) {
      double F[9], fG[9];
      for (int k = 0; k < 9; ++k) F[k] = deform_host[9 * (size_t)g + k];
      hn_canonical_sums<4, 3>(lo, hi, part, [&](int i, double* s) { cell_sums_one(a, i, F, s); });
      double s[4] = {part[0][0], part[1][0], part[2][0], part[3][0]};
      const RelaxCoef c = cell_graph_decide(a, step, g, s, G, fG);
      hn_canonical_sums<1, -1>(lo, hi, part, [&](int i, double* t) { t[0] = t[0] + cell_velocity_one(a, i, F, c); });
      cell_rows_finish(a, g, c, fG, part[0][0], G);
    }
    relax_graph_store(G, gf_new_host, gi_new_host, g);
    cell_log_row(a, step, g, G);
    all &= G.converged != 0;
  }
  for (int g = 0; g < num_graphs && code == 0; ++g) {
    for (int k = 0; k < 5; ++k) gf_host[5 * (size_t)g + k] = gf_new_host[5 * (size_t)g + k];
    for (int k = 0; k < 4; ++k) gi_host[4 * (size_t)g + k] = gi_new_host[4 * (size_t)g + k];
  }
  cell_commit(state_host, step, code, all);
  return HN_OK;
}
