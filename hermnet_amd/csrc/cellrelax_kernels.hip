// gfx950: the device-resident cell relaxation (hermnet_amd/relax.py: DeviceCellRelax) -- ASE's UnitCellFilter under ASE's
// FIRE inside the replayed step.  As relax_kernels.hip: hermnet_cellrelax_advance in front of the neighbour search moves the
// atoms AND the cell (the search, the edge geometry and the virial kernels read the float32 cell it writes),
// hermnet_cellrelax_finish behind the force backward takes forces and virial, so that a replay of the hipGraph IS one force-
// and-stress evaluation of the optimiser for every structure of a batch on its own.
//
// The arithmetic is cellrelax_step.h's (FIRE itself: relax_step.h's, unchanged); the finish -- the per-graph step and the
// commit -- is relax_driver.h's, shared with the plain relaxation and with the host twins at the end of this file: what this
// file adds to it is CellFilter, the cell's part of every stage.  Contraction is off for the whole file; the per-graph sums
// take resident_step.h's canonical order over the atoms and then the three cell rows in row order.  No float atomics.
//
// One cell per step: the advance's FIRST kernel (a lane per graph) makes F, F^-1, C, the float32 cell and det F from the
// moved rows G; its second (a lane per atom) reads that F.  The step protocol is resident_step.h's; what this driver adds:
// the cell moves BEFORE the evaluation, so a void step takes it back too (G from its backup, the rest made of it again by
// the same function), and a step is also void on a virial that is not finite or det F <= 0.  The halt code is derived from
// arrays no kernel of finish writes (energy, virial, total, det_f), so every workgroup derives the same code.
#include <hip/hip_runtime.h>
#include "cellrelax_step.h"
#include "relax_driver.h"

#pragma clang fp contract(off)

namespace {

// Per-graph cell state, shared by both entry points.
struct CellState {
  const double *cell0, *inv_cell0, *cell_factor;   // [B,9], [B,9], [B]: constant
  double *rows, *rows0, *rows_v;                   // G, its start-of-step backup, the rows' velocities [B,9]
  double *deform, *deform_inv, *det_f, *cell64;    // F, F^-1 [B,9], det F [B] (of the last advance), C [B,9]
  float* cell32;                                   // the step's cell tensor [B,9]
};

// The plain driver's arguments (x: the Cartesian coordinates; its cell / inv_cell stay null: the wrap here is by cell0, in
// the reference frame) and the cell driver's own.
struct CellAdvanceArgs {
  RelaxAdvanceArgs r;
  double *q, *q0;
  CellState c;
};

struct CellFinishArgs {
  RelaxFinishArgs r;
  int flags;
  const float* virial;
  const double* pressure;
  double mask[9];                                  // the entry-wise factors of proj: by value, from a HOST array
  double* q;
  const double* q0;
  CellState c;
  double* obs;
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
  if (a.r.gi[4 * (size_t)g + 2]) return;                             // a converged graph is never touched again
  const double scale = a.r.gf[5 * (size_t)g + 2];
  for (int k = 0; k < 9; ++k) {
    const double r = a.c.rows[9 * (size_t)g + k];
    a.c.rows0[9 * (size_t)g + k] = r;
    a.c.rows[9 * (size_t)g + k] = r + scale * a.c.rows_v[9 * (size_t)g + k];
  }
  cell_from_rows(a.c, g);
}

__host__ __device__ inline void cell_advance_one(const CellAdvanceArgs& args, int i) {
  const RelaxAdvanceArgs& a = args.r;
  const CellState& c = args.c;
  const long g = hn_graph_of(a.batch, i, a.num_graphs);
  double x[3];
  for (int k = 0; k < 3; ++k) x[k] = a.x[3 * (size_t)i + k];
  if (!a.gi[4 * (size_t)g + 2]) {
    double q[3], F[9];
    int image[3];
    for (int k = 0; k < 3; ++k) {
      q[k] = args.q[3 * (size_t)i + k];
      image[k] = a.image[3 * (size_t)i + k];
      args.q0[3 * (size_t)i + k] = q[k];
      a.x0[3 * (size_t)i + k] = x[k];
      a.image0[3 * (size_t)i + k] = image[k];
    }
    if (!(a.fixed && a.fixed[i])) {                                  // an atom that is held keeps q: it rides the cell
      double v[3];
      for (int k = 0; k < 3; ++k) v[k] = a.v[3 * (size_t)i + k];
      const int wrap = a.flags & HN_MD_WRAP;
      relax_advance_atom(q, image, v, a.gf[5 * (size_t)g + 2], wrap ? c.cell0 + 9 * g : nullptr, c.inv_cell0 + 9 * g);
      for (int k = 0; k < 3; ++k) {
        args.q[3 * (size_t)i + k] = q[k];
        a.image[3 * (size_t)i + k] = image[k];
      }
    }
    for (int k = 0; k < 9; ++k) F[k] = c.deform[9 * g + k];
    cellrelax_to_cart(q, F, x);
    for (int k = 0; k < 3; ++k) a.x[3 * (size_t)i + k] = x[k];
  }
  for (int k = 0; k < 3; ++k) a.pos32[3 * (size_t)i + k] = (float)x[k];
}

// relax_driver.h's filter of the cell relaxation: atoms in the reference frame (q, fq = f F) and three cell rows beside them.
struct CellFilter {
  typedef CellFinishArgs Args;
  struct Context {
    double F[9], fG[9];                                              // the graph's F; the rows' force (lead lane)
  };
  static HN_HD const RelaxFinishArgs& base(const Args& a) { return a.r; }

  // resident_step.h's code, and HN_HALT_NONFINITE for a virial that is not finite or det F <= 0.  As hn_step_code: on the
  // device every lane of the workgroup calls it and every lane gets the code.
  static HN_HD long code(const Args& a) {
    const int B = a.r.num_graphs;
    int bad = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    for (int g = threadIdx.x; g < B; g += blockDim.x) bad |= cellrelax_bad_graph(a.virial + 9 * (size_t)g, a.c.det_f[g]);
    bad = __syncthreads_or(bad);
#else
    for (int g = 0; g < B; ++g) bad |= cellrelax_bad_graph(a.virial + 9 * (size_t)g, a.c.det_f[g]);
#endif
    const long code = hn_step_code(a.r.energy, B, a.r.total, a.r.capacity);
    return bad ? (code | HN_HALT_NONFINITE) : code;
  }

  // A void step, graph g's atoms and cell back to the start of the step.
  static HN_HD void restore_atom(const Args& a, int i) {
    for (int k = 0; k < 3; ++k) a.q[3 * (size_t)i + k] = a.q0[3 * (size_t)i + k];
  }
  static HN_HD void restore_graph(const Args& a, int g) {
    for (int k = 0; k < 9; ++k) a.c.rows[9 * (size_t)g + k] = a.c.rows0[9 * (size_t)g + k];
    const double det = a.c.det_f[g];
    cell_from_rows(a.c, g);
    a.c.det_f[g] = det;                                              // what the halt code was derived from stays
  }

  static HN_HD void load(const Args& a, int g, Context& ctx) {
    for (int k = 0; k < 9; ++k) ctx.F[k] = a.c.deform[9 * (size_t)g + k];
  }
  static HN_HD void force(const Args& a, const Context& ctx, int i, double fq[3]) {
    double f[3];
    relax_force(a.r.forces, a.r.fixed, i, f);
    cellrelax_atom_force(f, ctx.F, fq);
  }

  // The cell rows' force and their terms of the sums s, the enthalpy; obs = (volume, pressure, stress [9]) of this evaluation.
  static HN_HD void graph_terms(const Args& a, int g, double s[4], RelaxGraph& G, Context& ctx) {
    double vol, pr, stress[9];
    const double p = a.pressure[g];
    cellrelax_cell_force(a.virial + 9 * (size_t)g, a.c.cell64 + 9 * (size_t)g, a.c.deform_inv + 9 * (size_t)g, a.c.cell_factor[g],
                         p, a.mask, a.flags, ctx.fG, &vol, &pr, stress);
    cellrelax_add_rows(ctx.fG, a.c.rows_v + 9 * (size_t)g, s);
    G.energy = (double)a.r.energy[g] + p * vol;
    double* obs = a.obs + 11 * (size_t)g;
    obs[0] = vol;
    obs[1] = pr;
    for (int k = 0; k < 9; ++k) obs[2 + k] = stress[k];
  }

  // The rows' new velocities; their terms join the atoms' s.
  static HN_HD double clamp_sum(const Args& a, int g, const RelaxCoef& c, double s, const Context& ctx) {
    return cellrelax_rows_velocity(a.c.rows_v + 9 * (size_t)g, ctx.fG, c, s);
  }

  static HN_HD void log_row(const Args& a, long step, int g, const RelaxGraph& G) {
    double* row = relax_log_row(a.r, step, g, G, 6);
    row[4] = a.obs[11 * (size_t)g];
    row[5] = a.obs[11 * (size_t)g + 1];
  }
};

__global__ __launch_bounds__(256) void cellrelax_advance_graphs_kernel(CellAdvanceArgs a) {
  if (a.r.state[HN_STATE_CODE] != 0) return;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g < a.r.num_graphs) cell_advance_graph(a, g);
}

__global__ __launch_bounds__(256) void cellrelax_advance_atoms_kernel(CellAdvanceArgs a) {
  if (a.r.state[HN_STATE_CODE] != 0) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.r.n) cell_advance_one(a, i);
}

// One workgroup per graph: relax_driver.h's step.
__global__ __launch_bounds__(256) void cellrelax_graph_kernel(CellFinishArgs a) {
  __shared__ double part[4][256];
  __shared__ RelaxCoef coef;
  const long step = a.r.state[HN_STATE_STEP];
  if (a.r.state[HN_STATE_CODE] != 0 || a.r.state[HN_STATE_DONE] != 0) return;
  relax_graph_step<CellFilter>(a, blockIdx.x, step, CellFilter::code(a), part, &coef);
}

// One workgroup: relax_driver.h's commit.
__global__ __launch_bounds__(256) void cellrelax_commit_kernel(CellFinishArgs a) {
  const long step = a.r.state[HN_STATE_STEP];
  if (a.r.state[HN_STATE_CODE] != 0 || a.r.state[HN_STATE_DONE] != 0) return;
  relax_commit(a.r, step, CellFilter::code(a), threadIdx.x, blockDim.x);
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
  if (!relax_advance_args_ok(a.r) || !cell_state_ok(a.c, a.r.num_graphs, host)) return false;
  return a.r.n == 0 || (a.q && a.q0);
}

bool cell_finish_args_ok(const CellFinishArgs& a, bool host) {
  if (!relax_finish_args_ok(a.r) || (a.flags & ~(HN_CELLRELAX_HYDROSTATIC | HN_CELLRELAX_CONSTANT_VOLUME))) return false;
  if (!a.virial || !a.pressure || !a.obs || !cell_state_ok(a.c, a.r.num_graphs, host)) return false;
  return a.r.n == 0 || (a.q && a.q0);
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
  const CellAdvanceArgs a = {{num_atoms, num_graphs, flags, x, x0, v, image, image0, fixed, batch, nullptr, nullptr, pos32, state,
                              gf, gi},
                             q, q0,
                             {cell0, inv_cell0, cell_factor, rows, rows0, const_cast<double*>(rows_v), deform, deform_inv, det_f,
                              cell64, cell32}};
  if (!cell_advance_args_ok(a, false)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cellrelax_advance_graphs_kernel, dim3((unsigned)((num_graphs + 255) / 256)), dim3(256), 0, s, a);
  if (num_atoms > 0)                                                 // (without atoms the cells still move: the launch above)
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
  const CellFinishArgs a = with_mask(
      {{num_atoms, num_graphs, graph_ptr, forces, energy, total, capacity, dt, dtmax, maxstep, fmax, fmax_graph, x, v, x0, image,
        image0, f_prev, fixed, pos32, gf, gi, gf_new, gi_new, log, log_steps, state},
       flags, virial, pressure, {0.0}, q, q0,
       {cell0, inv_cell0, cell_factor, rows, const_cast<double*>(rows0), rows_v, deform, deform_inv, det_f, cell64, cell32},
       obs}, mask_host);
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
  const CellAdvanceArgs a = {{num_atoms, num_graphs, flags, x_host, x0_host, v_host, image_host, image0_host, fixed_host,
                              batch_host, nullptr, nullptr, pos32_host, state_host, gf_host, gi_host},
                             q_host, q0_host,
                             {cell0_host, inv_cell0_host, cell_factor_host, rows_host, rows0_host, const_cast<double*>(rows_v_host),
                              deform_host, deform_inv_host, det_f_host, cell64_host, cell32_host}};
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
  const CellFinishArgs a = with_mask(
      {{num_atoms, num_graphs, graph_ptr_host, forces_host, energy_host, total_host, capacity, dt, dtmax, maxstep, fmax,
        fmax_graph_host, x_host, v_host, x0_host, image_host, image0_host, f_prev_host, fixed_host, pos32_host, gf_host, gi_host,
        gf_new_host, gi_new_host, log_host, log_steps, state_host},
       flags, virial_host, pressure_host, {0.0}, q_host, q0_host,
       {cell0_host, inv_cell0_host, cell_factor_host, rows_host, const_cast<double*>(rows0_host), rows_v_host, deform_host,
        deform_inv_host, det_f_host, cell64_host, cell32_host},
       obs_host}, mask_host);
  if (!cell_finish_args_ok(a, true)) return HN_ERR_BAD_ARG;
  relax_host_finish<CellFilter>(a);
  return HN_OK;
}
