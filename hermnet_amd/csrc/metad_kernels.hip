// gfx950: multiple-walker metadynamics inside the replayed MD step (hermnet_amd/metad.py: DeviceMetaD).  A stage of four
// launches between the force backward and the unchanged hermnet_md_finish adds the bias force of a shared list of Gaussian
// hills to the step's forces, logs the collective variables and deposits hills -- without leaving the replay.  The
// definitions, the protocol and the arithmetic are metad_step.h's, shared with the host twins at the end of this file.
// Contraction is off for the whole file.
//
// The per-atom CV pass is the hot path: a coordination number is all pairs of a walker in float64.  One lane per atom,
// 256-lane workgroups, blockIdx.y = walker.  The partners are staged through LDS in tiles of 256 atoms -- fractional
// coordinates [component][lane] in float64 and a role byte, 6.4 KB -- so a step of a lane's pair loop reads ONE LDS address
// per wave (a broadcast).  Every lane walks ALL partners in ascending j and keeps its own count and its own gradient in
// registers: a pair is visited from both ends, nothing is scattered, there is no atomic, and the order of every sum is the
// order of the host's serial loop whatever the tiling.
#include <hip/hip_runtime.h>
#include "metad_step.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void metad_cv_kernel(MetadArgs a) {
  __shared__ double sj[3][MT_TILE];
  __shared__ unsigned char rj[MT_TILE];
  long step;
  const int phase = mt_phase(a, &step);
  if (phase == MT_IDLE || phase == MT_VOID) return;
  const int g = blockIdx.y, l = threadIdx.x;
  const int lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.n);
  const int i = lo + blockIdx.x * MT_TILE + l, tiles = (hi - lo + MT_TILE - 1) / MT_TILE;
  const bool mine = i < hi;
  double cell[9];
  mt_cell(a, g, cell);
  for (int d = 0; d < a.num_cvs; ++d) {
    if (a.cv_kind[2 * d] == MT_DISTANCE) {
      if (mine) mt_distance_atom(a, d, g, i);
      continue;
    }
    double si[3] = {0.0, 0.0, 0.0}, acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int ri = mine ? mt_atom(a, d, g, i, si) : 0;
    for (int t = 0; t < tiles; ++t) {
      __syncthreads();                 // the tile before this one has been walked
      mt_stage(a, d, g, t, l, sj, rj);
      __syncthreads();
      if (mine) mt_coord_lane(a, d, g, i, t, sj, rj, si, ri, cell, acc);
    }
    if (mine) mt_coord_store(a, d, i, acc);
  }
}

template <bool BIAS>
__global__ __launch_bounds__(256) void metad_walker_kernel(MetadArgs a) {
  __shared__ double part[6][256];
  long step;
  const int phase = mt_phase(a, &step);
  if (phase == MT_IDLE || phase == MT_VOID) return;
  mt_walker(a, blockIdx.x, phase, step, BIAS, part);
}

__global__ __launch_bounds__(256) void metad_apply_kernel(MetadArgs a) {
  long step;
  const int phase = mt_phase(a, &step);
  if (phase == MT_IDLE) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) mt_apply_one(a, i, phase);
}

__global__ __launch_bounds__(256) void metad_deposit_kernel(MetadArgs a) {
  long step;
  const int phase = mt_phase(a, &step);
  mt_deposit(a, phase, step, threadIdx.x, 256);
}

__global__ __launch_bounds__(256) void metad_report_kernel(MetadArgs a, double* values, double* grads) {
  mt_report_lane(a, blockIdx.x * 256 + threadIdx.x, values, grads);
}

void mt_launch_cv(const MetadArgs& a, hipStream_t s) {
  if (a.n > 0)
    hipLaunchKernelGGL(metad_cv_kernel, dim3((unsigned)((a.n_rep + MT_TILE - 1) / MT_TILE), (unsigned)a.num_graphs), dim3(256), 0, s, a);
}

// The per-atom pass on the host: the lanes of a workgroup in turn, tile by tile.
void mt_host_cv_pass(const MetadArgs& a) {
  static thread_local double sj[3][MT_TILE], si[MT_TILE][3], acc[MT_TILE][4];
  static thread_local unsigned char rj[MT_TILE];
  static thread_local int ri[MT_TILE];
  for (int g = 0; g < a.num_graphs; ++g) {
    const int lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.n), tiles = (hi - lo + MT_TILE - 1) / MT_TILE;
    double cell[9];
    mt_cell(a, g, cell);
    for (int bx = 0; bx < tiles; ++bx)
      for (int d = 0; d < a.num_cvs; ++d) {
        const int first = lo + bx * MT_TILE, count = hi - first < MT_TILE ? hi - first : MT_TILE;
        if (a.cv_kind[2 * d] == MT_DISTANCE) {
          for (int l = 0; l < count; ++l) mt_distance_atom(a, d, g, first + l);
          continue;
        }
        for (int l = 0; l < count; ++l) {
          for (int k = 0; k < 4; ++k) acc[l][k] = 0.0;
          ri[l] = mt_atom(a, d, g, first + l, si[l]);
        }
        for (int t = 0; t < tiles; ++t) {
          for (int l = 0; l < MT_TILE; ++l) mt_stage(a, d, g, t, l, sj, rj);
          for (int l = 0; l < count; ++l) mt_coord_lane(a, d, g, first + l, t, sj, rj, si[l], ri[l], cell, acc[l]);
        }
        for (int l = 0; l < count; ++l) mt_coord_store(a, d, first + l, acc[l]);
      }
  }
}

MetadArgs mt_cv_only(int num_atoms, int num_graphs, int num_cvs, const int* graph_ptr, const double* x, const int* image,
                     const float* cell, const double* inv_cell, const int* cv_kind, const double* cv_par,
                     const unsigned char* cv_role, const double* cv_weight, double* cv_atom, double* cv_walker) {
  MetadArgs a = {};
  a.n = num_atoms;
  a.num_graphs = num_graphs;
  a.n_rep = num_graphs > 0 ? num_atoms / num_graphs : 0;
  a.num_cvs = num_cvs;
  a.graph_ptr = graph_ptr;
  a.x = x;
  a.image = image;
  a.cell32 = cell;
  a.inv_cell = inv_cell;
  a.cv_kind = cv_kind;
  a.cv_par = cv_par;
  a.cv_role = cv_role;
  a.cv_weight = cv_weight;
  a.cv_atom = cv_atom;
  a.cv_walker = cv_walker;
  a.pace = a.max_hills = a.log_steps = 1;
  return a;
}

}  // namespace

extern "C" int hermnet_metad_bias(int num_atoms, int num_graphs, int num_cvs, const int* graph_ptr, const double* x,
                                  const int* image, const float* cell, const double* inv_cell, const int* cv_kind,
                                  const double* cv_par, const unsigned char* cv_role, const double* cv_weight,
                                  const double* sigma_par, double height, double inv_kt, long pace, long max_hills,
                                  const float* forces, const float* energy, const long* total, long capacity, const long* state,
                                  double* cv_atom, double* cv_walker, long* hill_count, double* hill_centres,
                                  double* hill_heights, float* forces_b, double* bias_forces, double* cv_log, long log_steps,
                                  void* stream) {
  const MetadArgs a = {num_atoms, num_graphs, num_graphs > 0 ? num_atoms / num_graphs : 0, num_cvs, graph_ptr, x, image, cell,
                       inv_cell, cv_kind, cv_par, cv_role, cv_weight, sigma_par, height, inv_kt, pace, max_hills, forces, energy,
                       total, capacity, state, cv_atom, cv_walker, hill_count, hill_centres, hill_heights, forces_b,
                       bias_forces, cv_log, log_steps};
  if (!mt_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  mt_launch_cv(a, s);
  hipLaunchKernelGGL(metad_walker_kernel<true>, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  if (num_atoms > 0) hipLaunchKernelGGL(metad_apply_kernel, dim3((unsigned)((num_atoms + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(metad_deposit_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_metad_cv(int num_atoms, int num_graphs, int num_cvs, const int* graph_ptr, const double* x, const int* image,
                                const float* cell, const double* inv_cell, const int* cv_kind, const double* cv_par,
                                const unsigned char* cv_role, const double* cv_weight, double* cv_atom, double* cv_walker,
                                double* values, double* grads, void* stream) {
  const MetadArgs a = mt_cv_only(num_atoms, num_graphs, num_cvs, graph_ptr, x, image, cell, inv_cell, cv_kind, cv_par, cv_role,
                                 cv_weight, cv_atom, cv_walker);
  if (!mt_cv_args_ok(a) || !values || (num_atoms > 0 && !grads)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  mt_launch_cv(a, s);
  hipLaunchKernelGGL(metad_walker_kernel<false>, dim3((unsigned)num_graphs), dim3(256), 0, s, a);
  const int lanes = num_atoms > num_graphs * num_cvs ? num_atoms : num_graphs * num_cvs;
  hipLaunchKernelGGL(metad_report_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, a, values, grads);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twins: the same functions in a CPU loop (all pointers HOST pointers) ----------------------------------------------
extern "C" int hermnet_host_metad_bias(int num_atoms, int num_graphs, int num_cvs, const int* graph_ptr_host, const double* x_host,
                                       const int* image_host, const float* cell_host, const double* inv_cell_host,
                                       const int* cv_kind_host, const double* cv_par_host, const unsigned char* cv_role_host,
                                       const double* cv_weight_host, const double* sigma_par_host, double height, double inv_kt,
                                       long pace, long max_hills, const float* forces_host, const float* energy_host,
                                       const long* total_host, long capacity, const long* state_host, double* cv_atom_host,
                                       double* cv_walker_host, long* hill_count_host, double* hill_centres_host,
                                       double* hill_heights_host, float* forces_b_host, double* bias_forces_host,
                                       double* cv_log_host, long log_steps) {
  const MetadArgs a = {num_atoms, num_graphs, num_graphs > 0 ? num_atoms / num_graphs : 0, num_cvs, graph_ptr_host, x_host,
                       image_host, cell_host, inv_cell_host, cv_kind_host, cv_par_host, cv_role_host, cv_weight_host,
                       sigma_par_host, height, inv_kt, pace, max_hills, forces_host, energy_host, total_host, capacity,
                       state_host, cv_atom_host, cv_walker_host, hill_count_host, hill_centres_host, hill_heights_host,
                       forces_b_host, bias_forces_host, cv_log_host, log_steps};
  if (!mt_args_ok(a) || !mt_host_args_ok(a)) return HN_ERR_BAD_ARG;
  long step;
  const int phase = mt_phase(a, &step);
  if (phase == MT_IDLE) return HN_OK;
  if (phase != MT_VOID) {
    double part[6][256];
    mt_host_cv_pass(a);
    for (int g = 0; g < num_graphs; ++g) mt_walker(a, g, phase, step, true, part);
  }
  for (int i = 0; i < num_atoms; ++i) mt_apply_one(a, i, phase);
  mt_deposit(a, phase, step, 0, 1);
  return HN_OK;
}

extern "C" int hermnet_host_metad_cv(int num_atoms, int num_graphs, int num_cvs, const int* graph_ptr_host, const double* x_host,
                                     const int* image_host, const float* cell_host, const double* inv_cell_host,
                                     const int* cv_kind_host, const double* cv_par_host, const unsigned char* cv_role_host,
                                     const double* cv_weight_host, double* cv_atom_host, double* cv_walker_host,
                                     double* values_host, double* grads_host) {
  const MetadArgs a = mt_cv_only(num_atoms, num_graphs, num_cvs, graph_ptr_host, x_host, image_host, cell_host, inv_cell_host,
                                 cv_kind_host, cv_par_host, cv_role_host, cv_weight_host, cv_atom_host, cv_walker_host);
  if (!mt_cv_args_ok(a) || !values_host || (num_atoms > 0 && !grads_host) || !mt_host_args_ok(a)) return HN_ERR_BAD_ARG;
  double part[6][256];
  mt_host_cv_pass(a);
  for (int g = 0; g < num_graphs; ++g) mt_walker(a, g, MT_PRIME, 0, false, part);
  const int lanes = num_atoms > num_graphs * num_cvs ? num_atoms : num_graphs * num_cvs;
  for (int i = 0; i < lanes; ++i) mt_report_lane(a, i, values_host, grads_host);
  return HN_OK;
}

extern "C" int hermnet_host_metad_exp(long n, const double* a_host, double* out_host) {
  if (n < 0 || (n > 0 && (!a_host || !out_host))) return HN_ERR_BAD_ARG;
  for (long i = 0; i < n; ++i) out_host[i] = mt_exp(a_host[i]);
  return HN_OK;
}
