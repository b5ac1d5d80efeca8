// gfx950: the MD observers behind a resident driver's finish (hermnet_amd/observe.py: Frames, RDF, MSD).  Every `stride`
// committed steps a replay records a frame into a device ring, adds to a species-resolved pair histogram, or appends a row
// of displacement sums -- without leaving the replay.  The definitions, the protocol and the arithmetic are
// observe_step.h's, shared with the host twins at the end of this file.  Two launches per observer: its workers, then the
// one workgroup that alone writes the observer's words.  Contraction is off for the whole file.
//
// The pair histogram is the hot path: all pairs of a graph in float64, 5e7 per sample at 10,000 atoms.  The work list
// (graph, tile_i, tile_j >= tile_i) of 256-atom tiles is made once on the host; one 256-lane workgroup per entry stages tile
// j's fractional coordinates and species in LDS ([component][lane]: a step of the pair loop reads ONE address per wave off
// the diagonal, consecutive ones on it), each lane walks its atom of tile i against them and counts into a uint32 LDS
// histogram [P x bins] (at most 32 KB, beside the bin edges); the nonzero bins are then added to the global int64 counts
// with one integer atomicAdd each.  Integer sums do not depend on their order: the counts are reproducible bit for bit.
// No float atomics.
#include <hip/hip_runtime.h>
#include "observe_step.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void obs_frames_kernel(ObsFramesArgs a) {
  long step;
  if (!obs_due(a.state, a.obs, a.stride, &step)) return;
  obs_frame_lane(a, a.obs[HN_OBS_TAKEN] % a.frames, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(64) void obs_frames_commit_kernel(ObsFramesArgs a) {
  if (threadIdx.x == 0) obs_frames_commit(a);
}

__global__ __launch_bounds__(256) void obs_msd_kernel(ObsMsdArgs a) {
  __shared__ double part[4][256];
  long step;
  if (!obs_due(a.state, a.obs, a.stride, &step)) return;
  obs_msd_group(a, blockIdx.x / a.num_species, blockIdx.x % a.num_species, part);
}

__global__ __launch_bounds__(64) void obs_msd_commit_kernel(ObsMsdArgs a) {
  if (threadIdx.x == 0) obs_msd_commit(a);
}

__global__ __launch_bounds__(256) void obs_rdf_kernel(ObsRdfArgs a) {
  __shared__ double sj[3][HN_OBS_TILE];
  __shared__ int zj[HN_OBS_TILE];
  extern __shared__ double dyn[];                    // edge2 [bins+1] | hist [P x bins] uint32
  long step;
  if (!obs_due(a.state, a.obs, a.stride, &step)) return;
  const int g = a.work[3 * blockIdx.x], ti = a.work[3 * blockIdx.x + 1], tj = a.work[3 * blockIdx.x + 2];
  if (g < 0 || g >= a.num_graphs || ti < 0 || tj < ti || !obs_rdf_graph_ok(a, g)) return;
  double* edge2 = dyn;
  uint32_t* hist = (uint32_t*)(dyn + a.bins + 1);
  const int cells = obs_num_pairs(a.num_species) * a.bins, l = threadIdx.x;
  for (int k = l; k <= a.bins; k += 256) edge2[k] = a.edge2[k];
  for (int k = l; k < cells; k += 256) hist[k] = 0u;
  obs_rdf_stage(a, g, tj, l, sj, zj);
  __syncthreads();
  obs_rdf_lane(a, g, ti, tj, l, sj, zj, edge2, hist);
  __syncthreads();
  unsigned long long* out = (unsigned long long*)a.counts + (size_t)obs_rdf_slot(a, g) * cells;
  for (int k = l; k < cells; k += 256)
    if (hist[k] != 0u) atomicAdd(out + k, (unsigned long long)hist[k]);
}

__global__ __launch_bounds__(64) void obs_rdf_commit_kernel(ObsRdfArgs a) {
  if (threadIdx.x == 0) obs_rdf_commit(a);
}

size_t obs_rdf_lds(const ObsRdfArgs& a) {
  return sizeof(double) * (size_t)(a.bins + 1) + sizeof(uint32_t) * (size_t)obs_num_pairs(a.num_species) * a.bins;
}

// What the host twin can check and the device entry point cannot: the work list names tiles of graphs that exist.
bool obs_rdf_work_ok(const ObsRdfArgs& a) {
  for (int w = 0; w < a.num_work; ++w) {
    const int g = a.work[3 * w], ti = a.work[3 * w + 1], tj = a.work[3 * w + 2];
    if (g < 0 || g >= a.num_graphs || ti < 0 || tj < ti) return false;
  }
  return true;
}

}  // namespace

extern "C" int hermnet_observe_frames(int num_atoms, int num_graphs, long stride, long frames, const double* x, const double* v,
                                      const int* image, const float* cell, const long* state, long* obs, long* steps,
                                      float* positions, float* velocities, int* images, float* cells, void* stream) {
  const ObsFramesArgs a = {num_atoms, num_graphs, stride, frames, x, v, image, cell, state, obs, steps, positions, velocities,
                           images, cells};
  if (!obs_frames_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(obs_frames_kernel, dim3((unsigned)((obs_frames_lanes(a) + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(obs_frames_commit_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_observe_msd(int num_atoms, int num_graphs, int num_species, long stride, long rows, const int* graph_ptr,
                                   const int* species, const double* x, const int* image, const float* cell, const long* state,
                                   long* obs, long* steps, double* x_origin, int* image_origin, double* sums, void* stream) {
  const ObsMsdArgs a = {num_atoms, num_graphs, num_species, stride, rows, graph_ptr, species, x, image, cell, state, obs, steps,
                        x_origin, image_origin, sums};
  if (!obs_msd_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(obs_msd_kernel, dim3((unsigned)(num_graphs * num_species)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(obs_msd_commit_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_observe_rdf(int num_atoms, int num_graphs, int num_species, int bins, long slots, long stride,
                                   double r_max2, const int* graph_ptr, const int* species, const double* x, const float* cell,
                                   const double* inv_cell, const long* slot_of, const double* edge2, const int* work,
                                   int num_work, const long* state, long* obs, long* counts, long* samples, long* skipped,
                                   double* volume_sum, void* stream) {
  const ObsRdfArgs a = {num_atoms, num_graphs, num_species, bins, slots, stride, r_max2,
                        r_max2 > 0.0 ? (float)((double)bins / sqrt(r_max2)) : 0.0f, graph_ptr, species, x, cell, inv_cell, slot_of,
                        edge2, work, num_work, state, obs, counts, samples, skipped, volume_sum};
  if (!obs_rdf_args_ok(a)) return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (num_work > 0) hipLaunchKernelGGL(obs_rdf_kernel, dim3((unsigned)num_work), dim3(256), obs_rdf_lds(a), s, a);
  hipLaunchKernelGGL(obs_rdf_commit_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

// ---- host twins: the same functions in a CPU loop (all pointers HOST pointers) ----------------------------------------------
extern "C" int hermnet_host_observe_frames(int num_atoms, int num_graphs, long stride, long frames, const double* x_host,
                                           const double* v_host, const int* image_host, const float* cell_host,
                                           const long* state_host, long* obs_host, long* steps_host, float* positions_host,
                                           float* velocities_host, int* images_host, float* cells_host) {
  const ObsFramesArgs a = {num_atoms, num_graphs, stride, frames, x_host, v_host, image_host, cell_host, state_host, obs_host,
                           steps_host, positions_host, velocities_host, images_host, cells_host};
  if (!obs_frames_args_ok(a)) return HN_ERR_BAD_ARG;
  long step;
  if (obs_due(a.state, a.obs, a.stride, &step))
    for (int i = 0; i < obs_frames_lanes(a); ++i) obs_frame_lane(a, a.obs[HN_OBS_TAKEN] % a.frames, i);
  obs_frames_commit(a);
  return HN_OK;
}

extern "C" int hermnet_host_observe_msd(int num_atoms, int num_graphs, int num_species, long stride, long rows,
                                        const int* graph_ptr_host, const int* species_host, const double* x_host,
                                        const int* image_host, const float* cell_host, const long* state_host, long* obs_host,
                                        long* steps_host, double* x_origin_host, int* image_origin_host, double* sums_host) {
  const ObsMsdArgs a = {num_atoms, num_graphs, num_species, stride, rows, graph_ptr_host, species_host, x_host, image_host,
                        cell_host, state_host, obs_host, steps_host, x_origin_host, image_origin_host, sums_host};
  if (!obs_msd_args_ok(a)) return HN_ERR_BAD_ARG;
  long step;
  if (obs_due(a.state, a.obs, a.stride, &step)) {
    double part[4][256];
    for (int w = 0; w < num_graphs * num_species; ++w) obs_msd_group(a, w / num_species, w % num_species, part);
  }
  obs_msd_commit(a);
  return HN_OK;
}

extern "C" int hermnet_host_observe_rdf(int num_atoms, int num_graphs, int num_species, int bins, long slots, long stride,
                                        double r_max2, const int* graph_ptr_host, const int* species_host, const double* x_host,
                                        const float* cell_host, const double* inv_cell_host, const long* slot_of_host,
                                        const double* edge2_host, const int* work_host, int num_work, const long* state_host,
                                        long* obs_host, long* counts_host, long* samples_host, long* skipped_host,
                                        double* volume_sum_host) {
  const ObsRdfArgs a = {num_atoms, num_graphs, num_species, bins, slots, stride, r_max2,
                        r_max2 > 0.0 ? (float)((double)bins / sqrt(r_max2)) : 0.0f, graph_ptr_host, species_host, x_host, cell_host,
                        inv_cell_host, slot_of_host, edge2_host, work_host, num_work, state_host, obs_host, counts_host,
                        samples_host, skipped_host, volume_sum_host};
  if (!obs_rdf_args_ok(a) || !obs_rdf_work_ok(a)) return HN_ERR_BAD_ARG;
  long step;
  if (obs_due(a.state, a.obs, a.stride, &step)) {
    const int cells = obs_num_pairs(num_species) * bins;
    static thread_local double sj[3][HN_OBS_TILE];
    static thread_local int zj[HN_OBS_TILE];
    static thread_local uint32_t hist[HN_OBS_RDF_MAX_HIST];
    for (int w = 0; w < num_work; ++w) {
      const int g = a.work[3 * w], ti = a.work[3 * w + 1], tj = a.work[3 * w + 2];
      if (!obs_rdf_graph_ok(a, g)) continue;
      for (int k = 0; k < cells; ++k) hist[k] = 0u;
      for (int l = 0; l < HN_OBS_TILE; ++l) obs_rdf_stage(a, g, tj, l, sj, zj);
      for (int l = 0; l < HN_OBS_TILE; ++l) obs_rdf_lane(a, g, ti, tj, l, sj, zj, a.edge2, hist);
      long* out = a.counts + (size_t)obs_rdf_slot(a, g) * cells;
      for (int k = 0; k < cells; ++k) out[k] += (long)hist[k];
    }
  }
  obs_rdf_commit(a);
  return HN_OK;
}
