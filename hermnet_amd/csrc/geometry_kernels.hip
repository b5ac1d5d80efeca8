// gfx950 kernels for the per-step edge geometry and its force back-propagation.
//
//   hermnet_edge_geometry_fwd  <- HVNet.with_edge              /root/reference/HermNet/hermnet.py:133-152
//   hermnet_edge_geometry_bwd  <- autograd of the same w.r.t. pos (callers: plugin/ase_interface/calculator.py:77-83,
//                                 plugin/lmp_interface/lmp_calc.py:50-56)
//   hermnet_edge_geometry_bwd_virial <- the same position gradient plus the per-atom virial
//                                 W_i = -1/2 sum_{e touching i} D_e (x) gD_e (no reference counterpart: DESIGN section 1)
//   hermnet_graph_virial      <- the per-graph sums of those rows, W_b = sum_{i in b} W_i (the stress of a graph), as an
//                                 ordered two-stage reduction
// Both are tiny, HBM-streaming kernels (E * ~50 B); one thread per edge / one wave per atom.
#include <hip/hip_runtime.h>
#include "../../include/hermnet_hip.h"

namespace {

__global__ __launch_bounds__(256) void edge_geometry_fwd_kernel(
    const float* __restrict__ pos, const int* __restrict__ src_id, const int* __restrict__ tgt_id,
    const float* __restrict__ shift, const float* __restrict__ cell, const int* __restrict__ batch,
    int E, float4* __restrict__ edge) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int j = src_id[e], i = tgt_id[e];
  float dx = pos[3 * j + 0] - pos[3 * i + 0];
  float dy = pos[3 * j + 1] - pos[3 * i + 1];
  float dz = pos[3 * j + 2] - pos[3 * i + 2];
  if (shift != nullptr) {
    // einsum('ni,nij->nj', edge_shift, cell[batch[j]])  (hermnet.py:139)
    const float* c = cell + 9 * (batch ? batch[j] : 0);
    const float s0 = shift[3 * e + 0], s1 = shift[3 * e + 1], s2 = shift[3 * e + 2];
    dx += s0 * c[0] + s1 * c[3] + s2 * c[6];
    dy += s0 * c[1] + s1 * c[4] + s2 * c[7];
    dz += s0 * c[2] + s1 * c[5] + s2 * c[8];
  }
  float d = sqrtf(dx * dx + dy * dy + dz * dz);
  // isclose(d, 0, rtol=1e-5, atol=1e-6) -> 1e-6   (hermnet.py:146-147)
  if (fabsf(d) <= 1.0e-6f) d = 1.0e-6f;
  edge[e] = make_float4(dx / d, dy / d, dz / d, d);
}

// gpos[a] = sum_{e in out(a)} gD[e] - sum_{e in in(a)} gD[e]; one wave per atom, lanes over edges.
__global__ __launch_bounds__(256) void edge_geometry_bwd_kernel(
    const float4* __restrict__ gD, const int* __restrict__ in_rowptr, const int* __restrict__ in_edges,
    const int* __restrict__ out_rowptr, const int* __restrict__ out_edges, int N, float* __restrict__ gpos) {
  const int a = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (a >= N) return;
  const int lane = threadIdx.x & 63;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int k = out_rowptr[a] + lane; k < out_rowptr[a + 1]; k += 64) {
    const float4 g = gD[out_edges ? out_edges[k] : k];
    sx += g.x; sy += g.y; sz += g.z;
  }
  for (int k = in_rowptr[a] + lane; k < in_rowptr[a + 1]; k += 64) {
    const float4 g = gD[in_edges ? in_edges[k] : k];
    sx -= g.x; sy -= g.y; sz -= g.z;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sx += __shfl_xor(sx, m, 64);
    sy += __shfl_xor(sy, m, 64);
    sz += __shfl_xor(sz, m, 64);
  }
  if (lane == 0) {
    gpos[3 * a + 0] = sx;
    gpos[3 * a + 1] = sy;
    gpos[3 * a + 2] = sz;
  }
}

// Same sums with the out-edges taken from the CSC order of the relation build (edges by (relation(target),
// row(source))): the out-adjacency of row a is the union of its T CSC segments, so no third edge order is needed.
// Edges whose target has an unknown element are in no segment; they carry no message, hence no gradient.
__global__ __launch_bounds__(256) void edge_geometry_bwd_csc_kernel(
    const float4* __restrict__ gD, const int* __restrict__ in_rowptr, const int* __restrict__ csc_rowptr,
    const int* __restrict__ csc_pos, int T, int N, float* __restrict__ gpos) {
  const int a = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (a >= N) return;
  const int lane = threadIdx.x & 63;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int t = 0; t < T; ++t) {
    const int beg = csc_rowptr[(size_t)t * N + a], end = csc_rowptr[(size_t)t * N + a + 1];
    for (int k = beg + lane; k < end; k += 64) {
      const float4 g = gD[csc_pos[k]];
      sx += g.x; sy += g.y; sz += g.z;
    }
  }
  for (int k = in_rowptr[a] + lane; k < in_rowptr[a + 1]; k += 64) {
    const float4 g = gD[k];
    sx -= g.x; sy -= g.y; sz -= g.z;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sx += __shfl_xor(sx, m, 64);
    sy += __shfl_xor(sy, m, 64);
    sz += __shfl_xor(sz, m, 64);
  }
  if (lane == 0) {
    gpos[3 * a + 0] = sx;
    gpos[3 * a + 1] = sy;
    gpos[3 * a + 2] = sz;
  }
}

// The position gradient of the two kernels above plus the per-atom virial W_a = -1/2 sum_{e touching a} D_e (x) gD_e
// (row-major [a][alpha*3+beta] = D_alpha gD_beta, unsymmetrised): each edge is split equally between its two atoms, an edge
// between an atom and its own periodic image (in both walks of the row) counts fully.  D_e is recomputed with the
// forward kernel's arithmetic (not rhat * d: d is clamped near 0).  Same wave per row, lane-to-edge assignment, walk order
// and xor tree as the gradient-only kernels, so gpos is bit for bit theirs; nine more accumulators alongside.
// CSC: the out-edges from the T CSC segments (edge_geometry_bwd_csc_kernel), else from out_rowptr / out_edges
// (edge_geometry_bwd_kernel with in_edges = NULL).
__device__ __forceinline__ float3 edge_vector(const float* __restrict__ pos, const int* __restrict__ src_id,
                                              const int* __restrict__ tgt_id, const float* __restrict__ shift,
                                              const float* __restrict__ cell, const int* __restrict__ batch, int e) {
  const int j = src_id[e], i = tgt_id[e];
  float dx = pos[3 * j + 0] - pos[3 * i + 0];
  float dy = pos[3 * j + 1] - pos[3 * i + 1];
  float dz = pos[3 * j + 2] - pos[3 * i + 2];
  if (shift != nullptr) {
    const float* c = cell + 9 * (batch ? batch[j] : 0);
    const float s0 = shift[3 * e + 0], s1 = shift[3 * e + 1], s2 = shift[3 * e + 2];
    dx += s0 * c[0] + s1 * c[3] + s2 * c[6];
    dy += s0 * c[1] + s1 * c[4] + s2 * c[7];
    dz += s0 * c[2] + s1 * c[5] + s2 * c[8];
  }
  return make_float3(dx, dy, dz);
}

template <bool CSC>
__global__ __launch_bounds__(256) void edge_geometry_bwd_virial_kernel(
    const float4* __restrict__ gD, const int* __restrict__ in_rowptr, const int* __restrict__ csc_rowptr,
    const int* __restrict__ csc_pos, int T, const int* __restrict__ out_rowptr, const int* __restrict__ out_edges,
    const float* __restrict__ pos, const int* __restrict__ src_id, const int* __restrict__ tgt_id,
    const float* __restrict__ shift, const float* __restrict__ cell, const int* __restrict__ batch, int N,
    float* __restrict__ gpos, float* __restrict__ atom_virial) {
  const int a = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (a >= N) return;
  const int lane = threadIdx.x & 63;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  float w[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) w[q] = 0.f;
  auto virial = [&](int e, const float4 g) {
    const float3 D = edge_vector(pos, src_id, tgt_id, shift, cell, batch, e);
    w[0] += D.x * g.x; w[1] += D.x * g.y; w[2] += D.x * g.z;
    w[3] += D.y * g.x; w[4] += D.y * g.y; w[5] += D.y * g.z;
    w[6] += D.z * g.x; w[7] += D.z * g.y; w[8] += D.z * g.z;
  };
  if (CSC) {
    for (int t = 0; t < T; ++t) {
      const int beg = csc_rowptr[(size_t)t * N + a], end = csc_rowptr[(size_t)t * N + a + 1];
      for (int k = beg + lane; k < end; k += 64) {
        const int e = csc_pos[k];
        const float4 g = gD[e];
        sx += g.x; sy += g.y; sz += g.z;
        virial(e, g);
      }
    }
  } else {
    for (int k = out_rowptr[a] + lane; k < out_rowptr[a + 1]; k += 64) {
      const int e = out_edges ? out_edges[k] : k;
      const float4 g = gD[e];
      sx += g.x; sy += g.y; sz += g.z;
      virial(e, g);
    }
  }
  for (int k = in_rowptr[a] + lane; k < in_rowptr[a + 1]; k += 64) {
    const float4 g = gD[k];
    sx -= g.x; sy -= g.y; sz -= g.z;
    virial(k, g);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sx += __shfl_xor(sx, m, 64);
    sy += __shfl_xor(sy, m, 64);
    sz += __shfl_xor(sz, m, 64);
#pragma unroll
    for (int q = 0; q < 9; ++q) w[q] += __shfl_xor(w[q], m, 64);
  }
  if (lane == 0) {
    gpos[3 * a + 0] = sx;
    gpos[3 * a + 1] = sy;
    gpos[3 * a + 2] = sz;
#pragma unroll
    for (int q = 0; q < 9; ++q) atom_virial[9 * (size_t)a + q] = -0.5f * w[q];
  }
}

// Per-graph virial W_b = sum_{atoms i of graph b} W_i from the rows the kernel above wrote -- two stages, fixed order, no
// atomics.  The atoms are taken in "graph order": position k holds atom perm[k] (perm = stable argsort of batch, NULL =
// identity), so a graph's atoms are one contiguous range of positions and padding rows are never touched.
// Stage 1: one workgroup per fixed chunk of kVirChunk positions -> the chunk's sum (xor tree per wave, waves in order).
// Stage 2: one workgroup per graph: its range [lo, hi) by binary search on batch[perm[.]], then the chunk sums of the
// chunks that lie wholly inside it plus the atoms of the ragged head and tail, strided over the threads in a fixed order.
constexpr int kVirChunk = 256;

__device__ __forceinline__ void virial_block_sum(float (&w)[9], float (*lds)[9]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int q = 0; q < 9; ++q) w[q] += __shfl_xor(w[q], m, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) lds[wave][q] = w[q];
  }
  __syncthreads();
}

__device__ __forceinline__ void virial_add_atom(float (&w)[9], const float* __restrict__ atom_virial,
                                                const long* __restrict__ row_of_node, const long* __restrict__ perm, long k) {
  const long a = perm ? perm[k] : k;
  const float* r = atom_virial + 9 * (size_t)row_of_node[a];
#pragma unroll
  for (int q = 0; q < 9; ++q) w[q] += r[q];
}

__global__ __launch_bounds__(kVirChunk) void graph_virial_chunk_kernel(
    const float* __restrict__ atom_virial, const long* __restrict__ row_of_node, const long* __restrict__ perm, int N,
    float* __restrict__ chunk_sums) {
  __shared__ float lds[kVirChunk / 64][9];
  float w[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) w[q] = 0.f;
  const long k = (long)blockIdx.x * kVirChunk + threadIdx.x;
  if (k < N) virial_add_atom(w, atom_virial, row_of_node, perm, k);
  virial_block_sum(w, lds);
  if (threadIdx.x < 9) {
    float s = lds[0][threadIdx.x];
    for (int v = 1; v < kVirChunk / 64; ++v) s += lds[v][threadIdx.x];
    chunk_sums[9 * (size_t)blockIdx.x + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(kVirChunk) void graph_virial_finish_kernel(
    const float* __restrict__ atom_virial, const long* __restrict__ row_of_node, const long* __restrict__ perm,
    const int* __restrict__ batch, int N, int B, const float* __restrict__ chunk_sums, float* __restrict__ graph_virial) {
  __shared__ float lds[kVirChunk / 64][9];
  __shared__ int range[2];
  const int b = blockIdx.x;
  if (threadIdx.x < 2) {
    // first position whose graph index is >= b (thread 0) / >= b + 1 (thread 1); one graph: everything
    int lo = 0, hi = N;
    if (B > 1) {
      const int want = b + (int)threadIdx.x;
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (batch[perm ? perm[mid] : mid] < want) lo = mid + 1; else hi = mid;
      }
    } else if (threadIdx.x == 1) {
      lo = N;
    }
    range[threadIdx.x] = lo;
  }
  __syncthreads();
  const int lo = range[0], hi = range[1];
  float w[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) w[q] = 0.f;
  int c0 = (lo + kVirChunk - 1) / kVirChunk, c1 = hi / kVirChunk;      // whole chunks inside the range: [c0, c1)
  if (c0 >= c1) { c0 = c1 = 0; }
  const int head_end = c0 < c1 ? c0 * kVirChunk : hi;                  // atoms [lo, head_end) and [tail_beg, hi) singly
  const int tail_beg = c0 < c1 ? c1 * kVirChunk : hi;
  for (int k = lo + (int)threadIdx.x; k < head_end; k += kVirChunk) virial_add_atom(w, atom_virial, row_of_node, perm, k);
  for (int c = c0 + (int)threadIdx.x; c < c1; c += kVirChunk) {
#pragma unroll
    for (int q = 0; q < 9; ++q) w[q] += chunk_sums[9 * (size_t)c + q];
  }
  for (int k = tail_beg + (int)threadIdx.x; k < hi; k += kVirChunk) virial_add_atom(w, atom_virial, row_of_node, perm, k);
  virial_block_sum(w, lds);
  if (threadIdx.x < 9) {
    float s = lds[0][threadIdx.x];
    for (int v = 1; v < kVirChunk / 64; ++v) s += lds[v][threadIdx.x];
    graph_virial[9 * (size_t)b + threadIdx.x] = s;
  }
}

}  // namespace

extern "C" int hermnet_edge_geometry_fwd(const float* pos, const int* src_id, const int* tgt_id,
                                         const float* shift, const float* cell, const int* batch,
                                         int num_edges, float* edge, void* stream) {
  if (num_edges < 0) return HN_ERR_BAD_ARG;
  if (num_edges == 0) return HN_OK;
  if (!pos || !src_id || !tgt_id || !edge) return HN_ERR_BAD_ARG;
  if (shift && !cell) return HN_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int block = 256;
  hipLaunchKernelGGL(edge_geometry_fwd_kernel, dim3((num_edges + block - 1) / block), dim3(block), 0, s,
                     pos, src_id, tgt_id, shift, cell, batch, num_edges, reinterpret_cast<float4*>(edge));
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_edge_geometry_bwd(const float* gD, const int* in_rowptr, const int* in_edges,
                                         const int* out_rowptr, const int* out_edges,
                                         int num_nodes, float* gpos, void* stream) {
  if (num_nodes < 0) return HN_ERR_BAD_ARG;
  if (num_nodes == 0) return HN_OK;
  if (!in_rowptr || !out_rowptr || !gpos) return HN_ERR_BAD_ARG;   // gD may be NULL for an edge-less graph (never read)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int block = 256;  // 4 atoms per block
  hipLaunchKernelGGL(edge_geometry_bwd_kernel, dim3((num_nodes + 3) / 4), dim3(block), 0, s,
                     reinterpret_cast<const float4*>(gD), in_rowptr, in_edges, out_rowptr, out_edges,
                     num_nodes, gpos);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_edge_geometry_bwd_csc(const float* gD, const int* csr_rowptr, const int* csc_rowptr,
                                             const int* csc_pos, int num_rel, int num_nodes, float* gpos,
                                             void* stream) {
  if (num_nodes < 0 || num_rel <= 0) return HN_ERR_BAD_ARG;
  if (num_nodes == 0) return HN_OK;
  if (!csr_rowptr || !csc_rowptr || !gpos) return HN_ERR_BAD_ARG;   // gD / csc_pos may be NULL for an edge-less graph
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(edge_geometry_bwd_csc_kernel, dim3((num_nodes + 3) / 4), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(gD), csr_rowptr, csc_rowptr, csc_pos, num_rel, num_nodes, gpos);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_edge_geometry_bwd_virial(const float* gD, const int* csr_rowptr, const int* csc_rowptr,
                                                const int* csc_pos, int num_rel, const int* out_rowptr,
                                                const int* out_edges, const float* pos, const int* src_id,
                                                const int* tgt_id, const float* shift, const float* cell,
                                                const int* batch, int num_nodes, float* gpos, float* atom_virial,
                                                void* stream) {
  if (num_nodes < 0 || num_rel < 0) return HN_ERR_BAD_ARG;
  const bool csc = csc_rowptr != nullptr, out = out_rowptr != nullptr;
  if (csc == out) return HN_ERR_BAD_ARG;                  // exactly one out-adjacency
  if (csc && num_rel == 0) return HN_ERR_BAD_ARG;
  if (shift && !cell) return HN_ERR_BAD_ARG;
  if (num_nodes == 0) return HN_OK;
  // gD / csc_pos / out_edges / src_id / tgt_id may be NULL for an edge-less graph (never read)
  if (!csr_rowptr || !pos || !gpos || !atom_virial) return HN_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((num_nodes + 3) / 4), block(256);     // 4 atoms per block, one wave each
  if (csc)
    hipLaunchKernelGGL(edge_geometry_bwd_virial_kernel<true>, grid, block, 0, s, reinterpret_cast<const float4*>(gD),
                       csr_rowptr, csc_rowptr, csc_pos, num_rel, nullptr, nullptr, pos, src_id, tgt_id, shift, cell,
                       batch, num_nodes, gpos, atom_virial);
  else
    hipLaunchKernelGGL(edge_geometry_bwd_virial_kernel<false>, grid, block, 0, s, reinterpret_cast<const float4*>(gD),
                       csr_rowptr, nullptr, nullptr, 0, out_rowptr, out_edges, pos, src_id, tgt_id, shift, cell,
                       batch, num_nodes, gpos, atom_virial);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" size_t hermnet_graph_virial_workspace(int num_nodes) {
  const size_t chunks = num_nodes > 0 ? ((size_t)num_nodes + kVirChunk - 1) / kVirChunk : 0;
  return (chunks > 0 ? chunks : 1) * 9 * sizeof(float);
}

extern "C" int hermnet_graph_virial(const float* atom_virial, const long* row_of_node, const long* graph_perm,
                                    const int* batch, int num_nodes, int num_graphs, void* workspace,
                                    size_t workspace_bytes, float* graph_virial, void* stream) {
  if (num_nodes < 0 || num_graphs < 0) return HN_ERR_BAD_ARG;
  if (!graph_virial && num_graphs > 0) return HN_ERR_BAD_ARG;
  if (num_nodes > 0 && (!atom_virial || !row_of_node || !workspace)) return HN_ERR_BAD_ARG;
  if (num_nodes > 0 && num_graphs > 1 && !batch) return HN_ERR_BAD_ARG;
  if (num_nodes > 0 && workspace_bytes < hermnet_graph_virial_workspace(num_nodes)) return HN_ERR_BAD_ARG;
  if (num_graphs == 0 || num_nodes == 0) return HN_OK;     // (no atoms: there are no rows to sum, graph_virial is left alone)
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int chunks = (num_nodes + kVirChunk - 1) / kVirChunk;
  float* sums = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(graph_virial_chunk_kernel, dim3(chunks), dim3(kVirChunk), 0, s, atom_virial, row_of_node, graph_perm,
                     num_nodes, sums);
  hipLaunchKernelGGL(graph_virial_finish_kernel, dim3(num_graphs), dim3(kVirChunk), 0, s, atom_virial, row_of_node,
                     graph_perm, batch, num_nodes, num_graphs, sums, graph_virial);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}
