// gfx950 device-side construction of the relation-ordered graph: the build's replacement for
// `in_subgraph` (HermNet/utils.py:11-24, called per relation per layer at hermnet.py:52-54).
// Instead of N_t O(E) scans per relation per layer, the edge list is grouped per neighbour list by
// counting sort (claim -> scan -> place -> per-group rank sort; identical to a stable sort by key,
// deterministic) -- no host sync, everything int32.  Per list: 7 launches (zero, claim of both keys,
// block sums, scan + row pointers, CSR placement + row_active, CSR rank sort + per-edge arrays + CSC
// placement, CSC rank sort), 5 more for the optional out-adjacency, 6 once per atom set for the rows.
// The only atomics are the claims: one per distinct key per wave, value-returning, so that the
// placements are plain stores.  configs[1] (E = 431,340): 74 us per list (141 us with a histogram and two
// cursor scatters of one atomic per lane each, and one wave per group re-reading it from memory); the claim
// of row(target) on a source-grouped list (22 us: 431k one-per-lane atomics at the memory side's request
// rate) and the CSR rank sort's gathers by edge id (23 us) are what is left (profiles/relation_build_trace.md).
//
// Orders produced (see include/hermnet_hip.h):
//   rows : atoms sorted by (relation, id), each relation's block starting at row_start[t]
//   CSR  : edges by (row(target), edge id)
//   CSC  : edges by (relation(target), row(source), CSR position)
//   out  : CSR positions by row(source)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/hermnet_hip.h"

#include "scan_i32.h"

namespace {

constexpr int kBlock = 256;
inline dim3 grid_for(long n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

__device__ __forceinline__ int relation_of(long z, const int* __restrict__ zlist, int T) {
  for (int t = 0; t < T; ++t)
    if ((long)zlist[t] == z) return t;     // first matching element; T = "not in elems" (hermnet.py:53)
  return T;
}

__global__ __launch_bounds__(kBlock) void count_relations_kernel(const long* __restrict__ z, int NA,
                                                                const int* __restrict__ zlist, int T,
                                                                int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < NA) atomicAdd(&counts[relation_of(z[i], zlist, T)], 1);   // integer atomics: exact, order-free
}

__global__ __launch_bounds__(kBlock) void atom_keys_kernel(const long* __restrict__ z, int NA,
                                                          const int* __restrict__ zlist, int T,
                                                          unsigned* __restrict__ key, int* __restrict__ val) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < NA) { key[i] = (unsigned)relation_of(z[i], zlist, T); val[i] = i; }
}

// sorted position p -> row = p - first_sorted[rel] + row_start[rel]
__global__ __launch_bounds__(kBlock) void assign_rows_kernel(
    const unsigned* __restrict__ rel_sorted, const int* __restrict__ node_order, int NA,
    const int* __restrict__ row_start, int T, const long* __restrict__ z, int* __restrict__ row_of_node,
    int* __restrict__ z_rows, float* __restrict__ row_real) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= NA) return;
  const int rel = (int)rel_sorted[p];
  // first sorted position of this relation = number of sorted entries with a smaller relation:
  // binary search on the sorted relation list
  int lo = 0, hi = NA;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int)rel_sorted[mid] < rel) lo = mid + 1; else hi = mid; }
  const int atom = node_order[p];
  const int row = p - lo + row_start[rel];
  row_of_node[atom] = row;
  z_rows[row] = (int)z[atom];
  row_real[row] = 1.0f;
}

__device__ __forceinline__ int relation_of_row(int row, const int* __restrict__ row_start, int T) {
  int t = 0;
  while (t < T && row >= row_start[t + 1]) ++t;   // row_start[T] = first unknown row
  return t;
}


// ---- grouping by key without a global sort -------------------------------------------------------
// "Group the indices 0..n-1 by key[i], ascending index inside a group" is what every edge order
// needs (keys: row(target) | relation(target)*N + row(source) | row(source)).  A counting sort does it
// in O(n): every entry CLAIMS a place in its key's counter (integer atomics; the value the atomic returns
// is the entry's arrival number inside its group, so the histogram pass is the only pass with atomics),
// exclusive scan, placement at rowptr[key] + arrival number with plain stores (order inside a group
// arbitrary), then a rank sort of every group (groups are neighbour lists: tens of entries).
// The result is deterministic and identical to a stable sort by key.

// Arrival number of this lane's entry in counters[key]: the lanes of the wave that hold the same key elect their
// lowest lane, which adds their count with ONE atomic; the others take base + rank among equals.  Atomics run at the
// memory side at a fixed request rate, and requests to one address serialise, so a wave pays per distinct key: ~2 for
// the grouped key of a neighbour list, one for all the NULL edges of a padded list, 64 for a key that the list is not
// grouped by (or for an ungrouped list).  Every lane of the wave must call this (`valid` = the lane has an entry).
__device__ __forceinline__ int wave_claim(int* __restrict__ counters, int key, bool valid) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid), mine = 0;
  while (todo) {                                             // one turn per distinct key of the wave
    const int k = __builtin_amdgcn_readlane(key, __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1));
    const bool eq = valid && key == k;
    const unsigned long long m = __ballot(eq);
    if (eq) mine = m;
    todo &= ~m;
  }
  const int leader = valid ? __ffsll((long long)mine) - 1 : lane;
  int base = 0;
  if (valid && lane == leader) base = atomicAdd(&counters[key], __popcll(mine));
  base = __shfl(base, leader, 64);
  return base + __popcll(mine & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBlock) void claim_kernel(const int* __restrict__ key, int n, int* __restrict__ counters,
                                                      int* __restrict__ arrival) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  const int a = wave_claim(counters, valid ? key[i] : 0, valid);
  if (valid) arrival[i] = a;
}

// What the HVNet build hangs on its placement launch (both optional):
//   tail : the CSR positions behind the last row -- the NULL edges of a padded list -- get benign values (atom 0 onto
//          itself, no shift): the edge-parallel kernels (geometry, radial table) may compute on them, nothing reads the results
//   rows : row_active = real row of a relation that receives >= 1 edge (hermnet.py:56-57), or the caller's override
struct PlaceExtras {
  int E;                                // tail: positions [real_end[0], E); 0 = no tail fill
  const int* real_end;                  // &csr_rowptr[N] = number of real edges
  int *csr_src, *src_id, *tgt_id, *rt_csr;
  float* shift_csr;                     // or nullptr
  int N, T;                             // rows: N = 0 = none
  const int *csc_rowptr, *row_start;
  const unsigned char* rel_active;
  const float* row_real;
  float* row_active;
};

__device__ __forceinline__ void row_active_of(int r, const int* __restrict__ csc_rowptr, const int* __restrict__ row_start,
                                              int N, int T, const unsigned char* __restrict__ rel_active,
                                              const float* __restrict__ row_real, float* __restrict__ row_active) {
  const int t = relation_of_row(r, row_start, T);
  float on = 0.0f;
  if (t < T) {
    const bool act = rel_active ? rel_active[t] != 0
                                : (csc_rowptr[(size_t)(t + 1) * N] - csc_rowptr[(size_t)t * N]) > 0;
    on = act ? row_real[r] : 0.0f;
  }
  row_active[r] = on;
}

// (the build without edges launches no placement)
__global__ __launch_bounds__(kBlock) void row_active_kernel(const int* __restrict__ csc_rowptr,
                                                           const int* __restrict__ row_start, int N, int T,
                                                           const unsigned char* __restrict__ rel_active,
                                                           const float* __restrict__ row_real,
                                                           float* __restrict__ row_active) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < N) row_active_of(r, csc_rowptr, row_start, N, T, rel_active, row_real, row_active);
}

// slots[rowptr[key[i]] + arrival[i]] = i: the scatter of the counting sort, without atomics
__global__ __launch_bounds__(kBlock) void place_kernel(const int* __restrict__ key, const int* __restrict__ arrival, int n,
                                                      const int* __restrict__ rowptr, int* __restrict__ slots,
                                                      PlaceExtras x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) slots[rowptr[key[i]] + arrival[i]] = i;
  if (i < x.E && i >= x.real_end[0]) {
    x.csr_src[i] = 0; x.src_id[i] = 0; x.tgt_id[i] = 0; x.rt_csr[i] = 0;
    if (x.shift_csr != nullptr) { x.shift_csr[3 * i + 0] = 0.f; x.shift_csr[3 * i + 1] = 0.f; x.shift_csr[3 * i + 2] = 0.f; }
  }
  if (i < x.N) row_active_of(i, x.csc_rowptr, x.row_start, x.N, x.T, x.rel_active, x.row_real, x.row_active);
}

// ---- rank sort of every group: emit(rowptr[g] + rank(v), v, g), rank = number of smaller members (members are unique).
// Four consecutive groups (a quad) share a wave when they are small: 16-lane quarters for groups of <= 16 members, two
// turns of 32-lane halves for <= 32, otherwise the whole wave per group (in 64-member pieces beyond that).  Every member
// sits in a register and is compared through cross-lane reads: a group of <= 64 members is read from memory once.
// `waves_per_quad` 1: one wave takes all the turns of its quad (small groups: a quarter of the waves); 4: a wave per
// group, of which only the needed ones work (large groups: the turns run side by side).  The host picks by n / ngroups;
// either is correct for any sizes.  Group g = [rowptr[g] - off, rowptr[g + 1] - off) of `slots`.
// `fetch(v, g)` loads what `emit(pos, v, g, fetched)` will store: issued before the comparisons, whose cross-lane reads hide
// the latency of those gathers.
template <class Fetch, class Emit>
__device__ __forceinline__ void rank_sort_groups(const int* __restrict__ rowptr, int off, int ngroups, int waves_per_quad,
                                                 const int* __restrict__ slots, Fetch fetch, Emit emit) {
  const int wave = blockIdx.x * (kBlock >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int quad = wave / waves_per_quad, sub = wave - quad * waves_per_quad;
  const int g0 = quad * 4;
  if (g0 >= ngroups) return;
  // the five boundaries of the quad, read once: quarter q of the wave holds the ones of group g0 + q
  const int lo = rowptr[min(g0 + (lane >> 4), ngroups)] - off, hi = rowptr[min(g0 + (lane >> 4) + 1, ngroups)] - off;
  const int b0 = __builtin_amdgcn_readlane(lo, 0), b1 = __builtin_amdgcn_readlane(lo, 16), b2 = __builtin_amdgcn_readlane(lo, 32),
            b3 = __builtin_amdgcn_readlane(lo, 48), b4 = __builtin_amdgcn_readlane(hi, 48);   // (equal behind the last group)
  const int nmax = max(max(b1 - b0, b2 - b1), max(b3 - b2, b4 - b3));
  const int W = nmax <= 16 ? 16 : (nmax <= 32 ? 32 : 64);     // lanes per group (wave-uniform)
  const int wsh = W == 16 ? 4 : (W == 32 ? 5 : 6);
  const int per = 64 >> wsh, turns = 4 / per;
  const int first = lane & ~(W - 1), li = lane - first;
  for (int turn = sub; turn < turns; turn += waves_per_quad) {
    const int q = turn * per + (lane >> wsh);
    const int g = g0 + q;
    const int beg = q == 0 ? b0 : (q == 1 ? b1 : (q == 2 ? b2 : b3));
    const int n = (q == 0 ? b1 : (q == 1 ? b2 : (q == 2 ? b3 : b4))) - beg;     // 0 behind the last group
    // the largest group of this turn bounds the loops for the whole wave
    const int nm = max(max(__builtin_amdgcn_readlane(n, 0), __builtin_amdgcn_readlane(n, 16)),
                       max(__builtin_amdgcn_readlane(n, 32), __builtin_amdgcn_readlane(n, 48)));
    for (int a0 = 0; a0 < nm; a0 += W) {                      // (W = 64 whenever nm > W)
      const bool has = a0 + li < n;
      const int v = has ? slots[beg + a0 + li] : 0x7FFFFFFF;  // (no member is as large: never counted as smaller)
      decltype(fetch(0, 0)) got = {};
      if (has) got = fetch(v, g);
      int rank = 0;
      for (int c0 = 0; c0 < nm; c0 += W) {
        const int w = c0 == a0 ? v : (c0 + li < n ? slots[beg + c0 + li] : 0x7FFFFFFF);
        // eight reads in flight; the lanes behind the last member hold the sentinel, and first + j stays inside the group's lanes
        const int cnt = min(W, (nm - c0 + 7) & ~7);
        for (int j = 0; j < cnt; j += 8) {
#pragma unroll
          for (int u = 0; u < 8; ++u) rank += __shfl(w, first + j + u, 64) < v ? 1 : 0;
        }
      }
      if (has) emit(beg + rank, v, g, got);
    }
  }
}

inline dim3 rank_sort_grid(long ngroups, int waves_per_quad) {
  const long waves = (ngroups + 3) / 4 * waves_per_quad;
  return dim3((unsigned)((waves + (kBlock >> 6) - 1) / (kBlock >> 6)));
}
inline int rank_sort_waves_per_quad(long n, long ngroups) { return n > 16 * ngroups ? 4 : 1; }

__global__ __launch_bounds__(kBlock) void group_rank_sort_kernel(const int* __restrict__ rowptr, int ngroups, int waves_per_quad,
                                                                const int* __restrict__ slots, int* __restrict__ out) {
  rank_sort_groups(rowptr, 0, ngroups, waves_per_quad, slots, [](int, int) { return 0; },
                   [=](int pos, int v, int, int) { out[pos] = v; });
}

// Zero fill and copy as kernels, not hipMemsetAsync / hipMemcpyAsync: under hipGraph replay (ROCm 7.2) the captured
// memset nodes of this build did not survive eager memsets issued between two replays -- the second replay left the
// histogram un-zeroed (bisected with tools/graph_probe.py: garbage row pointers, then an out-of-bounds rank sort).
__global__ __launch_bounds__(kBlock) void zero_i32_kernel(int* __restrict__ dst, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = 0;
}

__global__ __launch_bounds__(kBlock) void iota_scaled_kernel(int* __restrict__ dst, int n, int scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = i * scale;
}

struct GroupWork {
  int* counters;    // [max keys + 1]
  int* arrival;     // [n]
  int* slots;       // [n]
  void* scan_temp;
  size_t scan_bytes;
};

// rowptr [nkeys+1], out [n]
int group_by_key(const int* key, int n, int nkeys, int* rowptr, int* out, const GroupWork& w, hipStream_t s) {
  hipLaunchKernelGGL(zero_i32_kernel, grid_for((long)nkeys + 1), dim3(kBlock), 0, s, w.counters, (long)nkeys + 1);
  if (n > 0) hipLaunchKernelGGL(claim_kernel, grid_for(n), dim3(kBlock), 0, s, key, n, w.counters, w.arrival);
  if (exclusive_scan_i32(w.counters, rowptr, nkeys + 1, w.scan_temp, w.scan_bytes, s) != HN_OK) return HN_ERR_LAUNCH;
  if (n == 0) return HN_OK;
  PlaceExtras none = {};
  hipLaunchKernelGGL(place_kernel, grid_for(n), dim3(kBlock), 0, s, key, w.arrival, n, rowptr, w.slots, none);
  const int wpq = rank_sort_waves_per_quad(n, nkeys);
  hipLaunchKernelGGL(group_rank_sort_kernel, rank_sort_grid(nkeys, wpq), dim3(kBlock), 0, s, rowptr, nkeys, wpq, w.slots, out);
  return HN_OK;
}

// ---- fused edge orders: both claims in one pass over the edge list, ONE scan over the concatenated counters
// [ row(target) : N + 1 | relation(target) * N + row(source) : (T + 1) N + 1 ], the CSR-ordered arrays and the CSC
// placement inside the CSR rank sort, csc_tgt inside the CSC rank sort: 7 launches for the (bit-identical) orders.
__global__ __launch_bounds__(kBlock) void edge_claim_kernel(const long* __restrict__ edge_index, int E,
                                                           const int* __restrict__ row_of_node,
                                                           const int* __restrict__ row_start, int T, int N, int NA,
                                                           int* __restrict__ key1, int* __restrict__ arrival1,
                                                           int* __restrict__ arrival2, int* __restrict__ counters) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = e < E;
  // A NULL edge of a padded list (hermnet_neighbor_fill_padded) goes to the counters' closing slots -- row N of the CSR
  // counters, key (T+1) N of the CSC ones -- so that it lands behind every row and in no segment.  An endpoint outside
  // [0, NA) is not followed: the edge is filed as a NULL edge -- a damaged list gives a wrong energy, never an
  // out-of-bounds read or counter.
  int k1 = N, k2 = (T + 1) * N;
  if (valid) {
    const long tgt = edge_index[(size_t)E + e], src = edge_index[e];
    if (src >= 0 && src < NA && tgt >= 0 && tgt < NA) {
      const int rs = row_of_node[src];
      k1 = row_of_node[tgt];
      k2 = relation_of_row(k1, row_start, T) * N + rs;          // == T*N + rs for unknown-element targets
    }
  }
  const int a1 = wave_claim(counters, k1, valid);
  const int a2 = wave_claim(counters + N + 1, k2, valid);
  if (valid) { key1[e] = k1; arrival1[e] = a1; arrival2[e] = a2; }
}

// scan_apply for the concatenated counters [ n1 + 1 | n2 + ... ]: the running offsets go to `all` (where the placements
// look their groups up) and, in their final form, straight to csr_rowptr [n1 + 1] and csc_rowptr [n2 + 1] (second part:
// minus the E edges in front).  HVNet: n1 = N, n2 = T N; HTNet: n1 = target rows, n2 = relations x source rows.
// `sums_are_totals`: `sums` holds the raw block totals and every block adds up the ones in front of it -- the launch
// between the block sums and this one saved, for the few hundred blocks of a build.
__global__ __launch_bounds__(kBlock) void scan_apply_orders_kernel(const int* __restrict__ in, int n, const int* __restrict__ sums,
                                                                  int sums_are_totals, int* __restrict__ all, int n1, long n2,
                                                                  int E, int* __restrict__ csr_rowptr, int* __restrict__ csc_rowptr) {
  __shared__ int lds[4];
  const int base = blockIdx.x * kScanTile + threadIdx.x * 4;
  int x[4], v = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) { x[q] = (base + q < n) ? in[base + q] : 0; v += x[q]; }
  int total;
  int run = block_exclusive_scan(v, lds, total);
  if (sums_are_totals) {
    int front = 0, before;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += kBlock) front += sums[b];
    (void)block_exclusive_scan(front, lds, before);
    run += before;
  } else {
    run += sums[blockIdx.x];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = base + q;
    if (i < n) {
      all[i] = run;
      if (i <= n1) csr_rowptr[i] = run;
      else if (i - (n1 + 1) <= n2) csc_rowptr[i - (n1 + 1)] = run - E;
    }
    run += x[q];
  }
}

constexpr int kScanFusedBlocks = 2048;     // beyond: the scan of the block sums gets its own launch back

int scan_orders(const int* counters, int n, void* temp, size_t temp_bytes, int* all, int n1, long n2, int E,
                int* csr_rowptr, int* csc_rowptr, hipStream_t s) {
  const int nb = (n + kScanTile - 1) / kScanTile;
  int* sums = reinterpret_cast<int*>(temp);
  if (temp_bytes < scan_temp_bytes(n)) return HN_ERR_BAD_ARG;
  const int fused = nb <= kScanFusedBlocks ? 1 : 0;
  hipLaunchKernelGGL(scan_block_sums_kernel, dim3(nb), dim3(kBlock), 0, s, counters, n, sums);
  if (!fused) hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kBlock), 0, s, sums, nb);
  hipLaunchKernelGGL(scan_apply_orders_kernel, dim3(nb), dim3(kBlock), 0, s, counters, n, sums, fused, all, n1, n2, E,
                     csr_rowptr, csc_rowptr);
  return HN_OK;
}

// What the CSR rank sort does with a sorted member: the CSR-ordered per-edge arrays, and the placement of the CSR
// position in its CSC group (rp2 = the second part of the scanned counters, E in front).
struct CsrEmitArgs {
  const long* edge_index;
  const float* shift;         // or nullptr
  int E;
  const int* row_of_node;
  const int* arrival2;
  const int* rp2;
  int *csr_perm, *csr_src, *src_id, *tgt_id, *rt_csr, *slots2;
  float* shift_csr;
};

struct CsrFetched { int s, t, rs, arrival; float sh[3]; };

__device__ __forceinline__ CsrFetched csr_fetch(const CsrEmitArgs& a, int e, int stride, int x) {
  CsrFetched f;
  f.s = (int)a.edge_index[e];
  f.t = (int)a.edge_index[(size_t)stride + e];
  f.arrival = a.arrival2[x];
  if (a.shift != nullptr) { f.sh[0] = a.shift[3 * e + 0]; f.sh[1] = a.shift[3 * e + 1]; f.sh[2] = a.shift[3 * e + 2]; }
  f.rs = a.row_of_node[f.s];
  return f;
}

__device__ __forceinline__ void csr_emit(const CsrEmitArgs& a, int k, int e, const CsrFetched& f, int rt, int k2) {
  a.csr_perm[k] = e;
  a.csr_src[k] = f.rs;
  a.src_id[k] = f.s;
  a.tgt_id[k] = f.t;
  a.rt_csr[k] = rt;
  if (a.shift != nullptr) {
    a.shift_csr[3 * k + 0] = f.sh[0];
    a.shift_csr[3 * k + 1] = f.sh[1];
    a.shift_csr[3 * k + 2] = f.sh[2];
  }
  a.slots2[a.rp2[k2] - a.E + f.arrival] = k;
}

// CSR: edges grouped by row(target), ascending edge id inside a row
__global__ __launch_bounds__(kBlock) void csr_rank_sort_kernel(const int* __restrict__ rowptr, int N, int waves_per_quad,
                                                              const int* __restrict__ slots, CsrEmitArgs a,
                                                              const int* __restrict__ row_start, int T) {
  rank_sort_groups(rowptr, 0, N, waves_per_quad, slots, [=](int e, int) { return csr_fetch(a, e, a.E, e); },
                   [=](int k, int e, int rt, const CsrFetched& f) {
                     csr_emit(a, k, e, f, rt, relation_of_row(rt, row_start, T) * N + f.rs);
                   });
}

// rank sort of the CSC groups (group g = [rp[g] - E, rp[g+1] - E) of the concatenated scan) + csc_tgt
__global__ __launch_bounds__(kBlock) void csc_rank_sort_kernel(const int* __restrict__ rp2, int E, int ngroups, int waves_per_quad,
                                                              const int* __restrict__ slots, const int* __restrict__ rt_csr,
                                                              int* __restrict__ csc_pos, int* __restrict__ csc_tgt) {
  rank_sort_groups(rp2, E, ngroups, waves_per_quad, slots, [=](int v, int) { return rt_csr[v]; },
                   [=](int pos, int v, int, int rt) {
                     csc_pos[pos] = v;
                     csc_tgt[pos] = rt;
                   });
}

// ---- HTNet (round 3): the triadic relation orders with the same counting sort.  Relation (c; {p, q}) = centre element c,
// unordered pair of neighbour elements; P = T (T + 1) / 2 pairs, enumerated p-major (k(p, q) = p T - p (p - 1) / 2 + q - p).
// A directed edge j -> i is listed once for every pair that contains element(j): expanded edge x = e T + m stands for the
// pair {element(j), m}.  SOURCE rows: the atoms in (element, id) order, blocks of B rows (Ns rows); TARGET rows: block
// (c P + k) B + (position of i inside its element), one block per relation.  All atoms must be of listed elements.
struct TriMap { int T, P, B, Ns; };

__device__ __forceinline__ void tri_keys(const TriMap& m, int rs, int rt, int mm, int& vt, int& k2) {
  const int a = rs / m.B, c = rt / m.B, loc = rt - c * m.B;
  const int p = a < mm ? a : mm, q = a < mm ? mm : a;
  const int rel = c * m.P + p * m.T - p * (p - 1) / 2 + (q - p);
  vt = rel * m.B + loc;
  k2 = rel * m.Ns + rs;
}

__global__ __launch_bounds__(kBlock) void tri_claim_kernel(const long* __restrict__ edge_index, int E0, TriMap m,
                                                          const int* __restrict__ row_of_node, int Nt,
                                                          int* __restrict__ key1, int* __restrict__ arrival1,
                                                          int* __restrict__ arrival2, int* __restrict__ counters) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = x < E0 * m.T;
  int vt = 0, k2 = 0;
  if (valid) {
    const int e = x / m.T;
    tri_keys(m, row_of_node[edge_index[e]], row_of_node[edge_index[(size_t)E0 + e]], x - e * m.T, vt, k2);
  }
  const int a1 = wave_claim(counters, vt, valid);
  const int a2 = wave_claim(counters + Nt + 1, k2, valid);
  if (valid) { key1[x] = vt; arrival1[x] = a1; arrival2[x] = a2; }
}

// CSR of the expanded list: members are expanded edges x, csr_perm = ORIGINAL edge id
__global__ __launch_bounds__(kBlock) void tri_rank_sort_kernel(const int* __restrict__ rowptr, int Nt, int waves_per_quad,
                                                              const int* __restrict__ slots, CsrEmitArgs a, int E0, TriMap m) {
  rank_sort_groups(rowptr, 0, Nt, waves_per_quad, slots, [=](int x, int) { return csr_fetch(a, x / m.T, E0, x); },
                   [=](int k, int x, int, const CsrFetched& f) {
                     const int e = x / m.T;
                     int vt, k2;
                     tri_keys(m, f.rs, a.row_of_node[f.t], x - e * m.T, vt, k2);
                     csr_emit(a, k, e, f, vt, k2);
                   });
}

// target rows: real = the atom exists; active = its relation has at least one edge (hermnet.py:56-57); res_row = the
// atom's own source row (residual, rmnet.py:24-26)
__global__ __launch_bounds__(kBlock) void tri_rows_kernel(TriMap m, int Nt, const int* __restrict__ elem_counts,
                                                         const int* __restrict__ csr_rowptr,
                                                         const unsigned char* __restrict__ rel_active,
                                                         float* __restrict__ row_real, float* __restrict__ row_active,
                                                         int* __restrict__ res_row) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= Nt) return;
  const int rel = r / m.B, loc = r - rel * m.B, el = rel / m.P;
  const float real = loc < elem_counts[el] ? 1.0f : 0.0f;
  row_real[r] = real;
  const bool act = rel_active ? rel_active[rel] != 0 : (csr_rowptr[(rel + 1) * m.B] - csr_rowptr[rel * m.B]) > 0;
  row_active[r] = act ? real : 0.0f;
  res_row[r] = el * m.B + loc;
}

int bits_for(unsigned max_key_exclusive) {
  int b = 1;
  while (b < 32 && (1u << b) < max_key_exclusive) ++b;
  return b;
}

size_t sort_temp_bytes(int n) {
  size_t bytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned*)nullptr, (unsigned*)nullptr,
                                           (const int*)nullptr, (int*)nullptr, n, 0, 32, (hipStream_t)0);
  return bytes;
}

size_t work_temp_bytes(int n, int nkeys) {
  const size_t a = sort_temp_bytes(n), b = ((size_t)(nkeys + 1 + 1023) / 1024 + 1) * sizeof(int);   // = scan_temp_bytes
  return a > b ? a : b;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// atoms sorted by (relation, id) into rows: node_order, row_of_node, z_rows, row_real of `out`
int build_rows(const long* atomic_number, int NA, const int* z_list, int T, const int* row_start, int N,
               const hn_relations_out* out, unsigned* keyA, unsigned* keyB, int* valA, void* temp, size_t tbytes,
               hipStream_t s) {
  hipLaunchKernelGGL(zero_i32_kernel, grid_for(N), dim3(kBlock), 0, s, out->z_rows, (long)N);
  hipLaunchKernelGGL(zero_i32_kernel, grid_for(N), dim3(kBlock), 0, s, reinterpret_cast<int*>(out->row_real), (long)N);
  if (NA > 0) {
    hipLaunchKernelGGL(atom_keys_kernel, grid_for(NA), dim3(kBlock), 0, s, atomic_number, NA, z_list, T, keyA, valA);
    if (hipcub::DeviceRadixSort::SortPairs(temp, tbytes, keyA, keyB, valA, out->node_order, NA, 0, bits_for(T + 1), s)
        != hipSuccess) return HN_ERR_LAUNCH;
    hipLaunchKernelGGL(assign_rows_kernel, grid_for(NA), dim3(kBlock), 0, s, keyB, out->node_order, NA, row_start,
                       T, atomic_number, out->row_of_node, out->z_rows, out->row_real);
  }
  return HN_OK;
}

// Per-step flags of an atom-sharded step (hermnet_shard_step_flags): which (target element, source element) pairs are joined
// by an edge of this rank's list, whether the padded list is complete, whether an atom has left the plan's skin.
__global__ __launch_bounds__(kBlock) void shard_flags_kernel(const long* __restrict__ ei, long columns, const long* __restrict__ z,
                                                             int num_atoms, const long* __restrict__ total, long capacity,
                                                             int* __restrict__ has_in, const float* __restrict__ pos,
                                                             const float* __restrict__ pos_ref, long num_pos, float max_dist2) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i < columns) {
    const long src = ei[i], tgt = ei[columns + i];
    int slot = 128 * 128;                                   // NULL edges of a padded list
    if (tgt >= 0 && tgt < num_atoms && src >= 0 && src < num_atoms) {
      const long zt = z[tgt], zs = z[src];
      slot = (int)(zt < 0 ? 0 : (zt > 127 ? 127 : zt)) * 128 + (int)(zs < 0 ? 0 : (zs > 127 ? 127 : zs));
    }
    if (has_in[slot] == 0) has_in[slot] = 1;               // (every writer writes 1)
  }
  if (i < num_pos) {
    const float dx = pos[3 * i] - pos_ref[3 * i], dy = pos[3 * i + 1] - pos_ref[3 * i + 1], dz = pos[3 * i + 2] - pos_ref[3 * i + 2];
    if (dx * dx + dy * dy + dz * dz > max_dist2) has_in[128 * 128 + 2] = 1;
  }
  if (i == 0 && total != nullptr) has_in[128 * 128 + 1] = (total[1] != 0 || total[0] > capacity) ? 1 : 0;
}


}  // namespace

extern "C" int hermnet_relation_counts(const long* atomic_number, int num_atoms, const int* z_list, int num_rel,
                                       int* counts, void* stream) {
  if (num_atoms < 0 || num_rel <= 0 || !z_list || !counts) return HN_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(zero_i32_kernel, grid_for(num_rel + 1), dim3(kBlock), 0, s, counts, (long)num_rel + 1);
  if (num_atoms == 0) return HN_OK;
  if (!atomic_number) return HN_ERR_BAD_ARG;
  hipLaunchKernelGGL(count_relations_kernel, grid_for(num_atoms), dim3(kBlock), 0, s, atomic_number, num_atoms,
                     z_list, num_rel, counts);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" size_t hermnet_build_relations_workspace(int num_atoms, int num_rows, int num_edges, int num_rel) {
  (void)num_rows; (void)num_rel;
  const size_t n = (size_t)(num_edges > num_atoms ? num_edges : num_atoms) + 1;
  const size_t nk = (size_t)(num_rel + 1) * (size_t)num_rows + 2;
  // 5 index buffers of n + the concatenated counters and their scan + sort/scan storage
  const size_t nall = nk + (size_t)num_rows + 4;     // concatenated counters of both edge orders
  return align256(work_temp_bytes((int)n, (int)nall)) + 5 * align256(n * sizeof(unsigned)) + 2 * align256(nall * sizeof(int)) + 256;
}

extern "C" int hermnet_build_relations(const long* atomic_number, const long* edge_index, const float* shift,
                                       int num_atoms, int num_edges, const int* z_list, int num_rel,
                                       const int* row_start, int num_rows,
                                       const unsigned char* rel_active, const hn_relations_out* out, int rows_ready,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  const int NA = num_atoms, E = num_edges, T = num_rel, N = num_rows;
  if (NA < 0 || E < 0 || T <= 0 || N < NA || !out || !z_list || !row_start) return HN_ERR_BAD_ARG;
  if ((size_t)(T + 1) * (size_t)N >= 0xFFFFFFFFull) return HN_ERR_BAD_ARG;   // keys are 32-bit
  if (workspace_bytes < hermnet_build_relations_workspace(NA, N, E, T) || !workspace) return HN_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t n = (size_t)(E > NA ? E : NA) + 1;
  char* w = reinterpret_cast<char*>(workspace);
  const size_t tb = align256(work_temp_bytes((int)n, (int)((size_t)(T + 1) * N + 2 + (size_t)N + 4)));
  void* temp = w; w += tb;
  unsigned* keyA = reinterpret_cast<unsigned*>(w); w += align256(n * sizeof(unsigned));
  unsigned* keyB = reinterpret_cast<unsigned*>(w); w += align256(n * sizeof(unsigned));
  int* valA = reinterpret_cast<int*>(w); w += align256(n * sizeof(unsigned));
  unsigned* key3 = reinterpret_cast<unsigned*>(w); w += align256(n * sizeof(unsigned));
  unsigned* rt_sorted = reinterpret_cast<unsigned*>(w); w += align256(n * sizeof(unsigned));
  size_t tbytes = tb;

  // ---- rows (rows_ready: node_order / row_of_node / z_rows / row_real of `out` were filled by an earlier call with
  // the same atomic numbers and row layout -- they depend on nothing else)
  if (!rows_ready) {
    const int rcr = build_rows(atomic_number, NA, z_list, T, row_start, N, out, keyA, keyB, valA, temp, tbytes, s);
    if (rcr != HN_OK) return rcr;
  }
  // ---- edge orders by counting sort (claim -> scan -> place -> per-group rank sort; see the kernels above)
  int* key1 = reinterpret_cast<int*>(keyA);
  int* arrival1 = reinterpret_cast<int*>(keyB);
  int* slots = valA;
  int* arrival2 = reinterpret_cast<int*>(key3);
  int* rt_csr = reinterpret_cast<int*>(rt_sorted);
  int* slots2 = key1;                                                       // (key1 is done with once the CSR is placed)
  const size_t nall = (size_t)(N + 1) + (size_t)(T + 1) * N + 1;            // concatenated counters
  int* counters = reinterpret_cast<int*>(w); w += align256(sizeof(int) * (nall + 2));
  int* rp_all = reinterpret_cast<int*>(w); w += align256(sizeof(int) * (nall + 2));
  const bool want_out = out->out_rowptr != nullptr && out->out_edges != nullptr;
  hipLaunchKernelGGL(zero_i32_kernel, grid_for((long)nall), dim3(kBlock), 0, s, counters, (long)nall);
  if (E > 0)
    hipLaunchKernelGGL(edge_claim_kernel, grid_for(E), dim3(kBlock), 0, s, edge_index, E, out->row_of_node, row_start, T, N, NA,
                       key1, arrival1, arrival2, counters);
  const int rcs = scan_orders(counters, (int)nall, temp, tb, rp_all, N, (long)T * N, E, out->csr_rowptr, out->csc_rowptr, s);
  if (rcs != HN_OK) return rcs;
  if (E > 0) {
    // CSR: edges grouped by row(target) (the NULL edges of a padded list behind the last row); row_active rides along
    PlaceExtras x = {};
    x.E = E; x.real_end = out->csr_rowptr + N;
    x.csr_src = out->csr_src; x.src_id = out->src_id; x.tgt_id = out->tgt_id; x.rt_csr = rt_csr;
    x.shift_csr = shift != nullptr ? out->shift_csr : nullptr;
    x.N = N; x.T = T; x.csc_rowptr = out->csc_rowptr; x.row_start = row_start; x.rel_active = rel_active;
    x.row_real = out->row_real; x.row_active = out->row_active;
    hipLaunchKernelGGL(place_kernel, grid_for(E > N ? E : N), dim3(kBlock), 0, s, key1, arrival1, E, rp_all, slots, x);
    // ascending edge id inside a row + the CSR-ordered arrays + CSC: CSR positions placed by (relation(target), row(source));
    // edges to unknown-element targets fall into the extra key range [T*N, (T+1)*N) and are simply not covered by
    // csc_rowptr[0 .. T*N]
    CsrEmitArgs a = {edge_index, shift, E, out->row_of_node, arrival2, rp_all + N + 1, out->csr_perm, out->csr_src,
                     out->src_id, out->tgt_id, rt_csr, slots2, out->shift_csr};
    const int wpq1 = rank_sort_waves_per_quad(E, N);
    hipLaunchKernelGGL(csr_rank_sort_kernel, rank_sort_grid(N, wpq1), dim3(kBlock), 0, s, rp_all, N, wpq1, slots, a, row_start, T);
    const int ng2 = (T + 1) * N, wpq2 = rank_sort_waves_per_quad(E, ng2);
    hipLaunchKernelGGL(csc_rank_sort_kernel, rank_sort_grid(ng2, wpq2), dim3(kBlock), 0, s, rp_all + N + 1, E, ng2, wpq2, slots2,
                       rt_csr, out->csc_pos, out->csc_tgt);
  } else if (N > 0) {
    hipLaunchKernelGGL(row_active_kernel, grid_for(N), dim3(kBlock), 0, s, out->csc_rowptr, row_start, N, T,
                       rel_active, out->row_real, out->row_active);
  }
  // out adjacency: CSR positions grouped by row(source) -- optional: hermnet_edge_geometry_bwd_csc reads the same
  // information from the CSC order
  if (want_out) {
    GroupWork gw;
    gw.counters = counters;
    gw.arrival = arrival1;
    gw.slots = slots;
    gw.scan_temp = temp;
    gw.scan_bytes = tb;
    int rcg;
    if ((rcg = group_by_key(out->csr_src, E, N, out->out_rowptr, out->out_edges, gw, s)) != HN_OK) return rcg;
  }
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" size_t hermnet_build_triadic_workspace(int num_atoms, int num_edges, int num_elem, int block) {
  const size_t T = (size_t)num_elem, P = T * (T + 1) / 2, TR = T * P;
  const size_t Ns = T * (size_t)block, Nt = TR * (size_t)block, E = T * (size_t)num_edges;
  const size_t n = (E > (size_t)num_atoms ? E : (size_t)num_atoms) + 1;
  const size_t nall = (Nt + 1) + TR * Ns + 1;
  return align256(work_temp_bytes((int)n, (int)(nall + 4))) + 5 * align256(n * sizeof(unsigned)) + 2 * align256((nall + 2) * sizeof(int)) +
         align256((T + 1) * sizeof(int)) + 256;
}

extern "C" int hermnet_build_triadic(const long* atomic_number, const long* edge_index, const float* shift,
                                     int num_atoms, int num_edges, const int* z_list, int num_elem, int block,
                                     const int* elem_counts, const unsigned char* rel_active,
                                     const hn_relations_out* out, float* tgt_row_real, int* res_row, int rows_ready,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  const int NA = num_atoms, E0 = num_edges, T = num_elem, B = block;
  if (NA < 0 || E0 < 0 || T <= 0 || B < 0 || !out || !z_list || !elem_counts || !tgt_row_real || !res_row) return HN_ERR_BAD_ARG;
  const long P = (long)T * (T + 1) / 2, TR = T * P, Ns = (long)T * B, Nt = TR * B, E = (long)T * E0;
  if (TR * Ns + Nt + 8 >= 0x7FFFFFFFl || E >= 0x7FFFFFFFl || Ns < NA) return HN_ERR_BAD_ARG;      // keys and counters are int32
  if (!workspace || workspace_bytes < hermnet_build_triadic_workspace(NA, E0, T, B)) return HN_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t n = (size_t)(E > NA ? E : NA) + 1;
  const size_t nall = (size_t)(Nt + 1) + (size_t)(TR * Ns) + 1;
  char* w = reinterpret_cast<char*>(workspace);
  const size_t tb = align256(work_temp_bytes((int)n, (int)(nall + 4)));
  void* temp = w; w += tb;
  unsigned* keyA = reinterpret_cast<unsigned*>(w); w += align256(n * sizeof(unsigned));
  unsigned* keyB = reinterpret_cast<unsigned*>(w); w += align256(n * sizeof(unsigned));
  int* valA = reinterpret_cast<int*>(w); w += align256(n * sizeof(unsigned));
  int* rt_csr = reinterpret_cast<int*>(w); w += align256(n * sizeof(unsigned));
  int* arrival2 = reinterpret_cast<int*>(w); w += align256(n * sizeof(unsigned));
  int* counters = reinterpret_cast<int*>(w); w += align256(sizeof(int) * (nall + 2));
  int* rp_all = reinterpret_cast<int*>(w); w += align256(sizeof(int) * (nall + 2));
  int* row_start = reinterpret_cast<int*>(w); w += align256(sizeof(int) * (T + 1));
  const TriMap m = {T, (int)P, B, (int)Ns};
  if (!rows_ready) {      // source rows: the HVNet layout with every element padded to `block` rows
    // (row_start[t] = t B, written by a kernel: the stream may be capturing)
    hipLaunchKernelGGL(zero_i32_kernel, grid_for(T + 1), dim3(kBlock), 0, s, row_start, (long)T + 1);
    hipLaunchKernelGGL(iota_scaled_kernel, grid_for(T + 1), dim3(kBlock), 0, s, row_start, T + 1, B);
    const int rcr = build_rows(atomic_number, NA, z_list, T, row_start, (int)Ns, out, keyA, keyB, valA, temp, tb, s);
    if (rcr != HN_OK) return rcr;
  }
  int* key1 = reinterpret_cast<int*>(keyA);
  int* arrival1 = reinterpret_cast<int*>(keyB);
  int* slots = valA;
  int* slots2 = key1;
  hipLaunchKernelGGL(zero_i32_kernel, grid_for((long)nall), dim3(kBlock), 0, s, counters, (long)nall);
  if (E > 0)
    hipLaunchKernelGGL(tri_claim_kernel, grid_for(E), dim3(kBlock), 0, s, edge_index, E0, m, out->row_of_node, (int)Nt, key1,
                       arrival1, arrival2, counters);
  const int rcs = scan_orders(counters, (int)nall, temp, tb, rp_all, (int)Nt, TR * Ns, (int)E, out->csr_rowptr, out->csc_rowptr, s);
  if (rcs != HN_OK) return rcs;
  if (E > 0) {
    PlaceExtras none = {};
    hipLaunchKernelGGL(place_kernel, grid_for(E), dim3(kBlock), 0, s, key1, arrival1, (int)E, rp_all, slots, none);
    CsrEmitArgs a = {edge_index, shift, (int)E, out->row_of_node, arrival2, rp_all + Nt + 1, out->csr_perm, out->csr_src,
                     out->src_id, out->tgt_id, rt_csr, slots2, out->shift_csr};
    const int wpq1 = rank_sort_waves_per_quad(E, Nt);
    hipLaunchKernelGGL(tri_rank_sort_kernel, rank_sort_grid(Nt, wpq1), dim3(kBlock), 0, s, rp_all, (int)Nt, wpq1, slots, a, E0, m);
    const int ng2 = (int)(TR * Ns), wpq2 = rank_sort_waves_per_quad(E, ng2);
    hipLaunchKernelGGL(csc_rank_sort_kernel, rank_sort_grid(ng2, wpq2), dim3(kBlock), 0, s, rp_all + Nt + 1, (int)E, ng2, wpq2, slots2,
                       rt_csr, out->csc_pos, out->csc_tgt);
  }
  if (Nt > 0)
    hipLaunchKernelGGL(tri_rows_kernel, grid_for(Nt), dim3(kBlock), 0, s, m, (int)Nt, elem_counts, out->csr_rowptr, rel_active,
                       tgt_row_real, out->row_active, res_row);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_shard_step_flags(const long* edge_index, long columns, const long* atomic_number, int num_atoms,
                                        const long* total, long capacity, int* has_in, const float* pos, const float* pos_ref,
                                        long num_pos, float max_dist2, void* stream) {
  if (columns < 0 || num_atoms < 0 || num_pos < 0 || !has_in || (columns > 0 && (!edge_index || !atomic_number)) ||
      (num_pos > 0 && (!pos || !pos_ref)))
    return HN_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  // (a kernel, not hipMemsetAsync: captured memset nodes do not survive eager memsets between two replays, see above)
  hipLaunchKernelGGL(zero_i32_kernel, grid_for(128 * 128 + 3), dim3(kBlock), 0, s, has_in, (long)(128 * 128 + 3));
  const long n = columns > num_pos ? columns : num_pos;
  hipLaunchKernelGGL(shard_flags_kernel, grid_for(n > 0 ? n : 1), dim3(kBlock), 0, s, edge_index, columns, atomic_number, num_atoms,
                     total, capacity, has_in, pos, pos_ref, num_pos, max_dist2);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}
