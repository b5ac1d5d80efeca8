// gfx950 cutoff neighbour search (cell list) -- the input producer of the hot path.
//
// Replaces /root/reference/HermNet/data.py:14-24 `neighbor_search`, which calls
// ase.neighborlist.primitive_neighbor_list('ijS', ...) (periodic) or torch_cluster.radius_graph
// on the HOST every step (plugin/ase_interface/calculator.py:49, plugin/lmp_interface/lmp_calc.py:224).
// Same conventions as the host implementation in hermnet_amd/neighbor.py (which it must match
// bit for bit on well-separated inputs): pair (i, j, S) listed iff |pos_j - pos_i + S cell| < rc
// (strict), no (i, i, 0), self images allowed, output sorted by (i, j, Sx, Sy, Sz); float64
// arithmetic on the float32 coordinates.
//
// Pipeline: wrap + bin (fractional bins >= rc wide) -> sort atoms by bin -> ONE pass over the candidates that counts
// an atom's pairs and stashes their 64-bit (i, j, S) keys in a per-atom slot of kStash entries -> exclusive scan ->
// (host reads E) -> per-atom rank sort of the stashed keys, decoded straight into edge_index / edge_shift.
// Round 3: the keys of an atom are written by its own wave, so the list is already grouped by i and only needs
// ordering INSIDE an atom (tens of entries): the global radix sort of E 64-bit keys (0.16 ms at 431k pairs) and the
// second pass over the candidates (0.07 ms) are gone.  An atom with more than kStash pairs makes the caller take the
// two-pass form (count, then fill).  Integer/streaming work.
#include <hip/hip_runtime.h>
#include "scan_i32.h"
#include <stdint.h>
#include "../../include/hermnet_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxImg = 8;                 // |S| per axis after un-wrapping must stay below this
constexpr int kCode = 2 * kMaxImg + 1;     // 17 values per axis
constexpr int kStash = 160;                // keys kept per atom by the counting pass (fcc at rc = 5 A: 43)
inline dim3 grid_for(long n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

struct NbrGeom {
  double cell[9];     // rows = lattice vectors (identity for open systems)
  double inv[9];      // inverse
  double lo[3];       // open systems: lower corner of the bounding box
  int nbins[3];
  int reach[3];       // neighbour bins to visit on each side
  int periodic;       // all three axes periodic, or none
  double rc2;
};


// THE geometry of the cell list: inverse cell, plane spacings, bins at least rc wide, reach, the box of an open structure,
// and the grid coarsened to at most 8 N + 64 bins.  This one text serves the host (hermnet_neighbor_count / _fill and the
// probe hermnet_host_neighbor_geometry) and one device thread (nbr_geom_kernel, nbr_batch_geom_kernel, which widen their
// float32 inputs): float64 without fused multiply-adds on both sides, so every form of the search bins alike and lists
// alike, bit for bit.  `cell` [9] (rows = lattice vectors), or NULL with the corners lo / hi of an open structure's
// bounding box.  false = degenerate, `g` half written: a singular cell, one so small that a cutoff sphere reaches beyond
// kMaxImg bins, a determinant, plane spacing or span that is not finite.  The clamps are taken in double BEFORE the int
// casts.  (The host once cast first -- undefined for a non-finite cell or box, which it now refuses with
// HN_ERR_BAD_ARG; for every other input the numbers are what they were.)
__host__ __device__ inline bool nbr_make_geom(const double* cell, const double* lo, const double* hi, double rc, int N,
                                              NbrGeom& g) {
#pragma clang fp contract(off)
  g.rc2 = rc * rc;
  g.periodic = cell != nullptr;
  if (cell) {
    const double* c = cell;
    for (int k = 0; k < 9; ++k) g.cell[k] = c[k];
    const double det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
    if (!(fabs(det) >= 1e-12) || !(fabs(det) <= 1.0e300)) return false;      // (also NaN / Inf)
    g.inv[0] = (c[4] * c[8] - c[5] * c[7]) / det; g.inv[1] = (c[2] * c[7] - c[1] * c[8]) / det; g.inv[2] = (c[1] * c[5] - c[2] * c[4]) / det;
    g.inv[3] = (c[5] * c[6] - c[3] * c[8]) / det; g.inv[4] = (c[0] * c[8] - c[2] * c[6]) / det; g.inv[5] = (c[2] * c[3] - c[0] * c[5]) / det;
    g.inv[6] = (c[3] * c[7] - c[4] * c[6]) / det; g.inv[7] = (c[1] * c[6] - c[0] * c[7]) / det; g.inv[8] = (c[0] * c[4] - c[1] * c[3]) / det;
  } else {
    for (int k = 0; k < 9; ++k) { g.cell[k] = (k % 4 == 0) ? 1.0 : 0.0; g.inv[k] = 0.0; }
  }
  for (int k = 0; k < 3; ++k) {
    // extent along axis k: the plane spacing 1 / |column k of inv|, or the side of the open box
    const double h = cell ? 1.0 / sqrt(g.inv[k] * g.inv[k] + g.inv[3 + k] * g.inv[3 + k] + g.inv[6 + k] * g.inv[6 + k])
                          : hi[k] - lo[k] + 2e-6;
    if (!(h > 0.0) || !(h <= 1.0e300)) return false;
    const double q = floor(h / rc);
    int nb = q > 1024.0 ? 1024 : (int)q;
    if (nb < 1) nb = 1;
    g.nbins[k] = nb;
    if (cell) {
      const double r = ceil(rc / (h / nb) - 1e-12);
      int reach = r > (double)(kMaxImg + 1) ? kMaxImg + 1 : (int)r;
      if (reach < 1) reach = 1;
      if (reach > kMaxImg) return false;                         // cell far smaller than the cutoff
      g.reach[k] = reach;
      g.lo[k] = 0.0;
    } else {
      g.lo[k] = lo[k] - 1e-6;
      g.inv[4 * k] = nb / h;                                     // 1 / bin width (>= rc wide)
      g.reach[k] = 1;
    }
  }
  // sparse box: coarsen the grid (bins only get wider, still >= rc) until the workspace's 8 N + 64 counters hold it
  while ((long)g.nbins[0] * g.nbins[1] * g.nbins[2] > 8l * N + 64) {
    int kmax = 0;
    for (int k = 1; k < 3; ++k) if (g.nbins[k] > g.nbins[kmax]) kmax = k;
    if (g.nbins[kmax] <= 1) break;
    const int nb = (g.nbins[kmax] + 1) / 2;
    if (!g.periodic) g.inv[4 * kmax] *= (double)nb / g.nbins[kmax];
    g.nbins[kmax] = nb;
  }
  return true;
}

// What a kernel puts in place of a degenerate geometry: zero matrices, one bin, a negative cutoff (no distance is below it:
// no pair is listed).  On it the following kernels stay inside their arrays; reach -1 visits no bin at all.
__device__ __forceinline__ void nbr_inert_geom(NbrGeom& g, int periodic, int reach) {
  g.periodic = periodic;
  for (int k = 0; k < 9; ++k) { g.cell[k] = 0.0; g.inv[k] = 0.0; }
  for (int k = 0; k < 3; ++k) { g.nbins[k] = 1; g.reach[k] = reach; g.lo[k] = 0.0; }
  g.rc2 = -1.0;
}

__device__ __forceinline__ void frac_of(const NbrGeom& g, const double* p, double* f) {
  // p @ inv  (row vector times matrix)
  f[0] = p[0] * g.inv[0] + p[1] * g.inv[3] + p[2] * g.inv[6];
  f[1] = p[0] * g.inv[1] + p[1] * g.inv[4] + p[2] * g.inv[7];
  f[2] = p[0] * g.inv[2] + p[1] * g.inv[5] + p[2] * g.inv[8];
}

__device__ __forceinline__ void cart_of(const NbrGeom& g, const double* f, double* p) {
  p[0] = f[0] * g.cell[0] + f[1] * g.cell[3] + f[2] * g.cell[6];
  p[1] = f[0] * g.cell[1] + f[1] * g.cell[4] + f[2] * g.cell[7];
  p[2] = f[0] * g.cell[2] + f[1] * g.cell[5] + f[2] * g.cell[8];
}

// The geometry reaches a kernel by value (G = NbrGeom: made on the host from a host copy of the cell) or through a pointer
// (G = const NbrGeom*: made on the device by nbr_geom_kernel from the cell in device memory, so that a captured search
// follows a cell that changes between replays).
// A batch of structures (G = NbrBatch) has one geometry per structure, made on the device by nbr_batch_geom_kernel:
// atom i reads the geometry of its structure graph[i] and files its bins behind those of the structures in front of it
// (bin_base: exclusive scan of the per-structure bin counts), so a wave only ever walks its own structure's grid.
struct NbrBatch {
  const NbrGeom* geom;     // [B]
  const int* graph;        // [N] structure of every atom, inside [0, B)
  const int* bin_base;     // [B+1]
};
__device__ __forceinline__ const NbrGeom& geom_of(const NbrGeom& g, int) { return g; }
__device__ __forceinline__ const NbrGeom& geom_of(const NbrGeom* g, int) { return *g; }
__device__ __forceinline__ const NbrGeom& geom_of(const NbrBatch& g, int i) { return g.geom[g.graph[i]]; }
__device__ __forceinline__ int bin_base_of(const NbrGeom&, int) { return 0; }
__device__ __forceinline__ int bin_base_of(const NbrGeom*, int) { return 0; }
__device__ __forceinline__ int bin_base_of(const NbrBatch& g, int i) { return g.bin_base[g.graph[i]]; }

// wrapped fractional coordinate, integer wrap, bin id
template <class G>
__global__ __launch_bounds__(kBlock) void nbr_bin_kernel(const float* __restrict__ pos, int N, G geom,
                                                        double* __restrict__ fw, int* __restrict__ wrap,
                                                        unsigned* __restrict__ bin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const NbrGeom& g = geom_of(geom, i);
  const double p[3] = {(double)pos[3 * i], (double)pos[3 * i + 1], (double)pos[3 * i + 2]};
  double f[3];
  int b[3];
  if (g.periodic) {
    frac_of(g, p, f);
    for (int k = 0; k < 3; ++k) {
      const double w = floor(f[k]);
      wrap[3 * i + k] = (int)w;
      f[k] -= w;
      int bk = (int)(f[k] * g.nbins[k]);
      b[k] = bk >= g.nbins[k] ? g.nbins[k] - 1 : bk;
    }
  } else {
    for (int k = 0; k < 3; ++k) {
      f[k] = p[k];
      wrap[3 * i + k] = 0;
      int bk = (int)((p[k] - g.lo[k]) * g.inv[4 * k]);     // inv diagonal = 1 / bin width
      b[k] = bk < 0 ? 0 : (bk >= g.nbins[k] ? g.nbins[k] - 1 : bk);
    }
  }
  fw[3 * i] = f[0]; fw[3 * i + 1] = f[1]; fw[3 * i + 2] = f[2];
  bin[i] = (unsigned)(bin_base_of(geom, i) + (b[0] * g.nbins[1] + b[1]) * g.nbins[2] + b[2]);
}

// Atoms grouped by bin with a counting sort (histogram -> exclusive scan = bin_start -> scatter through per-bin cursors).
// The order INSIDE a bin is whatever the atomics give: it only decides the order in which an atom's keys reach its
// stash slot, and those are rank-sorted before they are decoded -- the list does not depend on it.  (Round 4: replaces a
// library radix sort + scan, whose look-back state does not survive hipGraph replays interleaved with eager runs --
// csrc/relation_kernels.hip found that out for the relation build -- so that search + step can be ONE captured graph.)
__global__ __launch_bounds__(kBlock) void nbr_zero_kernel(int* __restrict__ dst, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = 0;
}
__global__ __launch_bounds__(kBlock) void nbr_bin_hist_kernel(const unsigned* __restrict__ bin, int N, int* __restrict__ hist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) atomicAdd(&hist[bin[i]], 1);
}
__global__ __launch_bounds__(kBlock) void nbr_bin_scatter_kernel(const unsigned* __restrict__ bin, int N,
                                                                const int* __restrict__ start, int* __restrict__ fill,
                                                                int* __restrict__ ids_sorted) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) ids_sorted[start[bin[i]] + atomicAdd(&fill[bin[i]], 1)] = i;
}

// Visit every candidate (j, image) of atom i.  MODE 0 counts and stashes the keys at keys[i * kStash ...] (flags: bit 0
// |S| overflow, bit 1 an atom with more than kStash pairs), MODE 1 writes the keys at keys[offset[i] ...] (two-pass form).
// key = ((i * N + j) * 17^3 + code(S)),  S = image - wrap_j + wrap_i (shift for the caller's coordinates).
template <int MODE, class G>
__global__ __launch_bounds__(kBlock) void nbr_pairs_kernel(const double* __restrict__ fw, const int* __restrict__ wrap,
                                                          const int* __restrict__ sorted_ids,
                                                          const int* __restrict__ bin_start, int N, G geom,
                                                          const long* __restrict__ offset, int* __restrict__ count,
                                                          unsigned long long* __restrict__ keys,
                                                          int* __restrict__ overflow,
                                                          const unsigned char* __restrict__ target_ok, int target_is_j,
                                                          int stash) {
  // one WAVE per atom: the lanes share the candidates of a bin (one atom per thread left the chip at 40 workgroups
  // for 10k atoms, each thread walking ~200 candidates serially: 0.2 ms per pass)
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= N) return;
  const NbrGeom& g = geom_of(geom, i);
  const int bin0 = bin_base_of(geom, i);
  const int lane = threadIdx.x & 63;
  // `target_ok` (atom-sharded lists, sharding.py): only pairs whose TARGET atom is flagged are listed -- the target is j
  // in the periodic convention ([i; j]), i in the open-system one ([j; i])
  if (target_ok != nullptr && !target_is_j && !target_ok[i]) {
    if (MODE == 0 && lane == 0) count[i] = 0;
    return;
  }
  const bool mask_j = target_ok != nullptr && target_is_j;
  const double fi[3] = {fw[3 * i], fw[3 * i + 1], fw[3 * i + 2]};
  double pi[3];
  if (g.periodic) cart_of(g, fi, pi); else { pi[0] = fi[0]; pi[1] = fi[1]; pi[2] = fi[2]; }
  int bi[3];
  for (int k = 0; k < 3; ++k) {
    int bk;
    if (g.periodic) bk = (int)(fi[k] * g.nbins[k]); else bk = (int)((fi[k] - g.lo[k]) * g.inv[4 * k]);
    bi[k] = bk < 0 ? 0 : (bk >= g.nbins[k] ? g.nbins[k] - 1 : bk);
  }
  constexpr bool FILL = MODE == 1;
  long out = FILL ? offset[i] : (long)i * stash;
  int n = 0;
  for (int ox = -g.reach[0]; ox <= g.reach[0]; ++ox)
    for (int oy = -g.reach[1]; oy <= g.reach[1]; ++oy)
      for (int oz = -g.reach[2]; oz <= g.reach[2]; ++oz) {
        int tb[3] = {bi[0] + ox, bi[1] + oy, bi[2] + oz};
        int img[3] = {0, 0, 0};
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
          if (g.periodic) {
            // floor division: image shift carried by leaving the cell through this face
            int q = tb[k] >= 0 ? tb[k] / g.nbins[k] : -((-tb[k] + g.nbins[k] - 1) / g.nbins[k]);
            img[k] = q;
            tb[k] -= q * g.nbins[k];
          } else if (tb[k] < 0 || tb[k] >= g.nbins[k]) {
            ok = false;
          }
        }
        if (!ok) continue;
        const int b = bin0 + (tb[0] * g.nbins[1] + tb[1]) * g.nbins[2] + tb[2];
        const int s_end = bin_start[b + 1];
        for (int s0 = bin_start[b]; s0 < s_end; s0 += 64) {      // (wave-uniform loop: ballots are well defined)
          const int s = s0 + lane;
          bool hit = false;
          int j = 0;
          if (s < s_end) {
            j = sorted_ids[s];
            double fj[3] = {fw[3 * j] + img[0], fw[3 * j + 1] + img[1], fw[3 * j + 2] + img[2]};
            double pj[3];
            if (g.periodic) cart_of(g, fj, pj); else { pj[0] = fj[0]; pj[1] = fj[1]; pj[2] = fj[2]; }
            const double dx = pj[0] - pi[0], dy = pj[1] - pi[1], dz = pj[2] - pi[2];
            const double d2 = dx * dx + dy * dy + dz * dz;
            hit = (d2 < g.rc2) && !(j == i && img[0] == 0 && img[1] == 0 && img[2] == 0);
            if (mask_j) hit = hit && target_ok[j] != 0;
          }
          const unsigned long long m = __ballot(hit);
          if (hit) {
            const int S[3] = {img[0] - wrap[3 * j] + wrap[3 * i], img[1] - wrap[3 * j + 1] + wrap[3 * i + 1],
                              img[2] - wrap[3 * j + 2] + wrap[3 * i + 2]};
            const bool over = S[0] < -kMaxImg || S[0] > kMaxImg || S[1] < -kMaxImg || S[1] > kMaxImg || S[2] < -kMaxImg ||
                              S[2] > kMaxImg;
            if (over) atomicOr(overflow, 1);
            const unsigned long long code =
                (unsigned long long)(((S[0] + kMaxImg) * kCode + (S[1] + kMaxImg)) * kCode + (S[2] + kMaxImg));
            // position inside the atom's key range: hits of earlier lanes first (the keys are sorted afterwards,
            // so only "each slot written once" matters)
            const int slot = __popcll(m & ((1ull << lane) - 1ull));
            // A shift outside the code's range (flag bit 0) has no key: its code would carry into the neighbouring axis
            // (S = (0, 0, 9) reads back as (0, 1, -8), a pair of this atom with a shift it does not have) or into the
            // pair field.  Such a hit takes a key from the top of the range instead, one per position of the atom's
            // run: above every real key (keys_fit), unique for the rank sort, and decoded as a NULL edge.
            if (FILL || n + slot < stash)
              keys[out + slot] = over ? ~0ull - (unsigned long long)(n + slot)
                                      : ((unsigned long long)i * (unsigned long long)N + (unsigned long long)j) *
                                            (unsigned long long)(kCode * kCode * kCode) + code;
          }
          const int nh = __popcll(m);
          out += nh;
          n += nh;
        }
      }
  if (!FILL && lane == 0) {
    count[i] = n;
    if (n > stash) atomicOr(overflow, 2);
  }
}

// One wave per atom: rank sort of its keys (unique, so rank = number of smaller keys) and decode into the caller's
// arrays at offset[i] + rank.  `stride` = kStash (stashed keys at src[i * kStash]) or 0 (keys at src[offset[i]]).
// (E = columns of edge_index; in capacity mode the list may hold more pairs than that: positions >= E are dropped and
// nbr_pad_kernel reports it)
__global__ __launch_bounds__(kBlock) void nbr_sort_decode_kernel(const unsigned long long* __restrict__ src, int stride,
                                                                const int* __restrict__ count, const long* __restrict__ offset,
                                                                int N, long E, float sign, int swap_rows,
                                                                long* __restrict__ edge_index, float* __restrict__ shift) {
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= N) return;
  const int lane = threadIdx.x & 63;
  const int cnt = count[i];
  const int n = stride ? min(cnt, stride) : cnt;               // (a stash holds at most `stride` keys of an atom)
  const long base = offset[i];
  const unsigned long long* keys = src + (stride ? (long)i * stride : base);
  const unsigned long long c3 = (unsigned long long)(kCode * kCode * kCode);
  for (int a = lane; a < n; a += 64) {
    const unsigned long long key = keys[a];
    int rank = 0;
    for (int b = 0; b < n; ++b) rank += keys[b] < key ? 1 : 0;
    const long e = base + rank;
    if (e >= E) continue;
    const unsigned long long pair = key / c3;
    const int code = (int)(key - pair * c3);
    const unsigned long long ii = pair / (unsigned long long)N;
    const long j = (long)(pair - ii * (unsigned long long)N);
    // a key whose image shift left the code's range (flag bit 0) lies above every real key (nbr_pairs_kernel): the pair it
    // decodes to is not this atom's -- such a column becomes a NULL edge, never an index that a later kernel would follow
    // out of bounds, and never a pair with a shift it does not have
    const bool ok = ii == (unsigned long long)i;
    edge_index[e] = ok ? (swap_rows ? j : (long)i) : -1;
    edge_index[E + e] = ok ? (swap_rows ? (long)i : j) : -1;
    if (shift != nullptr) {
      shift[3 * e + 0] = ok ? sign * (float)(code / (kCode * kCode) - kMaxImg) : 0.f;
      shift[3 * e + 1] = ok ? sign * (float)((code / kCode) % kCode - kMaxImg) : 0.f;
      shift[3 * e + 2] = ok ? sign * (float)(code % kCode - kMaxImg) : 0.f;
    }
  }
  // An atom with more pairs than its stash slot (flag bit 1): offset[] counts ALL its pairs, the stash holds the first
  // `stride` -- the columns base + n .. base + cnt - 1 belong to keys that were never kept.  They become NULL edges (the
  // list is incomplete and the caller repeats the search, but whatever runs on it before the flags are read -- the model
  // step of an MD loop does -- must not meet uninitialised indices).
  for (int a = n + lane; a < cnt; a += 64) {
    const long e = base + a;
    if (e >= E) break;
    edge_index[e] = -1;
    edge_index[E + e] = -1;
    if (shift != nullptr) { shift[3 * e] = 0.f; shift[3 * e + 1] = 0.f; shift[3 * e + 2] = 0.f; }
  }
}

// Capacity mode: the columns behind the list's last pair become NULL edges (-1, -1; shift 0) -- the relation build files
// them behind every row, so no row-walking kernel ever meets one -- and total[0] = number of pairs found, total[1] = flags
// (bit 0: image shift overflow, bit 1: an atom with more pairs than its stash slot, bit 2: more pairs than columns).
// With bits 1 or 2 set the list is incomplete: the caller repeats the search in its exact (two-call) form.
__global__ __launch_bounds__(kBlock) void nbr_pad_kernel(const long* __restrict__ offset, const int* __restrict__ overflow,
                                                        int N, long cap, long* __restrict__ edge_index,
                                                        float* __restrict__ shift, long* __restrict__ total) {
  const long found = offset[N];
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e == 0) {
    total[0] = found;
    total[1] = (long)(overflow[0] | (found > cap ? 4 : 0));
  }
  if (e < found || e >= cap) return;
  edge_index[e] = -1;
  edge_index[cap + e] = -1;
  if (shift != nullptr) { shift[3 * e] = 0.f; shift[3 * e + 1] = 0.f; shift[3 * e + 2] = 0.f; }
}

// (set / copy as kernels, not hipMemsetAsync / hipMemcpyAsync: captured memset nodes did not survive eager memsets
// between two replays on ROCm 7.2 -- csrc/relation_kernels.hip --, and the search is part of a captured MD step)
__global__ void nbr_clear_kernel(int* __restrict__ count_end, int* __restrict__ overflow) {
  if (threadIdx.x == 0) { count_end[0] = 0; overflow[0] = 0; overflow[1] = 0; }
}
__global__ void nbr_total_kernel(const long* __restrict__ offset_end, const int* __restrict__ overflow, long* __restrict__ total) {
  if (threadIdx.x == 0) { total[0] = offset_end[0]; total[1] = (long)overflow[0]; }
}

// The geometry of a cell in DEVICE memory, by one thread: the float32 values are widened (the numbers a host copy of the same
// tensor gives) and handed to nbr_make_geom, so the geometry -- and with it the list -- is bit for bit the host form's.
// A cell the host refuses cannot be a return code here: flag bit 3 is raised and the geometry is an inert one of reach 1,
// on which no pair is listed; the caller discards such a step.
__global__ void nbr_geom_kernel(const float* __restrict__ cell, double rc, int N, NbrGeom* __restrict__ out,
                                int* __restrict__ overflow) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double c[9];
  for (int k = 0; k < 9; ++k) c[k] = (double)cell[k];
  NbrGeom g;
  if (!nbr_make_geom(c, nullptr, nullptr, rc, N, g)) {
    nbr_inert_geom(g, 1, 1);
    overflow[0] = 8;
  }
  *out = g;
}

// ---- a batch of structures: everything about them is found on the device ----------------------------------------------
// Atom ranges ptr[B+1] of the structures from the non-decreasing `batch` (thread i looks at the boundary in front of atom
// i and writes the first atom of every structure that begins there, empty ones included) and the structure of every atom
// as an int inside [0, B).  A value outside [0, B) or a decrease raises flag bit 4: the ranges then mean nothing (`ptr` was
// zeroed, so they stay inside [0, N]) and nbr_batch_geom_kernel gives every structure a geometry on which no atom looks at
// any bin.
__global__ __launch_bounds__(kBlock) void nbr_batch_ptr_kernel(const long* __restrict__ batch, int N, int B,
                                                              int* __restrict__ graph, int* __restrict__ ptr,
                                                              int* __restrict__ overflow) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > N) return;
  const long hi = (long)B - 1;
  const long prev = i == 0 ? -1 : batch[i - 1], cur = i == N ? (long)B : batch[i];
  const long pc = i == 0 ? -1 : (prev < 0 ? 0 : (prev > hi ? hi : prev));
  const long cc = i == N ? (long)B : (cur < 0 ? 0 : (cur > hi ? hi : cur));
  if (i < N) {
    graph[i] = (int)cc;
    if (cur < 0 || cur > hi || (i > 0 && cur < prev)) atomicOr(overflow, 16);
  }
  for (long b = pc + 1; b <= cc; ++b) ptr[b] = i;
}

// One workgroup per structure: the bounding box of an open structure (min / max are exact in any order), then ONE thread
// makes its NbrGeom with nbr_make_geom (from the widened float32 cell or box, for the structure's own atom count: the
// single search's geometry, so the lists are the same bit for bit) and writes its bin count.  A degenerate cell raises flag
// bit 3 for that structure alone.  It, an empty structure and every structure of a batch with flag bit 4 get an inert
// geometry of reach -1: an atom of such a structure visits no bin and lists no pair.
__global__ __launch_bounds__(kBlock) void nbr_batch_geom_kernel(const float* __restrict__ pos, const int* __restrict__ ptr,
                                                               const float* __restrict__ cells, double rc, int B,
                                                               NbrGeom* __restrict__ geom, int* __restrict__ nbin_count,
                                                               int* __restrict__ overflow) {
  __shared__ float red[6][kBlock];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n0 = ptr[b], n1 = ptr[b + 1];
  const int nb_atoms = n1 > n0 ? n1 - n0 : 0;
  if (cells == nullptr) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int a = n0 + t; a < n1; a += kBlock)
      for (int k = 0; k < 3; ++k) { const float v = pos[3 * a + k]; lo[k] = fminf(lo[k], v); hi[k] = fmaxf(hi[k], v); }
    for (int k = 0; k < 3; ++k) { red[k][t] = lo[k]; red[3 + k][t] = hi[k]; }
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
      if (t < w)
        for (int k = 0; k < 3; ++k) {
          red[k][t] = fminf(red[k][t], red[k][t + w]);
          red[3 + k][t] = fmaxf(red[3 + k][t], red[3 + k][t + w]);
        }
      __syncthreads();
    }
  }
  if (t != 0) return;
  NbrGeom g;
  bool ok = nb_atoms > 0 && (atomicOr(overflow, 0) & 16) == 0;
  if (ok) {
    double in[9];                                  // the cell, or the box's corners: lo in in[0..2], hi in in[3..5]
    if (cells != nullptr) {
      for (int k = 0; k < 9; ++k) in[k] = (double)cells[9 * (long)b + k];
      ok = nbr_make_geom(in, nullptr, nullptr, rc, nb_atoms, g);
    } else {
      for (int k = 0; k < 6; ++k) in[k] = (double)red[k][0];
      ok = nbr_make_geom(nullptr, in, in + 3, rc, nb_atoms, g);
    }
    if (!ok) atomicOr(overflow, 8);
  }
  if (!ok) nbr_inert_geom(g, cells != nullptr, -1);
  geom[b] = g;
  nbin_count[b] = g.nbins[0] * g.nbins[1] * g.nbins[2];
  if (b == 0) nbin_count[B] = 0;
}
__global__ void nbr_zero_total_kernel(long* __restrict__ total) {
  if (threadIdx.x < 2) total[threadIdx.x] = 0;
}

// ---- host side: ONE workspace layout, ONE counting pass and ONE of each fill tail for the three forms of the search:
// the single search with its cell on the host (G = NbrGeom) or in device memory (const NbrGeom*), and the batch
// (NbrBatch).  An entry point checks its own arguments, carves the workspace, produces its geometry and calls these.
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct NbrWork {
  double* fw; int* wrap; unsigned* bin; int* bin_fill; int* ids_sorted; int* bin_start;
  int* count; long* offset; int* overflow; unsigned long long* stash;
  int* graph; int* ptr; int* nbin_count; int* bin_base; NbrGeom* geom;      // a batch's per-structure arrays (B > 0)
  void* temp; size_t temp_bytes;
  int stash_slot;          // keys per atom that `stash` holds
};

// Bins a workspace has counters for (B = 0: one structure, whose grid is coarsened to this bound; a batch: the sum of its
// structures' bounds).
long bins_bound(int N, int B) { return B ? 8l * N + 64l * B : 8l * (N > 0 ? N : 1) + 64; }

size_t workspace_for(int N, int B, int stash) {
  const long nbins = bins_bound(N, B);
  size_t bytes = align256(sizeof(double) * 3 * (size_t)N) + align256(sizeof(int) * 3 * (size_t)N) + 2 * align256(sizeof(int) * (size_t)N) +
                 2 * align256(sizeof(int) * (size_t)(nbins + 1)) + align256(sizeof(int) * (size_t)(N + 1)) +
                 align256(sizeof(long) * (size_t)(N + 1)) + 256 + align256(sizeof(unsigned long long) * (size_t)N * stash);
  if (B)
    bytes += align256(sizeof(int) * (size_t)(N > 0 ? N : 1)) + 3 * align256(sizeof(int) * ((size_t)B + 1)) +
             align256(sizeof(NbrGeom) * (size_t)B);
  return bytes + align256(scan_temp_bytes((int)nbins + 2)) + 512;      // (scratch of the longer scan: the bins' counters)
}

int clamp_stash(int stash) { return stash < 8 ? 8 : (stash > kStash ? kStash : stash); }

bool keys_fit(int N) { return (double)N * N * 4913.0 < 1.8e19; }      // the keys (i N + j) 17^3 + code(S) stay inside 64 bits

bool batch_shape_ok(int N, int B) { return N >= 0 && B > 0 && bins_bound(N, B) + 2 <= 0x7fffffffl && keys_fit(N); }

// The arrays of a workspace of `workspace_bytes` for N > 0 atoms (B = 0: one structure).  The per-atom stash slot is the
// largest one <= kStash whose workspace fits: every call of a search derives it from the same (N, B, workspace_bytes), so
// they agree.  false = not even the smallest slot (8 keys) fits.
bool carve(void* workspace, size_t workspace_bytes, int N, int B, NbrWork& w) {
  int lo = 0, hi = kStash;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (workspace_for(N, B, mid) <= workspace_bytes) lo = mid; else hi = mid - 1;
  }
  if (lo < 8) return false;
  w.stash_slot = lo;
  const long nbins = bins_bound(N, B);
  char* p = reinterpret_cast<char*>(workspace);
  auto take = [&](size_t bytes) { void* r = p; p += align256(bytes); return r; };
  w.fw = (double*)take(sizeof(double) * 3 * (size_t)N);
  w.wrap = (int*)take(sizeof(int) * 3 * (size_t)N);
  w.bin = (unsigned*)take(sizeof(unsigned) * (size_t)N);
  w.ids_sorted = (int*)take(sizeof(int) * (size_t)N);
  w.bin_start = (int*)take(sizeof(int) * (size_t)(nbins + 1));
  w.bin_fill = (int*)take(sizeof(int) * (size_t)(nbins + 1));
  w.count = (int*)take(sizeof(int) * (size_t)(N + 1));
  w.offset = (long*)take(sizeof(long) * (size_t)(N + 1));
  w.overflow = (int*)take(256);
  w.stash = (unsigned long long*)take(sizeof(unsigned long long) * (size_t)N * w.stash_slot);
  w.graph = w.ptr = w.nbin_count = w.bin_base = nullptr;
  w.geom = nullptr;
  if (B) {
    w.graph = (int*)take(sizeof(int) * (size_t)N);
    w.ptr = (int*)take(sizeof(int) * ((size_t)B + 1));
    w.nbin_count = (int*)take(sizeof(int) * ((size_t)B + 1));
    w.bin_base = (int*)take(sizeof(int) * ((size_t)B + 1));
    w.geom = (NbrGeom*)take(sizeof(NbrGeom) * (size_t)B);
  }
  w.temp = p;
  w.temp_bytes = workspace_bytes - (size_t)(p - (char*)workspace);
  return true;
}

int launched() { return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH; }

// The counting pass on a geometry that exists (G by value) or that earlier launches of the stream make (the two device
// forms): bin -> atoms sorted by bin -> every atom's pairs counted and their keys stashed -> offsets -> total_device =
// (pairs found, flags).  `nbins`: counters to clear and scan -- the grid's bins or, where only the device knows the grid,
// the workspace's bound (counters beyond the grid's bins stay zero).  `clear`: the pass resets the flags itself; the
// device forms did so before their geometry kernels, which raise flags of their own.
template <class G>
int count_pass(const float* pos, int N, G g, long nbins, const NbrWork& w, bool clear, const unsigned char* target_ok,
               int target_is_j, long* total_device, hipStream_t s) {
  hipLaunchKernelGGL(nbr_bin_kernel<G>, grid_for(N), dim3(kBlock), 0, s, pos, N, g, w.fw, w.wrap, w.bin);
  hipLaunchKernelGGL(nbr_zero_kernel, grid_for(nbins + 1), dim3(kBlock), 0, s, w.bin_fill, nbins + 1);
  hipLaunchKernelGGL(nbr_bin_hist_kernel, grid_for(N), dim3(kBlock), 0, s, w.bin, N, w.bin_fill);
  if (exclusive_scan_i32(w.bin_fill, w.bin_start, (int)nbins + 1, w.temp, w.temp_bytes, s) != HN_OK) return HN_ERR_BAD_ARG;
  hipLaunchKernelGGL(nbr_zero_kernel, grid_for(nbins + 1), dim3(kBlock), 0, s, w.bin_fill, nbins + 1);
  hipLaunchKernelGGL(nbr_bin_scatter_kernel, grid_for(N), dim3(kBlock), 0, s, w.bin, N, w.bin_start, w.bin_fill, w.ids_sorted);
  if (clear) hipLaunchKernelGGL(nbr_clear_kernel, dim3(1), dim3(64), 0, s, w.count + N, w.overflow);
  hipLaunchKernelGGL((nbr_pairs_kernel<0, G>), grid_for((long)N * 64), dim3(kBlock), 0, s, w.fw, w.wrap, w.ids_sorted, w.bin_start, N,
                     g, (const long*)nullptr, w.count, w.stash, w.overflow, target_ok, target_is_j, w.stash_slot);
  if (exclusive_scan_i32_to_long(w.count, w.offset, N + 1, w.temp, w.temp_bytes, s) != HN_OK) return HN_ERR_BAD_ARG;
  hipLaunchKernelGGL(nbr_total_kernel, dim3(1), dim3(64), 0, s, w.offset + N, w.overflow, total_device);
  return launched();
}

// The exact list after the host read of E: the stashed keys rank-sorted per atom and decoded, behind (stash_ok = 0: an atom
// had more pairs than its stash slot) a second pass over the candidates into `keys`.
template <class G>
int fill_exact(int N, G g, const NbrWork& w, const unsigned char* target_ok, int target_is_j, long num_edges, float shift_sign,
               int source_first, int stash_ok, unsigned long long* keys, long* edge_index, float* edge_shift, hipStream_t s) {
  if (!stash_ok)
    hipLaunchKernelGGL((nbr_pairs_kernel<1, G>), grid_for((long)N * 64), dim3(kBlock), 0, s, w.fw, w.wrap, w.ids_sorted, w.bin_start, N,
                       g, w.offset, (int*)nullptr, keys, w.overflow, target_ok, target_is_j, 0);
  hipLaunchKernelGGL(nbr_sort_decode_kernel, grid_for((long)N * 64), dim3(kBlock), 0, s, stash_ok ? w.stash : keys,
                     stash_ok ? w.stash_slot : 0, w.count, w.offset, N, num_edges, shift_sign, source_first, edge_index, edge_shift);
  return launched();
}

// The padded list: the stashed keys, rank-sorted per atom, into the first `capacity` columns, NULL edges behind them, and the
// count + flags for whoever reads them (the host: at the END of the step).
int fill_padded(int N, const NbrWork& w, long capacity, float shift_sign, int source_first, long* edge_index, float* edge_shift,
                long* total_device, hipStream_t s) {
  hipLaunchKernelGGL(nbr_sort_decode_kernel, grid_for((long)N * 64), dim3(kBlock), 0, s, w.stash, w.stash_slot, w.count, w.offset, N,
                     capacity, shift_sign, source_first, edge_index, edge_shift);
  hipLaunchKernelGGL(nbr_pad_kernel, grid_for(capacity), dim3(kBlock), 0, s, w.offset, w.overflow, N, capacity, edge_index,
                     edge_shift, total_device);
  return launched();
}

}  // namespace

extern "C" size_t hermnet_neighbor_workspace(int num_atoms) { return workspace_for(num_atoms, 0, kStash); }
extern "C" size_t hermnet_neighbor_workspace_for(int num_atoms, int stash_per_atom) {
  return workspace_for(num_atoms, 0, clamp_stash(stash_per_atom));
}
extern "C" size_t hermnet_neighbor_batch_workspace(int num_atoms, int num_graphs, int stash_per_atom) {
  return batch_shape_ok(num_atoms, num_graphs) ? workspace_for(num_atoms, num_graphs, clamp_stash(stash_per_atom)) : 0;
}

extern "C" int hermnet_host_neighbor_geometry(const double* cell_host, const double* lo_host, const double* hi_host, double rc,
                                              int num_atoms, double* geom_host, int* grid_host) {
  if (num_atoms < 1 || !(rc > 0.0) || !geom_host || !grid_host || (!cell_host && (!lo_host || !hi_host))) return HN_ERR_BAD_ARG;
  NbrGeom g;
  if (!nbr_make_geom(cell_host, lo_host, hi_host, rc, num_atoms, g)) return HN_ERR_BAD_ARG;
  for (int k = 0; k < 9; ++k) { geom_host[k] = g.cell[k]; geom_host[9 + k] = g.inv[k]; }
  for (int k = 0; k < 3; ++k) { geom_host[18 + k] = g.lo[k]; grid_host[k] = g.nbins[k]; grid_host[3 + k] = g.reach[k]; }
  geom_host[21] = g.rc2;
  grid_host[6] = g.periodic;
  return HN_OK;
}

extern "C" int hermnet_neighbor_count(const float* pos, int num_atoms, const double* cell_host,
                                      const double* lo_host, const double* hi_host, double rc,
                                      void* workspace, size_t workspace_bytes, const unsigned char* target_ok,
                                      long* total_device, void* stream) {
  const int N = num_atoms;
  if (N < 0 || rc <= 0.0 || !workspace || !total_device) return HN_ERR_BAD_ARG;
  if (!cell_host && (!lo_host || !hi_host)) return HN_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (N == 0) return hipMemsetAsync(total_device, 0, 2 * sizeof(long), s) == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
  if (!pos) return HN_ERR_BAD_ARG;
  NbrGeom g;
  NbrWork w;
  if (!nbr_make_geom(cell_host, lo_host, hi_host, rc, N, g) || !carve(workspace, workspace_bytes, N, 0, w)) return HN_ERR_BAD_ARG;
  return count_pass(pos, N, g, (long)g.nbins[0] * g.nbins[1] * g.nbins[2], w, true, target_ok, g.periodic, total_device, s);
}

// The cell in DEVICE memory (periodic cells; `cell` [9] float32, rows = lattice vectors): nothing about it is known on the
// host, so the launch sizes that follow the bin count take the bound the workspace is carved for, and the geometry lives
// in the workspace (the flags' 256-byte block: two ints of flags in front, the geometry behind them).
extern "C" int hermnet_neighbor_count_devcell(const float* pos, int num_atoms, const float* cell, double rc,
                                              void* workspace, size_t workspace_bytes, const unsigned char* target_ok,
                                              long* total_device, void* stream) {
  const int N = num_atoms;
  if (N <= 0 || !(rc > 0.0) || !pos || !cell || !workspace || !total_device) return HN_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  NbrWork w;
  if (!carve(workspace, workspace_bytes, N, 0, w)) return HN_ERR_BAD_ARG;
  static_assert(sizeof(NbrGeom) + 32 <= 256, "NbrGeom must fit behind the flags");
  NbrGeom* g = reinterpret_cast<NbrGeom*>(reinterpret_cast<char*>(w.overflow) + 32);
  hipLaunchKernelGGL(nbr_clear_kernel, dim3(1), dim3(64), 0, s, w.count + N, w.overflow);
  hipLaunchKernelGGL(nbr_geom_kernel, dim3(1), dim3(64), 0, s, cell, rc, N, g, w.overflow);
  return count_pass(pos, N, (const NbrGeom*)g, bins_bound(N, 0), w, false, target_ok, 1, total_device, s);
}

extern "C" int hermnet_neighbor_fill_padded(int num_atoms, void* workspace, size_t workspace_bytes, long capacity,
                                            float shift_sign, int source_first, long* edge_index, float* edge_shift,
                                            long* total_device, void* stream) {
  const int N = num_atoms;
  if (N <= 0 || capacity <= 0 || capacity > 0x7fffffffl || !workspace || !edge_index || !total_device) return HN_ERR_BAD_ARG;
  NbrWork w;
  if (!keys_fit(N) || !carve(workspace, workspace_bytes, N, 0, w)) return HN_ERR_BAD_ARG;
  return fill_padded(N, w, capacity, shift_sign, source_first, edge_index, edge_shift, total_device,
                     reinterpret_cast<hipStream_t>(stream));
}

extern "C" int hermnet_neighbor_fill(const float* pos, int num_atoms, const double* cell_host,
                                     const double* lo_host, const double* hi_host, double rc,
                                     void* workspace, size_t workspace_bytes, long num_edges, float shift_sign,
                                     int source_first, int stash_ok, unsigned long long* keys,
                                     const unsigned char* target_ok, long* edge_index, float* edge_shift,
                                     void* stream) {
  const int N = num_atoms;
  if (N <= 0 || num_edges < 0 || !workspace || !edge_index) return HN_ERR_BAD_ARG;
  if (num_edges == 0) return HN_OK;
  if (!keys_fit(N) || num_edges > 0x7fffffffl || (!stash_ok && !keys)) return HN_ERR_BAD_ARG;
  NbrGeom g;
  NbrWork w;
  if (!nbr_make_geom(cell_host, lo_host, hi_host, rc, N, g) || !carve(workspace, workspace_bytes, N, 0, w)) return HN_ERR_BAD_ARG;
  return fill_exact(N, g, w, target_ok, g.periodic, num_edges, shift_sign, source_first, stash_ok, keys, edge_index, edge_shift,
                    reinterpret_cast<hipStream_t>(stream));
}

// ---- the search of a batch of structures (`batch` [N] int64 non-decreasing, `cells` [B,9] float32 in device memory or
// NULL for open structures): one geometry per structure, all of them made on the device; the workspace is the single
// search's for 8 N + 64 B bins, with the per-structure arrays behind it.
extern "C" int hermnet_neighbor_batch_count(const float* pos, int num_atoms, const long* batch, int num_graphs,
                                            const float* cells, double rc, void* workspace, size_t workspace_bytes,
                                            long* total_device, void* stream) {
  const int N = num_atoms, B = num_graphs;
  if (!batch_shape_ok(N, B) || !(rc > 0.0) || !workspace || !total_device) return HN_ERR_BAD_ARG;
  if (N > 0 && (!pos || !batch)) return HN_ERR_BAD_ARG;
  NbrWork w;
  if (!carve(workspace, workspace_bytes, N, B, w)) return HN_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (N == 0) {
    hipLaunchKernelGGL(nbr_zero_total_kernel, dim3(1), dim3(64), 0, s, total_device);
    return launched();
  }
  hipLaunchKernelGGL(nbr_clear_kernel, dim3(1), dim3(64), 0, s, w.count + N, w.overflow);
  hipLaunchKernelGGL(nbr_zero_kernel, grid_for(B + 1l), dim3(kBlock), 0, s, w.ptr, B + 1l);
  hipLaunchKernelGGL(nbr_batch_ptr_kernel, grid_for(N + 1l), dim3(kBlock), 0, s, batch, N, B, w.graph, w.ptr, w.overflow);
  hipLaunchKernelGGL(nbr_batch_geom_kernel, dim3(B), dim3(kBlock), 0, s, pos, w.ptr, cells, rc, B, w.geom, w.nbin_count, w.overflow);
  if (exclusive_scan_i32(w.nbin_count, w.bin_base, B + 1, w.temp, w.temp_bytes, s) != HN_OK) return HN_ERR_BAD_ARG;
  return count_pass(pos, N, NbrBatch{w.geom, w.graph, w.bin_base}, bins_bound(N, B), w, false, nullptr, 0, total_device, s);
}

extern "C" int hermnet_neighbor_batch_fill(int num_atoms, int num_graphs, void* workspace, size_t workspace_bytes,
                                           long num_edges, float shift_sign, int source_first, int stash_ok,
                                           unsigned long long* keys, long* edge_index, float* edge_shift, void* stream) {
  const int N = num_atoms, B = num_graphs;
  if (!batch_shape_ok(N, B) || N == 0 || num_edges < 0 || num_edges > 0x7fffffffl || !workspace || !edge_index)
    return HN_ERR_BAD_ARG;
  if (num_edges > 0 && !stash_ok && !keys) return HN_ERR_BAD_ARG;
  NbrWork w;
  if (!carve(workspace, workspace_bytes, N, B, w)) return HN_ERR_BAD_ARG;
  if (num_edges == 0) return HN_OK;
  return fill_exact(N, NbrBatch{w.geom, w.graph, w.bin_base}, w, nullptr, 0, num_edges, shift_sign, source_first, stash_ok, keys,
                    edge_index, edge_shift, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int hermnet_neighbor_batch_fill_padded(int num_atoms, int num_graphs, void* workspace, size_t workspace_bytes,
                                                  long capacity, float shift_sign, int source_first, long* edge_index,
                                                  float* edge_shift, long* total_device, void* stream) {
  const int N = num_atoms, B = num_graphs;
  if (!batch_shape_ok(N, B) || N == 0 || capacity <= 0 || capacity > 0x7fffffffl || !workspace || !edge_index ||
      !total_device)
    return HN_ERR_BAD_ARG;
  NbrWork w;
  if (!carve(workspace, workspace_bytes, N, B, w)) return HN_ERR_BAD_ARG;
  return fill_padded(N, w, capacity, shift_sign, source_first, edge_index, edge_shift, total_device,
                     reinterpret_cast<hipStream_t>(stream));
}
