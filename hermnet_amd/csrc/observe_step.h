// MD observers behind a resident driver's finish (observe_kernels.hip; hermnet_amd/observe.py: Frames, RDF, MSD): ONE text
// for the device kernels, the host twins (hermnet_host_observe_*) and -- transcribed operation by operation --
// tests/observe_reference.py.  Contraction is off inside every function: only IEEE +, -, x, floor and comparisons on doubles,
// one rounding each, in the order written.  The one float sqrt (obs_bin) only GUESSES a bin; comparisons decide it, so the
// counts are the same integers on the device, on the host and in numpy whatever that sqrt rounds to.
//
// Protocol.  An observer's launches follow the driver's commit kernel, so they read the NEW `state`.  Each observer owns
// obs [4] int64 = (last sampled step, samples taken, reserved, reserved), obs[0] = -1 at the start.  A sample is DUE iff
//     state[HN_STATE_CODE] == 0  and  step % stride == 0  and  step > obs[0],        step = state[HN_STATE_STEP]
// so the prime of a construction samples the start configuration as step 0; a void step, a halted or a parked replay sample
// nothing (their code is not 0); the prime behind a resume() stands at a step that was sampled already.  Every workgroup of
// an observer's launches reads the obs words as the launch found them; the observer's LAST, single-workgroup kernel alone
// writes them (obs_commit) and the ring's steps[slot]: resident_step.h's single-writer rule.
//
// Frames  slot = obs[1] % frames;  positions[slot,i,:] = float(x[i,:]) (the wrapped float64 state), optionally images and
//         float(v);  cells[slot] = the step's float32 cell, the one this configuration lives in.
// MSD     the first sample stores the origin (x_o, image_o);  d = (x - x_o) + (image - image_o) cell with the CURRENT float32
//         cell widened (under a barostat: a stated convention);  one workgroup per (graph, species) takes (sum d_x, sum d_y,
//         sum d_z, sum |d|^2) with hn_canonical_sums over the graph's atoms, those of other species skipped in place.
// RDF     per atom the fractional coordinate s_k = (x0 inv[k] + x1 inv[3+k]) + x2 inv[6+k] (md_wrap_atom's order); per pair
//         i < j of one graph  ds = s_i - s_j,  ds -= floor(ds + 0.5),  d = ds cell as (a + b) + c,  r2 = (d0^2 + d1^2) + d2^2.
//         Open structures: s = x, d = ds.  Bin b iff edge2[b] <= r2 < edge2[b+1], edge2[b] = (b r_max / bins)^2 made on the
//         host.  Each unordered pair counts once in the histogram of its species pair (a <= b) at obs_pair_index.  The
//         minimum image by rounding is the nearest image for every vector shorter than half the smallest cell height, so a
//         graph is sampled only where r_max^2 |column k of inv|^2 <= 1/4 for k = 0, 1, 2 (obs_rdf_graph_ok); otherwise that
//         sample of that graph is skipped and counted in skipped[slot].  slot = slot_of[g] (a replica's rung) or g.
#ifndef HERMNET_OBSERVE_STEP_H
#define HERMNET_OBSERVE_STEP_H

#include "resident_step.h"

#define HN_OBS_LAST 0                 // obs[0]: the last sampled step (-1: none yet)
#define HN_OBS_TAKEN 1                // obs[1]: samples taken
#define HN_OBS_TILE 256               // atoms of an RDF tile = lanes of its workgroup
#define HN_OBS_RDF_MAX_BINS 1024      // the edges sit in LDS beside the histogram: 8 KB
#define HN_OBS_RDF_MAX_HIST 8192      // P x bins uint32 counters in LDS: 32 KB

namespace {

HN_HD inline bool obs_due(const long* state, const long* obs, long stride, long* step) {
  *step = state[HN_STATE_STEP];
  return state[HN_STATE_CODE] == 0 && *step % stride == 0 && *step > obs[HN_OBS_LAST];
}

// The single writer of an observer's words.
HN_HD inline void obs_commit(long* obs, long step) {
  obs[HN_OBS_LAST] = step;
  obs[HN_OBS_TAKEN] += 1;
}

// ---- frames -----------------------------------------------------------------------------------------------------------------
struct ObsFramesArgs {
  int n, num_graphs;
  long stride, frames;
  const double *x, *v;               // v: NULL where velocities are not recorded
  const int* image;                  // NULL where images are not recorded
  const float* cell32;               // [B,3,3], NULL: open structures
  const long* state;
  long *obs, *steps;                 // steps [frames]
  float *positions, *velocities;     // [frames,N,3]
  int* images;                       // [frames,N,3]
  float* cells;                      // [frames,B,3,3]
};

inline bool obs_frames_args_ok(const ObsFramesArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || a.stride < 1 || a.frames < 1 || !a.state || !a.obs || !a.steps) return false;
  if (a.cell32 && !a.cells) return false;
  if ((a.v != nullptr) != (a.velocities != nullptr) || (a.image != nullptr) != (a.images != nullptr)) return false;
  return a.n == 0 || (a.x && a.positions);
}

HN_HD inline int obs_frames_lanes(const ObsFramesArgs& a) { return a.n > 9 * a.num_graphs ? a.n : 9 * a.num_graphs; }

// Lane i of a due sample: atom i's row of the frame; the lanes below 9B copy the cell.
HN_HD inline void obs_frame_lane(const ObsFramesArgs& a, long slot, int i) {
  if (i < a.n) {
    const size_t at = 3 * ((size_t)slot * a.n + i);
    for (int k = 0; k < 3; ++k) {
      a.positions[at + k] = (float)a.x[3 * (size_t)i + k];
      if (a.v) a.velocities[at + k] = (float)a.v[3 * (size_t)i + k];
      if (a.image) a.images[at + k] = a.image[3 * (size_t)i + k];
    }
  }
  if (a.cell32 && i < 9 * a.num_graphs) a.cells[(size_t)slot * 9 * a.num_graphs + i] = a.cell32[i];
}

HN_HD inline void obs_frames_commit(const ObsFramesArgs& a) {
  long step;
  if (!obs_due(a.state, a.obs, a.stride, &step)) return;
  a.steps[a.obs[HN_OBS_TAKEN] % a.frames] = step;
  obs_commit(a.obs, step);
}

// ---- mean-squared displacement ----------------------------------------------------------------------------------------------
struct ObsMsdArgs {
  int n, num_graphs, num_species;
  long stride, rows;
  const int *graph_ptr, *species;    // species [N]: the index of the atom's atomic number among the sorted distinct ones
  const double* x;
  const int* image;
  const float* cell32;               // NULL: open structures (d = x - x_o)
  const long* state;
  long *obs, *steps;                 // steps [rows]
  double* x_origin;                  // [N,3]
  int* image_origin;                 // [N,3]
  double* sums;                      // [rows,B,S,4]
};

inline bool obs_msd_args_ok(const ObsMsdArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || a.num_species < 1 || a.stride < 1 || a.rows < 1) return false;
  if (!a.state || !a.obs || !a.steps || !a.graph_ptr || !a.sums) return false;
  return a.n == 0 || (a.species && a.x && a.image && a.x_origin && a.image_origin);
}

// Atom i's terms of the sums of (graph g, species s); the first sample stores the origin.
HN_HD inline void obs_msd_term(const ObsMsdArgs& a, int g, int s, bool first, int i, double* acc) {
#pragma clang fp contract(off)
  if (a.species[i] != s) return;
  double d[3], di[3];
  for (int k = 0; k < 3; ++k) {
    const size_t at = 3 * (size_t)i + k;
    if (first) {
      a.x_origin[at] = a.x[at];
      a.image_origin[at] = a.image[at];
    }
    d[k] = a.x[at] - a.x_origin[at];
    di[k] = (double)(a.image[at] - a.image_origin[at]);
  }
  if (a.cell32) {
    const float* c = a.cell32 + 9 * (size_t)g;
    for (int j = 0; j < 3; ++j) d[j] = d[j] + ((di[0] * (double)c[j] + di[1] * (double)c[3 + j]) + di[2] * (double)c[6 + j]);
  }
  for (int k = 0; k < 3; ++k) acc[k] = acc[k] + d[k];
  acc[3] = acc[3] + ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

// The workgroup (256 lanes; the host walks them) of (graph g, species s) of a due sample.
HN_HD inline void obs_msd_group(const ObsMsdArgs& a, int g, int s, double (*part)[256]) {
  const bool first = a.obs[HN_OBS_TAKEN] == 0;
  const long slot = a.obs[HN_OBS_TAKEN] % a.rows;
  const int lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.n);
  hn_canonical_sums<4, -1>(lo, hi, part, [&](int i, double* acc) { obs_msd_term(a, g, s, first, i, acc); });
  if (hn_lead_lane()) {
    double* row = a.sums + (((size_t)slot * a.num_graphs + g) * a.num_species + s) * 4;
    for (int k = 0; k < 4; ++k) row[k] = part[k][0];
  }
}

HN_HD inline void obs_msd_commit(const ObsMsdArgs& a) {
  long step;
  if (!obs_due(a.state, a.obs, a.stride, &step)) return;
  a.steps[a.obs[HN_OBS_TAKEN] % a.rows] = step;
  obs_commit(a.obs, step);
}

// ---- radial distribution function ---------------------------------------------------------------------------------------------
struct ObsRdfArgs {
  int n, num_graphs, num_species, bins;
  long slots, stride;
  double r_max2;                     // r_max^2: the validity check's
  float inv_dr;                      // bins / r_max: the bin guess's
  const int *graph_ptr, *species;
  const double* x;
  const float* cell32;               // [B,3,3]; NULL (with inv_cell): open structures
  const double* inv_cell;            // [B,3,3] float64
  const long* slot_of;               // [B] (DeviceREMD: rung) or NULL: slot = graph
  const double* edge2;               // [bins+1]
  const int* work;                   // [num_work,3] = (graph, tile_i, tile_j >= tile_i)
  int num_work;
  const long* state;
  long* obs;
  long *counts, *samples, *skipped;  // [slots,P,bins], [slots], [slots]
  double* volume_sum;                // [slots]
};

HN_HD inline int obs_num_pairs(int species) { return species * (species + 1) / 2; }

// Histogram of the species pair (a <= b) of S species: rows (0,0) (0,1) .. (0,S-1) (1,1) ..
HN_HD inline int obs_pair_index(int a, int b, int species) { return a * species - a * (a - 1) / 2 + (b - a); }

inline bool obs_rdf_args_ok(const ObsRdfArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || a.num_species < 1 || a.bins < 1 || a.slots < 1 || a.stride < 1 || a.num_work < 0) return false;
  if (a.bins > HN_OBS_RDF_MAX_BINS || (long)obs_num_pairs(a.num_species) * a.bins > HN_OBS_RDF_MAX_HIST) return false;
  if (!(a.r_max2 > 0.0) || !a.state || !a.obs || !a.graph_ptr || !a.edge2 || !a.counts || !a.samples || !a.skipped || !a.volume_sum)
    return false;
  if ((a.cell32 != nullptr) != (a.inv_cell != nullptr) || (a.num_work > 0 && !a.work)) return false;
  if (!a.slot_of && a.slots < a.num_graphs) return false;
  return a.n == 0 || (a.species && a.x);
}

HN_HD inline long obs_rdf_slot(const ObsRdfArgs& a, int g) {
  const long s = a.slot_of ? a.slot_of[g] : (long)g;
  return s < 0 ? 0 : (s >= a.slots ? a.slots - 1 : s);
}

// May graph g be sampled with the minimum image by rounding?  (Open structures: always.)
HN_HD inline bool obs_rdf_graph_ok(const ObsRdfArgs& a, int g) {
#pragma clang fp contract(off)
  if (!a.cell32) return true;
  const double* inv = a.inv_cell + 9 * (size_t)g;
  for (int k = 0; k < 3; ++k) {
    const double q = (inv[k] * inv[k] + inv[3 + k] * inv[3 + k]) + inv[6 + k] * inv[6 + k];
    if (!(a.r_max2 * q <= 0.25)) return false;
  }
  return true;
}

// The minimum-image rule, stated once (the RDF's pairs here; metad_step.h's collective variables): the fractional
// coordinate of a point in the cell whose float64 inverse is `inv` ...
HN_HD inline void obs_fractional(double x0, double x1, double x2, const double* inv, double s[3]) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; ++k) s[k] = (x0 * inv[k] + x1 * inv[3 + k]) + x2 * inv[6 + k];
}

// ... and the vector d from point j to point i by rounding their fractional difference to the nearest image and going
// back through the cell (open structures: the difference itself).  Returns |d|^2.
HN_HD inline double obs_min_image(const double si[3], double sj0, double sj1, double sj2, const double cell[9], bool periodic,
                                  double d[3]) {
#pragma clang fp contract(off)
  double ds[3] = {si[0] - sj0, si[1] - sj1, si[2] - sj2};
  if (periodic) {
    for (int k = 0; k < 3; ++k) ds[k] = ds[k] - floor(ds[k] + 0.5);
    for (int j = 0; j < 3; ++j) d[j] = (ds[0] * cell[j] + ds[1] * cell[3 + j]) + ds[2] * cell[6 + j];
  } else {
    for (int j = 0; j < 3; ++j) d[j] = ds[j];
  }
  return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
}

// Atom i's coordinate as the pairs read it: fractional in a cell, Cartesian in an open structure.
HN_HD inline void obs_rdf_coordinate(const ObsRdfArgs& a, int g, int i, double s[3]) {
  const double x0 = a.x[3 * (size_t)i], x1 = a.x[3 * (size_t)i + 1], x2 = a.x[3 * (size_t)i + 2];
  if (!a.cell32) {
    s[0] = x0;
    s[1] = x1;
    s[2] = x2;
    return;
  }
  obs_fractional(x0, x1, x2, a.inv_cell + 9 * (size_t)g, s);
}

HN_HD inline double obs_pair_r2(const double si[3], double sj0, double sj1, double sj2, const double cell[9], bool periodic) {
  double d[3];
  return obs_min_image(si, sj0, sj1, sj2, cell, periodic, d);
}

// The bin of r2 by comparisons alone (-1: none, r2 >= edge2[bins] or not a number); the float sqrt is only where to start.
HN_HD inline int obs_bin(double r2, const double* edge2, int bins, float inv_dr) {
  if (!(r2 < edge2[bins])) return -1;
  int b = (int)(sqrtf((float)r2) * inv_dr);
  b = b < 0 ? 0 : (b > bins - 1 ? bins - 1 : b);
  while (b > 0 && r2 < edge2[b]) --b;
  while (r2 >= edge2[b + 1]) ++b;      // ends: r2 < edge2[bins]
  return b;
}

HN_HD inline void obs_hist_add(uint32_t* h) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(h, 1u);                    // an LDS integer add: order-independent
#else
  *h += 1u;
#endif
}

// The atoms of tile t of graph g: the first one and how many (0: the tile lies behind the graph).
HN_HD inline int obs_tile(const ObsRdfArgs& a, int g, int t, int* first) {
  const int lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.n);
  *first = lo + t * HN_OBS_TILE;
  const int count = hi - *first;
  return t < 0 || count < 0 ? 0 : (count > HN_OBS_TILE ? HN_OBS_TILE : count);
}

// Phase 1, lane l of the work entry (g, ti, tj): atom l of tile j, staged as [component][lane] with its species.
HN_HD inline void obs_rdf_stage(const ObsRdfArgs& a, int g, int tj, int l, double (*sj)[HN_OBS_TILE], int* zj) {
  int first;
  if (l >= obs_tile(a, g, tj, &first)) return;
  double s[3];
  obs_rdf_coordinate(a, g, first + l, s);
  for (int k = 0; k < 3; ++k) sj[k][l] = s[k];
  zj[l] = a.species[first + l];
}

// Phase 2, lane l: atom l of tile i against the staged tile (behind itself where the two tiles are one).
HN_HD inline void obs_rdf_lane(const ObsRdfArgs& a, int g, int ti, int tj, int l, const double (*sj)[HN_OBS_TILE], const int* zj,
                               const double* edge2, uint32_t* hist) {
  int first_i, first_j;
  const int nj = obs_tile(a, g, tj, &first_j);
  if (l >= obs_tile(a, g, ti, &first_i)) return;
  double si[3], cell[9];
  obs_rdf_coordinate(a, g, first_i + l, si);
  const bool periodic = a.cell32 != nullptr;
  for (int k = 0; k < 9; ++k) cell[k] = periodic ? (double)a.cell32[9 * (size_t)g + k] : 0.0;
  const int zi = a.species[first_i + l];
  for (int m = ti == tj ? l + 1 : 0; m < nj; ++m) {
    const int b = obs_bin(obs_pair_r2(si, sj[0][m], sj[1][m], sj[2][m], cell, periodic), edge2, a.bins, a.inv_dr);
    if (b < 0) continue;
    const int zm = zj[m], lo = zi < zm ? zi : zm, hi = zi < zm ? zm : zi;
    if (lo < 0 || hi >= a.num_species) continue;
    obs_hist_add(hist + (size_t)obs_pair_index(lo, hi, a.num_species) * a.bins + b);
  }
}

// The commit's sequential part: per graph one more sample (and its volume) or one more skip, in the order of the graphs.
HN_HD inline void obs_rdf_commit(const ObsRdfArgs& a) {
#pragma clang fp contract(off)
  long step;
  if (!obs_due(a.state, a.obs, a.stride, &step)) return;
  for (int g = 0; g < a.num_graphs; ++g) {
    const long slot = obs_rdf_slot(a, g);
    if (!obs_rdf_graph_ok(a, g)) {
      a.skipped[slot] += 1;
      continue;
    }
    a.samples[slot] += 1;
    if (a.cell32) {
      const float* f = a.cell32 + 9 * (size_t)g;
      double c[9];
      for (int k = 0; k < 9; ++k) c[k] = (double)f[k];
      const double det = (c[0] * (c[4] * c[8] - c[5] * c[7]) + c[1] * (c[5] * c[6] - c[3] * c[8])) + c[2] * (c[3] * c[7] - c[4] * c[6]);
      a.volume_sum[slot] = a.volume_sum[slot] + (det < 0.0 ? -det : det);
    }
  }
  obs_commit(a.obs, step);
}

}  // namespace

#endif  // HERMNET_OBSERVE_STEP_H
