// Ring-polymer path-integral MD inside the replayed step (pimd_kernels.hip; hermnet_amd/pimd.py: DevicePIMD): ONE text for
// the device kernels, the host twins (hermnet_host_pimd_advance / _finish) and -- transcribed operation by operation --
// tests/pimd_reference.py.  Contraction is off inside every function, as in md_step.h: only IEEE +, x and floor on doubles,
// one rounding each, in the order written (the Gaussians' log / cos / sqrt are md_step.h's, unchanged).
//
// P beads = the P graphs of the batch, all the same system of n_rep atoms: atom a of bead j is row j n_rep + a.  The
// convention is Ceriotti, Parrinello, Markland, Manolopoulos, J. Chem. Phys. 133, 124104 (2010): every bead feels the full
// potential, the extended system is sampled at P T, omega_P = P kB T / hbar, springs 1/2 m omega_P^2 |q_j - q_(j+1)|^2
// (cyclic), normal modes q~_k = sum_j C[j][k] q_j with the real orthogonal C, omega_k = 2 omega_P sin(k pi / P).  The
// splitting is BAOAB (Liu, Li, Liu, J. Chem. Phys. 145, 024103 (2016)):
//   B     v += kick f_prev on every bead                                            (md_advance_atom's first line)
//   A(h)  per mode, exact:  q~' = cs q~ + sw v~,  v~' = cs v~ - ws q~ (the old q~)
//   O(dt) PILE-L:  v~ = c1_k v~ + sigma_(k,a) xi,  xi = md_gaussians(md_noise_words(seed, step, k n_rep + a))
//   A(h)  again;  back to beads q_j = sum_k C[j][k] q~_k;  the wrap by the centroid;  the second B is the finish's.
// Without a thermostat (flags without HN_MD_LANGEVIN: plain RPMD) there is no O and nothing between the two A(h), which are
// then ONE A(dt): the caller's cs / sw / ws are those of the whole step, and one ring of one bead is velocity Verlet as
// hermnet_md_advance writes it, bit for bit.  Everything that needs cos, sin, exp, sqrt or a division -- C, cs, sw, ws, c1,
// sigma, 1/P, 1/2 m omega_P^2 -- is made once on the host in float64.
//
// The wrap is one per ATOM: the centroid c = (ascending sum of the new q_j) (1/P) goes through md_wrap_atom, and every bead
// of the atom loses the same n cell and gains the same n in its image, so the springs need no minimum image (the search
// wraps on its own: beads slightly outside the cell are fine).  An atom of infinite mass (kick 0) is skipped by all of this:
// its beads stay where they were given, v stays as it is (0).
//
// A tile is A = 256 / P atoms x P lanes, lane l = a P + k.  Three phases with a barrier between them (the host twin walks
// the lanes of a phase in turn): lane (a, k) is bead k (kick; x, v into `sb`), then mode k (its six dot products read the
// atom's beads from `sb`, the result of A, O, A goes to `sm`), then bead k again (six dot products over `sm`, the new bead
// into `sb`); the lane k = 0 makes the centroid and n from `sb` and publishes them in `sn` / `sc`; every lane stores.
// LDS layout [component][lane] of doubles, unpadded: the lanes of one atom read ONE address at a time (a broadcast), and the
// atoms inside a 32-lane half sit P doubles apart, which repeats a bank only every 32 / gcd(P, 32) atoms -- more than a half
// holds for every P <= 128 but 96 (two-way there).  Stores are consecutive.
#ifndef HERMNET_PIMD_STEP_H
#define HERMNET_PIMD_STEP_H

#include "md_finish.h"

#define HN_PIMD_MAX_BEADS 128

namespace {

struct PimdAdvanceArgs {
  int n, beads, n_rep, flags;                      // n = beads * n_rep;  HN_MD_LANGEVIN: the O step;  HN_MD_WRAP
  double *x, *v, *x0, *v0;
  int *image, *image0;
  const float* f_prev;
  const double* kick;                              // [N]
  const double* cmat;                              // [P, P]: C[j][k] at j P + k
  const double *cs, *sw, *ws, *c1;                 // [P]
  const double* sigma;                             // [P, n_rep]
  double inv_beads;                                // 1 / P
  const float* cell;
  const double* inv_cell;
  float* pos32;
  double* centroid;                                // scratch [n_rep, 3]: the wrapped centroid; the finish reads it
  const long* state;
  uint64_t seed;
};

struct PimdFinishArgs {
  MdFinishArgs m;
  int n_rep;
  const double* spring_c;                          // [n_rep]: 1/2 m omega_P^2 (0 for an atom of infinite mass)
  const double* centroid;                          // [n_rep, 3]
};

inline bool pimd_advance_args_ok(const PimdAdvanceArgs& a) {
  if (a.n < 0 || a.beads < 1 || a.beads > HN_PIMD_MAX_BEADS || (a.flags & ~(HN_MD_LANGEVIN | HN_MD_WRAP))) return false;
  if (a.n % a.beads != 0 || a.n_rep != a.n / a.beads || !a.state) return false;
  if (a.n == 0) return true;
  if (!a.x || !a.v || !a.x0 || !a.v0 || !a.image || !a.image0 || !a.f_prev || !a.kick || !a.pos32 || !a.centroid) return false;
  if (!a.cmat || !a.cs || !a.sw || !a.ws) return false;
  if ((a.flags & HN_MD_LANGEVIN) && (!a.c1 || !a.sigma)) return false;
  if ((a.flags & HN_MD_WRAP) && (!a.cell || !a.inv_cell)) return false;
  return true;
}

inline bool pimd_finish_args_ok(const PimdFinishArgs& a) {
  if (!md_finish_args_ok(a.m) || a.m.num_graphs > HN_PIMD_MAX_BEADS) return false;
  if (a.m.n % a.m.num_graphs != 0 || a.n_rep != a.m.n / a.m.num_graphs) return false;
  return a.m.n == 0 || (a.spring_c && a.centroid);
}

// Atoms of a tile, and the atom / bead-or-mode of lane l in the tile that starts at atom `first`.
HN_HD inline int pimd_tile_atoms(int beads) { return 256 / beads; }
HN_HD inline bool pimd_lane(const PimdAdvanceArgs& a, int first, int l, int* atom, int* k) {
  const int t = l / a.beads;
  *k = l - t * a.beads;
  *atom = first + t;
  return t < pimd_tile_atoms(a.beads) && *atom < a.n_rep;
}

// The exact free flight of one mode over the time the tables were made for.
HN_HD inline void pimd_free_mode(double q[3], double v[3], double cs, double sw, double ws) {
#pragma clang fp contract(off)
  for (int c = 0; c < 3; ++c) {
    const double qn = cs * q[c] + sw * v[c];
    v[c] = cs * v[c] - ws * q[c];
    q[c] = qn;
  }
}

// A prime: the float32 input alone (md_advance_one's mode 1).
HN_HD inline void pimd_prime_lane(const PimdAdvanceArgs& a, int first, int l) {
  int atom, k;
  if (!pimd_lane(a, first, l, &atom, &k)) return;
  const size_t i = (size_t)k * a.n_rep + atom;
  for (int c = 0; c < 3; ++c) a.pos32[3 * i + c] = (float)a.x[3 * i + c];
}

// Phase 1, lane (atom, bead k): the backup, the kick, x and v into sb[0..3) / sb[3..6).
HN_HD inline void pimd_bead_in(const PimdAdvanceArgs& a, int first, int l, double (*sb)[256]) {
#pragma clang fp contract(off)
  int atom, k;
  if (!pimd_lane(a, first, l, &atom, &k)) return;
  const size_t i = (size_t)k * a.n_rep + atom;
  const double kick = a.kick[i];
  for (int c = 0; c < 3; ++c) {
    const double x = a.x[3 * i + c];
    double v = a.v[3 * i + c];
    a.x0[3 * i + c] = x;
    a.v0[3 * i + c] = v;
    a.image0[3 * i + c] = a.image[3 * i + c];
    if (kick != 0.0) v = v + kick * (double)a.f_prev[3 * i + c];
    sb[c][l] = x;
    sb[3 + c][l] = v;
  }
}

// Phase 2, lane (atom, mode k): to modes, A, (O, A), into sm.  An atom of infinite mass does nothing.
HN_HD inline void pimd_mode(const PimdAdvanceArgs& a, long step, int first, int l, const double (*sb)[256], double (*sm)[256]) {
#pragma clang fp contract(off)
  int atom, k;
  if (!pimd_lane(a, first, l, &atom, &k)) return;
  if (a.kick[atom] == 0.0) return;
  const int P = a.beads, base = l - k;
  double q[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < P; ++j) {
    const double cjk = a.cmat[(size_t)j * P + k];
    for (int c = 0; c < 3; ++c) {
      q[c] = q[c] + cjk * sb[c][base + j];
      v[c] = v[c] + cjk * sb[3 + c][base + j];
    }
  }
  const double cs = a.cs[k], sw = a.sw[k], ws = a.ws[k];
  pimd_free_mode(q, v, cs, sw, ws);
  if (a.flags & HN_MD_LANGEVIN) {
    uint32_t w[8];
    double xi[3];
    md_noise_words(a.seed, (uint64_t)step, (uint32_t)((size_t)k * a.n_rep + atom), w);
    md_gaussians(w, xi);
    const double c1 = a.c1[k], sigma = a.sigma[(size_t)k * a.n_rep + atom];
    for (int c = 0; c < 3; ++c) v[c] = c1 * v[c] + sigma * xi[c];
    pimd_free_mode(q, v, cs, sw, ws);
  }
  for (int c = 0; c < 3; ++c) {
    sm[c][l] = q[c];
    sm[3 + c][l] = v[c];
  }
}

// Phase 3, lane (atom, bead k): back to beads, into sb (every lane of the tile has left phase 2: sb is free).
HN_HD inline void pimd_bead_out(const PimdAdvanceArgs& a, int first, int l, const double (*sm)[256], double (*sb)[256]) {
#pragma clang fp contract(off)
  int atom, k;
  if (!pimd_lane(a, first, l, &atom, &k)) return;
  if (a.kick[atom] == 0.0) return;
  const int P = a.beads, base = l - k;
  double q[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
  for (int m = 0; m < P; ++m) {
    const double ckm = a.cmat[(size_t)k * P + m];
    for (int c = 0; c < 3; ++c) {
      q[c] = q[c] + ckm * sm[c][base + m];
      v[c] = v[c] + ckm * sm[3 + c][base + m];
    }
  }
  for (int c = 0; c < 3; ++c) {
    sb[c][l] = q[c];
    sb[3 + c][l] = v[c];
  }
}

// Phase 4, the lane k = 0 of an atom: the centroid of the new beads, wrapped where the driver wraps; n into sn (three
// doubles per lane slot), the wrapped centroid to the scratch the finish reads.
HN_HD inline void pimd_centroid(const PimdAdvanceArgs& a, int first, int l, const double (*sb)[256], double (*sn)[256]) {
#pragma clang fp contract(off)
  int atom, k;
  if (!pimd_lane(a, first, l, &atom, &k) || k != 0) return;
  double c[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < a.beads; ++j)
    for (int d = 0; d < 3; ++d) c[d] = c[d] + sb[d][l + j];
  for (int d = 0; d < 3; ++d) c[d] = c[d] * a.inv_beads;
  int n[3] = {0, 0, 0};
  if ((a.flags & HN_MD_WRAP) && a.kick[atom] != 0.0) {
    double cell[9], inv[9];
    hn_load_cell(a.cell, a.inv_cell, 0, cell, inv);
    md_wrap_atom(c, n, cell, inv);
  }
  for (int d = 0; d < 3; ++d) {
    sn[d][l] = (double)n[d];
    a.centroid[3 * (size_t)atom + d] = c[d];
  }
}

// Phase 5, lane (atom, bead k): every bead of the atom loses the same n cell; the stores.
HN_HD inline void pimd_store(const PimdAdvanceArgs& a, int first, int l, const double (*sb)[256], const double (*sn)[256]) {
#pragma clang fp contract(off)
  int atom, k;
  if (!pimd_lane(a, first, l, &atom, &k)) return;
  const size_t i = (size_t)k * a.n_rep + atom;
  double x[3], n[3];
  for (int c = 0; c < 3; ++c) {
    x[c] = sb[c][l];
    n[c] = sn[c][l - k];
  }
  if (a.flags & HN_MD_WRAP) {      // md_wrap_atom's second half, with the atom's n (0 for an atom of infinite mass)
    for (int c = 0; c < 3; ++c) {
      const double cj = (double)a.cell[c], c3 = (double)a.cell[3 + c], c6 = (double)a.cell[6 + c];
      x[c] = x[c] - ((n[0] * cj + n[1] * c3) + n[2] * c6);
      a.image[3 * i + c] = a.image[3 * i + c] + (int)n[c];
    }
  }
  for (int c = 0; c < 3; ++c) {
    a.x[3 * i + c] = x[c];
    a.v[3 * i + c] = sb[3 + c][l];
    a.pos32[3 * i + c] = (float)x[c];
  }
}

// ---- the finish's per-bead sums ---------------------------------------------------------------------------------------------
// Atom i of bead j adds to (E_kin_j, spring_j, vir_j): its kinetic energy, 1/2 m omega_P^2 |x_j - x_(j+1)|^2 (cyclic in j)
// and (x - centroid) . f with the step's new forces.  An atom of infinite mass adds nothing.
HN_HD inline void pimd_bead_terms(const PimdFinishArgs& a, int j, int i, double* s) {
#pragma clang fp contract(off)
  const int P = a.m.num_graphs, atom = i - j * a.n_rep;
  if (atom < 0 || atom >= a.n_rep || a.m.half_mass[i] == 0.0) return;
  const size_t nx = (size_t)(j + 1 == P ? 0 : j + 1) * a.n_rep + atom;
  double d[3], r[3], f[3];
  for (int c = 0; c < 3; ++c) {
    const double x = a.m.x[3 * (size_t)i + c];
    d[c] = x - a.m.x[3 * nx + c];
    r[c] = x - a.centroid[3 * (size_t)atom + c];
    f[c] = (double)a.m.forces[3 * (size_t)i + c];
  }
  s[0] = s[0] + a.m.ke_atom[i];
  s[1] = s[1] + a.spring_c[atom] * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  s[2] = s[2] + ((r[0] * f[0] + r[1] * f[1]) + r[2] * f[2]);
}

// Bead j's workgroup (256 lanes; the host walks them) of a committed step: the three sums in the canonical order and the log
// row of width 5 = (E_pot_j, E_kin_j, edges found, spring_j, vir_j).
HN_HD inline void pimd_log_bead(const PimdFinishArgs& a, long step, int j, double (*part)[256]) {
  const int lo = hn_graph_lo(a.m.graph_ptr, j), hi = hn_graph_hi(a.m.graph_ptr, j, a.m.n);
  hn_canonical_sums<3, -1>(lo, hi, part, [&](int i, double* s) { pimd_bead_terms(a, j, i, s); });
  if (hn_lead_lane()) {
    double* row = hn_log_row(a.m.log, step, a.m.log_steps, a.m.num_graphs, j, 5);
    row[0] = (double)a.m.energy[j];
    row[1] = part[0][0];
    row[2] = (double)a.m.total[0];
    row[3] = part[1][0];
    row[4] = part[2][0];
  }
}

}  // namespace

#endif  // HERMNET_PIMD_STEP_H
