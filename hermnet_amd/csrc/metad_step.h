// Multiple-walker metadynamics between the force backward and the finish of a replayed MD step (metad_kernels.hip;
// hermnet_amd/metad.py: DeviceMetaD): ONE text for the device kernels, the host twins (hermnet_host_metad_*) and --
// transcribed operation by operation -- tests/metad_reference.py.  Contraction is off inside every function: IEEE +, -, x, /,
// sqrt, floor and ldexp on doubles, one rounding each, in the order written.  No float atomics, no library exp, no pow.
//
// The B graphs are B walkers of ONE system of n_rep = N / B atoms (walker g: rows g n_rep .. (g + 1) n_rep) under one shared
// bias  V(s) = sum_k h_k prod_d mt_exp(-(s_d - c_kd)^2 / (2 sigma_d^2))  over the hill list (hill_count, hill_centres [K,D],
// hill_heights [K]).  D = 1 or 2 collective variables, cv_kind [D,2] int32 = (kind, p):
//   MT_DISTANCE      the length of the minimum-image vector between two weighted centres.  cv_weight [D,2,n_rep] holds the
//                    normalised weights of group a and of group b (0 outside a group); a centre is the canonical sum of
//                    w_i u_i over the UNWRAPPED u_i = x_i + image_i cell, so a group that straddles the boundary is whole.
//                    d = observe_step.h's minimum image of (centre a, centre b), s = sqrt(|d|^2), e = d / s (0 at s = 0),
//                    ds/dx_i = (wa_i - wb_i) e.
//   MT_COORDINATION  s = scale sum_{i in A} sum_{j in B, j != i} st(r_ij), cv_role [D,n_rep] bit 0 = in A, bit 1 = in B.
//                    w = r^2 / r0^2, p = nn / 2, sw = 1 / (1 + w^p) (the rational switch with mm = 2 nn: no singularity, no
//                    sqrt; w^p by p - 1 multiplications), st = (sw - s_c) inv_norm for r^2 < r_cut^2 and 0 beyond, so it
//                    reaches 0 at r_cut.  cv_par [D,8] = (1 / r0^2, r_cut^2, s_c = sw(w_c), inv_norm = 1 / (1 - s_c),
//                    2 inv_norm / r0^2, scale = 1 or 1 / |A|, -, -), made on the host.  Every atom OWNS its gradient: lane i
//                    walks all partners j of its walker in ascending j and adds (A_i B_j + B_i A_j) grad_i st(r_ij), so a
//                    pair is visited from both ends and nothing is scattered -- no atomics, and the order of a lane's sum
//                    is the order of a serial loop over j, whatever the tiling.
//
// The stage is four launches in front of the UNCHANGED hermnet_md_finish, which is handed forces_b in the place of the step's
// forces (f_prev therefore holds biased forces).  What a replay does is decided by mt_phase from the words the step began
// with and hn_step_code on the step's own energy / total, exactly as md_finish.h's md_committed decides it:
//   MT_IDLE    halted or parked: nothing is read or written.
//   MT_VOID    the evaluation is void: forces_b = forces, untouched; no hill, no row.  (The finish restores the atoms.)
//   MT_PRIME   mode 1: the bias is applied; no hill, no row.
//   MT_COMMIT  the bias is applied, row step % log_steps of cv_log [log_steps,B,D+2] = (s_1..s_D, V(s), height deposited or
//              0) is written, and where (step + 1) % pace == 0 every walker appends one hill at its own s in ascending walker
//              order; height h, or well-tempered h mt_exp(-V(s) inv_kt) with inv_kt = 1 / (kB (gamma - 1) T).
// With state step = s the advance has moved the atoms to x(s+1): CVs, bias forces, row and hill belong to x(s+1), and V is
// the bias of the hills counted when the step began -- every walker of one deposit sees the same list.
//   1  mt_stage / mt_coord_lane / mt_distance_atom   one lane per atom: cv_atom [D,N,6] = (c_i, grad_i, -, -) or (wa u, wb u)
//   2  mt_walker      one workgroup per walker: s by hn_canonical_sums over its atoms; V and dV/ds_d by hn_canonical_sums
//                     over the HILL index (lane l takes hills l, l + 256, ... ascending, then the same fold tree);
//                     cv_walker [B,16] = (s_0, s_1, V, dV/ds_0, dV/ds_1, height, e_0[3], e_1[3], ...) and the row
//   3  mt_apply_one   nb = sum_d dV/ds_d ds_d/dx_i from 0.0;  bias_forces = -nb;  forces_b = (float)((double)f - nb)
//   4  mt_deposit     one workgroup, the single writer of the hill list and of hill_count
//
// mt_exp: device and host library exp do not agree to the last bit, and this bias steers a trajectory.  k = floor(a log2(e)
// + 1/2), r = (a - k ln2_hi) - k ln2_lo (ln 2 in two parts, the high one with 21 trailing zero bits so that k ln2_hi is exact),
// a Horner polynomial of DEGREE 13 in r with the coefficients 1 / j!, ldexp by k.  |r| <= ln 2 / 2 + 1e-13, so the
// truncation term is r^14 / 14! < 5e-18, below the rounding of the sum (1.1e-16).  Arguments below -745 (and NaN) give 0.
#ifndef HERMNET_METAD_STEP_H
#define HERMNET_METAD_STEP_H

#include "observe_step.h"

#define MT_DISTANCE 1
#define MT_COORDINATION 2
#define MT_TILE 256          // atoms of a tile of the pair pass = lanes of its workgroup
#define MT_ATOM_WIDTH 6      // cv_atom [D,N,6]
#define MT_WALKER_WIDTH 16   // cv_walker [B,16]
#define MT_W_V 2
#define MT_W_DV 3
#define MT_W_HEIGHT 5
#define MT_W_E 6

#define MT_IDLE 0
#define MT_PRIME 1
#define MT_COMMIT 2
#define MT_VOID 3

namespace {

struct MetadArgs {
  int n, num_graphs, n_rep, num_cvs;
  const int* graph_ptr;
  const double* x;
  const int* image;
  const float* cell32;               // [B,3,3]
  const double* inv_cell;            // [B,3,3] float64
  const int* cv_kind;                // [D,2]
  const double* cv_par;              // [D,8]
  const unsigned char* cv_role;      // [D,n_rep]
  const double* cv_weight;           // [D,2,n_rep]
  const double* sigma_par;           // [D,2] = (1 / (2 sigma^2), 1 / sigma^2)
  double height, inv_kt;             // inv_kt = 0.0: no tempering
  long pace, max_hills;
  const float *forces, *energy;
  const long* total;
  long capacity;
  const long* state;                 // NULL (hermnet_metad_cv): always MT_PRIME
  double *cv_atom, *cv_walker;       // scratch [D,N,6], [B,16]
  long* hill_count;                  // [1]; mt_deposit
  double *hill_centres, *hill_heights;
  float* forces_b;                   // [N,3]: what the finish reads
  double *bias_forces, *cv_log;      // [N,3], [log_steps,B,D+2]
  long log_steps;
};

inline bool mt_cv_args_ok(const MetadArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || a.num_cvs < 1 || a.num_cvs > 2 || a.n % a.num_graphs != 0) return false;
  if (a.n_rep != a.n / a.num_graphs || !a.graph_ptr || !a.cell32 || !a.inv_cell || !a.cv_kind || !a.cv_par || !a.cv_walker) return false;
  return a.n == 0 || (a.x && a.image && a.cv_role && a.cv_weight && a.cv_atom);
}

inline bool mt_args_ok(const MetadArgs& a) {
  if (!mt_cv_args_ok(a) || a.pace < 1 || a.max_hills < 1 || a.log_steps < 1 || a.capacity < 0) return false;
  if (!a.sigma_par || !a.energy || !a.total || !a.state || !a.hill_count || !a.hill_centres || !a.hill_heights || !a.cv_log)
    return false;
  return a.n == 0 || (a.forces && a.forces_b && a.bias_forces);
}

// What only a host twin can check: the walkers tile the atoms in equal ranges, kinds and powers are the known ones.
inline bool mt_host_args_ok(const MetadArgs& a) {
  for (int g = 0; g <= a.num_graphs; ++g)
    if (a.graph_ptr[g] != g * a.n_rep) return false;
  for (int d = 0; d < a.num_cvs; ++d) {
    const int kind = a.cv_kind[2 * d], p = a.cv_kind[2 * d + 1];
    if (kind != MT_DISTANCE && (kind != MT_COORDINATION || p < 1 || p > 64)) return false;
  }
  return true;
}

// ---- exp ------------------------------------------------------------------------------------------------------------------------
HN_HD inline double mt_exp(double a) {
#pragma clang fp contract(off)
  if (!(a >= -745.0)) return 0.0;
  const double k = floor(a * 1.44269504088896338700e+00 + 0.5);
  const double r = (a - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
  double p = 1.0 / 6227020800.0;                                           // 1 / 13!
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  return ldexp(p, (int)k);
}

// w^k by k multiplications from 1.0 (k = 0: 1.0).
HN_HD inline double mt_powi(double w, int k) {
#pragma clang fp contract(off)
  double r = 1.0;
  for (int j = 0; j < k; ++j) r = r * w;
  return r;
}

// The shifted switch st(r2) and g with grad_i st = g d (d from j to i), for r2 < r_cut^2.
HN_HD inline void mt_switch(double r2, const double* par, int p, double* st, double* g) {
#pragma clang fp contract(off)
  const double w = r2 * par[0];
  const double wp1 = mt_powi(w, p - 1);
  const double sw = 1.0 / (1.0 + wp1 * w);
  *st = (sw - par[2]) * par[3];
  *g = -((((double)p * wp1) * (sw * sw)) * par[4]);
}

// ---- the step's phase -----------------------------------------------------------------------------------------------------------
// On the device every lane of the workgroup calls it (hn_step_code ends in a barrier) and every lane gets the same answer.
HN_HD inline int mt_phase(const MetadArgs& a, long* step) {
  *step = 0;
  if (!a.state) return MT_PRIME;
  *step = a.state[HN_STATE_STEP];
  const long mode = a.state[HN_STATE_MODE];
  if (a.state[HN_STATE_CODE] != 0) return MT_IDLE;
  if (hn_step_code(a.energy, a.num_graphs, a.total, a.capacity) != 0) return MT_VOID;
  return mode != 0 ? MT_PRIME : MT_COMMIT;
}

HN_HD inline long mt_hills(const MetadArgs& a) {
  const long k = a.hill_count ? a.hill_count[0] : 0;
  return k < 0 ? 0 : (k > a.max_hills ? a.max_hills : k);
}

HN_HD inline void mt_cell(const MetadArgs& a, int g, double cell[9]) {
  for (int k = 0; k < 9; ++k) cell[k] = (double)a.cell32[9 * (size_t)g + k];
}

// The atoms of tile t of walker g: the first one and how many (0: the tile lies behind the walker).
HN_HD inline int mt_tile(const MetadArgs& a, int g, int t, int* first) {
  const int lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.n);
  *first = lo + t * MT_TILE;
  const int count = hi - *first;
  return t < 0 || count < 0 ? 0 : (count > MT_TILE ? MT_TILE : count);
}

HN_HD inline int mt_role(const MetadArgs& a, int d, int g, int i) {
  const int local = i - hn_graph_lo(a.graph_ptr, g);
  return local < 0 || local >= a.n_rep ? 0 : (int)a.cv_role[(size_t)d * a.n_rep + local];
}

HN_HD inline double mt_weight(const MetadArgs& a, int d, int which, int g, int i) {
  const int local = i - hn_graph_lo(a.graph_ptr, g);
  return local < 0 || local >= a.n_rep ? 0.0 : a.cv_weight[((size_t)d * 2 + which) * a.n_rep + local];
}

// ---- launch 1: one lane per atom ------------------------------------------------------------------------------------------------
// Atom i's fractional coordinate and its role in CV d.
HN_HD inline int mt_atom(const MetadArgs& a, int d, int g, int i, double s[3]) {
  obs_fractional(a.x[3 * (size_t)i], a.x[3 * (size_t)i + 1], a.x[3 * (size_t)i + 2], a.inv_cell + 9 * (size_t)g, s);
  return mt_role(a, d, g, i);
}

// Lane l stages atom l of tile t as [component][lane] with its role byte.
HN_HD inline void mt_stage(const MetadArgs& a, int d, int g, int t, int l, double (*sj)[MT_TILE], unsigned char* rj) {
  int first;
  if (l >= mt_tile(a, g, t, &first)) return;
  double s[3];
  rj[l] = (unsigned char)mt_atom(a, d, g, first + l, s);
  for (int k = 0; k < 3; ++k) sj[k][l] = s[k];
}

// Atom i (fractional si, role ri) against the staged tile t in ascending j: acc = (sum B_j st, the gradient it owns).
HN_HD inline void mt_coord_lane(const MetadArgs& a, int d, int g, int i, int t, const double (*sj)[MT_TILE], const unsigned char* rj,
                                const double si[3], int ri, const double cell[9], double acc[4]) {
#pragma clang fp contract(off)
  if (ri == 0) return;
  const double* par = a.cv_par + 8 * (size_t)d;
  const int p = a.cv_kind[2 * d + 1];
  int first;
  const int count = mt_tile(a, g, t, &first);
  for (int m = 0; m < count; ++m) {
    if (first + m == i) continue;
    const int rm = rj[m];
    const bool ab = (ri & 1) && (rm & 2), ba = (ri & 2) && (rm & 1);
    if (!ab && !ba) continue;
    double dv[3], st, gr;
    const double r2 = obs_min_image(si, sj[0][m], sj[1][m], sj[2][m], cell, true, dv);
    if (!(r2 < par[1])) continue;
    mt_switch(r2, par, p, &st, &gr);
    if (ab) acc[0] = acc[0] + st;
    const double c = (ab && ba ? 2.0 : 1.0) * gr;
    for (int k = 0; k < 3; ++k) acc[1 + k] = acc[1 + k] + c * dv[k];
  }
}

HN_HD inline void mt_coord_store(const MetadArgs& a, int d, int i, const double acc[4]) {
#pragma clang fp contract(off)
  double* out = a.cv_atom + ((size_t)d * a.n + i) * MT_ATOM_WIDTH;
  const double scale = a.cv_par[8 * (size_t)d + 5];
  for (int k = 0; k < 4; ++k) out[k] = acc[k] * scale;
  out[4] = out[5] = 0.0;
}

// A distance's per-atom terms: (wa u, wb u) of the unwrapped u = x + image cell.
HN_HD inline void mt_distance_atom(const MetadArgs& a, int d, int g, int i) {
#pragma clang fp contract(off)
  double cell[9];
  mt_cell(a, g, cell);
  const double wa = mt_weight(a, d, 0, g, i), wb = mt_weight(a, d, 1, g, i);
  const int* im = a.image + 3 * (size_t)i;
  double* out = a.cv_atom + ((size_t)d * a.n + i) * MT_ATOM_WIDTH;
  for (int k = 0; k < 3; ++k) {
    const double u = a.x[3 * (size_t)i + k] + (((double)im[0] * cell[k] + (double)im[1] * cell[3 + k]) + (double)im[2] * cell[6 + k]);
    out[k] = wa * u;
    out[3 + k] = wb * u;
  }
}

// ---- launch 2: one workgroup per walker -----------------------------------------------------------------------------------------
HN_HD inline void mt_distance(const MetadArgs& a, int g, const double c[6], double* s, double e[3]) {
#pragma clang fp contract(off)
  double cell[9], sa[3], sb[3], dv[3];
  mt_cell(a, g, cell);
  obs_fractional(c[0], c[1], c[2], a.inv_cell + 9 * (size_t)g, sa);
  obs_fractional(c[3], c[4], c[5], a.inv_cell + 9 * (size_t)g, sb);
  const double r = sqrt(obs_min_image(sa, sb[0], sb[1], sb[2], cell, true, dv));
  *s = r;
  for (int k = 0; k < 3; ++k) e[k] = r > 0.0 ? dv[k] / r : 0.0;
}

// Hill k's terms of (V, dV/ds_0, dV/ds_1) at s.
HN_HD inline void mt_hill_term(const MetadArgs& a, int k, const double s[2], double* acc) {
#pragma clang fp contract(off)
  double gk = a.hill_heights[k], dd[2] = {0.0, 0.0};
  for (int d = 0; d < a.num_cvs; ++d) {
    dd[d] = s[d] - a.hill_centres[(size_t)k * a.num_cvs + d];
    gk = gk * mt_exp(-((dd[d] * dd[d]) * a.sigma_par[2 * d]));
  }
  acc[0] = acc[0] + gk;
  for (int d = 0; d < a.num_cvs; ++d) acc[1 + d] = acc[1 + d] + gk * (-(dd[d] * a.sigma_par[2 * d + 1]));
}

// Walker g (256 lanes together; the host walks them).  `bias`: with the hills (hermnet_metad_cv stops at the CVs).
HN_HD inline void mt_walker(const MetadArgs& a, int g, int phase, long step, bool bias, double (*part)[256]) {
#pragma clang fp contract(off)
  const int lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.n), D = a.num_cvs;
  double s[2] = {0.0, 0.0}, e[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, sums[3] = {0.0, 0.0, 0.0};
  for (int d = 0; d < D; ++d) {
    const double* atom = a.cv_atom + (size_t)d * a.n * MT_ATOM_WIDTH;
    if (a.cv_kind[2 * d] == MT_DISTANCE) {
      hn_canonical_sums<6, -1>(lo, hi, part, [&](int i, double* acc) {
        for (int k = 0; k < 6; ++k) acc[k] = acc[k] + atom[(size_t)i * MT_ATOM_WIDTH + k];
      });
      double c[6];
      for (int k = 0; k < 6; ++k) c[k] = part[k][0];
      mt_distance(a, g, c, &s[d], e[d]);
    } else {
      hn_canonical_sums<1, -1>(lo, hi, part, [&](int i, double* acc) { acc[0] = acc[0] + atom[(size_t)i * MT_ATOM_WIDTH]; });
      s[d] = part[0][0];
    }
    hn_barrier();      // every lane has read the sums before `part` is used again
  }
  if (bias) {
    hn_canonical_sums<3, -1>(0, (int)mt_hills(a), part, [&](int k, double* acc) { mt_hill_term(a, k, s, acc); });
    for (int k = 0; k < 3; ++k) sums[k] = part[k][0];
    hn_barrier();
  }
  if (!hn_lead_lane()) return;
  double* w = a.cv_walker + (size_t)g * MT_WALKER_WIDTH;
  double h = 0.0;
  if (bias && phase == MT_COMMIT && (step + 1) % a.pace == 0) h = a.inv_kt != 0.0 ? a.height * mt_exp(-(sums[0] * a.inv_kt)) : a.height;
  w[0] = s[0];
  w[1] = s[1];
  for (int k = 0; k < 3; ++k) w[MT_W_V + k] = sums[k];
  w[MT_W_HEIGHT] = h;
  for (int d = 0; d < 2; ++d)
    for (int k = 0; k < 3; ++k) w[MT_W_E + 3 * d + k] = e[d][k];
  if (bias && phase == MT_COMMIT) {
    double* row = hn_log_row(a.cv_log, step, a.log_steps, a.num_graphs, g, D + 2);
    for (int d = 0; d < D; ++d) row[d] = s[d];
    row[D] = sums[0];
    row[D + 1] = h;
  }
}

// ---- launch 3: one lane per atom ------------------------------------------------------------------------------------------------
HN_HD inline int mt_walker_of(const MetadArgs& a, int i) {
  const int g = a.n_rep > 0 ? i / a.n_rep : 0;
  return g >= a.num_graphs ? a.num_graphs - 1 : g;
}

// ds_d / dx_i.
HN_HD inline void mt_cv_grad(const MetadArgs& a, int d, int g, int i, double out[3]) {
#pragma clang fp contract(off)
  if (a.cv_kind[2 * d] == MT_DISTANCE) {
    const double w = mt_weight(a, d, 0, g, i) - mt_weight(a, d, 1, g, i);
    const double* e = a.cv_walker + (size_t)g * MT_WALKER_WIDTH + MT_W_E + 3 * d;
    for (int k = 0; k < 3; ++k) out[k] = w * e[k];
  } else {
    const double* atom = a.cv_atom + ((size_t)d * a.n + i) * MT_ATOM_WIDTH;
    for (int k = 0; k < 3; ++k) out[k] = atom[1 + k];
  }
}

HN_HD inline void mt_apply_one(const MetadArgs& a, int i, int phase) {
#pragma clang fp contract(off)
  if (phase == MT_VOID) {
    for (int k = 0; k < 3; ++k) a.forces_b[3 * (size_t)i + k] = a.forces[3 * (size_t)i + k];
    return;
  }
  const int g = mt_walker_of(a, i);
  const double* w = a.cv_walker + (size_t)g * MT_WALKER_WIDTH;
  double nb[3] = {0.0, 0.0, 0.0}, grad[3];
  for (int d = 0; d < a.num_cvs; ++d) {
    mt_cv_grad(a, d, g, i, grad);
    for (int k = 0; k < 3; ++k) nb[k] = nb[k] + w[MT_W_DV + d] * grad[k];
  }
  for (int k = 0; k < 3; ++k) {
    a.bias_forces[3 * (size_t)i + k] = -nb[k];
    a.forces_b[3 * (size_t)i + k] = (float)((double)a.forces[3 * (size_t)i + k] - nb[k]);
  }
}

// ---- launch 4: one workgroup (host: first = 0, stride = 1), the single writer of the hill list -------------------------------------
HN_HD inline void mt_deposit(const MetadArgs& a, int phase, long step, int first, int stride) {
  if (phase != MT_COMMIT || (step + 1) % a.pace != 0) return;
  const long count = mt_hills(a);
  for (int g = first; g < a.num_graphs; g += stride) {
    const long k = count + g;
    if (k >= a.max_hills) continue;
    const double* w = a.cv_walker + (size_t)g * MT_WALKER_WIDTH;
    for (int d = 0; d < a.num_cvs; ++d) a.hill_centres[(size_t)k * a.num_cvs + d] = w[d];
    a.hill_heights[k] = w[MT_W_HEIGHT];
  }
  hn_barrier();        // every lane has read the count
  if (hn_lead_lane()) a.hill_count[0] = count + a.num_graphs > a.max_hills ? a.max_hills : count + a.num_graphs;
}

// hermnet_metad_cv's last pass, lane i: atom i's gradients [D,N,3] and (the lanes below B D) the values [B,D].
HN_HD inline void mt_report_lane(const MetadArgs& a, int i, double* values, double* grads) {
  if (i < a.n)
    for (int d = 0; d < a.num_cvs; ++d) mt_cv_grad(a, d, mt_walker_of(a, i), i, grads + ((size_t)d * a.n + i) * 3);
  if (i < a.num_graphs * a.num_cvs) values[i] = a.cv_walker[(size_t)(i / a.num_cvs) * MT_WALKER_WIDTH + i % a.num_cvs];
}

}  // namespace

#endif  // HERMNET_METAD_STEP_H
