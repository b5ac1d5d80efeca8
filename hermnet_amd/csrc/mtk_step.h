// Nose-Hoover (MTK) barostat NPT inside the replayed MD step (mtk_kernels.hip; hermnet_amd/mtk.py: DeviceMTK): ONE text for
// the device kernels, the host twins (hermnet_host_mtk_advance / _finish) and -- transcribed operation by operation --
// tests/mtk_reference.py.  Contraction is off inside every function: IEEE +, x, floor, ldexp and the library's own exp
// (metad_step.h: mt_exp) on doubles, one rounding each, in the order written.  Divisions: npt_inverse3's (DeviceNPT's
// precedent) and the one of the log's pressure column, which steers nothing; every other one is made on the host.
//
// The integrator is the isotropic Martyna-Tobias-Klein barostat as made measure-preserving and reversible by Tuckerman,
// Alejandre, Lopez-Rendon, Jochim and Martyna (J. Phys. A 39, 5629 (2006)), and its per-axis form (LAMMPS: fix npt iso /
// aniso).  Per graph: v_g[3], the diagonal of the cell's rate in Cartesian axes ("isotropic": the three entries are one number
// v_eps; "axes": the entries outside `mask` stay 0), with the mass w = (dof + 3) kB T taup^2 (isotropic) or a third of that per
// axis; the particles' chain (nhc_step.h, unchanged) and a second chain of the same M / order / substeps on the barostat,
// whose K2 is w sum_coupled v_g^2 (isotropic: w v_eps^2) and whose dof is 1 or the number of coupled axes.
//
// One time step (NHC = nhc_half_step; hdt = dt / 2, qdt = dt / 4; W: the float32 virial with npt_step.h's sign, P = (sum m v v +
// sym W) / V; V = |det cell64| as it stands):
//    1  NHC_baro(hdt): its factor on v_g                                                            mtk_open_kernel
//    2  NHC_particles(hdt) from the canonical E_kin of v as it stands: s = scale[g][0]; K2 = (K2 s) s, K2_aa likewise
//    3  v_g += hdt G from w_prev, the virial of the last accepted evaluation (mtk_kick_baro):
//         isotropic  G   = (((1 + 3/dof) K2 + tr W) - (3 P0) V) inv_w
//         axes       G_a = (((K2_aa + W_aa) - P0 V) + K2 / dof) inv_w      on the axes of `mask`
//       then the factors (mtk_make_factors), rho_a = v_g,a + (sum_b v_g,b) / dof:
//         a_a = exp(-rho_a hdt)   b_a = exp(-rho_a qdt) sinhc(rho_a qdt)   rx_a = exp(v_g,a dt)   rv_a = exp(v_g,a hdt) sinhc(v_g,a hdt)
//       and the cell: column a of cell64 times rx_a, cell32 its rounding, inv_cell = npt_inverse3 of the widened cell32
//    4  v = (v s) a + (kick f_prev) b                                                               mtk_advance_kernel
//    5  x = x rx + (dt v) rv, the wrap in the new cell, pos32
//    6  [search, forces, virial in the new cell]
//    7  v = v a + (kick f) b   (v_g has not moved since step 3: the same numbers)                   mtk_finish_atoms_kernel
//    8  v_g += hdt G from the new K2, K2_aa, the step's own virial and the new volume               mtk_close_kernel
//    9  NHC_particles(hdt): s = scale[g][1]; NHC_baro(hdt); the log row; w_prev = the step's virial
//   10  v = v s                                                                                     mtk_scale_kernel
// Conserved: E_pot + E_kin + P0 V + w sum_coupled v_g^2 / 2 + E_nhc(particles) + E_nhc(barostat) = log columns 0 + 1 + 3 + 6.
//
// Limits that hold by bits.  taup = inf: w = inv_w = 0 and the barostat's chain is off, v_g stays 0, every factor is exactly
// 1.0 (mt_exp(+-0) = mtk_sinhc(0) = 1.0), and a graph whose three rx are exactly 1.0 leaves cell64, cell32 and inv_cell
// unwritten: that graph is hermnet_nhc_advance's / _finish's bit for bit.  tau = inf switches both chains off (NPH).
//
// Void steps.  The search must never read a cell that is not finite: a graph is FLAGGED (flag[g] = 1) where |v_g,a| dt >
// max_strain or a factor is not finite, and then takes identity factors -- its cell stays, its atoms make a plain drift.  The
// finish ORs the flags, and a virial entry that is not finite, into the step's code as HN_HALT_NONFINITE (mtk_code; every
// workgroup derives the same code from arrays no kernel of the finish writes).  The step is then void: atoms, v_g, both chains
// and the three forms of the cell return (`backup`), no row is written.  md_commit_kernel<> is md_finish.h's, unchanged: it
// reads e_code [B] in the place of the energies -- mtk_close_kernel writes energy[g] there, or NaN where mtk_code found more
// than hn_step_code.  A prime copies forces to f_prev and the virial to w_prev and touches nothing else.
#ifndef HERMNET_MTK_STEP_H
#define HERMNET_MTK_STEP_H

#include "nhc_step.h"
#include "npt_step.h"

#define HN_MTK_LOG_WIDTH 7
#define HN_MTK_FACTORS 12                      // factors [B,12] = a[3], b[3], rx[3], rv[3]
#define HN_MTK_PAR 5                           // par [B,5] = w, 1 / w, 1 + 3 / dof, 1 / dof, P0
#define HN_MTK_BACKUP(M) (2 * (M) + 30)        // backup [B,2M+30] = xi_b, v_xi_b, v_g[3], cell64[9], cell32[9] widened, inv_cell[9]

// sinh(x) / x: the even polynomial through x^10 with the coefficients 1 / (2k + 1)!, by Horner in x^2.  |x| <= 0.1 (the
// constructor's bound on max_strain): the truncation term x^12 / 13! is below 2e-22.
HN_HD inline double mtk_sinhc(double x) {
#pragma clang fp contract(off)
  const double y = x * x;
  double p = 1.0 / 39916800.0;                 // 1 / 11!
  p = p * y + 1.0 / 362880.0;
  p = p * y + 1.0 / 5040.0;
  p = p * y + 1.0 / 120.0;
  p = p * y + 1.0 / 6.0;
  p = p * y + 1.0;
  return p;
}

namespace {

// The barostats of the B graphs: constants made on the host, the state, the scratch and the backup.
struct MtkBaro {
  int coupling, mask;                // HN_MD_BARO_ISOTROPIC or _AXES; bit a: axis a is coupled (isotropic: 7)
  double max_strain;                 // the largest |v_g,a| dt of a step that is not refused
  const double* par;                 // [B,5]
  const double *dof_kt, *q, *inv_q;  // the barostat chain's [B], [B,M], [B,M]; off: q = inv_q = 0
  double *xi, *v_xi, *scale;         // the barostat's chain [B,M] and its last opening / closing factor [B,2]
  double *v_cell, *cell64;           // v_g [B,3]; the cell [B,9] float64: the truth
  float* cell32;                     // [B,9]: what the search reads
  double* inv_cell;                  // [B,9]: of the widened cell32
  float* w_prev;                     // [B,9]: the virial of the last accepted evaluation
  double *factors, *backup;          // [B,12]; [B,2M+30]
  long *flag, *refused;              // [B]: this step's factors were refused; how often
  float* e_code;                     // [B]: what md_commit_kernel<> reads as the energies
};

struct MtkAdvanceArgs {
  MdAdvanceArgs m;                   // hermnet_md_advance's, without a Langevin thermostat; cell, inv_cell: b's
  const int* graph_ptr;
  const double* half_mass;
  NhcChains c;
  MtkBaro b;
};

struct MtkFinishArgs {
  MdFinishArgs m;
  const long* batch;
  const float* virial;               // [B,9]: the step's own
  double dt;
  NhcChains c;
  MtkBaro b;
};

inline bool mtk_baro_ok(const MtkBaro& b) {
  if (b.coupling != HN_MD_BARO_ISOTROPIC && b.coupling != HN_MD_BARO_AXES) return false;
  if ((b.mask & ~7) || b.mask == 0 || !(b.max_strain > 0.0) || !(b.max_strain <= 0.1)) return false;
  if (b.coupling == HN_MD_BARO_ISOTROPIC && b.mask != 7) return false;
  return b.par && b.dof_kt && b.q && b.inv_q && b.xi && b.v_xi && b.scale && b.v_cell && b.cell64 && b.cell32 && b.inv_cell &&
         b.w_prev && b.factors && b.backup && b.flag && b.refused && b.e_code;
}

inline bool mtk_advance_args_ok(const MtkAdvanceArgs& a) {
  if (!md_advance_args_ok(a.m) || (a.m.flags & HN_MD_LANGEVIN) || !a.m.state || !a.graph_ptr || !(a.m.dt > 0.0)) return false;
  return nhc_chains_ok(a.c) && mtk_baro_ok(a.b) && (a.m.n == 0 || a.half_mass);
}

inline bool mtk_finish_args_ok(const MtkFinishArgs& a) {
  return md_finish_args_ok(a.m) && a.virial && a.dt > 0.0 && nhc_chains_ok(a.c) && mtk_baro_ok(a.b);
}

// The barostat's chain in the form nhc_half_step and nhc_energy read (they touch the tables alone).
HN_HD inline NhcChains mtk_baro_chain(const NhcChains& c, const MtkBaro& b) {
  const NhcChains r = {c.chain, c.order, c.substeps, c.delta, c.kt, b.dof_kt, b.q, b.inv_q, b.xi, b.v_xi, nullptr, nullptr, b.scale};
  return r;
}

HN_HD inline double mtk_abs(double a) { return a < 0.0 ? -a : a; }

// |det cell64[g]|.
HN_HD inline double mtk_volume(const MtkBaro& b, int g) {
  double c[9];
  for (int k = 0; k < 9; ++k) c[k] = b.cell64[9 * (size_t)g + k];
  return mtk_abs(npt_det3(c));
}

// sum_coupled v_g^2: one number where the coupling is isotropic.
HN_HD inline double mtk_rate2(const MtkBaro& b, const double vg[3]) {
#pragma clang fp contract(off)
  if (b.coupling == HN_MD_BARO_ISOTROPIC) return vg[0] * vg[0];
  double s = 0.0;
  for (int k = 0; k < 3; ++k)
    if (b.mask & (1 << k)) s = s + vg[k] * vg[k];
  return s;
}

// NHC_baro(hdt) of graph g on the caller's xi, v [M] and vg: slot 0 the opening one, 1 the closing one.
HN_HD inline void mtk_baro_half(const NhcChains& c, const MtkBaro& b, int g, double* xi, double* v, double vg[3], int slot) {
#pragma clang fp contract(off)
  const NhcChains bc = mtk_baro_chain(c, b);
  double k2 = b.par[HN_MTK_PAR * (size_t)g] * mtk_rate2(b, vg);
  const double s = nhc_half_step(bc, g, xi, v, &k2);
  b.scale[2 * (size_t)g + slot] = s;
  for (int k = 0; k < 3; ++k) vg[k] = vg[k] * s;
}

// v_g += hdt G (steps 3 and 8).  k2 = 2 E_kin, kaa[3] = sum m v_a v_a, w: a float32 virial [9].  A barostat that is off (inv_w
// = 0) is left alone, whatever the sums are.
HN_HD inline void mtk_kick_baro(const MtkBaro& b, int g, double hdt, double k2, const double kaa[3], const float* w, double vol,
                                double vg[3]) {
#pragma clang fp contract(off)
  const double* par = b.par + HN_MTK_PAR * (size_t)g;
  const double inv_w = par[1], p0 = par[4];
  if (inv_w == 0.0) return;
  if (b.coupling == HN_MD_BARO_ISOTROPIC) {
    const double trw = ((double)w[0] + (double)w[4]) + (double)w[8];
    const double gf = ((par[2] * k2 + trw) - (3.0 * p0) * vol) * inv_w;
    const double v = vg[0] + hdt * gf;
    vg[0] = vg[1] = vg[2] = v;
    return;
  }
  for (int k = 0; k < 3; ++k)
    if (b.mask & (1 << k)) {
      const double gf = (((kaa[k] + (double)w[4 * k]) - p0 * vol) + k2 * par[3]) * inv_w;
      vg[k] = vg[k] + hdt * gf;
    }
}

// The step's twelve factors from v_g; returns 1 where they are refused (then every factor is 1.0).
HN_HD inline int mtk_make_factors(const MtkBaro& b, int g, double dt, const double vg[3], double* f) {
#pragma clang fp contract(off)
  const double hdt = 0.5 * dt, qdt = 0.25 * dt, inv_dof = b.par[HN_MTK_PAR * (size_t)g + 3];
  int bad = 0;
  for (int k = 0; k < 3; ++k)
    if (!(mtk_abs(vg[k] * dt) <= b.max_strain)) bad = 1;
  if (!bad) {
    const double sum = (vg[0] + vg[1]) + vg[2];
    for (int k = 0; k < 3; ++k) {
      const double rho = vg[k] + sum * inv_dof;
      const double xa = rho * hdt, xb = rho * qdt, xr = vg[k] * hdt;
      f[k] = mt_exp(-xa);
      f[3 + k] = mt_exp(-xb) * mtk_sinhc(xb);
      f[6 + k] = mt_exp(vg[k] * dt);
      f[9 + k] = mt_exp(xr) * mtk_sinhc(xr);
    }
    for (int k = 0; k < HN_MTK_FACTORS; ++k) bad |= npt_not_finite(f[k]);
  }
  if (bad)
    for (int k = 0; k < HN_MTK_FACTORS; ++k) f[k] = 1.0;
  return bad;
}

// The four canonical sums of graph g in ONE call: E_kin exactly as nhc_step.h / md_finish.h make it (from v and half_mass
// where ke_atom is null, else from ke_atom), and sum m v_a v_a for the three axes (m = 2 half_mass: exact).
HN_HD inline void mtk_kinetic_sums(const int* graph_ptr, int n, int g, const double* v, const double* half_mass,
                                   const double* ke_atom, double (*part)[256], double* e_kin, double kaa[3]) {
#pragma clang fp contract(off)
  const int lo = hn_graph_lo(graph_ptr, g), hi = hn_graph_hi(graph_ptr, g, n);
  hn_canonical_sums<4, -1>(lo, hi, part, [&](int i, double* s) {
    const double v0 = v[3 * (size_t)i], v1 = v[3 * (size_t)i + 1], v2 = v[3 * (size_t)i + 2];
    const double m = 2.0 * half_mass[i];
    s[0] = s[0] + (ke_atom ? ke_atom[i] : half_mass[i] * ((v0 * v0 + v1 * v1) + v2 * v2));
    s[1] = s[1] + (m * v0) * v0;
    s[2] = s[2] + (m * v1) * v1;
    s[3] = s[3] + (m * v2) * v2;
  });
  *e_kin = part[0][0];
  for (int k = 0; k < 3; ++k) kaa[k] = part[1 + k][0];
}

// ---- the advance ------------------------------------------------------------------------------------------------------------
// Graph g of a step (mode 0): the backups, steps 1 to 3, the factors, the flag and the new cell in its three forms.
HN_HD inline void mtk_open_one(const MtkAdvanceArgs& a, int g, double e_kin, const double kaa_in[3]) {
#pragma clang fp contract(off)
  const NhcChains& c = a.c;
  const MtkBaro& b = a.b;
  const int M = c.chain;
  double* bk = b.backup + (size_t)g * HN_MTK_BACKUP(M);
  double xi[HN_NHC_MAX_CHAIN], v[HN_NHC_MAX_CHAIN], vg[3], cell[9];
  for (int j = 0; j < M; ++j) {
    bk[j] = xi[j] = b.xi[(size_t)g * M + j];
    bk[M + j] = v[j] = b.v_xi[(size_t)g * M + j];
  }
  for (int k = 0; k < 3; ++k) bk[2 * M + k] = vg[k] = b.v_cell[3 * (size_t)g + k];
  for (int k = 0; k < 9; ++k) {
    bk[2 * M + 3 + k] = cell[k] = b.cell64[9 * (size_t)g + k];
    bk[2 * M + 12 + k] = (double)b.cell32[9 * (size_t)g + k];
    bk[2 * M + 21 + k] = b.inv_cell[9 * (size_t)g + k];
  }
  mtk_baro_half(c, b, g, xi, v, vg, 0);                                        // 1
  for (int j = 0; j < M; ++j) {
    b.xi[(size_t)g * M + j] = xi[j];
    b.v_xi[(size_t)g * M + j] = v[j];
  }
  const double k2 = nhc_graph_one(c, g, e_kin, 0);                             // 2 (the particles' chain is backed up there)
  const double s = c.scale[2 * (size_t)g];
  double kaa[3];
  for (int k = 0; k < 3; ++k) kaa[k] = (kaa_in[k] * s) * s;
  mtk_kick_baro(b, g, 0.5 * a.m.dt, k2, kaa, b.w_prev + 9 * (size_t)g, mtk_abs(npt_det3(cell)), vg);    // 3
  for (int k = 0; k < 3; ++k) b.v_cell[3 * (size_t)g + k] = vg[k];
  double f[HN_MTK_FACTORS];
  b.flag[g] = mtk_make_factors(b, g, a.m.dt, vg, f);
  for (int k = 0; k < HN_MTK_FACTORS; ++k) b.factors[HN_MTK_FACTORS * (size_t)g + k] = f[k];
  if (f[6] == 1.0 && f[7] == 1.0 && f[8] == 1.0) return;                       // the cell stays, unwritten
  double wide[9], inv[9];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      const double ck = cell[3 * i + k] * f[6 + k];
      const float c32 = (float)ck;
      b.cell64[9 * (size_t)g + 3 * i + k] = ck;
      b.cell32[9 * (size_t)g + 3 * i + k] = c32;
      wide[3 * i + k] = (double)c32;
    }
  npt_inverse3(wide, inv);
  for (int k = 0; k < 9; ++k) b.inv_cell[9 * (size_t)g + k] = inv[k];
}

// Atom i: steps 4 and 5 with the wrap in the new cell (mode 0), pos32.
HN_HD inline void mtk_advance_one(const MtkAdvanceArgs& a, int i, long mode) {
#pragma clang fp contract(off)
  const MdAdvanceArgs& m = a.m;
  double x[3], v[3];
  for (int k = 0; k < 3; ++k) x[k] = m.x[3 * (size_t)i + k];
  if (mode == 0) {
    int image[3];
    float f[3];
    for (int k = 0; k < 3; ++k) {
      v[k] = m.v[3 * (size_t)i + k];
      image[k] = m.image[3 * (size_t)i + k];
      f[k] = m.f_prev[3 * (size_t)i + k];
      m.x0[3 * (size_t)i + k] = x[k];
      m.v0[3 * (size_t)i + k] = v[k];
      m.image0[3 * (size_t)i + k] = image[k];
    }
    const long g = hn_graph_of(m.batch, i, m.num_graphs);
    const double s = a.c.scale[2 * (size_t)g], kick = m.kick[i];
    const double* fac = a.b.factors + HN_MTK_FACTORS * (size_t)g;
    for (int k = 0; k < 3; ++k) {
      v[k] = v[k] * s;
      v[k] = v[k] * fac[k] + (kick * (double)f[k]) * fac[3 + k];
      x[k] = x[k] * fac[6 + k] + (m.dt * v[k]) * fac[9 + k];
    }
    if (m.flags & HN_MD_WRAP) {
      double cell[9], inv[9];
      hn_load_cell(m.cell, m.inv_cell, g, cell, inv);
      md_wrap_atom(x, image, cell, inv);
    }
    for (int k = 0; k < 3; ++k) {
      m.x[3 * (size_t)i + k] = x[k];
      m.v[3 * (size_t)i + k] = v[k];
      m.image[3 * (size_t)i + k] = image[k];
    }
  }
  for (int k = 0; k < 3; ++k) m.pos32[3 * (size_t)i + k] = (float)x[k];
}

// ---- the finish -------------------------------------------------------------------------------------------------------------
// What the barostat adds to the step's code for graph g: its flag (a step alone: a prime does not open) and a virial entry
// that is not finite.
HN_HD inline int mtk_bad_graph(const MtkFinishArgs& a, int g, long mode) {
  int bad = (mode == 0 && a.b.flag[g] != 0) ? 1 : 0;
  for (int k = 0; k < 9; ++k) bad |= hn_not_finite(a.virial[9 * (size_t)g + k]);
  return bad;
}

// The step's code: hn_step_code's, and HN_HALT_NONFINITE where a graph is bad; *extra: the latter.  On the device every lane
// of the workgroup calls it, and every lane gets the same answer.
HN_HD inline long mtk_code(const MtkFinishArgs& a, long mode, int* extra) {
  int bad = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  for (int g = threadIdx.x; g < a.m.num_graphs; g += blockDim.x) bad |= mtk_bad_graph(a, g, mode);
  bad = __syncthreads_or(bad);
#else
  for (int g = 0; g < a.m.num_graphs; ++g) bad |= mtk_bad_graph(a, g, mode);
#endif
  const long code = hn_step_code(a.m.energy, a.m.num_graphs, a.m.total, a.m.capacity);
  *extra = bad;
  return bad ? (code | HN_HALT_NONFINITE) : code;
}

// md_finish_one with step 7 in the place of the second kick.
HN_HD inline void mtk_finish_one(const MtkFinishArgs& a, int i, long code, long mode) {
#pragma clang fp contract(off)
  const MdFinishArgs& m = a.m;
  if (mode != 0) {
    if (code == 0)
      for (int k = 0; k < 3; ++k) m.f_prev[3 * (size_t)i + k] = m.forces[3 * (size_t)i + k];
    return;
  }
  if (code != 0) {        // the step is void: back to the state it began with
    hn_restore_atom(i, m.x, m.x0, m.image, m.image0, m.pos32);
    for (int k = 0; k < 3; ++k) m.v[3 * (size_t)i + k] = m.v0[3 * (size_t)i + k];
    return;
  }
  const double* fac = a.b.factors + HN_MTK_FACTORS * (size_t)hn_graph_of(a.batch, i, m.num_graphs);
  const double kick = m.kick[i];
  double v[3];
  for (int k = 0; k < 3; ++k) {
    const float f = m.forces[3 * (size_t)i + k];
    v[k] = m.v[3 * (size_t)i + k] * fac[k] + (kick * (double)f) * fac[3 + k];
    m.v[3 * (size_t)i + k] = v[k];
    m.f_prev[3 * (size_t)i + k] = f;
  }
  m.ke_atom[i] = m.half_mass[i] * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// What md_commit_kernel<> reads in the place of graph g's energy.
HN_HD inline void mtk_code_word(const MtkFinishArgs& a, int g, int extra) {
  a.b.e_code[g] = extra ? __builtin_nanf("") : a.m.energy[g];
}

// Graph g of a step that commits: steps 8 and 9, the log row, w_prev.
HN_HD inline void mtk_close_one(const MtkFinishArgs& a, long step, int g, double e_kin, const double kaa[3]) {
#pragma clang fp contract(off)
  const NhcChains& c = a.c;
  const MtkBaro& b = a.b;
  const int M = c.chain;
  const float* w = a.virial + 9 * (size_t)g;
  const double vol = mtk_volume(b, g);
  double vg[3], xi[HN_NHC_MAX_CHAIN], v[HN_NHC_MAX_CHAIN];
  for (int k = 0; k < 3; ++k) vg[k] = b.v_cell[3 * (size_t)g + k];
  mtk_kick_baro(b, g, 0.5 * a.dt, 2.0 * e_kin, kaa, w, vol, vg);               // 8
  nhc_graph_one(c, g, e_kin, 1);                                               // 9
  const double s = c.scale[2 * (size_t)g + 1];
  for (int j = 0; j < M; ++j) {
    xi[j] = b.xi[(size_t)g * M + j];
    v[j] = b.v_xi[(size_t)g * M + j];
  }
  mtk_baro_half(c, b, g, xi, v, vg, 1);
  for (int j = 0; j < M; ++j) {
    b.xi[(size_t)g * M + j] = xi[j];
    b.v_xi[(size_t)g * M + j] = v[j];
  }
  for (int k = 0; k < 3; ++k) b.v_cell[3 * (size_t)g + k] = vg[k];
  const NhcChains bc = mtk_baro_chain(c, b);
  const double* par = b.par + HN_MTK_PAR * (size_t)g;
  const double trk = (((kaa[0] * s) * s + (kaa[1] * s) * s) + (kaa[2] * s) * s);
  const double trw = ((double)w[0] + (double)w[4]) + (double)w[8];
  double* row = hn_log_row(a.m.log, step, a.m.log_steps, a.m.num_graphs, g, HN_MTK_LOG_WIDTH);
  row[0] = (double)a.m.energy[g];
  row[1] = (e_kin * s) * s;
  row[2] = (double)a.m.total[0];
  row[3] = nhc_energy(c, g, c.xi + (size_t)g * M, c.v_xi + (size_t)g * M) + nhc_energy(bc, g, xi, v);
  row[4] = ((trk + trw) / vol) / 3.0;
  row[5] = vol;
  row[6] = par[4] * vol + 0.5 * (par[0] * mtk_rate2(b, vg));
  for (int k = 0; k < 9; ++k) b.w_prev[9 * (size_t)g + k] = w[k];
}

// Graph g of a void step: the barostat, both chains and the three forms of the cell return; the flag is counted.
HN_HD inline void mtk_restore_one(const MtkFinishArgs& a, int g) {
  const MtkBaro& b = a.b;
  const int M = a.c.chain;
  const double* bk = b.backup + (size_t)g * HN_MTK_BACKUP(M);
  nhc_restore_one(a.c, g);
  for (int j = 0; j < M; ++j) {
    b.xi[(size_t)g * M + j] = bk[j];
    b.v_xi[(size_t)g * M + j] = bk[M + j];
  }
  for (int k = 0; k < 3; ++k) b.v_cell[3 * (size_t)g + k] = bk[2 * M + k];
  for (int k = 0; k < 9; ++k) {
    b.cell64[9 * (size_t)g + k] = bk[2 * M + 3 + k];
    b.cell32[9 * (size_t)g + k] = (float)bk[2 * M + 12 + k];
    b.inv_cell[9 * (size_t)g + k] = bk[2 * M + 21 + k];
  }
  if (b.flag[g] != 0) b.refused[g] = b.refused[g] + 1;
}

// Graph g of a prime whose evaluation stands: the virial the next step's opening reads.
HN_HD inline void mtk_prime_one(const MtkFinishArgs& a, int g) {
  for (int k = 0; k < 9; ++k) a.b.w_prev[9 * (size_t)g + k] = a.virial[9 * (size_t)g + k];
}

// The closing factor on atom i's velocity (a step that commits).
HN_HD inline void mtk_scale_one(const MtkFinishArgs& a, int i) {
#pragma clang fp contract(off)
  const double s = a.c.scale[2 * (size_t)hn_graph_of(a.batch, i, a.m.num_graphs) + 1];
  for (int k = 0; k < 3; ++k) a.m.v[3 * (size_t)i + k] = a.m.v[3 * (size_t)i + k] * s;
}

}  // namespace

#endif  // HERMNET_MTK_STEP_H
