// The arithmetic of the device-resident nudged elastic band (neb_kernels.hip; hermnet_amd/neb.py: DeviceNEB): ONE text for
// the three device kernels of hermnet_neb_finish, the host twin hermnet_host_neb_finish and -- transcribed operation by
// operation -- the numpy float64 reference of tests/neb_reference.py.  NEB with improved tangents (Henkelman & Jonsson, J.
// Chem. Phys. 113, 9978) and a climbing image, as ASE's NEB(method="improvedtangent", climb=...) states it, under ASE's
// FIRE on the WHOLE band (relax_step.h's scalars, unchanged).  Contraction is off inside every function.  Per-atom work is
// IEEE + and x on doubles, one rounding each, in the order written; `/` and sqrt appear in the per-image scalars
// (neb_image_scalars) and in relax_step.h's per-band scalars alone.
//
// A band is a run of images (graphs) band_ptr[k] .. band_ptr[k+1]-1 of equal atom count; the first and the last are end
// points: evaluated (the tangents need their energies) and never moved -- their gf / gi rows stay converged = 1, scale = 0,
// so hermnet_relax_advance, which the driver calls unchanged and without the wrap, leaves them alone.  The band's FIRE
// state is the gf / gi row of its FIRST INTERIOR image; the commit broadcasts it to every interior image's row.
//
// Interior image i, energies Em, E0, Ep (float32 widened), t1 = x_i - x_{i-1}, t2 = x_{i+1} - x_i (zero on held atoms):
//   T = c2 t2 + c1 t1 (neb_tangent_coef);   four canonical sums over the image's atoms: t1.t1, t2.t2, T.T, F.T (F:
//   relax_force's);   inv = 1/sqrt(T.T) or 0, ft = (F.T) inv, spring = k (sqrt(t2.t2) - sqrt(t1.t1)), par = spring - ft, or
//   -2 ft on the climbing image (the interior image of largest energy, ties to the lowest index);   g_a = F_a + par (T_a inv).
// Four more canonical sums per image over g and v (g.v, g.g, v.v, max |g_a|^2) are folded over the band's interior images in
// ascending image order starting from 0.0 (the maximum in the same order); FIRE decides on those; the clamp's v.v is summed
// per image, then over the images in the same order.
//
// The three launches (neb_image_force, neb_image_velocity, neb_commit) keep resident_step.h's protocol: the words the
// kernels branch on -- state, gf, gi -- are written by the commit alone; no workgroup reads what another workgroup of the
// same launch writes; no atomics.
#ifndef HERMNET_NEB_STEP_H
#define HERMNET_NEB_STEP_H

#include "relax_step.h"

namespace {

struct NebFinishArgs {
  int n, num_graphs, num_bands, climb;
  const int *graph_ptr, *band_ptr, *band_of;
  const float *forces, *energy;
  const long* total;
  long capacity;
  double dt, dtmax, maxstep;
  const double *k_band, *fmax_band;
  double *x, *v;
  const double* x0;
  int* image;
  const int* image0;
  float* f_prev;
  const unsigned char* fixed;
  float* pos32;
  double* gf;                                      // [B,5], [B,4]: relax_step.h's rows, per image; the commit
  long* gi;
  double* obs;                                     // [B,4] = (energy, max |g_a|, |t2|, ft) per image; neb_image_force
  long* climber;                                   // [K]: the climbing image's index within its band, -1: none; the commit
  double* g;                                       // scratch [N,3]: the NEB force; neb_image_force
  double* isum;                                    // scratch [B,4]: an image's (g.v, g.g, v.v, max |g_a|^2); neb_image_force
  double* csum;                                    // scratch [B]: an image's clamp sum; neb_image_velocity
  double* bf_new;                                  // scratch [K,5], [K,4], [K]: the band's new state; neb_image_velocity
  long* bi_new;
  long* climber_new;
  double* log;
  long log_steps;
  long* state;
};

inline bool neb_finish_args_ok(const NebFinishArgs& a) {
  if (a.n < 0 || a.num_graphs < 3 || a.num_bands < 1 || a.num_bands > a.num_graphs / 3) return false;
  if (a.log_steps < 1 || a.capacity < 0 || (a.climb != 0 && a.climb != 1)) return false;
  if (!(a.dt > 0.0) || !(a.dtmax > 0.0) || !(a.maxstep > 0.0)) return false;
  if (!a.state || !a.gf || !a.gi || !a.obs || !a.climber || !a.isum || !a.csum || !a.bf_new || !a.bi_new || !a.climber_new)
    return false;
  if (!a.energy || !a.total || !a.graph_ptr || !a.band_ptr || !a.band_of || !a.k_band || !a.fmax_band || !a.log) return false;
  if (a.n == 0) return true;
  return a.x && a.v && a.x0 && a.image && a.image0 && a.f_prev && a.forces && a.pos32 && a.g;
}

// Where image g stands: its band, the band's images [blo, bhi), the image that carries the band's state, whether g is
// interior, its atoms [lo, hi) and where its neighbours' atoms start.  Everything is clamped to what there is, so a broken
// band_ptr / band_of reads nothing out of bounds.
struct NebImage {
  int band, blo, bhi, first, interior, lo, hi, lom, lop;
};

HN_HD inline int neb_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

HN_HD inline void neb_band_range(const NebFinishArgs& a, int k, int* blo, int* bhi, int* first) {
  *blo = neb_clamp(a.band_ptr[k], 0, a.num_graphs);
  *bhi = neb_clamp(a.band_ptr[k + 1], *blo, a.num_graphs);
  *first = neb_clamp(*blo + 1, 0, a.num_graphs - 1);
}

HN_HD inline NebImage neb_image_of(const NebFinishArgs& a, int g) {
  NebImage m;
  m.band = neb_clamp(a.band_of[g], 0, a.num_bands - 1);
  neb_band_range(a, m.band, &m.blo, &m.bhi, &m.first);
  m.interior = g > m.blo && g + 1 < m.bhi;
  m.lo = hn_graph_lo(a.graph_ptr, g), m.hi = hn_graph_hi(a.graph_ptr, g, a.n);
  m.lom = m.interior ? hn_graph_lo(a.graph_ptr, g - 1) : m.lo;
  m.lop = m.interior ? hn_graph_lo(a.graph_ptr, g + 1) : m.lo;
  return m;
}

// The weights of the improved tangent T = c2 t2 + c1 t1.
HN_HD inline void neb_tangent_coef(double Em, double E0, double Ep, double* c1, double* c2) {
#pragma clang fp contract(off)
  if (Ep > E0 && E0 > Em) {
    *c1 = 0.0, *c2 = 1.0;
    return;
  }
  if (Ep < E0 && E0 < Em) {
    *c1 = 1.0, *c2 = 0.0;
    return;
  }
  const double dp = fabs(Ep - E0), dm = fabs(Em - E0);
  const double hi = dp > dm ? dp : dm, lo = dp > dm ? dm : dp;
  if (Ep > Em)
    *c1 = lo, *c2 = hi;
  else
    *c1 = hi, *c2 = lo;
}

// Atom i of an interior image: t1, t2 and the raw tangent (all zero where it is held).
HN_HD inline void neb_tangent_atom(const NebFinishArgs& a, const NebImage& m, int i, double c1, double c2, double t1[3],
                                   double t2[3], double T[3]) {
#pragma clang fp contract(off)
  const int held = a.fixed && a.fixed[i];
  const int im = neb_clamp(m.lom + (i - m.lo), 0, a.n - 1), ip = neb_clamp(m.lop + (i - m.lo), 0, a.n - 1);
  for (int k = 0; k < 3; ++k) {
    const double x = a.x[3 * (size_t)i + k];
    t1[k] = held ? 0.0 : x - a.x[3 * (size_t)im + k];
    t2[k] = held ? 0.0 : a.x[3 * (size_t)ip + k] - x;
    T[k] = c2 * t2[k] + c1 * t1[k];
  }
}

// The band's climbing image (its index among the graphs), -1 without `climb` or without an interior image.
HN_HD inline int neb_climbing_image(const NebFinishArgs& a, int blo, int bhi) {
  int best = -1;
  if (!a.climb) return best;
  for (int j = blo + 1; j + 1 < bhi; ++j)
    if (best < 0 || a.energy[j] > a.energy[best]) best = j;
  return best;
}

// The per-image scalars: what multiplies the unit tangent in the NEB force, and what the snapshot shows.
struct NebScalars {
  double inv, par, ft, seg;
};

HN_HD inline void neb_image_scalars(double t1t1, double t2t2, double TT, double FT, double k, int climbing, NebScalars* s) {
#pragma clang fp contract(off)
  s->inv = TT == 0.0 ? 0.0 : 1.0 / sqrt(TT);
  s->ft = FT * s->inv;
  s->seg = sqrt(t2t2);
  const double spring = k * (s->seg - sqrt(t1t1));
  s->par = climbing ? -2.0 * s->ft : spring - s->ft;
}

// First launch, image g (on the device the 256 lanes of g's workgroup call it together, `part` and `sc` in LDS; on the host
// one call does the image): restore on a void step; otherwise tangent, scalars, g into the scratch, the image's partials.
HN_HD inline void neb_image_force(const NebFinishArgs& a, int g, long code, double (*part)[256], NebScalars* sc) {
#pragma clang fp contract(off)
  const NebImage m = neb_image_of(a, g);
  if (a.gi[4 * (size_t)m.first + 2]) return;                        // the band has converged: nothing of it is written again
  if (code != 0) {
    if (!m.interior) return;
#if defined(__HIP_DEVICE_COMPILE__)
    const int first = m.lo + threadIdx.x, stride = 256;
#else
    const int first = m.lo, stride = 1;
#endif
    for (int i = first; i < m.hi; i += stride) hn_restore_atom(i, a.x, a.x0, a.image, a.image0, a.pos32);
    return;
  }
  if (!m.interior) {
    if (hn_lead_lane()) {
      a.obs[4 * (size_t)g] = (double)a.energy[g];
      a.obs[4 * (size_t)g + 1] = a.obs[4 * (size_t)g + 2] = a.obs[4 * (size_t)g + 3] = 0.0;
    }
    return;
  }
  double c1, c2;
  neb_tangent_coef((double)a.energy[g - 1], (double)a.energy[g], (double)a.energy[g + 1], &c1, &c2);
  hn_canonical_sums<4, -1>(m.lo, m.hi, part, [&](int i, double* s) {
    double t1[3], t2[3], T[3], F[3];
    neb_tangent_atom(a, m, i, c1, c2, t1, t2, T);
    relax_force(a.forces, a.fixed, i, F);
    s[0] = s[0] + relax_dot3(t1, t1);
    s[1] = s[1] + relax_dot3(t2, t2);
    s[2] = s[2] + relax_dot3(T, T);
    s[3] = s[3] + relax_dot3(F, T);
  });
  if (hn_lead_lane())
    neb_image_scalars(part[0][0], part[1][0], part[2][0], part[3][0], a.k_band[m.band], neb_climbing_image(a, m.blo, m.bhi) == g,
                      sc);
  hn_barrier();
  const NebScalars s = *sc;
  hn_canonical_sums<4, 3>(m.lo, m.hi, part, [&](int i, double* p) {
    double t1[3], t2[3], T[3], F[3], gg[3], v[3];
    neb_tangent_atom(a, m, i, c1, c2, t1, t2, T);
    relax_force(a.forces, a.fixed, i, F);
    for (int k = 0; k < 3; ++k) {
      gg[k] = F[k] + s.par * (T[k] * s.inv);
      a.g[3 * (size_t)i + k] = gg[k];
      v[k] = a.v[3 * (size_t)i + k];
    }
    const double g2 = relax_dot3(gg, gg);
    p[0] = p[0] + relax_dot3(gg, v);
    p[1] = p[1] + g2;
    p[2] = p[2] + relax_dot3(v, v);
    p[3] = g2 > p[3] ? g2 : p[3];
  });
  if (hn_lead_lane()) {
    for (int k = 0; k < 4; ++k) a.isum[4 * (size_t)g + k] = part[k][0];
    a.obs[4 * (size_t)g] = (double)a.energy[g];
    a.obs[4 * (size_t)g + 1] = sqrt(part[3][0]);
    a.obs[4 * (size_t)g + 2] = s.seg;
    a.obs[4 * (size_t)g + 3] = s.ft;
  }
}

// Second launch, image g: the band's sums folded from its images' partials, FIRE's decision on a local copy of the band's
// state (every interior image of the band takes the same one), the image's velocities and accepted forces, its clamp
// partial; the first interior image's lead lane leaves the band's new state in the scratch.
HN_HD inline void neb_image_velocity(const NebFinishArgs& a, int g, long step, long code, double (*part)[256], RelaxCoef* coef) {
#pragma clang fp contract(off)
  if (code != 0) return;
  const NebImage m = neb_image_of(a, g);
  if (!m.interior) return;
  RelaxGraph G = relax_graph_load(a.gf, a.gi, m.first);
  if (G.converged) return;
  if (hn_lead_lane()) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = m.blo + 1; j + 1 < m.bhi; ++j) {
      for (int k = 0; k < 3; ++k) s[k] = s[k] + a.isum[4 * (size_t)j + k];
      s[3] = a.isum[4 * (size_t)j + 3] > s[3] ? a.isum[4 * (size_t)j + 3] : s[3];
    }
    *coef = relax_graph_update(s[0], s[1], s[2], s[3], a.fmax_band[m.band], a.dt, a.dtmax, step, G);
    if (g == m.first) {
      G.energy = 0.0;                                               // (an image's energy is its own: the commit's)
      relax_graph_store(G, a.bf_new, a.bi_new, m.band);
      const int top = neb_climbing_image(a, m.blo, m.bhi);
      a.climber_new[m.band] = top < 0 ? -1 : top - m.blo;
    }
  }
  hn_barrier();
  const RelaxCoef c = *coef;
  hn_canonical_sums<1, -1>(m.lo, m.hi, part, [&](int i, double* s) {
    double v[3], f[3];
    for (int k = 0; k < 3; ++k) {
      v[k] = a.v[3 * (size_t)i + k];
      f[k] = a.g[3 * (size_t)i + k];
    }
    relax_velocity_atom(v, f, c, a.fixed && a.fixed[i]);
    for (int k = 0; k < 3; ++k) {
      a.v[3 * (size_t)i + k] = v[k];
      a.f_prev[3 * (size_t)i + k] = a.forces[3 * (size_t)i + k];
    }
    s[0] = s[0] + relax_dot3(v, v);
  });
  if (hn_lead_lane()) a.csum[g] = part[0][0];
}

// Third launch, the single writer (lane `first` of `stride` takes bands first, first + stride, ...): per band that was
// moving the clamp and the scale, the band's state into its interior images' rows (each with its own energy) and the
// climbing image; every image's log row; then the step count and `done`, or the halt.
HN_HD inline void neb_commit(const NebFinishArgs& a, long step, long code, int first, int stride) {
#pragma clang fp contract(off)
  int all = 1;
  if (code == 0)
    for (int k = first; k < a.num_bands; k += stride) {
      int blo, bhi, lead;
      neb_band_range(a, k, &blo, &bhi, &lead);
      RelaxGraph G = relax_graph_load(a.gf, a.gi, lead);
      if (!G.converged) {
        G = relax_graph_load(a.bf_new, a.bi_new, k);
        if (!G.converged) {
          double s = 0.0;
          for (int j = blo + 1; j + 1 < bhi; ++j) s = s + a.csum[j];
          G.scale = relax_graph_scale(s, G.dt, a.maxstep);
        }
        for (int j = blo + 1; j + 1 < bhi; ++j) {
          G.energy = (double)a.energy[j];
          relax_graph_store(G, a.gf, a.gi, j);
        }
        a.climber[k] = a.climber_new[k];
      }
      all &= G.converged != 0;
      for (int j = blo; j < bhi; ++j) {
        double* row = hn_log_row(a.log, step, a.log_steps, a.num_graphs, j, 4);
        row[0] = a.obs[4 * (size_t)j];
        row[1] = a.obs[4 * (size_t)j + 1];
        row[2] = G.dt;
        row[3] = (double)a.total[0];
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
  all = __syncthreads_and(all);
#endif
  if (!hn_lead_lane() || hn_commit_halt(a.state, step, code)) return;
  a.state[HN_STATE_STEP] = step + 1;
  if (all) a.state[HN_STATE_DONE] = 1;
}

}  // namespace

#endif  // HERMNET_NEB_STEP_H
