// The per-atom arithmetic of the device-resident integrator (md_kernels.hip): ONE text for the device kernels, their host
// twins (hermnet_host_md_advance / _finish) and -- transcribed operation by operation -- the numpy float64 references of
// tests/test_md_host.py.  Only IEEE +, x and floor on doubles, one rounding each (contraction off), in the order written:
// device, host and numpy agree bit for bit.  Everything that needs exp / sqrt / a division (kick, c1, sigma, the inverse
// cell) is made once on the host in float64; log / cos / sqrt appear in the Gaussian noise alone (md_gaussians).  Behind
// the arithmetic: the advance's arguments, their check, and what one atom's advance and one atom's noise are.
#ifndef HERMNET_MD_STEP_H
#define HERMNET_MD_STEP_H

#include "resident_step.h"

// ---- Philox4x32-10 (Salmon et al., SC'11; the Random123 known answers are checked in tests/test_md_host.py) --------------
HN_HD inline void md_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The eight words of (seed, step, atom): counter (atom, step low, step high, stream), stream 0 then stream 1.
HN_HD inline void md_noise_words(uint64_t seed, uint64_t step, uint32_t atom, uint32_t w[8]) {
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t ctr[4] = {atom, (uint32_t)step, (uint32_t)(step >> 32), 0u};
  md_philox4x32_10(ctr, key, w);
  ctr[3] = 1u;
  md_philox4x32_10(ctr, key, w + 4);
}

// Two words -> a 53-bit integer; u1 = (k + 1) 2^-53 in (0, 1] (its log is finite), u2 = k 2^-53 in [0, 1).
HN_HD inline double md_u53(uint32_t hi, uint32_t lo) {
  return (double)(((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6));
}

// Three standard Gaussians by Box-Muller in float64: stream 0 gives the pair (cos, sin), stream 1 the third (cos).
HN_HD inline void md_gaussians(const uint32_t w[8], double xi[3]) {
  const double two_pi = 6.283185307179586476925286766559, s = 1.0 / 9007199254740992.0;
  const double ra = sqrt(-2.0 * log((md_u53(w[0], w[1]) + 1.0) * s)), ta = two_pi * (md_u53(w[2], w[3]) * s);
  const double rb = sqrt(-2.0 * log((md_u53(w[4], w[5]) + 1.0) * s)), tb = two_pi * (md_u53(w[6], w[7]) * s);
  xi[0] = ra * cos(ta);
  xi[1] = ra * sin(ta);
  xi[2] = rb * cos(tb);
}

// ---- the step (its wrap and its halt code are the protocol's: resident_step.h) ---------------------------------------------
// The first half of a step, up to the coordinates the forces are evaluated at.  NVE (velocity Verlet): v += kick f,
// x += dt v.  Langevin (BAOAB): v += kick f, x += dt/2 v, v = c1 v + sigma xi, x += dt/2 v.  f: the last accepted forces.
HN_HD inline void md_advance_atom(double x[3], double v[3], const float f[3], double kick, double dt, int langevin, double c1,
                                  double sigma, const double xi[3]) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; ++k) v[k] = v[k] + kick * (double)f[k];
  if (!langevin) {
    for (int k = 0; k < 3; ++k) x[k] = x[k] + dt * v[k];
  } else {
    const double h = 0.5 * dt;
    for (int k = 0; k < 3; ++k) x[k] = x[k] + h * v[k];
    for (int k = 0; k < 3; ++k) v[k] = c1 * v[k] + sigma * xi[k];
    for (int k = 0; k < 3; ++k) x[k] = x[k] + h * v[k];
  }
}

// The second half kick with the new forces; returns the atom's kinetic energy half_mass |v|^2.
HN_HD inline double md_finish_atom(double v[3], const float f[3], double kick, double half_mass) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; ++k) v[k] = v[k] + kick * (double)f[k];
  return half_mass * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// ---- the advance of hermnet_md_advance and the noise of hermnet_md_noise, per atom (the kernels and the host twins loop) ----
// In the unnamed namespace of the including source, as everything that names a kernel's argument type.
namespace {

struct MdAdvanceArgs {
  int n, num_graphs, flags;
  double *x, *v, *x0, *v0;
  int *image, *image0;
  const float* f_prev;
  const double *kick, *c1, *sigma;
  const long* batch;
  const float* cell;
  const double* inv_cell;
  float* pos32;
  const long* state;
  double dt;
  uint64_t seed;
};

inline bool md_advance_args_ok(const MdAdvanceArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || (a.flags & ~(HN_MD_LANGEVIN | HN_MD_WRAP))) return false;
  if (a.n == 0) return true;
  if (!a.x || !a.v || !a.x0 || !a.v0 || !a.image || !a.image0 || !a.f_prev || !a.kick || !a.pos32 || !a.state) return false;
  if ((a.flags & HN_MD_LANGEVIN) && (!a.c1 || !a.sigma)) return false;
  if ((a.flags & HN_MD_WRAP) && (!a.cell || !a.inv_cell)) return false;
  return true;
}

HN_HD inline void md_advance_one(const MdAdvanceArgs& a, int i, long step, long mode) {
  double x[3], v[3];
  for (int k = 0; k < 3; ++k) x[k] = a.x[3 * (size_t)i + k];
  if (mode == 0) {
    int image[3];
    float f[3];
    for (int k = 0; k < 3; ++k) {
      v[k] = a.v[3 * (size_t)i + k];
      image[k] = a.image[3 * (size_t)i + k];
      f[k] = a.f_prev[3 * (size_t)i + k];
      a.x0[3 * (size_t)i + k] = x[k];
      a.v0[3 * (size_t)i + k] = v[k];
      a.image0[3 * (size_t)i + k] = image[k];
    }
    const long g = hn_graph_of(a.batch, i, a.num_graphs);
    const int langevin = a.flags & HN_MD_LANGEVIN;
    double xi[3] = {0.0, 0.0, 0.0};
    if (langevin) {
      uint32_t w[8];
      md_noise_words(a.seed, (uint64_t)step, (uint32_t)i, w);
      md_gaussians(w, xi);
    }
    md_advance_atom(x, v, f, a.kick[i], a.dt, langevin, langevin ? a.c1[g] : 0.0, langevin ? a.sigma[i] : 0.0, xi);
    if (a.flags & HN_MD_WRAP) {
      double cell[9], inv[9];
      hn_load_cell(a.cell, a.inv_cell, g, cell, inv);
      md_wrap_atom(x, image, cell, inv);
    }
    for (int k = 0; k < 3; ++k) {
      a.x[3 * (size_t)i + k] = x[k];
      a.v[3 * (size_t)i + k] = v[k];
      a.image[3 * (size_t)i + k] = image[k];
    }
  }
  for (int k = 0; k < 3; ++k) a.pos32[3 * (size_t)i + k] = (float)x[k];
}

// Atom i's eight words and three Gaussians of (seed, step) into the caller's arrays (either may be null).
HN_HD inline void md_noise_one(uint64_t seed, uint64_t step, int i, uint32_t* words, double* gauss) {
  uint32_t w[8];
  double xi[3];
  md_noise_words(seed, step, (uint32_t)i, w);
  md_gaussians(w, xi);
  if (words)
    for (int k = 0; k < 8; ++k) words[8 * (size_t)i + k] = w[k];
  if (gauss)
    for (int k = 0; k < 3; ++k) gauss[3 * (size_t)i + k] = xi[k];
}

}  // namespace

#endif  // HERMNET_MD_STEP_H
