// The FIRE finish of the device-resident relaxations, stated once for relax_kernels.hip (atoms) and cellrelax_kernels.hip
// (atoms + cell): the per-graph step and the single writer's commit, ONE text for the four places that run it -- the two
// per-graph kernels and the two host twins.  What the drivers share besides: the argument structs of the plain driver (the
// cell driver's embed them) and their checks.
//
// The protocol (resident_step.h's, and what the relaxation adds): finish derives the halt code; on a void step every graph
// that is not converged returns to where the step began and nothing else happens; a converged graph is copied and logged
// unchanged; a moving graph takes four canonical sums over its atoms, its lead lane decides (FIRE: relax_step.h), a barrier,
// the atoms' new velocities and the clamp's sum over them, the new state into the scratch copy gf_new / gi_new and the log
// row.  The commit -- the last, single-workgroup kernel -- copies the scratch to gf / gi, counts the step, sets `done` once
// every graph has converged, or records the halt.
//
// What differs between the drivers is a FILTER: a struct of static functions over its own argument struct `Args`,
//   base(args)                          the RelaxFinishArgs inside
//   code(args)                          the step's halt code (every lane of a workgroup calls it)
//   restore_atom(args, i)               what a void step takes back of atom i beside hn_restore_atom
//   restore_graph(args, g)              ... and of graph g (lead lane)
//   Context, load(args, g, ctx)         what the graph's atoms need of the graph, loaded once
//   force(args, ctx, i, f)              atom i's generalised force
//   graph_terms(args, g, s, G, ctx)     lead lane, in front of FIRE's update: the graph's own terms of the sums s, G.energy
//   clamp_sum(args, g, c, s, ctx)       lead lane, behind the atoms' velocities: the graph's own velocities; the clamp's sum
//   log_row(args, step, g, G)           the graph's log row
// (relax_kernels.hip: PlainFilter, cellrelax_kernels.hip: CellFilter).  Contraction is off inside every function.
//
// Everything is in the unnamed namespace of the source that includes this: the kernels' argument types keep the names the
// launch records in profiles/ show.
#ifndef HERMNET_RELAX_DRIVER_H
#define HERMNET_RELAX_DRIVER_H

#include "relax_step.h"

namespace {

struct RelaxAdvanceArgs {
  int n, num_graphs, flags;
  double *x, *x0;
  const double* v;
  int *image, *image0;
  const unsigned char* fixed;
  const long* batch;
  const float* cell;                               // the plain driver's wrap alone reads these two
  const double* inv_cell;
  float* pos32;
  const long* state;
  const double* gf;
  const long* gi;
};

struct RelaxFinishArgs {
  int n, num_graphs;
  const int* graph_ptr;
  const float *forces, *energy;
  const long* total;
  long capacity;
  double dt, dtmax, maxstep, fmax;
  const double* fmax_graph;
  double *x, *v;
  const double* x0;
  int* image;
  const int* image0;
  float* f_prev;
  const unsigned char* fixed;
  float* pos32;
  double* gf;
  long* gi;
  double* gf_new;
  long* gi_new;
  double* log;
  long log_steps;
  long* state;
};

// What both advances ask (the wrap's cell is each driver's own).
inline bool relax_advance_args_ok(const RelaxAdvanceArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || (a.flags & ~HN_MD_WRAP)) return false;
  if (!a.state || !a.gf || !a.gi) return false;
  if (a.n == 0) return true;
  return a.x && a.x0 && a.v && a.image && a.image0 && a.pos32;
}

inline bool relax_finish_args_ok(const RelaxFinishArgs& a) {
  if (a.n < 0 || a.num_graphs < 1 || a.log_steps < 1 || a.capacity < 0) return false;
  if (!(a.dt > 0.0) || !(a.dtmax > 0.0) || !(a.maxstep > 0.0) || !(a.fmax > 0.0)) return false;
  if (!a.state || !a.gf || !a.gi || !a.gf_new || !a.gi_new || !a.energy || !a.total || !a.graph_ptr || !a.log) return false;
  if (a.n == 0) return true;
  return a.x && a.v && a.x0 && a.image && a.image0 && a.f_prev && a.forces && a.pos32;
}

// An atom's terms of the four sums (f: the filter's force), added to the lane's partials.
HN_HD inline void relax_sums_one(const RelaxFinishArgs& a, int i, const double f[3], double s[4]) {
#pragma clang fp contract(off)
  double v[3];
  for (int k = 0; k < 3; ++k) v[k] = a.v[3 * (size_t)i + k];
  const double f2 = relax_dot3(f, f);
  s[0] = s[0] + relax_dot3(f, v);
  s[1] = s[1] + f2;
  s[2] = s[2] + relax_dot3(v, v);
  s[3] = f2 > s[3] ? f2 : s[3];
}

// The atom's new velocity and its accepted forces; returns its term of the clamp's sum.
HN_HD inline double relax_velocity_one(const RelaxFinishArgs& a, int i, const double f[3], const RelaxCoef& c) {
#pragma clang fp contract(off)
  double v[3];
  for (int k = 0; k < 3; ++k) v[k] = a.v[3 * (size_t)i + k];
  relax_velocity_atom(v, f, c, a.fixed && a.fixed[i]);
  for (int k = 0; k < 3; ++k) {
    a.v[3 * (size_t)i + k] = v[k];
    a.f_prev[3 * (size_t)i + k] = a.forces[3 * (size_t)i + k];
  }
  return relax_dot3(v, v);
}

// The first four entries of a graph's log row of `width`; returns the row.
HN_HD inline double* relax_log_row(const RelaxFinishArgs& a, long step, int g, const RelaxGraph& G, int width) {
  double* row = hn_log_row(a.log, step, a.log_steps, a.num_graphs, g, width);
  row[0] = G.energy;
  row[1] = G.fnorm;
  row[2] = G.dt;
  row[3] = (double)a.total[0];
  return row;
}

// Graph g's finish.  On the device the 256 lanes of g's workgroup call it together (`part`, `coef` in LDS); on the host one
// call does the graph.  `code`: Filter::code's, which every caller derives for itself.
template <class Filter>
HN_HD inline void relax_graph_step(const typename Filter::Args& args, int g, long step, long code, double (*part)[256],
                                   RelaxCoef* coef) {
#pragma clang fp contract(off)
  const RelaxFinishArgs& a = Filter::base(args);
  const int lo = hn_graph_lo(a.graph_ptr, g), hi = hn_graph_hi(a.graph_ptr, g, a.n);
  RelaxGraph G = relax_graph_load(a.gf, a.gi, g);
  if (code != 0) {
    if (G.converged) return;
#if defined(__HIP_DEVICE_COMPILE__)
    const int first = lo + threadIdx.x, stride = 256;
#else
    const int first = lo, stride = 1;
#endif
    for (int i = first; i < hi; i += stride) {
      hn_restore_atom(i, a.x, a.x0, a.image, a.image0, a.pos32);
      Filter::restore_atom(args, i);
    }
    if (hn_lead_lane()) Filter::restore_graph(args, g);
    return;
  }
  if (G.converged) {
    if (hn_lead_lane()) {
      relax_graph_store(G, a.gf_new, a.gi_new, g);
      Filter::log_row(args, step, g, G);
    }
    return;
  }
  typename Filter::Context ctx;
  Filter::load(args, g, ctx);
  hn_canonical_sums<4, 3>(lo, hi, part, [&](int i, double* s) {
    double f[3];
    Filter::force(args, ctx, i, f);
    relax_sums_one(a, i, f, s);
  });
  if (hn_lead_lane()) {
    double s[4] = {part[0][0], part[1][0], part[2][0], part[3][0]};
    Filter::graph_terms(args, g, s, G, ctx);
    *coef = relax_graph_update(s[0], s[1], s[2], s[3], a.fmax_graph ? a.fmax_graph[g] : a.fmax, a.dt, a.dtmax, step, G);
  }
  hn_barrier();
  const RelaxCoef c = *coef;
  hn_canonical_sums<1, -1>(lo, hi, part, [&](int i, double* s) {
    double f[3];
    Filter::force(args, ctx, i, f);
    s[0] = s[0] + relax_velocity_one(a, i, f, c);
  });
  if (hn_lead_lane()) {
    const double s = Filter::clamp_sum(args, g, c, part[0][0], ctx);
    if (!G.converged) G.scale = relax_graph_scale(s, G.dt, a.maxstep);
    relax_graph_store(G, a.gf_new, a.gi_new, g);
    Filter::log_row(args, step, g, G);
  }
}

// The single writer: on a completed step the scratch copy becomes the state (lane `first` of `stride` takes graphs first,
// first + stride, ...: the one workgroup's lanes on the device, (0, 1) on the host), the step is counted and `done` is set
// once every graph has converged; a void step records its halt.
HN_HD inline void relax_commit(const RelaxFinishArgs& a, long step, long code, int first, int stride) {
  int all = 1;
  if (code == 0)
    for (int g = first; g < a.num_graphs; g += stride) {
      for (int k = 0; k < 5; ++k) a.gf[5 * (size_t)g + k] = a.gf_new[5 * (size_t)g + k];
      for (int k = 0; k < 4; ++k) a.gi[4 * (size_t)g + k] = a.gi_new[4 * (size_t)g + k];
      all &= a.gi_new[4 * (size_t)g + 2] != 0;
    }
#if defined(__HIP_DEVICE_COMPILE__)
  all = __syncthreads_and(all);
#endif
  if (!hn_lead_lane() || hn_commit_halt(a.state, step, code)) return;
  a.state[HN_STATE_STEP] = step + 1;
  if (all) a.state[HN_STATE_DONE] = 1;
}

// A host twin's finish behind its argument check: the loop over the graphs a launch of the per-graph kernel is, then the commit.
template <class Filter>
inline void relax_host_finish(const typename Filter::Args& args) {
  const RelaxFinishArgs& a = Filter::base(args);
  const long step = a.state[HN_STATE_STEP];
  if (a.state[HN_STATE_CODE] != 0 || a.state[HN_STATE_DONE] != 0) return;
  const long code = Filter::code(args);
  double part[4][256];
  RelaxCoef coef;
  for (int g = 0; g < a.num_graphs; ++g) relax_graph_step<Filter>(args, g, step, code, part, &coef);
  relax_commit(a, step, code, 0, 1);
}

}  // namespace

#endif  // HERMNET_RELAX_DRIVER_H
