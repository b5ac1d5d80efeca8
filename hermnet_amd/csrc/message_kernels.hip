// gfx950 (MI355X / CDNA4) kernels for HermNet's relational message + segmented scatter-add.
//
// Replaces, per HeteroVertexConv layer and for all relations at once (files under /root/reference):
//   RadialBasis.forward               rmnet.py:168-172   (Gaussian taps * envelope, in registers)
//   rbf_proj Linear(R, 3H) on edges   rmnet.py:55        (banded contraction against an LDS weight tile)
//   MessagePassing.propagate gather   rmnet.py:58        (row gathers of xh[src], vec[src])
//   PaiNNMessage.message              rmnet.py:61-67     (in registers)
//   PaiNNMessage.aggregate scatter    rmnet.py:69-73     (segmented sum over the CSR row, no atomics)
//   residual                          rmnet.py:24-26     (epilogue, single write of x1 / vec1)
//   in_subgraph                       utils.py:11-24     (replaced by the relation-ordered CSR/CSC)
//
// Mapping (wave = 64 lanes).  A wave owns one target (fwd) or source (bwd) row at a time.  A lane
// owns VW = 4 adjacent channels of a 64-channel column block, so 16 lanes cover the block and the
// wave processes 4 consecutive edges of the row's segment at once (four 16-lane quarters).  A lane
// group moves one 256-byte row segment per load and reads the LDS weight tile with conflict-free
// ds_read_b128.  Groups are combined once per row; nothing is accumulated in HBM, there are no
// atomics, results are bit-reproducible.
//
// The kernels are VALU-issue bound (rocprofv3: VALU busy 56-72 %, LDS < 15 %); see DESIGN.md section 4.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/hermnet_hip.h"
#include "hermnet_math.h"
#include "message_bwd_cl.h"
int hn_option(int option);      // host_api.cpp

#define HN_LDS_ROW (3 * HN_CB)      // floats per tap row in LDS: [part][64]
// Phase fence for the instruction scheduler: without it hipcc hoists the LDS reads of all three
// parts (and the next edges' loads) to the top of the iteration and spills.
#ifndef HN_SB
#define HN_SB __builtin_amdgcn_sched_barrier(0)
#endif

namespace {

struct MsgArgs {
  // graph
  int N, E, T;
  int Nsrc;              // rows of the source space (xh, vec gathers); = N unless the targets are virtual rows (HTNet)
  const int* res_row;    // [N] source row entering the residual of target row r, or null (= r)
  const int* type_rowptr;
  const int* csr_rowptr;
  const int* csr_src;
  const int* csc_rowptr;
  const int* csc_tgt;
  const int* csc_pos;
  // radial basis
  const float* offset;
  int R;
  float inv_rc, coeff;
  int env_kind, env_p;
  // tensors
  int H;
  const float* xh;     // [T,N,3H]
  const float* vec;    // [N,3,H] or null
  const float* x;      // [N,H]
  const float* wt;     // [T,R,3H]
  const float* brbf;   // [T,3H]
  const float4* edge;  // [E] (rx,ry,rz,d)
  const float* fwd_taps;   // fwd: [E][HN_FWD_TAPS_FLOATS] tap records in CSR order (hermnet_edge_radial_tables), or null
  float* x1;           // fwd out
  float* vec1;         // fwd out
  const float* xh_bias;  // [T,3H] or null: bias of the x_proj output, added on load (xh holds the GEMM without it)
  const float* gx1;    // bwd in
  const float* gvec1;  // bwd in
  float* gxh;          // bwd out [T,N,3H]
  float* gvec;         // bwd out [N,3,H] or null
  float* gx;           // bwd out [N,H]
  float4* gedge;       // bwd out [H/64,E]
  int rows_per_block;
  int xcd_remap;       // 1 = XCD-contiguous block order (see xcd_contiguous)
  const int* row_ranges;   // fwd: [T][2] target rows [lo, hi) of every relation this launch covers, or null = whole blocks
  int zero_unknown;        // fwd: 1 = this launch also zeroes the rows of unknown-element atoms
  // fwd, tap-row windows (num_rbf too large for one LDS tile; see hermnet_message_scatter_fwd): the launch stages the
  // padded tile rows [win_base, win_base + win_rows) and owns the edges whose first tap row lies in [win_lo, win_hi);
  // win_accumulate = 1: its sums are added to the rows the launch over the other window wrote (residual included there)
  int win_base, win_rows, win_lo, win_hi, win_accumulate;
};

// ---- per-lane vectors of VW channels -------------------------------------------------------------
constexpr int VW = 4;          // channels per lane = edges a wave takes at once
constexpr int LPE = 64 / VW;   // lanes per edge

struct Vec {
  float v[VW];
  __device__ __forceinline__ static Vec zero() {
    Vec r;
#pragma unroll
    for (int i = 0; i < VW; ++i) r.v[i] = 0.f;
    return r;
  }
  __device__ __forceinline__ static Vec load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    Vec r;
    const float* f = reinterpret_cast<const float*>(&t);
#pragma unroll
    for (int i = 0; i < VW; ++i) r.v[i] = f[i];
    return r;
  }
};

// Elementwise ops are written on explicit <2 x float> pairs so that they select the packed fp32
// instructions (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32, scalars broadcast by op_sel): the SLP
// vectoriser packs only some of these chains on its own.
typedef float hn_f2 __attribute__((ext_vector_type(2)));
#define HN_PAIRWISE(expr)                                   \
  Vec r;                                                    \
  _Pragma("unroll") for (int i = 0; i < VW; i += 2) {       \
    const hn_f2 rv = (expr);                                \
    r.v[i] = rv.x;                                          \
    r.v[i + 1] = rv.y;                                      \
  }                                                         \
  return r;
#define HN_P(x) (hn_f2{(x).v[i], (x).v[i + 1]})
#define HN_S(x) (hn_f2{(x), (x)})

__device__ __forceinline__ Vec v_fma(const Vec& a, const Vec& b, const Vec& c) {   // a * b + c
  HN_PAIRWISE(__builtin_elementwise_fma(HN_P(a), HN_P(b), HN_P(c)))
}
__device__ __forceinline__ Vec v_sfma(float s, const Vec& a, const Vec& c) {   // s * a + c
  HN_PAIRWISE(__builtin_elementwise_fma(HN_S(s), HN_P(a), HN_P(c)))
}
__device__ __forceinline__ Vec v_mul(const Vec& a, const Vec& b) {
  HN_PAIRWISE(HN_P(a) * HN_P(b))
}
__device__ __forceinline__ Vec v_scale(const Vec& a, float s) {
  HN_PAIRWISE(HN_P(a) * HN_S(s))
}
__device__ __forceinline__ Vec v_add(const Vec& a, const Vec& b) {
  HN_PAIRWISE(HN_P(a) + HN_P(b))
}
__device__ __forceinline__ float v_hsum(const Vec& a) {
  float s = a.v[0];
#pragma unroll
  for (int i = 1; i < VW; ++i) s += a.v[i];
  return s;
}

// ---- cross-lane sums ---------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Sum over the four 16-lane rows (lane groups): row g of the result holds the sum over the four rows of a.v[g] --
// three v_permlane swaps (gfx950) and three adds on the VALU instead of eight LDS-routed shuffles.  The caller then
// owns channel `first channel + g` of the reduced vector: a dword store per lane, 256 contiguous bytes per wave.
__device__ __forceinline__ float rows_reduce4(const Vec& a) {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  // permlane16_swap: odd rows of the first operand <-> even rows of the second
  const u2 s01 = __builtin_amdgcn_permlane16_swap(__float_as_uint(a.v[0]), __float_as_uint(a.v[1]), false, false);
  const u2 s23 = __builtin_amdgcn_permlane16_swap(__float_as_uint(a.v[2]), __float_as_uint(a.v[3]), false, false);
  const float u = __uint_as_float(s01[0]) + __uint_as_float(s01[1]);   // rows: v0(r0+r1), v1(r0+r1), v0(r2+r3), v1(r2+r3)
  const float w = __uint_as_float(s23[0]) + __uint_as_float(s23[1]);   //       v2(r0+r1), v3(r0+r1), v2(r2+r3), v3(r2+r3)
  // permlane32_swap: upper half of the first operand <-> lower half of the second
  const u2 h = __builtin_amdgcn_permlane32_swap(__float_as_uint(u), __float_as_uint(w), false, false);
  return __uint_as_float(h[0]) + __uint_as_float(h[1]);               // rows: sum v0, sum v1, sum v2, sum v3
}

// Sum over the 16 lanes of each lane group (all channels of one edge); every lane gets its group's total.
__device__ __forceinline__ float group_allsum(float v) {
  v += dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]  : lane ^ 1
  v += dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]  : lane ^ 2
  v += dpp_mov<0x141>(v);   // row_half_mirror      : other quad of the 8-lane group
  v += dpp_mov<0x140>(v);   // row_mirror           : other half of the 16-lane DPP row
  return v;
}

// ---- LDS staging ---------------------------------------------------------------------------------
// Zero-padded weight tile of (relation t, column block cb) and the tap centres:
//   wl[(k + HN_PAD) * 192 + part * 64 + c] = wt[t][k][part * H + cb * 64 + c]   (0 outside 0 <= k < R)
//   mu[k + HN_PAD] = offset[clamp(k)]
// (`row0`, `nrows`: the window of padded rows held by wl -- all of them unless the launch works on a tap-row window; mu
// always covers every row)
template <int NTHREADS>
__device__ __forceinline__ void stage_weights(const MsgArgs& a, int t, int cb, float* wl, float* mu, int row0, int nrows) {
  const int rows = a.R + 2 * HN_PAD + 1;
  const int n4 = nrows * (HN_LDS_ROW / 4);
  constexpr int INFLIGHT = 8;   // independent 16-byte loads per thread before the first LDS write
  for (int base = threadIdx.x; base < n4; base += NTHREADS * INFLIGHT) {
    float4 v[INFLIGHT];
#pragma unroll
    for (int q8 = 0; q8 < INFLIGHT; ++q8) {
      const int idx = base + q8 * NTHREADS;
      const int kk = idx / (HN_LDS_ROW / 4);
      const int q = idx - kk * (HN_LDS_ROW / 4);
      const int k = kk + row0 - HN_PAD;
      v[q8] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < n4 && k >= 0 && k < a.R) {
        // 16 float4 per 64-channel part: part = q >> 4, c4 = q & 15
        v[q8] = *reinterpret_cast<const float4*>(
            a.wt + ((size_t)(t * a.R + k) * 3 * a.H + (q >> 4) * a.H + cb * HN_CB + (q & 15) * 4));
      }
    }
#pragma unroll
    for (int q8 = 0; q8 < INFLIGHT; ++q8) {
      const int idx = base + q8 * NTHREADS;
      if (idx < n4) *reinterpret_cast<float4*>(wl + (size_t)idx * 4) = v[q8];   // LDS image is idx-linear
    }
  }
  for (int kk = threadIdx.x; kk < rows; kk += NTHREADS) {
    int k = kk - HN_PAD;
    k = k < 0 ? 0 : (k >= a.R ? a.R - 1 : k);
    mu[kk] = a.offset[k];
  }
}

// ---- radial basis ----------------------------------------------------------------------------------
// Tap values of one edge, evaluated cooperatively: lane m < 12 of the edge's lane group computes
// tap m (same fp32 operation order as the reference, rmnet.py:156-172:  g = exp(coeff (u - mu_m)^2))
// and parks {g, g (u - mu_m)} in the wave's LDS scratch; every lane then reads the 12 pairs back
// as broadcasts.  One exp per edge and lane instead of twelve.
__device__ __forceinline__ void coop_taps(const float* mu, float2* tb, int lo, float u, float coeff, int gl) {
  if (gl < HN_TAPS) {
    const float diff = u - mu[lo + HN_PAD + gl];
    const float g = __expf(coeff * (diff * diff));
    tb[gl] = make_float2(g, g * diff);
  }
}

template <bool WITH_DER>
__device__ __forceinline__ void rbf_taps(const float2* tb, float (&g)[HN_TAPS], float (&gd)[HN_TAPS]) {
#pragma unroll
  for (int m = 0; m < HN_TAPS; ++m) {
    const float2 t = tb[m];
    g[m] = t.x;
    if (WITH_DER) gd[m] = t.y;
  }
}

// Banded contraction of one part (s, a or b) for this lane's VW channels:
//   S0 = sum_m g_m W[lo+m][part],  (WITH_DER) S1 = sum_m gd_m W[lo+m][part].
// One conflict-free LDS read per tap, double buffered behind the FMAs of the previous tap.
template <bool WITH_DER>
__device__ __forceinline__ void rbf_part(const float* wcol, const float (&g)[HN_TAPS], const float (&gd)[HN_TAPS],
                                         Vec& S0, Vec& S1) {
  S0 = Vec::zero();
  if (WITH_DER) S1 = Vec::zero();
  Vec wa = Vec::load(wcol), wb;
#pragma unroll
  for (int m = 0; m < HN_TAPS; m += 2) {
    wb = Vec::load(wcol + (m + 1) * HN_LDS_ROW);
    S0 = v_sfma(g[m], wa, S0);
    if (WITH_DER) S1 = v_sfma(gd[m], wa, S1);
    if (m + 2 < HN_TAPS) wa = Vec::load(wcol + (m + 2) * HN_LDS_ROW);
    S0 = v_sfma(g[m + 1], wb, S0);
    if (WITH_DER) S1 = v_sfma(gd[m + 1], wb, S1);
  }
}

// XCD-aware block order.  Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share an XCD and its
// 4 MiB L2), so with the identity mapping every XCD walks the WHOLE row range and sees every gather table in full
// (15-46 MB at config 2: L2 misses, Infinity-Cache hits).  Rows are in (relation, atom id) order and atom ids of a
// structure are spatially coherent, so giving XCD k the k-th contiguous eighth of the blocks confines its gathers to
// the rows near one slab of the structure -- a few MB that its L2 can hold.  Speed only; any mapping is correct.
__device__ __forceinline__ int xcd_contiguous(int b, int nb, int on) {
  const int per = nb >> 3;
  if (!on || b >= per * 8) return b;        // (the nb % 8 trailing blocks keep their place)
  return (b & 7) * per + (b >> 3);
}

// Decode blockIdx.x -> (relation t, first row, one-past-last row) for blocks of `rpb` rows
// laid out relation after relation.  Returns -1 for a work block, else the index of the
// surplus block (0, 1, ...) past the last work block.
__device__ __forceinline__ int decode_block(const MsgArgs& a, int bx, int& t, int& r0, int& r1) {
  for (t = 0; t < a.T; ++t) {
    // (atom shards: the targets that read no halo row run while the halo exchange is in flight, the others after
    // it -- two launches over complementary [lo, hi) ranges of every relation's row block)
    const int lo = a.row_ranges ? a.row_ranges[2 * t] : a.type_rowptr[t];
    const int hi = a.row_ranges ? a.row_ranges[2 * t + 1] : a.type_rowptr[t + 1];
    const int nb = hi > lo ? (hi - lo + a.rows_per_block - 1) / a.rows_per_block : 0;
    if (bx < nb) {
      r0 = lo + bx * a.rows_per_block;
      r1 = min(r0 + a.rows_per_block, hi);
      return -1;
    }
    bx -= nb;
  }
  return bx;
}

// ------------------------------------------------------------------------------------------
// Forward: one workgroup = (relation, column block, chunk of target rows).
// ------------------------------------------------------------------------------------------
// With the step's tap records (REC) a wave fetches the four records of its edge slots with ONE coalesced 256-byte load
// (lane l: word l % 16 of the record of slot l / 16) an iteration ahead, parks them in its LDS scratch and every lane group
// reads its own back as broadcasts (3 x ds_read_b128 + ds_read_b64): one VGPR of look-ahead.  (Whole records loaded into
// registers, 4 x dwordx4 per lane: 203 VGPRs, layer 0 spills at its 128; measured slower than no records)
struct FwdIn {
  float4 g;        // (rx, ry, rz, d)
  float rec;       // REC: word `gl` of the edge's tap record
  Vec xs, xa, xb;
  Vec vj[3];
  bool live;
};

// NW waves per workgroup: 8 with vec rows, 16 for layer 0 (no vec rows, <= 128 VGPRs).
// WIN: the launch works on a window of the tap rows (MsgArgs::win_*): an edge it does not own is a padding slot (lv = 0)
// reading a clamped tile row; with win_accumulate the epilogue adds to the other launch's rows.
// REC: everything that depends on the edge alone -- the twelve taps, the envelope, the tile row -- comes from the per-edge
// records written once per step (MsgArgs::fwd_taps) instead of being evaluated here, in every layer and column block; the
// records hold the values this kernel computes without them, so both forms return the same bits.
template <bool HAS_VEC, int NW, bool WIN, bool REC>
__global__ __launch_bounds__(NW * 64, NW / 4) void message_scatter_fwd_kernel(MsgArgs a) {
  extern __shared__ __align__(16) float lds[];
  const int tile_rows = WIN ? a.win_rows : a.R + 2 * HN_PAD + 1;
  float* wl = lds;
  float* mu = lds + tile_rows * HN_LDS_ROW;
  float2* tapbase = reinterpret_cast<float2*>(mu + ((a.R + 2 * HN_PAD + 1 + 3) & ~3));

  const int cb = blockIdx.y;
  int t, r0, r1;
  const int surplus = decode_block(a, xcd_contiguous(blockIdx.x, gridDim.x, a.xcd_remap), t, r0, r1);
  if (surplus >= 0) {
    // the first surplus block zeroes the rows of unknown-type atoms (they are never targets)
    if (surplus == 0 && a.zero_unknown) {
      const int c = cb * HN_CB + (threadIdx.x & 63);
      for (int r = a.type_rowptr[a.T] + (int)(threadIdx.x >> 6); r < a.N; r += NW) {
        a.x1[(size_t)r * a.H + c] = 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) a.vec1[((size_t)r * 3 + d) * a.H + c] = 0.f;
      }
    }
    return;
  }
  stage_weights<NW * 64>(a, t, cb, wl, mu, WIN ? a.win_base : 0, tile_rows);
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int grp = lane / LPE;            // lane group = edge slot
  const int gl = lane % LPE;
  float2* tb = tapbase + (wave * VW + grp) * 16;   // this lane group's tap scratch
  const int H = a.H;
  const int col = cb * HN_CB + VW * gl;  // first of this lane's VW channels
  const float inv_sqrt3h = 0.57735026918962576f * rsqrtf((float)H);  // (1/sqrt3)(1/sqrtH)
  const float inv_sqrth = rsqrtf((float)H);
  const float* xh_t = a.xh + (size_t)t * a.Nsrc * 3 * H;

  Vec bias[3], xbias[3];
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    bias[p] = Vec::load(a.brbf + (size_t)t * 3 * H + p * H + col);
    xbias[p] = a.xh_bias ? Vec::load(a.xh_bias + (size_t)t * 3 * H + p * H + col) : Vec::zero();
  }
  // (a copy per use: with the arrays referenced directly hipcc hoists their packing into register pairs out of the edge
  // loop, which reschedules the vec kernel at its 192-VGPR budget -- a change to measure, not to make in passing)
  auto bias_of = [&](int p) { return bias[p]; };
  auto xbias_of = [&](int p) { return xbias[p]; };

  for (int r = r0 + wave; r < r1; r += NW) {
    const int beg = a.csr_rowptr[r], end = a.csr_rowptr[r + 1];
    Vec ax = Vec::zero();
    Vec av[3] = {Vec::zero(), Vec::zero(), Vec::zero()};

    for (int base = beg; base < end; base += 64) {
      const int cnt = min(64, end - base);
      // one coalesced index load per 64 edges; lane groups pick their entries with a lane shuffle
      const int my_src = lane < cnt ? a.csr_src[base + lane] : 0;
      const int nit = (cnt + VW - 1) / VW;

      // Prefetch: geometry of the next edges (16 B, decides taps and LDS rows) at the top of an iteration, their rows
      // at the end -- the tap and S0 arithmetic of the next iteration then starts at once while its rows are in flight.
      // (The last iteration re-loads its own: no branch, so the loads stay asynchronous.)
      auto load_geom = [&](int it, FwdIn& in) {
        const int idx = VW * it + grp;
        in.live = idx < cnt;
        in.g = a.edge[base + (in.live ? idx : 0)];
        if (REC) {   // (always the record of an edge of this row: no look-ahead past the table's end)
          in.rec = a.fwd_taps[(size_t)(base + (in.live ? idx : 0)) * HN_FWD_TAPS_FLOATS + gl];
        }
      };
      auto load_rows = [&](int it, FwdIn& in) {
        const int j = __shfl(my_src, VW * it + grp, 64);
        const float* xr = xh_t + (size_t)j * 3 * H + col;
        // (masked at use, not here: touching the registers now would wait for the loads)
        in.xs = Vec::load(xr); in.xa = Vec::load(xr + H); in.xb = Vec::load(xr + 2 * H);
        if (HAS_VEC) {
          const float* vr = a.vec + (size_t)j * 3 * H + col;
#pragma unroll
          for (int d = 0; d < 3; ++d) in.vj[d] = Vec::load(vr + d * H);
        }
      };

      auto load_edges = [&](int it) {
        FwdIn in;
        load_geom(it, in);
        load_rows(it, in);
        return in;
      };

      FwdIn cur = load_edges(0);
      for (int it = 0; it < nit; ++it) {
        FwdIn nxt;
        load_geom(min(it + 1, nit - 1), nxt);
        __builtin_amdgcn_sched_barrier(0);
        float g[HN_TAPS], gd[HN_TAPS];
        float env_val;
        int trow;                                             // padded tile row of tap 0
        if (REC) {
          float t[HN_FWD_TAPS_FLOATS];
          float* tf = reinterpret_cast<float*>(tb);
          tf[gl] = cur.rec;       // (one wave's LDS operations execute in order: no barrier before the reads)
#pragma unroll
          for (int q = 0; q < 3; ++q) *reinterpret_cast<float4*>(t + 4 * q) = *reinterpret_cast<const float4*>(tf + 4 * q);
          *reinterpret_cast<float2*>(t + 12) = *reinterpret_cast<const float2*>(tf + 12);
#pragma unroll
          for (int m = 0; m < HN_TAPS; ++m) g[m] = t[m];
          env_val = t[12];
          trow = __float_as_int(t[13]);
        } else {
          const float u = cur.g.w * a.inv_rc;
          const HnEnv env = hn_envelope(u, a.env_kind, a.env_p);
          const int lo = hn_window_lo(u, a.R);
          env_val = env.val;
          trow = lo + HN_PAD;
          coop_taps(mu, tb, lo, u, a.coeff, gl);
          rbf_taps<false>(tb, g, gd);
        }
        bool own = true;
        if (WIN) { own = trow >= a.win_lo && trow < a.win_hi; trow = min(max(trow - a.win_base, 0), a.win_rows - HN_TAPS); }
        const float* wcol = wl + trow * HN_LDS_ROW + VW * gl;
        HN_SB;
        // padding slots (segment length not a multiple of VW) contribute nothing: every term is
        // linear in rbfh = bias + env * S0 (rmnet.py:55), so scale it by 0 for them
        const float lv = (cur.live && own) ? 1.0f : 0.0f;
        const float ev = env_val * lv;
        Vec S0, S1;
        // message (rmnet.py:61-67), one part at a time to keep the register footprint small
        rbf_part<false>(wcol, g, gd, S0, S1);   // part s -> dx
        ax = v_fma(v_add(cur.xs, xbias_of(0)), v_sfma(ev, S0, v_scale(bias_of(0), lv)), ax);
        HN_SB;
        rbf_part<false>(wcol + 2 * HN_CB, g, gd, S0, S1);   // part b -> rhat term
        const Vec mb = v_scale(v_mul(v_add(cur.xb, xbias_of(2)), v_sfma(ev, S0, v_scale(bias_of(2), lv))), inv_sqrth);
        av[0] = v_sfma(cur.g.x, mb, av[0]);
        av[1] = v_sfma(cur.g.y, mb, av[1]);
        av[2] = v_sfma(cur.g.z, mb, av[2]);
        HN_SB;
        if (HAS_VEC) {
          rbf_part<false>(wcol + HN_CB, g, gd, S0, S1);   // part a -> vec_j term
          const Vec ma = v_scale(v_mul(v_add(cur.xa, xbias_of(1)), v_sfma(ev, S0, v_scale(bias_of(1), lv))), inv_sqrt3h);
#pragma unroll
          for (int d = 0; d < 3; ++d) av[d] = v_fma(cur.vj[d], ma, av[d]);
        }
        HN_SB;
        load_rows(min(it + 1, nit - 1), cur);
        cur.g = nxt.g;
        cur.live = nxt.live;
        if (REC) cur.rec = nxt.rec;
      }
    }
    // combine the lane groups, then the residual epilogue (rmnet.py:24-26).  rows_reduce4 leaves ONE channel (col + grp)
    // of every reduced row in each lane: dword accesses, all lanes
    const int rres = a.res_row ? a.res_row[r] : r;      // row of (x, vec) that enters the residual
    const int c1 = col + grp;
    const size_t xo = (size_t)r * H + c1;
    if (WIN && a.win_accumulate) {          // the other launch wrote residual + its edges' sums
      a.x1[xo] += rows_reduce4(ax) * 0.70710678118654752f;
#pragma unroll
      for (int d = 0; d < 3; ++d) a.vec1[((size_t)r * 3 + d) * H + c1] += rows_reduce4(av[d]);
      continue;
    }
    a.x1[xo] = (a.x[(size_t)rres * H + c1] + rows_reduce4(ax)) * 0.70710678118654752f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const size_t vo = ((size_t)r * 3 + d) * H + c1;
      a.vec1[vo] = (HAS_VEC ? a.vec[((size_t)rres * 3 + d) * H + c1] : 0.f) + rows_reduce4(av[d]);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Backward (forces): one workgroup = (column block, chunk of SOURCE rows); it loops over the
// relations of the targets, restaging the weight tile per relation.  Sums keyed by the source row
// stay in registers for the whole CSC segment: gxh[t][row] is written once per relation; gvec[row]
// is written at t = 0 (with the residual's identity term) and read-modify-written by the same
// lanes for t > 0.  The per-edge cross-lane sum (dE/dD, 3 floats over one lane group) is 4 DPP
// steps.
// ------------------------------------------------------------------------------------------
struct BwdIn {
  float4 g;     // (rx, ry, rz, d)
  Vec gx1;      // d/dx1 of the target row
  Vec gd[3];    // d/dvec1 of the target row
  int pos;
  bool live;
};

constexpr int BWD_NW = 8;   // waves per workgroup

template <bool HAS_VEC>
__global__ __launch_bounds__(BWD_NW * 64, BWD_NW / 4) void message_scatter_bwd_kernel(MsgArgs a) {
  constexpr int NW = BWD_NW;
  extern __shared__ __align__(16) float lds[];
  float* wl = lds;
  float* mu = lds + (a.R + 2 * HN_PAD + 1) * HN_LDS_ROW;
  float2* tapbase = reinterpret_cast<float2*>(mu + ((a.R + 2 * HN_PAD + 1 + 3) & ~3));

  const int cb = blockIdx.y;
  const int r0 = blockIdx.x * a.rows_per_block;
  const int r1 = min(r0 + a.rows_per_block, a.N);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int grp = lane / LPE;
  const int gl = lane % LPE;
  float2* tb = tapbase + (wave * VW + grp) * 16;
  const int H = a.H;
  const int col = cb * HN_CB + VW * gl;
  const int nk = a.type_rowptr[a.T];     // rows below nk have a known type (are targets)
  const float inv_sqrt3h = 0.57735026918962576f * rsqrtf((float)H);
  const float inv_sqrth = rsqrtf((float)H);
  const float inv_sqrt2 = 0.70710678118654752f;
  float4* gedge = a.gedge + (size_t)cb * a.E;

  for (int t = 0; t < a.T; ++t) {
    __syncthreads();   // previous tile no longer in use
    stage_weights<NW * 64>(a, t, cb, wl, mu, 0, a.R + 2 * HN_PAD + 1);
    __syncthreads();
    // first row of relation t in the [T,N,...] arrays (unsigned N: a plain 32 x 32 -> 64-bit product, one SGPR fewer)
    const size_t tN = (size_t)t * (unsigned)a.N;
    const float* xh_t = a.xh + tN * 3 * H;
    float* gxh_t = a.gxh + tN * 3 * H;
    Vec bias[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) bias[p] = Vec::load(a.brbf + (size_t)t * 3 * H + p * H + col);

    for (int r = r0 + wave; r < r1; r += NW) {
      const int beg = a.csc_rowptr[tN + r], end = a.csc_rowptr[tN + r + 1];
      const float* xr = xh_t + (size_t)r * 3 * H + col;
      Vec xs = Vec::load(xr), xa = Vec::load(xr + H), xb = Vec::load(xr + 2 * H);
      if (a.xh_bias) {   // per source segment: free next to the per-edge work
        const float* xbp = a.xh_bias + (size_t)t * 3 * H + col;
        xs = v_add(xs, Vec::load(xbp)); xa = v_add(xa, Vec::load(xbp + H)); xb = v_add(xb, Vec::load(xbp + 2 * H));
      }
      Vec vj[3] = {Vec::zero(), Vec::zero(), Vec::zero()};
      if (HAS_VEC) {
        const float* vr = a.vec + (size_t)r * 3 * H + col;
#pragma unroll
        for (int d = 0; d < 3; ++d) vj[d] = Vec::load(vr + d * H);
      }
      Vec gs = Vec::zero(), ga = Vec::zero(), gb = Vec::zero();
      Vec gv[3] = {Vec::zero(), Vec::zero(), Vec::zero()};
      // gvec[row] is read-modify-written across the relations (t = 0 starts from the residual's identity term):
      // the old value is requested here, a whole segment ahead of its use
      float prev1[3] = {0.f, 0.f, 0.f};
      if (HAS_VEC) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const size_t vo = ((size_t)r * 3 + d) * H + col + grp;
          prev1[d] = t == 0 ? (r < nk ? a.gvec1[vo] : 0.f) : a.gvec[vo];
        }
      }

      for (int base = beg; base < end; base += 64) {
        const int cnt = min(64, end - base);
        const int my_tgt = lane < cnt ? a.csc_tgt[base + lane] : 0;
        const int my_pos = lane < cnt ? a.csc_pos[base + lane] : 0;
        const int nit = (cnt + VW - 1) / VW;

        auto load_geom = [&](int it, BwdIn& in) {     // prefetch: as in the forward kernel
          const int idx = VW * it + grp;
          in.pos = __shfl(my_pos, idx, 64);
          in.live = idx < cnt;
          in.g = a.edge[in.pos];
        };
        auto load_rows = [&](int it, BwdIn& in) {
          const int i = __shfl(my_tgt, VW * it + grp, 64);
          in.gx1 = Vec::load(a.gx1 + (size_t)i * H + col);
          const float* gvr = a.gvec1 + (size_t)i * 3 * H + col;
#pragma unroll
          for (int d = 0; d < 3; ++d) in.gd[d] = Vec::load(gvr + d * H);   // padding slots are masked at use
        };

        auto load_edges = [&](int it) {
          BwdIn in;
          load_geom(it, in);
          load_rows(it, in);
          return in;
        };

        BwdIn cur = load_edges(0);
        for (int it = 0; it < nit; ++it) {
          BwdIn nxt;
          load_geom(min(it + 1, nit - 1), nxt);
          __builtin_amdgcn_sched_barrier(0);
          const float4 g = cur.g;
          const float u = g.w * a.inv_rc;
          const HnEnv env = hn_envelope(u, a.env_kind, a.env_p);
          const int lo = hn_window_lo(u, a.R);
          const float* wcol = wl + (lo + HN_PAD) * HN_LDS_ROW + VW * gl;
          float g_[HN_TAPS], gd_[HN_TAPS];
          coop_taps(mu, tb, lo, u, a.coeff, gl);
          rbf_taps<true>(tb, g_, gd_);
          HN_SB;
          // d rbfh / d d = inv_rc * (env' S0 + env * 2 coeff S1)
          const float c0 = a.inv_rc * env.der, c1 = a.inv_rc * env.sval * 2.0f * a.coeff;
          const float rd[3] = {g.x, g.y, g.z};
          // padding slots: every term is linear in (gx1, gvec1), so scale those by 0
          const float lv = cur.live ? 1.0f : 0.0f;
          const Vec gdx = v_scale(cur.gx1, lv * inv_sqrt2);
          const Vec g0 = v_scale(cur.gd[0], lv), g1 = v_scale(cur.gd[1], lv), g2 = v_scale(cur.gd[2], lv);
          Vec pdv;                       // partial dE/dd per channel
          Vec S0, S1;
          // ---- part s: dx = sum xs * rs
          rbf_part<true>(wcol, g_, gd_, S0, S1);
          {
            const Vec rs = v_sfma(env.val, S0, bias[0]);
            const Vec drs = v_sfma(c0, S0, v_scale(S1, c1));
            gs = v_fma(gdx, rs, gs);
            pdv = v_mul(v_mul(gdx, xs), drs);
          }
          HN_SB;
          // ---- part a: dvec += vec_j * (xa * ra) / sqrt(3H)
          if (HAS_VEC) {
            rbf_part<true>(wcol + HN_CB, g_, gd_, S0, S1);
            const Vec ra = v_sfma(env.val, S0, bias[1]);
            const Vec dra = v_sfma(c0, S0, v_scale(S1, c1));
            const Vec A = v_scale(v_fma(g0, vj[0], v_fma(g1, vj[1], v_mul(g2, vj[2]))), inv_sqrt3h);
            ga = v_fma(A, ra, ga);
            const Vec w = v_scale(v_mul(xa, ra), inv_sqrt3h);
            gv[0] = v_fma(g0, w, gv[0]);
            gv[1] = v_fma(g1, w, gv[1]);
            gv[2] = v_fma(g2, w, gv[2]);
            pdv = v_fma(v_mul(A, xa), dra, pdv);
          }
          HN_SB;
          // ---- part b: dvec += rhat * (xb * rb) / sqrt(H)
          Vec q;
          {
            rbf_part<true>(wcol + 2 * HN_CB, g_, gd_, S0, S1);
            const Vec rb = v_sfma(env.val, S0, bias[2]);
            const Vec drb = v_sfma(c0, S0, v_scale(S1, c1));
            const Vec B = v_scale(v_sfma(rd[0], g0, v_sfma(rd[1], g1, v_scale(g2, rd[2]))), inv_sqrth);
            gb = v_fma(B, rb, gb);
            pdv = v_fma(v_mul(B, xb), drb, pdv);
            q = v_scale(v_mul(xb, rb), inv_sqrth);
          }
          HN_SB;
          const float pd = v_hsum(pdv);
          const float pr[3] = {v_hsum(v_mul(g0, q)), v_hsum(v_mul(g1, q)), v_hsum(v_mul(g2, q))};   // dE/d rhat
          // Cartesian gradient w.r.t. D (d = |D|, rhat = D/d): gD = pd rhat + (pr - (pr.rhat) rhat)/d
          const float dotp = pr[0] * rd[0] + pr[1] * rd[1] + pr[2] * rd[2];
          const float invd = __builtin_amdgcn_rcpf(g.w);   // 1 ulp; the full-precision divide costs ~10 instructions
          float gD[3];
#pragma unroll
          for (int d = 0; d < 3; ++d) gD[d] = group_allsum(fmaf(pd - dotp * invd, rd[d], pr[d] * invd));
          if (cur.live && gl == 0) gedge[cur.pos] = make_float4(gD[0], gD[1], gD[2], 0.f);
          HN_SB;
          load_rows(min(it + 1, nit - 1), cur);
          cur.g = nxt.g;
          cur.pos = nxt.pos;
          cur.live = nxt.live;
        }
      }
      // combine lane groups: every lane ends up with ONE channel (col + grp) of each reduced row (gxh s/a/b, gx,
      // gvec[0..2]): dword stores, all lanes active
      const bool known = r < nk;
      const int c1 = col + grp;
      float* go = gxh_t + (size_t)r * 3 * H + c1;
      go[0] = rows_reduce4(gs);
      go[H] = rows_reduce4(ga);
      go[2 * H] = rows_reduce4(gb);
      if (t == 0) a.gx[(size_t)r * H + c1] = (known ? a.gx1[(size_t)r * H + c1] : 0.f) * inv_sqrt2;
      if (HAS_VEC) {
#pragma unroll
        for (int d = 0; d < 3; ++d) a.gvec[((size_t)r * 3 + d) * H + c1] = prev1[d] + rows_reduce4(gv[d]);
      }
    }
  }
}

int fill_args(const hn_graph* g, const hn_rbf_desc* rbf, int hidden, MsgArgs& a) {
  if (!g || !rbf || hidden <= 0 || hidden % HN_CB != 0) return HN_ERR_BAD_ARG;
  if (g->num_rel <= 0 || rbf->num_rbf < 2) return HN_ERR_BAD_ARG;
  a.N = g->num_nodes; a.E = g->num_edges; a.T = g->num_rel;
  a.Nsrc = g->num_src > 0 ? g->num_src : g->num_nodes; a.res_row = g->res_row;
  a.type_rowptr = g->type_rowptr; a.csr_rowptr = g->csr_rowptr; a.csr_src = g->csr_src;
  a.csc_rowptr = g->csc_rowptr; a.csc_tgt = g->csc_tgt; a.csc_pos = g->csc_pos;
  a.offset = rbf->offset; a.R = rbf->num_rbf; a.inv_rc = rbf->inv_rc; a.coeff = rbf->coeff;
  a.env_kind = rbf->env_kind; a.env_p = rbf->env_p;
  a.H = hidden;
  return HN_OK;
}

// tuning knobs: process-wide options (host_api.cpp: hermnet_set_option), read at every launch

int num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
    else n = 256;
  }
  return n;
}

// Rows per workgroup such that the grid is a whole number of "rounds" of one workgroup per CU
// (the 116 KB weight tile allows one resident workgroup per CU): `work` = rows x column blocks,
// `slack` = workgroups lost to per-relation rounding.  Targets ~64 rows per workgroup (each workgroup stages
// the 116 KB weight tile once per relation: fewer, longer workgroups amortise it; measured on config 2).
int pick_rows(int rows, int ncb, int slack, int override_rows) {
  if (override_rows > 0) return override_rows;
  const long work = (long)rows * ncb;
  const int cus = num_cus();
  long rounds = (work + (long)cus * 32) / ((long)cus * 64);
  if (rounds < 1) rounds = 1;
  long wgs = (long)cus * rounds - slack;
  if (wgs < 1) wgs = 1;
  long rpb = (work + wgs - 1) / wgs;
  if (rpb < 8) rpb = 8;
  return (int)rpb;
}

// LDS image: weight tile [rows][192] | tap centres mu [rows, padded to 4] | per-wave tap scratch
// (float2 {g, g*diff} x 16 per lane group).
// (`tile_rows`: rows of the weight tile held at once -- all of them unless the launch works on a tap-row window)
size_t lds_bytes(int R, int tile_rows = 0) {
  const size_t rows = (size_t)(R + 2 * HN_PAD + 1);
  const size_t held = tile_rows > 0 ? (size_t)tile_rows : rows;
  // (+ 6 * HN_CB floats no kernel reads any more -- the bias slots of retired 12/16-wave forms: dropping them changes
  // the LDS request and with it, at some num_rbf, the occupancy; that is a change of its own, to be measured)
  return (held * HN_LDS_ROW + ((rows + 3) & ~(size_t)3)) * sizeof(float) + 16 * 4 * 16 * sizeof(float2) +
         6 * HN_CB * sizeof(float);
}

typedef void (*kern_t)(MsgArgs);

// Opt in to > 64 KB of dynamic LDS once per kernel (not per launch: it is a host-side attribute, and
// per-launch calls are neither free nor welcome while a stream is being captured into a hipGraph).
int ensure_lds(kern_t k, size_t lds) {
  constexpr int kMax = 64;
  static kern_t done[kMax];
  static size_t done_lds[kMax];
  static int ndone = 0;
  for (int i = 0; i < ndone; ++i)
    if (done[i] == k && done_lds[i] >= lds) return HN_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess)
    return HN_ERR_LDS;
  if (ndone < kMax) { done[ndone] = k; done_lds[ndone] = lds; ++ndone; }
  return HN_OK;
}

}  // namespace

extern "C" int hermnet_message_scatter_fwd_taps(const hn_graph* g, const hn_rbf_desc* rbf, int hidden,
                                                const float* xh, const float* xh_bias, const float* vec, const float* x,
                                                const float* wt, const float* brbf, const float* edge,
                                                const float* fwd_taps, float* x1, float* vec1, const int* target_ranges,
                                                int zero_unknown_rows, int range_rows, void* stream) {
  MsgArgs a = {};
  int rc = fill_args(g, rbf, hidden, a);
  if (rc) return rc;
  if (!xh || !x || !wt || !brbf || !x1 || !vec1 || (g->num_edges > 0 && !edge)) return HN_ERR_BAD_ARG;
  if (a.N == 0) return HN_OK;
  a.xh = xh; a.xh_bias = xh_bias; a.vec = vec; a.x = x; a.wt = wt; a.brbf = brbf;
  a.edge = reinterpret_cast<const float4*>(edge);
  a.fwd_taps = fwd_taps;
  a.x1 = x1; a.vec1 = vec1;
  a.row_ranges = target_ranges; a.zero_unknown = (target_ranges == nullptr) || zero_unknown_rows;
  const int rpb_fwd = hn_option(HN_OPT_FWD_ROWS);
  // (a launch over row ranges sizes its workgroups for the rows it covers: a workgroup of the full launch lives as long
  // as the whole kernel, so a launch over a tenth of the rows with the same chunking would take just as long)
  const int rows = (target_ranges && range_rows > 0 && range_rows < a.N) ? range_rows : a.N;
  a.rows_per_block = pick_rows(rows, hidden / HN_CB, a.T * (hidden / HN_CB), rpb_fwd);
  a.xcd_remap = 1;
  // blocks: sum_t ceil(N_t / rpb) <= N / rpb + T, plus one surplus block that zeroes unknown rows
  dim3 grid((unsigned)(rows / a.rows_per_block + a.T + 1), (unsigned)(hidden / HN_CB));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // 8 waves per workgroup with vec rows, 16 for layer 0 (tools/kbench.py on MI355X, config 2)
  const int nw = vec ? 8 : 16;
  size_t lds = lds_bytes(a.R);
  if (lds > 160 * 1024) {
    // num_rbf > 176: the tile of one (relation, column block) no longer fits the LDS.  Two launches over tap-row windows
    // (the same split as the backward's, message_bwd_cl.hip: hn_bwd_cl_launch): the first owns the edges whose first tap
    // row is below `split`, writes residual + their sums; the second owns the rest and adds its sums.
    const int rows_all = a.R + 2 * HN_PAD + 1, split = (rows_all - HN_PAD + 1) / 2;
    const int held = split + HN_PAD > rows_all - split ? split + HN_PAD : rows_all - split;
    lds = lds_bytes(a.R, held);
    if (lds > 160 * 1024) return HN_ERR_LDS;
    kern_t k = fwd_taps ? (vec ? message_scatter_fwd_kernel<true, 8, true, true> : message_scatter_fwd_kernel<false, 16, true, true>)
                        : (vec ? message_scatter_fwd_kernel<true, 8, true, false> : message_scatter_fwd_kernel<false, 16, true, false>);
    if (ensure_lds(k, lds) != HN_OK) return HN_ERR_LDS;
    a.win_base = 0; a.win_rows = split + HN_PAD; a.win_lo = 0; a.win_hi = split; a.win_accumulate = 0;
    hipLaunchKernelGGL(k, grid, dim3(nw * 64), lds, s, a);
    a.win_base = split; a.win_rows = rows_all - split; a.win_lo = split; a.win_hi = 0x7fffffff; a.win_accumulate = 1;
    a.zero_unknown = 0;
    hipLaunchKernelGGL(k, grid, dim3(nw * 64), lds, s, a);
    return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
  }
  kern_t k = fwd_taps ? (vec ? message_scatter_fwd_kernel<true, 8, false, true> : message_scatter_fwd_kernel<false, 16, false, true>)
                      : (vec ? message_scatter_fwd_kernel<true, 8, false, false> : message_scatter_fwd_kernel<false, 16, false, false>);
  if (ensure_lds(k, lds) != HN_OK) return HN_ERR_LDS;
  hipLaunchKernelGGL(k, grid, dim3(nw * 64), lds, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_message_scatter_fwd(const hn_graph* g, const hn_rbf_desc* rbf, int hidden,
                                           const float* xh, const float* xh_bias, const float* vec, const float* x,
                                           const float* wt, const float* brbf, const float* edge,
                                           float* x1, float* vec1, const int* target_ranges, int zero_unknown_rows,
                                           int range_rows, void* stream) {
  return hermnet_message_scatter_fwd_taps(g, rbf, hidden, xh, xh_bias, vec, x, wt, brbf, edge, nullptr, x1, vec1,
                                          target_ranges, zero_unknown_rows, range_rows, stream);
}

extern "C" int hermnet_message_scatter_bwd(const hn_graph* g, const hn_rbf_desc* rbf, int hidden,
                                           const float* xh, const float* xh_bias, const float* vec,
                                           const float* wt, const float* brbf, const float* edge,
                                           const float* gx1, const float* gvec1,
                                           float* gxh, float* gvec, float* gx, float* gedge,
                                           int split_t, const float* edge_table, float* gvec_partials,
                                           const int* source_ranges, const int* source_ranges_host, int num_ranges,
                                           void* stream) {
  MsgArgs a = {};
  int rc = fill_args(g, rbf, hidden, a);
  if (rc) return rc;
  if (!xh || !wt || !brbf || !gx1 || !gvec1 || !gxh || (g->num_edges > 0 && !gedge)) return HN_ERR_BAD_ARG;
  if (vec && !gvec && gx) return HN_ERR_BAD_ARG;
  const bool no_finish = gx == nullptr;        // the consumer sums the partials (include/hermnet_hip.h)
  if (g->num_edges > 0 && !edge) return HN_ERR_BAD_ARG;
  if (split_t != 0) return HN_ERR_BAD_ARG;     // retired (include/hermnet_hip.h)
  if (a.N == 0) return HN_OK;
  const int use_cl = hn_option(HN_OPT_BWD_LANES16) == 0;
  const bool virtual_targets = g->num_src > 0 || g->res_row != nullptr;
  const size_t gather_bytes = (size_t)a.N * 3 * hidden * sizeof(float);      // the channel-per-lane form gathers through
  const size_t src_rows = g->num_src > 0 ? (size_t)g->num_src : (size_t)a.N;
  const bool cl_ok = edge_table && gather_bytes < 0xffffffffull &&  // 32-bit buffer offsets
                     src_rows * 3 * hidden < 0x7fffffffull &&                   // 32-bit row offsets (elements)
                     (!vec || a.T == 1 || gvec_partials);
  if (virtual_targets && !cl_ok) return HN_ERR_BAD_ARG;
  if (num_ranges < 0 || (num_ranges > 0 && !(cl_ok && (use_cl || virtual_targets)))) return HN_ERR_BAD_ARG;   // ranges: that form only
  // (ranged launches without the finishing launch: the "proj" halo exchange, ABI v12 -- the halo source rows first, the rest
  // while their partial sums travel; the consumer sums the partials as for the unranged form)
  if (no_finish && !(cl_ok && use_cl && !virtual_targets && (!vec || gvec_partials)))
    return HN_ERR_BAD_ARG;
  if (cl_ok && (use_cl || virtual_targets)) {
    HnBwdClArgs b = {};
    b.N = a.N; b.Nsrc = g->num_src > 0 ? g->num_src : a.N; b.E = a.E; b.T = a.T;
    b.identity = virtual_targets ? 0 : 1;
    b.csc_rowptr = a.csc_rowptr; b.csc_tgt = a.csc_tgt; b.csc_pos = a.csc_pos;
    b.R = a.R; b.H = hidden; b.table = edge_table; b.edge = reinterpret_cast<const float4*>(edge);
    b.xh = xh; b.xh_bias = xh_bias; b.vec = vec; b.wt = wt; b.brbf = brbf; b.gx1 = gx1; b.gvec1 = gvec1;
    b.gxh = gxh; b.gvec = (a.T == 1 && !no_finish) ? gvec : gvec_partials; b.gvec_out = gvec; b.gx = gx;
    b.gedge = reinterpret_cast<float4*>(gedge);
    b.type_rowptr = g->type_rowptr;
    const int rpb_cl = hn_option(HN_OPT_BWD_CL_ROWS);
    b.xcd_remap = 1;
    b.src_ranges = source_ranges; b.num_ranges = num_ranges;
    return hn_bwd_cl_launch(b, vec != nullptr, true, rpb_cl, source_ranges_host, reinterpret_cast<hipStream_t>(stream));
  }
  a.xh = xh; a.xh_bias = xh_bias; a.vec = vec; a.wt = wt; a.brbf = brbf;
  a.edge = reinterpret_cast<const float4*>(edge);
  a.gx1 = gx1; a.gvec1 = gvec1; a.gxh = gxh; a.gvec = gvec; a.gx = gx;
  a.gedge = reinterpret_cast<float4*>(gedge);
  const int rpb_bwd = hn_option(HN_OPT_BWD_ROWS);
  a.rows_per_block = pick_rows(a.N, hidden / HN_CB, 0, rpb_bwd);
  const size_t lds = lds_bytes(a.R);
  if (lds > 160 * 1024) return HN_ERR_LDS;
  dim3 grid((unsigned)((a.N + a.rows_per_block - 1) / a.rows_per_block), (unsigned)(hidden / HN_CB));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  kern_t k = vec ? message_scatter_bwd_kernel<true> : message_scatter_bwd_kernel<false>;
  if (ensure_lds(k, lds) != HN_OK) return HN_ERR_LDS;
  hipLaunchKernelGGL(k, grid, dim3(BWD_NW * 64), lds, s, a);
  return hipGetLastError() == hipSuccess ? HN_OK : HN_ERR_LAUNCH;
}

extern "C" int hermnet_message_scatter_bwd_gedge(const hn_graph* g, const hn_rbf_desc* rbf, int hidden,
                                                 const float* xh, const float* wt, const float* brbf,
                                                 const float* edge, const float* gx1, const float* gvec1,
                                                 float* gedge, const float* edge_table, void* stream) {
  MsgArgs a = {};
  int rc = fill_args(g, rbf, hidden, a);
  if (rc) return rc;
  if (!xh || !wt || !brbf || !gx1 || !gvec1 || !edge_table || (g->num_edges > 0 && (!gedge || !edge))) return HN_ERR_BAD_ARG;
  if (g->num_src > 0 || g->res_row != nullptr) return HN_ERR_BAD_ARG;
  if (a.N == 0) return HN_OK;
  // the channel-per-lane form's limits (32-bit buffer and row offsets), as in hermnet_message_scatter_bwd
  if ((size_t)a.N * 3 * hidden * sizeof(float) >= 0xffffffffull || hn_option(HN_OPT_BWD_LANES16) != 0) return HN_ERR_BAD_ARG;
  HnBwdClArgs b = {};
  b.N = a.N; b.Nsrc = a.N; b.E = a.E; b.T = a.T;
  b.identity = 1;
  b.csc_rowptr = a.csc_rowptr; b.csc_tgt = a.csc_tgt; b.csc_pos = a.csc_pos;
  b.R = a.R; b.H = hidden; b.table = edge_table; b.edge = reinterpret_cast<const float4*>(edge);
  b.xh = xh; b.wt = wt; b.brbf = brbf; b.gx1 = gx1; b.gvec1 = gvec1;     // (xh includes x_proj's bias; no vec rows)
  b.gedge = reinterpret_cast<float4*>(gedge);
  b.type_rowptr = g->type_rowptr;
  b.xcd_remap = 1;
  return hn_bwd_cl_launch(b, false, false, hn_option(HN_OPT_BWD_CL_ROWS), nullptr, reinterpret_cast<hipStream_t>(stream));
}
