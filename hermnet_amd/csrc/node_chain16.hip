// gfx950: the PaiNNUpdate chain (node_update_fwd / node_update_bwd of node_chain.hip; rmnet.py:94-107, 29-31), the node
// projection and the read-out on 16-ROW tiles, width 128 -- for grids that 32-row tiles quantise badly.
//
// Why: BASELINE configs[1] has 10,041 target rows = 314 tiles of 32 rows on 256 CUs: 58 CUs get two workgroups, 198 get
// one, the launch lasts as long as the CUs with two (a makespan of 64 rows against 39 rows per CU on average: 0.61).  In
// 16-row tiles the same rows are 628 workgroups, three or two per CU: 48 rows against 39 (0.82), and a CU's two or three
// co-resident workgroups fill each other's epilogue phases.  What 16-row tiles cost is weight traffic (every fragment serves
// 16 rows instead of 32: twice the requests and bytes from L2), which is why the 32-row kernels stay in charge of large grids
// (hermnet_node_update_tile_rows picks per launch).
//
// Data flow as in node_chain.hip -- fp32 in and out, both operands of a product as three bf16 planes, the six largest partial
// products on v_mfma_f32_16x16x32_bf16 (mma16_panel_rb) --: weights streamed from L2 in MFMA operand order, here
// frag16(W)[((b * K/32 + Q) * 3 + s) * 64 + l] = 8 bf16 of plane 2 - s, W[16 b + (l & 15)][32 Q + 8 (l >> 4) .. +7], one
// coalesced 1 KiB load per 16-channel block and STEP (a plane of a 32-deep k-group); fp32 activations in [16][H + 8] LDS tiles
// (two ds_read_b128 per k-group at row l & 15, k = 32 Q + 8 (l >> 4): conflict-free with the +8 pad), split into planes by the
// consuming wave (split8); accumulators transposed: lane l holds tile row l & 15 and the channels 16 b + 4 (l >> 4) .. +3 of
// block b as ONE float4.  A wave owns 32 channels (two blocks) of every output part, so vec_dot, q * vdot and r * v1 stay
// lane-local.
//
// ONE node launch per layer boundary, each way.  A tile's update (layer l) and the node projection of the rows it has
// just produced (layer l + 1: LayerNorm -> [H -> H] -> ScaledSiLU -> [H -> 3H] for every relation; rmnet.py:52 behind
// rmnet.py:29-31, 94-107) are row-local, so `node_update_fwd16_kernel<FUSE>` runs both: x_out never leaves the chip between
// them.  The mirror `node_update_bwd16_kernel<FUSE>` runs the projection's backward of layer l + 1 in front of the update
// backward of layer l: the per-relation sums stay in registers (no [T, N, H] partial sums in memory), the LayerNorm backward
// runs on the tile.  The same phases also exist as kernels of their own (`node_pre_fwd16_kernel`, `node_pre_bwd16_kernel`):
// the unfused form is the A/B and the bit-for-bit check of the fused one.
#include "node_chain_common.h"

namespace {

// Workgroups per CU the register budget is cut for (launch bounds).  Every kernel here fits three workgroups (<= 168
// registers) -- what it takes: the vec_dot sums pinned where they are formed (hipcc sinks them behind the last product and
// keeps v1 / v2 of all three components alive, spilled), v1 re-read from vp instead of held in registers, a weight ring of two
// for four-block products.  Measured (tools/chain_bench.py, 10,041 rows, same box, alternating builds, profiles/r05_chain_bench1.log):
// the backward kernels gain a little from the third workgroup (fused 100.0 vs 101.8 us), the forward kernels LOSE (fused 102.0
// vs 97.2 us) -- with three resident the products of each run slower and the launch ends no earlier: the matrix pipe is not
// what a third workgroup's waves were waiting for.  So: forward 2, backward 3.
constexpr int kMinWFwd16 = 2, kMinWBwd16 = 3;

constexpr int kTR16 = 16;
constexpr int kScr16Ld = 36, kScr16Floats = 16 * kScr16Ld;     // per-wave transpose scratch [16][36]

// steps of weight fragments in flight per block (a step: one weight plane of a k-group, 1 .. 3 MFMAs per block; an L2 hit
// 500-800 cycles)
constexpr int ring16(int nb) { return nb >= 4 ? 2 : 4; }     // (64 registers for a ring of four at NB = 4 kept a third workgroup off the CU)

template <int NB>
struct Ring16 { f32x4 v[ring16(NB)][NB]; };

// Diagnostic builds (results wrong, time meaningful): -DHN_KO_BSTREAM=1 every weight request reads the stream's FIRST fragment
// (same instructions, every request an L1 hit: what the weight stream's bytes cost), =2 no weight request at all (what its
// instructions cost).  10,041 rows (profiles/r05_chain_ko.log): fused forward 98.4 / 96.2 / 75.2 us, fused backward
// 99.9 / 94.8 / 74.3 us for 0 / 1 / 2 -- the REQUESTS (one 1-KiB load per four MFMAs at 16 rows), not their bytes or their
// latency, are a quarter of these kernels' time.  Halving them with two row blocks per fragment (mixed 32- / 16-row tiles so
// that the busiest CU still holds three blocks) was prototyped on the projection kernel: bit-identical, 64.0 -> 59.6 us -- the
// 64-row kernel of node_chain.hip does the same work in 48 us; not pursued.
#ifndef HN_KO_BSTREAM
#define HN_KO_BSTREAM 0
#endif
__device__ __forceinline__ f32x4 wfrag(const f32x4* p, int idx) {
#if HN_KO_BSTREAM == 1
  return p[idx & 0];
#elif HN_KO_BSTREAM == 2
  return (f32x4){0.01f, -0.02f, 0.03f, 0.015f};
#else
  return p[idx];
#endif
}

template <int NB>
__device__ __forceinline__ void b16_preload(Ring16<NB>& r, const f32x4* const (&bp)[NB]) {
#pragma unroll
  for (int g = 0; g < ring16(NB) - 1; ++g)
#pragma unroll
    for (int j = 0; j < NB; ++j) r.v[g][j] = wfrag(bp[j], g * 64);
}

// ---------------------------------------------------------------------------------------------------------------------
// The products run on the BF16 matrix pipe at fp32 accuracy -- three-way bf16 splits, six partial products per k-group on
// v_mfma_f32_16x16x32_bf16 (node_chain_common.h: split8, "fp32 products on the BF16 matrix pipe").  Against the fp32 MFMAs,
// measured with the instruction mix alone (a diagnostic build, results wrong, time meaningful: profiles/r05_split_timing.log):
// update_fwd 55 -> 32 us, pre_fwd16 64 -> 30, fused forward 98 -> 61.
//
// Stream: a block's fragments are consumed as STEPS of one 1-KiB load each (lane l: 16 bytes = 8 bf16 of one weight plane,
// W_p[16 b + (l & 15)][32 Q + 8 (l >> 4) .. +7]), in the order [k-group Q of 32][plane 2, 1, 0]: three steps per 32 k.
// frag16(W)[((b * K/32 + Q) * 3 + s) * 64 + l].
// ---------------------------------------------------------------------------------------------------------------------
// float4s of one 16-channel block's fragment stream over K inputs (3 K / 32 steps of 64 lanes), floats of an [O, K] weight
constexpr int frag16_f4(int K) { return K * 6; }
constexpr size_t frag16_floats(size_t O, size_t K) { return O * K * 3 / 2; }

// acc[j] += W_j[:, 0 .. KP) . A^T; `As`: this lane's LDS pointer &tile[(l & 15) * LD + 4 (l >> 4)] (the tile is fp32).
// The ring holds steps 0 .. RS-2 on entry; MORE: the stream continues behind the panel (its first RS-1 steps are
// requested and sit in slots 0 .. RS-2 on exit).
// RB row blocks share every weight fragment: acc[rb][j] += W_j . A_rb^T for RB activation tiles (`As[rb]`: this lane's pointer
// into tile rb).  A fragment then feeds RB x (1 .. 3) MFMAs -- the weight stream, which is what a 16-row tile's time is made of
// (see the knock-outs above), is paid once for RB tiles.  RB > 1 keeps ONE set of planes per tile (split in front of the
// group's MFMAs); RB = 1 double-buffers them (the split runs beside the previous group's MFMAs).
template <int KP, int NB, int RB, bool MORE>
__device__ __forceinline__ void mma16_panel_rb(f32x4 (&acc)[RB][NB], const float* const (&As)[RB], const f32x4* const (&bp)[NB],
                                               Ring16<NB>& ring) {
  constexpr int GT = KP / 32, NSTEP = 3 * GT, RS = ring16(NB), PF = RS - 1, NX = RB == 1 ? 2 : 1;
  static_assert(KP % 32 == 0 && (!MORE || NSTEP % RS == 0), "panel / ring mismatch");
  const int g4 = 4 * ((threadIdx.x & 63) >> 4);                 // As + g4 = &tile[(l & 15) * LD + 8 (l >> 4)]
  f32x4 lo[RB], hi[RB];
  Split8 X[NX][RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    lo[rb] = *reinterpret_cast<const f32x4*>(As[rb] + g4);
    hi[rb] = *reinterpret_cast<const f32x4*>(As[rb] + g4 + 4);
    if (NX == 2) split8(lo[rb], hi[rb], X[0][rb]);
  }
#pragma unroll
  for (int Q = 0; Q < GT; ++Q) {
    if (NX == 1) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) split8(lo[rb], hi[rb], X[0][rb]);
    }
    if (Q + 1 < GT) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        lo[rb] = *reinterpret_cast<const f32x4*>(As[rb] + g4 + 32 * (Q + 1));
        hi[rb] = *reinterpret_cast<const f32x4*>(As[rb] + g4 + 32 * (Q + 1) + 4);
      }
    }
#pragma unroll
    for (int ps = 0; ps < 3; ++ps) {                 // the step of weight plane 2 - ps
      const int n = 3 * Q + ps;
      if (MORE || n + PF < NSTEP) {
#pragma unroll
        for (int j = 0; j < NB; ++j) ring.v[(n + PF) % RS][j] = wfrag(bp[j], (n + PF) * 64);
      }
      fence_sched();                                 // (the requests stay in front of the step's MFMAs: node_chain_common.h)
#pragma unroll
      for (int m = ps; m >= 0; --m)                  // activation planes ps .. 0: the smaller partial products first
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int j = 0; j < NB; ++j)
            acc[rb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(hn_bf16x8, ring.v[n % RS][j]),
                                                                 X[Q & (NX - 1)][rb].p[m], acc[rb][j], 0, 0, 0);
      if (NX == 2 && ps == 1 && Q + 1 < GT) {        // (VALU work beside the matrix pipe's)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) split8(lo[rb], hi[rb], X[(Q + 1) & 1][rb]);
      }
    }
  }
}

template <int KP, int NB, bool MORE>
__device__ __forceinline__ void mma16_panel(f32x4 (&acc)[NB], const float* As, const f32x4* const (&bp)[NB], Ring16<NB>& ring) {
  const float* const as1[1] = {As};
  mma16_panel_rb<KP, NB, 1, MORE>(reinterpret_cast<f32x4 (&)[1][NB]>(acc), as1, bp, ring);
}

// Coalesced store / load of this wave's [16 rows][32 channels] block pair through the wave-private scratch: lane l owns
// row l & 15 and the channels 16 s + 4 (l >> 4) .. +3 of sub-block s (v[s]); memory sees 2 x (8 rows x 128 bytes).
template <int LDG, bool NT = false>
__device__ __forceinline__ void store16(float* scr, int lane, const f32x4 (&v)[2], rsrc_t r, int off) {
  const int m = lane & 15, g = lane >> 4;
#pragma unroll
  for (int s = 0; s < 2; ++s) *reinterpret_cast<f32x4*>(scr + m * kScr16Ld + 16 * s + 4 * g) = v[s];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int rr = it * 8 + (lane >> 3), c = (lane & 7) * 4;
    if (NT) bst4_nt(r, off + rr * LDG + c, *reinterpret_cast<const f32x4*>(scr + rr * kScr16Ld + c));
    else bst4(r, off + rr * LDG + c, *reinterpret_cast<const f32x4*>(scr + rr * kScr16Ld + c));
  }
}
struct Load16 { f32x4 v[2]; };
template <int LDG>
__device__ __forceinline__ void issue16(Load16& b, int lane, rsrc_t r, int off) {
#pragma unroll
  for (int it = 0; it < 2; ++it) b.v[it] = bld4(r, off + (it * 8 + (lane >> 3)) * LDG + (lane & 7) * 4);
}
__device__ __forceinline__ void finish16(float* scr, int lane, const Load16& b, f32x4 (&out)[2]) {
#pragma unroll
  for (int it = 0; it < 2; ++it)
    *reinterpret_cast<f32x4*>(scr + (it * 8 + (lane >> 3)) * kScr16Ld + (lane & 7) * 4) = b.v[it];
#pragma unroll
  for (int s = 0; s < 2; ++s)
    out[s] = *reinterpret_cast<const f32x4*>(scr + (lane & 15) * kScr16Ld + 16 * s + 4 * (lane >> 4));
}

__device__ __forceinline__ f32x4 zero4() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x4 sqrt4(f32x4 v) { return (f32x4){sqrtf(v[0]), sqrtf(v[1]), sqrtf(v[2]), sqrtf(v[3])}; }
__device__ __forceinline__ f32x4 rcp_clamped4(f32x4 n) {
  return (f32x4){__builtin_amdgcn_rcpf(fmaxf(n[0], 1e-4f)), __builtin_amdgcn_rcpf(fmaxf(n[1], 1e-4f)),
                 __builtin_amdgcn_rcpf(fmaxf(n[2], 1e-4f)), __builtin_amdgcn_rcpf(fmaxf(n[3], 1e-4f))};
}

// cooperative [16][H] tile copy through registers (H / 64 float4 per thread)
template <int H>
struct Tile16Regs { f32x4 v[kTR16 * H / 4 / 256]; };
template <int H>
__device__ __forceinline__ void tile16_load(Tile16Regs<H>& r, rsrc_t src, int ld_src, int off0, int tid) {
  constexpr int V = H / 4, F4 = kTR16 * H / 4 / 256;
#pragma unroll
  for (int it = 0; it < F4; ++it) {
    const int idx = tid + it * 256, row = idx / V, c4 = idx % V;
    r.v[it] = bld4(src, row * ld_src + off0 + c4 * 4);
  }
}
template <int H, int LD>
__device__ __forceinline__ void tile16_store(float* tile, const Tile16Regs<H>& r, int tid) {
  constexpr int V = H / 4, F4 = kTR16 * H / 4 / 256;
#pragma unroll
  for (int it = 0; it < F4; ++it) {
    const int idx = tid + it * 256, row = idx / V, c4 = idx % V;
    *reinterpret_cast<f32x4*>(tile + row * LD + c4 * 4) = r.v[it];
  }
}

// =====================================================================================================================
// The node projection of one 16-row tile (rmnet.py:52 for every relation): the tile's LayerNorm input sits in `bufN`.
// =====================================================================================================================
// LayerNorm without affine of a [16][H] LDS tile, in place; statistics over the first Hr channels.  Sixteen adjacent lanes share
// a row, its float4s dealt round-robin (a wave normalises four rows: the four waves work side by side -- one wave doing the
// whole tile with four lanes per row took 7.9k cycles of a workgroup's life in which the other three waited at the barrier).
// The caller puts a barrier in front (tile written) and behind (tile normalised).
template <int H>
__device__ __forceinline__ void layernorm_tile16(float* tile, int tid, int nrows, int Hr, float eps, float* mean0, float* rstd0) {
  constexpr int LD = H + 8, TPR = 16, NF = H / 4 / TPR;
  const int lr = tid / TPR, q = tid % TPR;
  f32x4 v[NF];
#pragma unroll
  for (int k = 0; k < NF; ++k) v[k] = *reinterpret_cast<const f32x4*>(tile + lr * LD + (k * TPR + q) * 4);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NF; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if ((k * TPR + q) * 4 + e >= Hr) v[k][e] = 0.f;
      s += v[k][e];
    }
#pragma unroll
  for (int m = 1; m < TPR; m <<= 1) s += __shfl_xor(s, m, 64);
  const float inv_h = 1.0f / (float)Hr;
  float mu = s * inv_h;
  // corrected two-pass statistics (see node_chain.hip): the mean of the deviations is the rounding error of `mu`
  float qq = 0.f, dd = 0.f;
#pragma unroll
  for (int k = 0; k < NF; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[k][e] = (k * TPR + q) * 4 + e < Hr ? v[k][e] - mu : 0.f;
      dd += v[k][e];
      qq = fmaf(v[k][e], v[k][e], qq);
    }
#pragma unroll
  for (int m = 1; m < TPR; m <<= 1) {
    qq += __shfl_xor(qq, m, 64);
    dd += __shfl_xor(dd, m, 64);
  }
  const float dm = dd * inv_h;
  mu += dm;
#pragma unroll
  for (int k = 0; k < NF; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if ((k * TPR + q) * 4 + e < Hr) v[k][e] -= dm;
  float var = qq * inv_h;
  pin(var);                       // (the product stays a product: no contraction with the sum behind it, in any kernel)
  float dm2 = dm * dm;
  pin(dm2);
  var = fmaxf(var - dm2, 0.f);
  const float rs = rsqrtf(var + eps);
#pragma unroll
  for (int k = 0; k < NF; ++k) *reinterpret_cast<f32x4*>(tile + lr * LD + (k * TPR + q) * 4) = v[k] * rs;
  if (q == 0 && lr < nrows) { mean0[lr] = mu; rstd0[lr] = rs; }
}

// xh[t] = x_proj_t(LayerNorm(x)) for every relation t of `p`, rows [row0, row0 + nrows) -- their x in bufN, raw, behind a
// barrier.  bufA0 / bufA1: two more [16][H + 8] tiles (the hidden activations of even / odd relations: one barrier per
// relation).  Saves hb (pre-activations incl. bias), mean, rstd like node_pre_fwd_kernel.  Per wave and relation 64 + 192 MFMAs.
template <int H>
__device__ __forceinline__ void pre_fwd16_phase(const PreFwdArgs& p, float* bufN, float* bufA0, float* bufA1, float* scr,
                                                int row0, int nrows, int tid, int lane, int wave) {
  constexpr int LD = H + 8, NB16 = H / 16;
  const int mrow = lane & 15, ch = 4 * (lane >> 4), cw = 32 * wave;
  const f32x4* bp1[2];
  Ring16<2> r1;
  f32x4 acc1[2];
  // the first product's operands of relation t: requested in front of whatever stores precede the product (vmcnt is in order)
  auto request1 = [&](int t) {
    const f32x4* w1 = reinterpret_cast<const f32x4*>(p.w1f + (size_t)t * frag16_floats(H, H)) + lane;
#pragma unroll
    for (int s = 0; s < 2; ++s) bp1[s] = w1 + (size_t)(2 * wave + s) * frag16_f4(H);
    b16_preload(r1, bp1);
#pragma unroll
    for (int s = 0; s < 2; ++s) acc1[s] = ld4g(p.b1 + (size_t)t * H + cw + 16 * s + ch);
  };
  request1(0);
  layernorm_tile16<H>(bufN, tid, nrows, p.Hr, p.eps, p.mean + row0, p.rstd + row0);
  __syncthreads();
  STAMP(10);
  const float* An = bufN + mrow * LD + ch;
#pragma unroll 1
  for (int t = 0; t < p.T; ++t) {
    float* bufA = (t & 1) ? bufA1 : bufA0;
    const rsrc_t hb_r = tile_rsrc(p.hb + ((size_t)t * p.Ns + row0) * H, nrows * H);
    const rsrc_t xh_r = tile_rsrc(p.xh + ((size_t)t * p.Ns + row0) * 3 * H, nrows * 3 * H);
    // ---- h = n W1^T + b1
    mma16_panel<H, 2, false>(acc1, An, bp1, r1);
    const f32x4* w2 = reinterpret_cast<const f32x4*>(p.w2f + (size_t)t * frag16_floats(3 * H, H)) + lane;
    const f32x4* bp2[6];
#pragma unroll
    for (int pp = 0; pp < 3; ++pp)
#pragma unroll
      for (int s = 0; s < 2; ++s) bp2[2 * pp + s] = w2 + (size_t)(pp * NB16 + 2 * wave + s) * frag16_f4(H);
    Ring16<6> r2;
    b16_preload(r2, bp2);
    f32x4 acc2[6];
#pragma unroll
    for (int pp = 0; pp < 3; ++pp)
#pragma unroll
      for (int s = 0; s < 2; ++s) acc2[2 * pp + s] = ld4g(p.b2 + (size_t)t * 3 * H + pp * H + cw + 16 * s + ch);
    fence_sched();
    {
      f32x4 hv[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        hv[s] = acc1[s];                               // (incl. b1)
        *reinterpret_cast<f32x4*>(bufA + mrow * LD + cw + 16 * s + ch) = ssilu4(hv[s]);
      }
      store16<H, true>(scr, lane, hv, hb_r, cw);
    }
    __syncthreads();
    // ---- xh = a W2^T + b2
    mma16_panel<H, 6, false>(acc2, bufA + mrow * LD + ch, bp2, r2);
    if (t + 1 < p.T) request1(t + 1);
    fence_sched();
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) {
      const f32x4 v[2] = {acc2[2 * pp], acc2[2 * pp + 1]};
      store16<3 * H>(scr, lane, v, xh_r, pp * H + cw);
    }
    STAMP(11 + (t < 3 ? t : 3));
  }
}

// Dynamic LDS of this unit's kernels: the tiles they carve, then (unless said otherwise) the four waves' [16][36] scratch
constexpr size_t lds16_bytes(int tile_floats, int behind = 4 * kScr16Floats) { return (size_t)(tile_floats + behind) * sizeof(float); }
// the forward kernels, fused or not: three [16][H + 8] tiles
constexpr size_t fwd16_lds_bytes(int H) { return lds16_bytes(3 * kTR16 * (H + 8)); }
// node_update_fwd16_kernel<H, false, false> keeps vec1 and v1 on chip: five tiles (vec1[0 .. 2], the norm / a2, x1), the four
// waves' v1 park [3][2][64] float4 each (= three tiles' rows of H floats), then the scratch.  Two workgroups per CU (kMinWFwd16).
constexpr int kPark16Floats = 3 * 2 * 64 * 4;
constexpr size_t upd_fwd16_lds_bytes(int H) { return lds16_bytes(5 * kTR16 * (H + 8) + 4 * kPark16Floats); }
static_assert(2 * upd_fwd16_lds_bytes(128) <= 160 * 1024, "node_update_fwd16_kernel<128, false, false>: two workgroups per CU");

// The projection as a kernel of its own (the unfused form: A/B and bit-for-bit check of the fused kernel's second half)
template <int H>
__global__ __launch_bounds__(256, kMinWFwd16) void node_pre_fwd16_kernel(PreFwdArgs p) {
  constexpr int TR = kTR16, LD = H + 8;
  extern __shared__ __align__(16) float lds[];               // 3 x [TR][LD], then 4 x [16][36] scratch
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * TR, nrows = min(TR, p.Ns - row0);
  const rsrc_t x_r = tile_rsrc(p.x + (size_t)row0 * H, nrows * H);
  Tile16Regs<H> regs;
  tile16_load<H>(regs, x_r, H, 0, tid);
  tile16_store<H, LD>(lds + 2 * TR * LD, regs, tid);
  __syncthreads();
  pre_fwd16_phase<H>(p, lds + 2 * TR * LD, lds, lds + TR * LD, lds + 3 * TR * LD + wave * kScr16Floats, row0, nrows, tid, lane, wave);
}

// =====================================================================================================================
// node_update_fwd on 16-row tiles (H = 128: four waves x 32 channels); FUSE: + the next layer's node projection of the tile
// =====================================================================================================================
// NOVEC (the LAST layer of an energy / force evaluation: the read-out takes x only, so vec_out feeds nothing): the r third of
// the last product -- its weight fragments and MFMAs --, dvec = r v1 and the vec_out store are left out; q23 receives q only
// (its r half stays unwritten: the matching backward, NOGV below, does not read it).  Every accumulator block of p and q sees
// the MFMAs it sees in the general form, in the same order: x_out, vp, h2b, nrm and q are the same bits.
//
// Tile rows on chip (the general form, !FUSE && !NOVEC: `KEEP`).  The residual vec_out = vec1 + r v1 needs vec1 and v1 once more
// behind the last product.  vec1's three tiles stay alive to the end (the norm / a2 and x1 take two further tiles) and are read in
// accumulator layout; v1 of the Wv epilogue is parked in a wave-private region, written and read back by the same lane (no
// barrier, no wait for the vp stores).  Per row 6 H floats fewer through the CU's vector-memory path (vec1 3 H and v1 3 H were
// read a second time from global memory), and no s_waitcnt vmcnt(0) in front of the last product.  FUSE and NOVEC keep three
// tiles: FUSE re-reads both from memory as before, NOVEC has no dvec.
template <int H, bool FUSE, bool NOVEC = false>
__global__ __launch_bounds__(256, kMinWFwd16) void node_update_fwd16_kernel(UpdFwdArgs a, PreFwdArgs p) {
  static_assert(H == 128, "four waves x 32 channels");
  static_assert(!(FUSE && NOVEC), "the last layer has no layer above");
  constexpr int TR = kTR16, LD = H + 8, NB16 = H / 16;       // NB16: 16-channel blocks per part
  constexpr int NQ = NOVEC ? 2 : 3;                          // parts of the last product: (p | q) or (p | q | r)
  constexpr bool KEEP = !FUSE && !NOVEC;                     // vec1 and v1 stay on chip for the residual
  // 3 x [TR][LD], then 4 x [16][36] scratch; KEEP: 5 x [TR][LD], 4 x the v1 park, then the scratch
  extern __shared__ __align__(16) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* park = lds + 5 * TR * LD + wave * kPark16Floats + lane * 4;          // (KEEP) this lane's float4 (d, s): + (2 d + s) * 256
  float* scr = lds + (KEEP ? 5 * TR * LD + 4 * kPark16Floats : 3 * TR * LD) + wave * kScr16Floats;
  const TileInfo ti = find_tile(a.type_rowptr, a.T, a.N, TR, blockIdx.x);
  const int row0 = ti.row0, nrows = ti.nrows, t = ti.t;
  if (t >= a.T) {                                 // rows of unknown elements: zero
    constexpr int V = H / 4;
    for (int idx = tid; idx < nrows * V; idx += 256) {
      const int r = row0 + idx / V, c = (idx % V) * 4;
      *reinterpret_cast<f32x4*>(a.x_out + (size_t)r * H + c) = zero4();
#pragma unroll
      for (int d = 0; d < (NOVEC ? 0 : 3); ++d) *reinterpret_cast<f32x4*>(a.vec_out + ((size_t)r * 3 + d) * H + c) = zero4();
    }
    if constexpr (FUSE) {                         // (they are sources all the same: their projection runs on x = 0)
      for (int idx = tid; idx < TR * (H / 4); idx += 256)
        *reinterpret_cast<f32x4*>(lds + 2 * TR * LD + (idx / (H / 4)) * LD + (idx % (H / 4)) * 4) = zero4();
      __syncthreads();
      pre_fwd16_phase<H>(p, lds + 2 * TR * LD, lds, lds + TR * LD, scr, row0, nrows, tid, lane, wave);
    }
    return;
  }
  const f32x4* wv = reinterpret_cast<const f32x4*>(a.wvf + (size_t)t * frag16_floats(2 * H, H)) + lane;
  const f32x4* wx0 = reinterpret_cast<const f32x4*>(a.wx0f + (size_t)t * frag16_floats(H, 2 * H)) + lane;
  const f32x4* wx2 = reinterpret_cast<const f32x4*>(a.wx2f + (size_t)t * frag16_floats(3 * H, H)) + lane;
  // this wave's blocks of part p: b = p * NB16 + 2 wave + s
  const f32x4* bpv[4];
  const f32x4* bpx[2];
  const f32x4* bpq[2 * NQ];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int s = 0; s < 2; ++s) bpv[2 * p + s] = wv + (size_t)(p * NB16 + 2 * wave + s) * frag16_f4(H);
#pragma unroll
  for (int s = 0; s < 2; ++s) bpx[s] = wx0 + (size_t)(2 * wave + s) * frag16_f4(2 * H);
#pragma unroll
  for (int p = 0; p < NQ; ++p)
#pragma unroll
    for (int s = 0; s < 2; ++s) bpq[2 * p + s] = wx2 + (size_t)(p * NB16 + 2 * wave + s) * frag16_f4(H);

  const int mrow = lane & 15, ch = 4 * (lane >> 4), cw = 32 * wave;
  const rsrc_t x1_r = tile_rsrc(a.x1 + (size_t)row0 * H, nrows * H);
  const rsrc_t vec1_r = tile_rsrc(a.vec1 + (size_t)row0 * 3 * H, nrows * 3 * H);
  const rsrc_t act_r = tile_rsrc(a.row_active ? a.row_active + row0 : a.x1, a.row_active ? nrows : 0);
  const bool all_on = a.row_active == nullptr;
  const rsrc_t vp_r = tile_rsrc(a.vp + (size_t)row0 * 6 * H, nrows * 6 * H);
  const rsrc_t h2b_r = tile_rsrc(a.h2b + (size_t)row0 * H, nrows * H);
  const rsrc_t q23_r = tile_rsrc(a.q23 + (size_t)row0 * 2 * H, nrows * 2 * H);
  const rsrc_t xo_r = tile_rsrc(a.x_out + (size_t)row0 * H, nrows * H);
  const rsrc_t vo_r = tile_rsrc(NOVEC ? a.x_out : a.vec_out + (size_t)row0 * 3 * H, NOVEC ? 0 : nrows * 3 * H);
  const rsrc_t nrm_r = tile_rsrc(a.nrm + (size_t)row0 * H, nrows * H);
  f32x4 dot[2] = {zero4(), zero4()}, sq[2] = {zero4(), zero4()};

  // ---- vp[d] = vec1[d] Wv^T; vec_dot and |v2|^2 accumulate in registers (v1 for dvec = r v1 is parked in LDS -- KEEP -- or
  // re-read from vp: 24 registers held across the whole kernel keep a third workgroup off the CU)
  STAMP(0);
  STAMP_HWID();
  // The three components in ONE product (three activation tiles per weight fragment): streamed once per component, Wv is
  // 144 of the kernel's 264 fragment requests per wave, and the requests are what a tile's time is made of.
  Tile16Regs<H> regs;
  Ring16<4> rv;
  b16_preload(rv, bpv);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    tile16_load<H>(regs, vec1_r, 3 * H, d * H, tid);
    tile16_store<H, LD>(lds + d * TR * LD, regs, tid);
  }
  __syncthreads();
  tile16_load<H>(regs, x1_r, H, 0, tid);               // (in flight during the product)
  // (accumulators START at their bias -- a lane's float4 of a block is exactly the bias float4 of its channels --, loaded
  // in front of the preceding epilogue's stores: vmcnt retires in order, a bias load issued behind stores waits for them)
  f32x4 acch[2], accq[2 * NQ];
  {
    f32x4 accv[3][4];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
      for (int b = 0; b < 4; ++b) accv[d][b] = zero4();
    const float* const asv[3] = {lds + mrow * LD + ch, lds + TR * LD + mrow * LD + ch, lds + 2 * TR * LD + mrow * LD + ch};
    mma16_panel_rb<H, 4, 3, false>(accv, asv, bpv, rv);
#pragma unroll
    for (int s = 0; s < 2; ++s) acch[s] = ld4g(a.bx0 + (size_t)t * H + cw + 16 * s + ch);
    fence_sched();
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      f32x4 v1[2] = {accv[d][0], accv[d][1]}, v2[2] = {accv[d][2], accv[d][3]};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        dot[s] += v1[s] * v2[s];
        sq[s] += v2[s] * v2[s];
        pin4(dot[s]);
        pin4(sq[s]);
      }
      if constexpr (KEEP) {
#pragma unroll
        for (int s = 0; s < 2; ++s) *reinterpret_cast<f32x4*>(park + (2 * d + s) * 256) = v1[s];
      }
      store16<6 * H>(scr, lane, v1, vp_r, d * 2 * H + cw);
      store16<6 * H, true>(scr, lane, v2, vp_r, d * 2 * H + H + cw);
    }
    STAMP(3);
  }
  // ---- xin = [x1 | sqrt(|v2|^2 + 1e-8)]: x1 -> buffer 1, the norm -> buffer 0 (KEEP: tiles 4 and 3, behind the vec1 tiles)
  float* bufx = lds + (KEEP ? 4 : 1) * TR * LD;
  float* bufn = lds + (KEEP ? 3 : 0) * TR * LD;
  Ring16<2> rx;
  b16_preload(rx, bpx);
  if constexpr (!KEEP) __syncthreads();              // every wave has finished the product over the three vec tiles
  tile16_store<H, LD>(bufx, regs, tid);
  {
    f32x4 nv[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      nv[s] = sqrt4(sq[s] + 1e-8f);
      *reinterpret_cast<f32x4*>(bufn + mrow * LD + cw + 16 * s + ch) = nv[s];
    }
    store16<H, true>(scr, lane, nv, nrm_r, cw);
  }
  __syncthreads();
  STAMP(4);
  // ---- h2 = xin Wx0^T + bx0 (K = 2H: two panels)
  {
    const f32x4* bpx1[2] = {bpx[0] + (size_t)frag16_f4(H), bpx[1] + (size_t)frag16_f4(H)};
    mma16_panel<H, 2, true>(acch, bufx + mrow * LD + ch, bpx, rx);
    mma16_panel<H, 2, false>(acch, bufn + mrow * LD + ch, bpx1, rx);
  }
  STAMP(5);
  Ring16<2 * NQ> rq;
  b16_preload(rq, bpq);
#pragma unroll
  for (int p = 0; p < NQ; ++p)
#pragma unroll
    for (int s = 0; s < 2; ++s) accq[2 * p + s] = ld4g(a.bx2 + (size_t)t * 3 * H + p * H + cw + 16 * s + ch);
  __syncthreads();                                   // buffer 0 is free (x1 stays in buffer 1)
  {
    f32x4 hv[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int c0 = cw + 16 * s + ch;
      hv[s] = acch[s];                               // (incl. bx0)
      *reinterpret_cast<f32x4*>(bufn + mrow * LD + c0) = ssilu4(hv[s]);
    }
    store16<H, true>(scr, lane, hv, h2b_r, cw);
  }
  __syncthreads();
  // ---- (p | q | r) = a2 Wx2^T + bx2, then the update and the residual
  // FUSE: vec1 and v1 of component 0, requested before the product; the components behind it one epilogue step ahead.  (v1 was
  // stored by this wave's own lanes: the wait makes the stores of the three vp epilogues final before it is read back.)
  Load16 lvv, lv1;
  if constexpr (FUSE) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    issue16<3 * H>(lvv, lane, vec1_r, cw);
    issue16<6 * H>(lv1, lane, vp_r, cw);
  }
  const float on = (all_on | (bld(act_r, mrow) != 0.f)) ? 1.f : 0.f;
  fence_sched();
  STAMP(6);
  mma16_panel<H, 2 * NQ, false>(accq, bufn + mrow * LD + ch, bpq, rq);
  fence_sched();
  STAMP(7);
  const float inv_sqrt_h = rsqrtf((float)H);
  f32x4 q[2], r[2], xo[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int c0 = cw + 16 * s + ch;
    const f32x4 p = accq[s];                         // (incl. bx2)
    q[s] = accq[2 + s];
    if constexpr (!NOVEC) r[s] = accq[4 + s];
    const f32x4 x1v = *reinterpret_cast<const f32x4*>(bufx + mrow * LD + c0);
    xo[s] = (x1v + (p + q[s] * dot[s] * inv_sqrt_h) * kInvSqrt2) * on;
  }
  store16<2 * H, true>(scr, lane, q, q23_r, cw);
  if constexpr (!NOVEC) store16<2 * H, true>(scr, lane, r, q23_r, H + cw);
  store16<H>(scr, lane, xo, xo_r, cw);
  if constexpr (FUSE) {
    // the rows this tile has just produced are the next layer's LayerNorm input: a third tile takes them (buffers 0 / 1 may
    // still be read by slower waves), the barrier behind the vec_out stores publishes it
#pragma unroll
    for (int s = 0; s < 2; ++s) *reinterpret_cast<f32x4*>(lds + 2 * TR * LD + mrow * LD + cw + 16 * s + ch) = xo[s];
  }
#pragma unroll
  for (int d = 0; d < (NOVEC ? 0 : 3); ++d) {
    f32x4 vo[2], v1[2];
    if constexpr (KEEP) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        vo[s] = *reinterpret_cast<const f32x4*>(lds + d * TR * LD + mrow * LD + cw + 16 * s + ch);
        v1[s] = *reinterpret_cast<const f32x4*>(park + (2 * d + s) * 256);
      }
    } else {
      finish16(scr, lane, lvv, vo);
      finish16(scr, lane, lv1, v1);
      if (d < 2) {
        issue16<3 * H>(lvv, lane, vec1_r, (d + 1) * H + cw);
        issue16<6 * H>(lv1, lane, vp_r, (d + 1) * 2 * H + cw);
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) vo[s] = (vo[s] + r[s] * v1[s]) * on;
    store16<3 * H>(scr, lane, vo, vo_r, d * H + cw);
  }
  STAMP(8);
  if constexpr (FUSE) {
    __syncthreads();
    STAMP(9);
    pre_fwd16_phase<H>(p, lds + 2 * TR * LD, lds, lds + TR * LD, scr, row0, nrows, tid, lane, wave);
  }
}

// =====================================================================================================================
// The backward of the node projection on one 16-row tile:  gn_t = ((gxh[t] W2_t) * ScaledSiLU'(hb[t])) W1_t  per relation.
// =====================================================================================================================
// LDS floats of the phase: the gxh tile [16][3H + 8] (3H + 8 = 8 mod 64 like H + 8: the same conflict-free ds_read_b128 pattern),
// then the gh tile [16][H + 8]
constexpr int pre_bwd16_tile_floats(int H) { return kTR16 * (3 * H + 8); }
// (node_pre_bwd16_kernel and the fused update backward, which turns the gxh tile's space into its two [16][H + 8] tiles)
constexpr size_t pre_bwd16_lds_bytes(int H) { return lds16_bytes(pre_bwd16_tile_floats(H) + kTR16 * (H + 8)); }
// the update backward without the projection's: two [16][H + 8] tiles and the three that hold gv[d] (below); the last layer's
// (NOGV) has the two only
constexpr size_t upd_bwd16_lds_bytes(int H) { return lds16_bytes(5 * kTR16 * (H + 8)); }
constexpr size_t upd_bwd16_last_lds_bytes(int H) { return lds16_bytes(2 * kTR16 * (H + 8)); }
// (the grid of configs[1] is 628 tiles on 256 CUs: it needs the third resident workgroup, kMinWBwd16.  A sixth tile for gx
// would be 61,440 bytes a workgroup: two per CU.)
static_assert(3 * upd_bwd16_lds_bytes(128) <= 160 * 1024, "node_update_bwd16_kernel<128, false, false>: three workgroups per CU");

template <int H>
struct Tile16Regs3 { f32x4 v[kTR16 * 3 * H / 4 / 256]; };

// The 16-row form of materialise_pending (node_chain_common.h) for node_update_bwd16_kernel<128, false, false>: the same sums in
// the same order of operations -- gx_out through ln_prep / ln_out, gvec_out = ((p0 + p1) + p2 ...) + gvec1 --, but indexed like
// the kernel's elementwise pass (pass it: row it * 8 + tid / 32, channels 4 (tid & 31) .. + 3; gvec component d: the float4 at
// (row * 3 + d) * H + c, still 512 contiguous bytes per row and component), which takes them from these registers.  gx_out is
// stored as well (the kernel reloads it once, in accumulator layout, behind its next barrier); gvec_out is stored for the
// caller only, and not at all with a.hold_gvo.  Rows past the tile's end come out as zero, like an out-of-range tile load.
template <int H>
struct Pend16 { f32x4 gx[kTR16 / 8], gv[kTR16 / 8][3]; };

template <int H>
__device__ __forceinline__ void pending16(const UpdBwdArgs& a, int row0, int nrows, int tid, Pend16<H>& o) {
  static_assert(H == 128, "half a wave per row");
  constexpr int RP = kTR16 / 8;
  const PendingGrads& p = a.pend;
  const int identity_rows = a.type_rowptr[a.T];
  const int lane = tid & 63, wave = tid >> 6, c = (lane & 31) * 4;
  const long ps = (long)a.N * H;
  int rr[RP];
  size_t r[RP];
  // ---- gvec_out: every load of a relation's slice is issued before the first one is used
#pragma unroll
  for (int it = 0; it < RP; ++it) {
    const int lr = it * 8 + wave * 2 + (lane >> 5);
    rr[it] = lr < nrows ? row0 + lr : -1;
    r[it] = (size_t)(rr[it] >= 0 ? rr[it] : row0);
#pragma unroll
    for (int d = 0; d < 3; ++d) o.gv[it][d] = ld4g(p.gv + (r[it] * 3 + d) * H + c);
  }
  // ---- gx_out (requested behind the first slice of gvec, finished while the others arrive)
  f32x4 gg[RP], xv[RP], av[RP];
  float mu[RP], rs[RP];
#pragma unroll
  for (int it = 0; it < RP; ++it) {
    gg[it] = ld4g(p.gn + r[it] * H + c);
    xv[it] = ld4g(p.x + r[it] * H + c);
    av[it] = ld4g(p.gx1 + r[it] * H + c);
    mu[it] = p.mean[r[it]];
    rs[it] = p.rstd[r[it]];
  }
  for (int t = 1; t < p.nparts; ++t) {
#pragma unroll
    for (int it = 0; it < RP; ++it) gg[it] += ld4g(p.gn + t * ps + r[it] * H + c);
  }
#pragma unroll
  for (int it = 0; it < RP; ++it) {
    f32x4 gv, nh;
    float s1 = 0.f, s2 = 0.f;
    ln_prep(gg[it], xv[it], mu[it], rs[it], c, p.Hr, gv, nh, s1, s2);
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) {
      s1 += __shfl_xor(s1, m, 64);
      s2 += __shfl_xor(s2, m, 64);
    }
    const float m1 = s1 / (float)p.Hr, m2 = s2 / (float)p.Hr;
    o.gx[it] = ln_out(gv, nh, m1, m2, rs[it], c, p.Hr, rr[it] >= 0 && rr[it] < identity_rows, av[it], kInvSqrt2);
    if (rr[it] >= 0) *reinterpret_cast<f32x4*>(const_cast<float*>(a.gxo) + r[it] * H + c) = o.gx[it];
    else o.gx[it] = zero4();
  }
  for (int t = 1; t < p.nparts; ++t) {
#pragma unroll
    for (int it = 0; it < RP; ++it)
#pragma unroll
      for (int d = 0; d < 3; ++d) o.gv[it][d] += ld4g(p.gv + t * 3 * ps + (r[it] * 3 + d) * H + c);
  }
#pragma unroll
  for (int it = 0; it < RP; ++it)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (rr[it] >= 0) {
        if (rr[it] < identity_rows) o.gv[it][d] += ld4g(p.gvec1 + (r[it] * 3 + d) * H + c);
        if (!a.hold_gvo) *reinterpret_cast<f32x4*>(const_cast<float*>(a.gvo) + (r[it] * 3 + d) * H + c) = o.gv[it][d];
      } else {
        o.gv[it][d] = zero4();
      }
    }
}

// `parts` != null: gn_t goes to parts[t] (the unfused form: the consumer sums the relations and runs the LayerNorm backward);
// null: gsum = (gn_0 + gn_1) + gn_2 ... in this lane's accumulator positions (the same additions in the same order as the
// consumer's).  Per wave and relation 192 + 64 MFMAs, two barriers; relation t + 1's gxh tile travels during relation t's products.
template <int H>
__device__ __forceinline__ void pre_bwd16_phase(const float* gxh, const float* hb, const float* w2tf, const float* w1tf,
                                                float* parts, int Ns, int T, float* tileA, float* bufG, float* scr,
                                                int row0, int nrows, int tid, int lane, int wave, f32x4 (&gsum)[2]) {
  constexpr int LD = H + 8, LDA = 3 * H + 8, V3 = 3 * H / 4, F4 = kTR16 * 3 * H / 4 / 256;
  const int mrow = lane & 15, ch = 4 * (lane >> 4), cw = 32 * wave;
  Tile16Regs3<H> regs;
  Load16 lhb;
  Ring16<2> ra;
  const f32x4* bpa[2];
  auto request = [&](int t) {          // relation t's gxh tile (cooperative, coalesced), hb block and first weight groups
    const rsrc_t g_r = tile_rsrc(gxh + ((size_t)t * Ns + row0) * 3 * H, nrows * 3 * H);
#pragma unroll
    for (int it = 0; it < F4; ++it) {
      const int idx = tid + it * 256;
      regs.v[it] = bld4(g_r, (idx / V3) * 3 * H + (idx % V3) * 4);
    }
    issue16<H>(lhb, lane, tile_rsrc(hb + ((size_t)t * Ns + row0) * H, nrows * H), cw);
  };
  auto request_w = [&](int t) {
    const f32x4* w2t = reinterpret_cast<const f32x4*>(w2tf + (size_t)t * frag16_floats(H, 3 * H)) + lane;
#pragma unroll
    for (int s = 0; s < 2; ++s) bpa[s] = w2t + (size_t)(2 * wave + s) * frag16_f4(3 * H);
    b16_preload(ra, bpa);
  };
  auto stage = [&]() {
#pragma unroll
    for (int it = 0; it < F4; ++it) {
      const int idx = tid + it * 256;
      *reinterpret_cast<f32x4*>(tileA + (idx / V3) * LDA + (idx % V3) * 4) = regs.v[it];
    }
  };
  request(0);
  request_w(0);
  stage();
  __syncthreads();
  STAMP(1);
#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    Load16 hb_now = lhb;
    if (t + 1 < T) request(t + 1);                   // in flight during the product below
    fence_sched();
    // ---- ga = gxh[t] W2_t   (K = 3H)
    f32x4 acc[2] = {zero4(), zero4()};
    mma16_panel<3 * H, 2, false>(acc, tileA + mrow * LDA + ch, bpa, ra);
    const f32x4* w1t = reinterpret_cast<const f32x4*>(w1tf + (size_t)t * frag16_floats(H, H)) + lane;
    const f32x4* bpb[2] = {w1t + (size_t)(2 * wave) * frag16_f4(H), w1t + (size_t)(2 * wave + 1) * frag16_f4(H)};
    Ring16<2> rb;
    b16_preload(rb, bpb);
    fence_sched();
    __syncthreads();                                 // every wave has read the gxh tile (and the previous relation's gh tile)
    {
      f32x4 hbv[2];
      finish16(scr, lane, hb_now, hbv);
#pragma unroll
      for (int s = 0; s < 2; ++s) *reinterpret_cast<f32x4*>(bufG + mrow * LD + cw + 16 * s + ch) = acc[s] * dssilu4(hbv[s]);
    }
    if (t + 1 < T) { stage(); request_w(t + 1); }
    fence_sched();
    __syncthreads();
    // ---- gn_t = gh W1_t
    f32x4 acc2[2] = {zero4(), zero4()};
    mma16_panel<H, 2, false>(acc2, bufG + mrow * LD + ch, bpb, rb);
    if (parts != nullptr) {
      store16<H>(scr, lane, acc2, tile_rsrc(parts + ((size_t)t * Ns + row0) * H, nrows * H), cw);
    } else if (t == 0) {
      gsum[0] = acc2[0]; gsum[1] = acc2[1];
    } else {
      gsum[0] += acc2[0]; gsum[1] += acc2[1];
    }
    STAMP(2 + (t < 3 ? t : 3));
  }
}

template <int H>
__global__ __launch_bounds__(256, kMinWBwd16) void node_pre_bwd16_kernel(PreBwdArgs a) {
  constexpr int TR = kTR16, LD = H + 8;
  extern __shared__ __align__(16) float lds[];               // [TR][3H + 8], [TR][LD], then 4 x [16][36] scratch
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * TR, nrows = min(TR, a.Ns - row0);
  f32x4 unused[2];
  pre_bwd16_phase<H>(a.gxh, a.hb, a.w2tf, a.w1tf, a.gn, a.Ns, a.T, lds, lds + pre_bwd16_tile_floats(H),
                     lds + pre_bwd16_tile_floats(H) + TR * LD + wave * kScr16Floats, row0, nrows, tid, lane, wave, unused);
}

// =====================================================================================================================
// node_update_bwd on 16-row tiles; FUSE: the backward of the layer ABOVE's node projection runs in front, on the same rows
// =====================================================================================================================
// NOGV (the last layer: gvec_out is identically zero and is not passed, a.gvo is null): the backward of dvec = r v1 is left
// out -- the gq3 = sum_d gv[d] v1[d] panel of the first product with its weight fragments, and the gv terms of gv1 and gvec1;
// r (the second half of q23) is not read.  Same bits as the general form fed gvo = +0, for finite saved tensors and as long as
// no accumulator UNDERFLOWS to -0 (a negative partial result below ~1e-45 rounds to -0: the general form's extra +-0 product
// then turns it into +0 where this form keeps -0 -- the sign of a zero in gx1 / gvec1, nothing else):
//   * gq3 is (+0) + (+-0) = +0 there, so the third panel adds products (+-0) w to accumulators that come out of MFMAs that
//     started at +0: an accumulator that is not zero stays what it is, one that is zero is +0 (short of the underflow above, a
//     sum that starts at +0 does not become -0 in round-to-nearest: exact cancellation gives +0) and stays +0;
//   * gvec1's accumulator starts at gv = +0 either way;
//   * gv q3 + s v2 may differ from s v2 in the SIGN of a zero (-0 + +0 = +0), but only as an MFMA operand whose accumulator
//     started at +0: a +-0 product changes neither a non-zero sum nor a +0 one.
//
// Tile rows on chip (the general form, !FUSE && !NOGV: `KEEP`).  Gradients that arrive as partial sums (a.pend.gn) are summed
// by pending16 straight into the registers of the elementwise pass, which has the same row / channel mapping: no store ->
// barrier -> load of gx_out and gvec_out at the head of the workgroup.  gv[d], from those registers or loaded from gvo when
// nothing is pending, is parked in three further LDS tiles (before the `on` factor) and read from there in accumulator layout
// by the last three products: gvo crosses the CU boundary once instead of twice, or -- pending -- not at all as a load.  Per
// row and H floats: 49 -> 42 (pending; 39 with a.hold_gvo, which also drops the gvec_out store nobody reads: 15 MB per launch
// at 10,041 rows), 28 -> 25 without pending.  gx_out keeps its store and ONE reload in accumulator layout (lgx): a sixth tile
// would cost the third workgroup per CU (upd_bwd16_lds_bytes).  FUSE and NOGV keep their data flow and their LDS layout.
template <int H, bool FUSE, bool NOGV = false>
__global__ __launch_bounds__(256, kMinWBwd16) void node_update_bwd16_kernel(UpdBwdArgs a) {
  static_assert(H == 128, "four waves x 32 channels");
  static_assert(!(FUSE && NOGV), "the last layer has no layer above");
  constexpr int TR = kTR16, LD = H + 8, NB16 = H / 16, V = H / 4, F4 = TR * H / 4 / 256;
  constexpr bool KEEP = !FUSE && !NOGV;                      // pending sums handed over in registers, gv[d] in LDS tiles
  // 2 x [TR][LD] (KEEP: + 3 x [TR][LD] for gv[d]), then 4 x [16][36] scratch; FUSE: [TR][3H + 8] (later the two tiles),
  // [TR][LD], then the scratch
  extern __shared__ __align__(16) float lds[];
  float* buf0 = lds;
  float* buf1 = lds + TR * LD;
  float* bufgv = lds + 2 * TR * LD;                          // (KEEP) gv[d]: + d * TR * LD
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* scr = lds + (FUSE ? pre_bwd16_tile_floats(H) + TR * LD : (KEEP ? 5 : 2) * TR * LD) + wave * kScr16Floats;
  const TileInfo ti = find_tile(a.type_rowptr, a.T, a.N, TR, blockIdx.x);
  const int row0 = ti.row0, nrows = ti.nrows, t = ti.t;
  if (t >= a.T) {
    for (int idx = tid; idx < nrows * V; idx += 256) {
      const int r = row0 + idx / V, c = (idx % V) * 4;
      *reinterpret_cast<f32x4*>(a.gx1 + (size_t)r * H + c) = zero4();
#pragma unroll
      for (int d = 0; d < 3; ++d) *reinterpret_cast<f32x4*>(a.gvec1 + ((size_t)r * 3 + d) * H + c) = zero4();
    }
    return;
  }
  STAMP(0);
  STAMP_HWID();
  if constexpr (FUSE) {
    // the projection's backward of the layer above on these rows: its sum over the relations stays in registers, goes through
    // one LDS tile into the LayerNorm backward, and gx_out / gvec_out of the tile are formed as in the unfused form
    f32x4 gsum[2];
    float* bufG = lds + pre_bwd16_tile_floats(H);
    pre_bwd16_phase<H>(a.pend.gxh, a.pend.hb, a.pend.w2tf, a.pend.w1tf, nullptr, a.N, a.pend.nparts, lds, bufG, scr, row0, nrows,
                       tid, lane, wave, gsum);
    // (into the gxh tile's space: its last readers -- the last relation's first product -- are two barriers back)
#pragma unroll
    for (int s = 0; s < 2; ++s) *reinterpret_cast<f32x4*>(lds + (lane & 15) * LD + 32 * wave + 16 * s + 4 * (lane >> 4)) = gsum[s];
    __syncthreads();
    materialise_pending<H, TR, true>(a, row0, nrows, tid, lds, LD);
    STAMP(6);
  } else if constexpr (!KEEP) {
    if (a.pend.gn != nullptr) materialise_pending<H, TR>(a, row0, nrows, tid);   // (incoming gradients still in partial sums)
  }
  // KEEP: incoming gradients that still sit in partial sums are formed in the registers the elementwise pass below takes them from
  const bool pending = KEEP && a.pend.gn != nullptr;         // (wave-uniform: a kernel argument)
  Pend16<H> pg;
  if constexpr (KEEP) {
    if (pending) pending16<H>(a, row0, nrows, tid, pg);
  }
  const f32x4* wx2t = reinterpret_cast<const f32x4*>(a.wx2tf + (size_t)t * frag16_floats(H, 3 * H)) + lane;   // [H, 3H]
  const f32x4* wx0t = reinterpret_cast<const f32x4*>(a.wx0tf + (size_t)t * frag16_floats(2 * H, H)) + lane;   // [2H, H]
  const f32x4* wvt = reinterpret_cast<const f32x4*>(a.wvtf + (size_t)t * frag16_floats(H, 2 * H)) + lane;     // [H, 2H]
  const f32x4* bpa[2];
  const f32x4* bpx[4];
  const f32x4* bpg[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bpa[s] = wx2t + (size_t)(2 * wave + s) * frag16_f4(3 * H);
    bpg[s] = wvt + (size_t)(2 * wave + s) * frag16_f4(2 * H);
  }
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int s = 0; s < 2; ++s) bpx[2 * p + s] = wx0t + (size_t)(p * NB16 + 2 * wave + s) * frag16_f4(H);
  Ring16<2> ra;
  b16_preload(ra, bpa);
  const int mrow = lane & 15, ch = 4 * (lane >> 4), cw = 32 * wave;
  const float inv_sqrt_h = rsqrtf((float)H);
  const rsrc_t gxo_r = tile_rsrc(a.gxo + (size_t)row0 * H, nrows * H);
  const bool no_gvo = NOGV || a.hold_gvo != 0;               // (held: gvo may be null, gv[d] comes from the pending sums)
  const rsrc_t gvo_r = tile_rsrc(no_gvo ? a.gxo : a.gvo + (size_t)row0 * 3 * H, no_gvo ? 0 : nrows * 3 * H);
  const rsrc_t vp_r = tile_rsrc(a.vp + (size_t)row0 * 6 * H, nrows * 6 * H);
  const rsrc_t h2b_r = tile_rsrc(a.h2b + (size_t)row0 * H, nrows * H);
  const rsrc_t q23_r = tile_rsrc(a.q23 + (size_t)row0 * 2 * H, nrows * 2 * H);
  const rsrc_t nrm_r = tile_rsrc(a.nrm + (size_t)row0 * H, nrows * H);
  const rsrc_t act_r = tile_rsrc(a.row_active ? a.row_active + row0 : a.gxo, a.row_active ? nrows : 0);
  const bool all_on = a.row_active == nullptr;
  const rsrc_t gx1_r = tile_rsrc(a.gx1 + (size_t)row0 * H, nrows * H);
  const rsrc_t gvec1_r = tile_rsrc(a.gvec1 + (size_t)row0 * 3 * H, nrows * 3 * H);

  // ---- gq = (gx/sqrt2 | gx vdot/sqrt2 | sum_d gv[d] v1[d]) elementwise, a float4 per thread and position
  Tile16Regs<H> g3;
#pragma unroll
  for (int it = 0; it < F4; ++it) {
    const int idx = tid + it * 256, lr = idx / V, c = (idx % V) * 4;
    const float on = (all_on | (bld(act_r, lr) != 0.f)) ? 1.f : 0.f;
    f32x4 gxr, gvr[3];                                       // gx_out, gvec_out[d] of this position, before the `on` factor
    if (pending) {
      gxr = pg.gx[it];
#pragma unroll
      for (int d = 0; d < 3; ++d) gvr[d] = pg.gv[it][d];
    } else {
      gxr = bld4(gxo_r, lr * H + c);
      if constexpr (!NOGV) {
#pragma unroll
        for (int d = 0; d < 3; ++d) gvr[d] = bld4(gvo_r, (lr * 3 + d) * H + c);
      }
    }
    const f32x4 gx = gxr * on;
    f32x4 vd = zero4(), gq3 = zero4();
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const f32x4 v1 = bld4(vp_r, (lr * 3 + d) * 2 * H + c);
      const f32x4 v2 = bld4(vp_r, (lr * 3 + d) * 2 * H + H + c);
      vd += v1 * v2;
      if constexpr (!NOGV) {
        // (KEEP: parked for the accumulator-layout reads of the last three products; the barrier in front of the first
        // product publishes the tiles, nobody writes them again)
        if constexpr (KEEP) *reinterpret_cast<f32x4*>(bufgv + d * TR * LD + lr * LD + c) = gvr[d];
        const f32x4 gv = gvr[d] * on;
        gq3 += gv * v1;
      }
    }
    *reinterpret_cast<f32x4*>(buf0 + lr * LD + c) = gx * kInvSqrt2;
    *reinterpret_cast<f32x4*>(buf1 + lr * LD + c) = gx * vd * (inv_sqrt_h * kInvSqrt2);
    g3.v[it] = gq3;
  }
  // h2b, gx and q of this wave's accumulator positions: requested now, transposed behind the first product.  (KEEP: gx behind
  // the barrier -- with pending sums its rows were stored by other waves of this workgroup, in pending16.)
  Load16 lh2, lgx, lq2;
  issue16<H>(lh2, lane, h2b_r, cw);
  if constexpr (!KEEP) issue16<H>(lgx, lane, gxo_r, cw);
  issue16<2 * H>(lq2, lane, q23_r, cw);
  __syncthreads();
  if constexpr (KEEP) issue16<H>(lgx, lane, gxo_r, cw);
  STAMP(7);
  // ---- ga2 = gq Wx2  (K = 3H: three panels)
  f32x4 acc[2] = {zero4(), zero4()};
  {
    const f32x4* bp1[2] = {bpa[0] + (size_t)frag16_f4(H), bpa[1] + (size_t)frag16_f4(H)};
    const f32x4* bp2[2] = {bpa[0] + (size_t)frag16_f4(2 * H), bpa[1] + (size_t)frag16_f4(2 * H)};
    mma16_panel<H, 2, true>(acc, buf0 + mrow * LD + ch, bpa, ra);
    if constexpr (!NOGV) {
      __syncthreads();                               // buffer 0 is free
      tile16_store<H, LD>(buf0, g3, tid);
      mma16_panel<H, 2, true>(acc, buf1 + mrow * LD + ch, bp1, ra);
      __syncthreads();                               // third part in place, buffer 1 free
      mma16_panel<H, 2, false>(acc, buf0 + mrow * LD + ch, bp2, ra);
    } else {
      mma16_panel<H, 2, false>(acc, buf1 + mrow * LD + ch, bp1, ra);
      __syncthreads();                               // both buffers free
    }
  }
  STAMP(8);
  Ring16<4> rx;
  b16_preload(rx, bpx);
  fence_sched();
  // ---- gh2 = ga2 * ScaledSiLU'(h2b) -> buffer 1;  s = gvdot / sqrt(H) = gx q / sqrt(2H) per accumulator position
  const float onr = (all_on | (bld(act_r, mrow) != 0.f)) ? 1.f : 0.f;
  f32x4 s_[2], accx[4];
  {
    f32x4 ph2[2], gxv[2], q2[2];
    finish16(scr, lane, lh2, ph2);
    finish16(scr, lane, lgx, gxv);
    finish16(scr, lane, lq2, q2);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      *reinterpret_cast<f32x4*>(buf1 + mrow * LD + cw + 16 * s + ch) = acc[s] * dssilu4(ph2[s]);
      gxv[s] *= onr;
      s_[s] = gxv[s] * q2[s] * (kInvSqrt2 * inv_sqrt_h);
      accx[s] = gxv[s];                  // gxin's gx1 part accumulates onto the identity term gx
      accx[2 + s] = zero4();
    }
  }
  // inputs of the later epilogues, requested one product ahead
  Load16 lnr, lgv, lq3, lw1, lw2;
  issue16<H>(lnr, lane, nrm_r, cw);
  if constexpr (!NOGV) {
    if constexpr (!KEEP) issue16<3 * H>(lgv, lane, gvo_r, cw);
    issue16<2 * H>(lq3, lane, q23_r, H + cw);
  }
  issue16<6 * H>(lw1, lane, vp_r, cw);
  issue16<6 * H>(lw2, lane, vp_r, H + cw);
  fence_sched();
  __syncthreads();
  STAMP(9);
  // ---- gxin = gh2 Wx0 (gx1 part | g|v2| part)
  mma16_panel<H, 4, false>(accx, buf1 + mrow * LD + ch, bpx, rx);
  STAMP(10);
  Ring16<2> rg;
  b16_preload(rg, bpg);
  fence_sched();
  f32x4 gnn[2], pgv[2], pq3[2], pw1[2], pw2[2];
  {
    f32x4 nv[2], gx1v[2];
    finish16(scr, lane, lnr, nv);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      gnn[s] = accx[2 + s] * rcp_clamped4(nv[s]);     // (rows past the tile's end load 0: their products are zero anyway)
      gx1v[s] = accx[s];
    }
    store16<H>(scr, lane, gx1v, gx1_r, cw);
  }
  if constexpr (!NOGV) {
    if constexpr (!KEEP) finish16(scr, lane, lgv, pgv);
    finish16(scr, lane, lq3, pq3);
  }
  finish16(scr, lane, lw1, pw1);
  finish16(scr, lane, lw2, pw2);
  // ---- gvec1[d] = gv[d] + (gv1[d] | gv2[d]) Wv,  gv1 = gv q3 + s v2,  gv2 = s v1 + gnn v2  (the accumulator starts at gv[d])
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    f32x4 accg[2];
    if constexpr (KEEP) {
#pragma unroll
      for (int s = 0; s < 2; ++s) pgv[s] = *reinterpret_cast<const f32x4*>(bufgv + d * TR * LD + mrow * LD + cw + 16 * s + ch);
    }
    __syncthreads();                                 // the previous product has read both buffers
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int c0 = cw + 16 * s + ch;
      if constexpr (NOGV) {
        accg[s] = zero4();
        *reinterpret_cast<f32x4*>(buf0 + mrow * LD + c0) = s_[s] * pw2[s];
      } else {
        const f32x4 gv = pgv[s] * onr;
        accg[s] = gv;
        *reinterpret_cast<f32x4*>(buf0 + mrow * LD + c0) = gv * pq3[s] + s_[s] * pw2[s];
      }
      *reinterpret_cast<f32x4*>(buf1 + mrow * LD + c0) = s_[s] * pw1[s] + gnn[s] * pw2[s];
    }
    fence_sched();
    Load16 ngv, nw1, nw2;
    if (d < 2) {                                     // in flight during the product below
      if constexpr (FUSE) issue16<3 * H>(ngv, lane, gvo_r, (d + 1) * H + cw);
      issue16<6 * H>(nw1, lane, vp_r, (d + 1) * 2 * H + cw);
      issue16<6 * H>(nw2, lane, vp_r, (d + 1) * 2 * H + H + cw);
    }
    fence_sched();
    __syncthreads();
    const f32x4* bpg1[2] = {bpg[0] + (size_t)frag16_f4(H), bpg[1] + (size_t)frag16_f4(H)};
    mma16_panel<H, 2, true>(accg, buf0 + mrow * LD + ch, bpg, rg);
    mma16_panel<H, 2, false>(accg, buf1 + mrow * LD + ch, bpg1, rg);
    if (d < 2) b16_preload(rg, bpg);
    fence_sched();
    if (d < 2) {
      if constexpr (FUSE) finish16(scr, lane, ngv, pgv);
      finish16(scr, lane, nw1, pw1);
      finish16(scr, lane, nw2, pw2);
    }
    store16<3 * H>(scr, lane, accg, gvec1_r, d * H + cw);
    STAMP(11 + d);
  }
}

// =====================================================================================================================
// The read-out (hermnet.py:112-116, 129) on 16-row tiles: Linear(H -> C) on the matrix pipe, ScaledSiLU and the C -> 1 Linear in
// the epilogue; H = 128, C = 64.  The VALU form of csrc/node_kernels.hip (every workgroup stages the whole weight in LDS)
// takes 24 us forward + 16 us backward at 10k rows for 0.3 GFLOP.
// =====================================================================================================================
struct HeadArgs {
  const float* x;        // fwd: x [N, H];  bwd: h [N, C] (saved pre-activations)
  const float* wf;       // fwd: frag16(W0 [C, H]);  bwd: frag16(W0^T [H, C])
  const float* b0;       // [C]
  const float* w2;       // [C]
  const float* b2;       // [1] or null
  const float* ge;       // bwd: [N]
  const float* mask;     // [N] or null
  float* h;              // fwd: [N, C] saved
  float* out;            // fwd: e [N];  bwd: gx [N, H]
  int N;
};
// forward: the [16][H + 8] tile, then [4][16] partial row sums; backward: the [16][C + 8] tile, then the scratch
constexpr size_t head16_fwd_lds_bytes(int H) { return lds16_bytes(kTR16 * (H + 8), 4 * 16); }
constexpr size_t head16_bwd_lds_bytes(int C) { return lds16_bytes(kTR16 * (C + 8)); }

template <int H, int C>
__global__ __launch_bounds__(256) void energy_head16_fwd_kernel(HeadArgs a) {
  static_assert(H == 128 && C == 64, "four waves x 16 output channels");
  constexpr int TR = kTR16, LD = H + 8;
  extern __shared__ __align__(16) float lds[];               // [TR][LD], then [4][16] partial row sums
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * TR, nrows = min(TR, a.N - row0);
  const int mrow = lane & 15, ch = 4 * (lane >> 4);
  const f32x4* bp[1] = {reinterpret_cast<const f32x4*>(a.wf) + (size_t)wave * frag16_f4(H) + lane};
  Ring16<1> ring;
  b16_preload(ring, bp);
  f32x4 acc[1] = {ld4g(a.b0 + 16 * wave + ch)};
  const f32x4 w2v = ld4g(a.w2 + 16 * wave + ch);
  Tile16Regs<H> regs;
  tile16_load<H>(regs, tile_rsrc(a.x + (size_t)row0 * H, nrows * H), H, 0, tid);
  tile16_store<H, LD>(lds, regs, tid);
  __syncthreads();
  mma16_panel<H, 1, false>(acc, lds + mrow * LD + ch, bp, ring);
  const f32x4 hv = acc[0];
  if (mrow < nrows) *reinterpret_cast<f32x4*>(a.h + (size_t)(row0 + mrow) * C + 16 * wave + ch) = hv;
  const f32x4 av = ssilu4(hv);                               // (incl. the 1 / 0.6)
  float s = av[0] * w2v[0];
  s = fmaf(av[1], w2v[1], s);
  s = fmaf(av[2], w2v[2], s);
  s = fmaf(av[3], w2v[3], s);
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  float* part = lds + TR * LD;
  if (lane < 16) part[wave * 16 + lane] = s;
  __syncthreads();
  if (tid < nrows) {
    const float e = ((part[tid] + part[16 + tid]) + (part[32 + tid] + part[48 + tid])) + (a.b2 ? a.b2[0] : 0.f);
    a.out[row0 + tid] = e * (a.mask ? a.mask[row0 + tid] : 1.0f);
  }
}

template <int H, int C>
__global__ __launch_bounds__(256) void energy_head16_bwd_kernel(HeadArgs a) {
  static_assert(H == 128 && C == 64, "four waves x 32 output channels");
  constexpr int TR = kTR16, LDC = C + 8;
  extern __shared__ __align__(16) float lds[];               // [TR][LDC], then 4 x [16][36] scratch
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = blockIdx.x * TR, nrows = min(TR, a.N - row0);
  const int mrow = lane & 15, ch = 4 * (lane >> 4);
  float* scr = lds + TR * LDC + wave * kScr16Floats;
  const f32x4* w = reinterpret_cast<const f32x4*>(a.wf) + lane;
  const f32x4* bp[2] = {w + (size_t)(2 * wave) * frag16_f4(C), w + (size_t)(2 * wave + 1) * frag16_f4(C)};
  Ring16<2> ring;
  b16_preload(ring, bp);
  {   // gh = ge mask w2 ScaledSiLU'(h): one float4 per thread
    const int lr = tid / (C / 4), c = (tid % (C / 4)) * 4;
    f32x4 g = zero4();
    if (lr < nrows) {
      const int row = row0 + lr;
      const float f = a.ge[row] * (a.mask ? a.mask[row] : 1.0f);
      g = dssilu4(ld4g(a.x + (size_t)row * C + c)) * ld4g(a.w2 + c) * f;
    }
    *reinterpret_cast<f32x4*>(lds + lr * LDC + c) = g;
  }
  __syncthreads();
  f32x4 acc[2] = {zero4(), zero4()};
  mma16_panel<C, 2, false>(acc, lds + mrow * LDC + ch, bp, ring);
  store16<H>(scr, lane, acc, tile_rsrc(a.out + (size_t)row0 * H, nrows * H), 32 * wave);
}

constexpr int kH16 = 128, kC16 = 64;      // the width this unit's kernels are instantiated at; the read-out's columns
inline dim3 grid16(int rows) { return dim3((unsigned)((rows + kTR16 - 1) / kTR16)); }
bool head16_supported(int hidden, int cols) { return hidden == kH16 && cols == kC16; }

}  // namespace

#ifdef HN_STAMPS
extern "C" int hermnet_debug_stamps16(unsigned long long* out_host, int count) {
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(hn_stamps), (size_t)count * sizeof(unsigned long long)) == hipSuccess ? 0 : 3;
}
#endif

// ---- what node_chain.hip's hermnet_node_update_fwd / _bwd reach with tile_rows = 16 (node_chain_common.h declares them; the
// caller has checked the argument blocks and hn_update16_supported).  The weight pointers of the argument blocks must hold frag16
// copies (include/hermnet_hip.h: hermnet_node_update_fwd, "16-row form").
int hn_update16_supported(int hidden) { return hidden == kH16; }

int hn_update16_fwd(const UpdFwdArgs& a, int tiles, void* stream) {
  return launch_chain<node_update_fwd16_kernel<kH16, false>>(dim3((unsigned)tiles), upd_fwd16_lds_bytes(kH16), stream, a, PreFwdArgs{});
}

int hn_update16_bwd(const UpdBwdArgs& a, int tiles, void* stream) {
  if (a.pend.gxh != nullptr)        // fused: the projection's backward of the layer above in front
    return launch_chain<node_update_bwd16_kernel<kH16, true>>(dim3((unsigned)tiles), pre_bwd16_lds_bytes(kH16), stream, a);
  return launch_chain<node_update_bwd16_kernel<kH16, false>>(dim3((unsigned)tiles), upd_bwd16_lds_bytes(kH16), stream, a);
}

// hermnet_node_update_bwd (16-row form, `pending` in its gn_parts form) whose gvec_out never leaves the chip: the kernel takes
// gv[d] from the pending sums in registers and LDS, the store nobody reads is skipped (UpdBwdArgs::hold_gvo).
extern "C" int hermnet_node_update_bwd_held(const float* gx_out, const float* gvec_out, const float* vp, const float* h2b,
                                            const float* q23, const float* nrm, const float* wx2t_frag16,
                                            const float* wx0t_frag16, const float* wvt_frag16, const float* row_active,
                                            const int* type_rowptr, const int* type_rowptr_host, float* gx1, float* gvec1,
                                            int num_nodes, int num_rel, int hidden, int tile_rows,
                                            const hn_pending_grads* pending, void* stream) {
  (void)gvec_out;                                  // neither read nor written
  UpdBwdArgs a = {gx_out, nullptr, vp, h2b, q23, nrm, wx2t_frag16, wx0t_frag16, wvt_frag16, row_active, type_rowptr, gx1, gvec1,
                  num_nodes, num_rel, {}, 1};
  if (!pending || tile_rows != 16) return HN_ERR_BAD_ARG;
  const int rc = upd_bwd_refused(a, type_rowptr_host, hn_update16_supported(hidden), false);
  if (rc >= 0) return rc;
  const hn_pending_grads& p = *pending;
  if (!p.gn_parts || p.gxh || !p.gvec_parts || !p.x || !p.mean || !p.rstd || !p.gx1 || !p.gvec1 || p.num_parts < 1 ||
      p.hidden_real > hidden)
    return HN_ERR_BAD_ARG;
  a.pend = {p.gn_parts, p.gvec_parts, p.x, p.mean, p.rstd, p.gx1, p.gvec1, p.num_parts, real_width(p.hidden_real, hidden),
            nullptr, nullptr, nullptr, nullptr};
  return hn_update16_bwd(a, HN_TILES(16), stream);
}

// ---- the layer boundary as ONE node launch each way ---------------------------------------------------------------------------
extern "C" int hermnet_node_fused_supported(int hidden) { return hn_update16_supported(hidden); }

// update of layer l + node projection of layer l + 1 on the same 16-row tiles (p.x is unused: the rows come from the update)
extern "C" int hermnet_node_update_pre_fwd(const float* x1, const float* vec1, const float* wv_frag16, const float* wx0_frag16,
                                           const float* bx0, const float* wx2_frag16, const float* bx2,
                                           const float* row_active, const int* type_rowptr, const int* type_rowptr_host,
                                           float* vp, float* h2b, float* q23, float* nrm, float* x_out, float* vec_out,
                                           int num_nodes, int num_rel, int hidden, const float* w1_frag16, const float* b1,
                                           const float* w2_frag16, const float* b2, float* hb, float* xh, float* mean,
                                           float* rstd, int next_num_rel, int hidden_real, float eps, void* stream) {
  if (next_num_rel <= 0 || hidden_real > hidden) return HN_ERR_BAD_ARG;
  const UpdFwdArgs a = {x1, vec1, wv_frag16, wx0_frag16, bx0, wx2_frag16, bx2, row_active, type_rowptr, vp, h2b, q23, nrm, x_out,
                        vec_out, num_nodes, num_rel};
  const int rc = upd_fwd_refused(a, type_rowptr_host, hn_update16_supported(hidden), false);
  if (rc >= 0) return rc;
  if (!w1_frag16 || !b1 || !w2_frag16 || !b2 || !hb || !xh || !mean || !rstd) return HN_ERR_BAD_ARG;
  const PreFwdArgs p = {x_out, w1_frag16, b1, w2_frag16, b2, hb, xh, mean, rstd, nullptr, num_nodes, next_num_rel,
                        real_width(hidden_real, hidden), eps, nullptr, 0, 0};
  return launch_chain<node_update_fwd16_kernel<kH16, true>>(dim3((unsigned)HN_TILES(16)), fwd16_lds_bytes(kH16), stream, a, p);
}

extern "C" int hermnet_node_pre_fwd16(const float* x, const float* w1_frag16, const float* b1, const float* w2_frag16,
                                      const float* b2, float* hb, float* xh, float* mean, float* rstd, int num_src,
                                      int num_rel, int hidden, int hidden_real, float eps, void* stream) {
  if (num_src < 0 || num_rel <= 0 || hidden_real > hidden || !hn_update16_supported(hidden)) return HN_ERR_BAD_ARG;
  if (num_src == 0) return HN_OK;
  if (!x || !w1_frag16 || !b1 || !w2_frag16 || !b2 || !hb || !xh || !mean || !rstd) return HN_ERR_BAD_ARG;
  const PreFwdArgs p = {x, w1_frag16, b1, w2_frag16, b2, hb, xh, mean, rstd, nullptr, num_src, num_rel,
                        real_width(hidden_real, hidden), eps, nullptr, 0, 0};
  return launch_chain<node_pre_fwd16_kernel<kH16>>(grid16(num_src), fwd16_lds_bytes(kH16), stream, p);
}

extern "C" int hermnet_node_pre_bwd16(const float* gxh, const float* hb, const float* w2t_frag16, const float* w1t_frag16,
                                      float* gn_parts, int num_src, int num_rel, int hidden, void* stream) {
  if (num_src < 0 || num_rel <= 0 || !hn_update16_supported(hidden)) return HN_ERR_BAD_ARG;
  if (num_src == 0) return HN_OK;
  if (!gxh || !hb || !w2t_frag16 || !w1t_frag16 || !gn_parts) return HN_ERR_BAD_ARG;
  const PreBwdArgs a = {gxh, hb, w2t_frag16, w1t_frag16, gn_parts, nullptr, num_src, num_rel, nullptr, 0, 0};
  return launch_chain<node_pre_bwd16_kernel<kH16>>(grid16(num_src), pre_bwd16_lds_bytes(kH16), stream, a);
}

// ---- the read-out on the matrix pipe (hidden 128 -> 64) ---------------------------------------------------------------------------
extern "C" int hermnet_energy_head16_supported(int hidden, int cols) { return head16_supported(hidden, cols); }

extern "C" int hermnet_energy_head16_fwd(const float* x, const float* w0_frag16, const float* b0, const float* w2, const float* b2,
                                         const float* row_mask, float* h, float* e, int rows, int hidden, int cols, void* stream) {
  if (rows < 0 || !head16_supported(hidden, cols)) return HN_ERR_BAD_ARG;
  if (rows == 0) return HN_OK;
  if (!x || !w0_frag16 || !b0 || !w2 || !h || !e) return HN_ERR_BAD_ARG;
  const HeadArgs a = {x, w0_frag16, b0, w2, b2, nullptr, row_mask, h, e, rows};
  return launch_chain<energy_head16_fwd_kernel<kH16, kC16>>(grid16(rows), head16_fwd_lds_bytes(kH16), stream, a);
}

extern "C" int hermnet_energy_head16_bwd(const float* ge, const float* h, const float* w0t_frag16, const float* w2,
                                         const float* row_mask, float* gx, int rows, int hidden, int cols, void* stream) {
  if (rows < 0 || !head16_supported(hidden, cols)) return HN_ERR_BAD_ARG;
  if (rows == 0) return HN_OK;
  if (!ge || !h || !w0t_frag16 || !w2 || !gx) return HN_ERR_BAD_ARG;
  const HeadArgs a = {h, w0t_frag16, nullptr, w2, nullptr, ge, row_mask, nullptr, gx, rows};
  return launch_chain<energy_head16_bwd_kernel<kH16, kC16>>(grid16(rows), head16_bwd_lds_bytes(kC16), stream, a);
}

// ---- the LAST layer of an energy / force evaluation (NOVEC / NOGV) --------------------------------------------------------------
// The read-out takes x only: vec_out feeds nothing, its gradient is identically zero.  16-row tiles, width 128.
extern "C" int hermnet_node_update_fwd_last(const float* x1, const float* vec1, const float* wv_frag16, const float* wx0_frag16,
                                            const float* bx0, const float* wx2_frag16, const float* bx2,
                                            const float* row_active, const int* type_rowptr, const int* type_rowptr_host,
                                            float* vp, float* h2b, float* q2, float* nrm, float* x_out, int num_nodes,
                                            int num_rel, int hidden, void* stream) {
  const UpdFwdArgs a = {x1, vec1, wv_frag16, wx0_frag16, bx0, wx2_frag16, bx2, row_active, type_rowptr, vp, h2b, q2, nrm, x_out,
                        nullptr, num_nodes, num_rel};
  const int rc = upd_fwd_refused(a, type_rowptr_host, hn_update16_supported(hidden) && !use_wide(hidden), true);
  if (rc >= 0) return rc;
  return launch_chain<node_update_fwd16_kernel<kH16, false, true>>(dim3((unsigned)HN_TILES(16)), fwd16_lds_bytes(kH16), stream, a,
                                                                  PreFwdArgs{});
}

extern "C" int hermnet_node_update_bwd_last(const float* gx_out, const float* vp, const float* h2b, const float* q2,
                                            const float* nrm, const float* wx2t_frag16, const float* wx0t_frag16,
                                            const float* wvt_frag16, const float* row_active, const int* type_rowptr,
                                            const int* type_rowptr_host, float* gx1, float* gvec1, int num_nodes, int num_rel,
                                            int hidden, const hn_pending_grads* pending, void* stream) {
  if (pending) return HN_ERR_BAD_ARG;             // no layer above the last one can have handed anything down
  const UpdBwdArgs a = {gx_out, nullptr, vp, h2b, q2, nrm, wx2t_frag16, wx0t_frag16, wvt_frag16, row_active, type_rowptr, gx1,
                        gvec1, num_nodes, num_rel, {}};
  const int rc = upd_bwd_refused(a, type_rowptr_host, hn_update16_supported(hidden) && !use_wide(hidden), true);
  if (rc >= 0) return rc;
  return launch_chain<node_update_bwd16_kernel<kH16, false, true>>(dim3((unsigned)HN_TILES(16)), upd_bwd16_last_lds_bytes(kH16), stream, a);
}
