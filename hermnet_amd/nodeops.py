"""Thin Python wrappers (allocate outputs, pass pointers) around the node-level fused
kernels of `csrc/node_kernels.hip`.  One call = one kernel launch on the current stream, through `ops._call` under its
timer label."""

import ctypes

import torch

from . import _lib
from .ops import _call

P = _lib.ptr


def _new(like, *shape):
    return torch.empty(*shape, dtype=like.dtype, device=like.device)


def layernorm_fwd(x, eps=1e-5, h_real=0):
    """LayerNorm without affine over the last axis -> (n, mean [rows], rstd [rows]).  `h_real` (0 = all): width of
    the statistics when the rows are zero-padded (padded outputs are zero)."""
    rows, H = x.shape
    n, mean, rstd = _new(x, rows, H), _new(x, rows), _new(x, rows)
    _call("layernorm_fwd", "hermnet_layernorm_fwd", P(x), P(n), P(mean), P(rstd), rows, H, h_real, eps)
    return n, mean, rstd


def layernorm_bwd(g, x, mean, rstd, add=None, h_real=0):
    """Gradient of layernorm_fwd w.r.t. x, plus `add`."""
    rows, H = x.shape
    gx = _new(x, rows, H)
    _call("layernorm_bwd", "hermnet_layernorm_bwd", P(g), P(x), P(mean), P(rstd), P(add), P(gx), rows, H, h_real)
    return gx


def ssilu_fwd(h, bias=None, rows_per_bias=0):
    """a = ScaledSiLU(h + bias); h [rows, cols]; bias [groups, cols] (group = row // rows_per_bias) or None."""
    a = _new(h, *h.shape)
    cols = h.size(-1)
    _call("ssilu_fwd", "hermnet_ssilu_fwd", P(h), P(bias), rows_per_bias, P(a), h.numel() // cols, cols)
    return a


def ssilu_bwd(g, h, N, T, C, gs_n, gs_t, bias=None, rows_per_bias=0):
    gh = _new(h, N, T * C)
    _call("ssilu_bwd", "hermnet_ssilu_bwd", P(g), P(h), P(bias), rows_per_bias, P(gh), N, T, C, gs_n, gs_t)
    return gh


def update_mid(vp, x1, rows, H):
    vdot, xin = _new(x1, x1.size(0), H), _new(x1, x1.size(0), 2 * H)
    _call("update_mid", "hermnet_update_mid", P(vp), P(x1), P(vdot), P(xin), rows, H)
    return vdot, xin


def update_out(q, vdot, vp, x1, vec1, mask, N, nk, H, qbias=None, rows_per_bias=0):
    xo, vo = _new(x1, N, H), _new(x1, N, 3, H)
    _call("update_out", "hermnet_update_out", P(q), P(qbias), rows_per_bias, P(vdot), P(vp), P(x1), P(vec1), P(mask), P(xo),
          P(vo), N, nk, H)
    return xo, vo


def update_out_bwd(gxo, gvo, q, vdot, vp, mask, N, nk, H, qbias=None, rows_per_bias=0):
    gq, gvdot, gvp = _new(gxo, N, 3 * H), _new(gxo, N, H), _new(gxo, N, 3, 2 * H)
    gx1, gvec1 = _new(gxo, N, H), _new(gxo, N, 3, H)
    _call("update_out_bwd", "hermnet_update_out_bwd", P(gxo), P(gvo), P(q), P(qbias), rows_per_bias, P(vdot), P(vp), P(mask),
          P(gq), P(gvdot), P(gvp), P(gx1), P(gvec1), N, nk, H)
    return gq, gvdot, gvp, gx1, gvec1


def update_mid_bwd(gvdot, gxin, vp, xin, gvp, gx1, rows, H):
    _call("update_mid_bwd", "hermnet_update_mid_bwd", P(gvdot), P(gxin), P(vp), P(xin), P(gvp), P(gx1), rows, H)


def energy_head_fwd(h, w, b, mask=None):
    """e[n] = (sum_c ScaledSiLU(h[n,c]) w[c] + b[0]) * mask[n]  (b: 1-element device tensor or None)."""
    rows, C = h.shape
    e = _new(h, rows)
    _call("energy_head_fwd", "hermnet_energy_head_fwd", P(h), P(w), P(b), P(mask), P(e), rows, C)
    return e


def energy_head_bwd(ge, h, w, mask=None):
    rows, C = h.shape
    gh = _new(h, rows, C)
    _call("energy_head_bwd", "hermnet_energy_head_bwd", P(ge), P(h), P(w), P(mask), P(gh), rows, C)
    return gh


def head_fused_supported(H, C):
    return C in (64, 128, 256) and H in (64, 128, 256) and H * C * 4 <= 65536


def energy_head_fused_fwd(x, w0t, b0, w2, b2, mask=None):
    """x [rows,H] -> (h [rows,C] pre-activation, e [rows]) in one launch (no library GEMM); w0t = out_energy[0].weight^T."""
    rows, H = x.shape
    C = w0t.size(1)
    h, e = _new(x, rows, C), _new(x, rows)
    _call("energy_head_fused_fwd", "hermnet_energy_head_fused_fwd", P(x), P(w0t), P(b0), P(w2), P(b2), P(mask), P(h), P(e),
          rows, H, C)
    return h, e


def energy_head_fused_bwd(ge, h, w0, w2, mask=None):
    rows, C = h.shape
    H = w0.size(1)
    gx = _new(h, rows, H)
    _call("energy_head_fused_bwd", "hermnet_energy_head_fused_bwd", P(ge), P(h), P(w0), P(w2), P(mask), P(gx), rows, H, C)
    return gx


def head16_supported(H, C):
    return bool(_lib.load().hermnet_energy_head16_supported(int(H), int(C)))


def energy_head16_fwd(x, w0f16, b0, w2, b2, mask=None):
    """The read-out with its H -> C product on the matrix pipe (16-row tiles, H = 128, C = 64): (h [rows,C], e [rows])."""
    rows, H = x.shape
    C = b0.numel()
    h, e = _new(x, rows, C), _new(x, rows)
    _call("energy_head16_fwd", "hermnet_energy_head16_fwd", P(x), P(w0f16), P(b0), P(w2), P(b2), P(mask), P(h), P(e),
          rows, H, C)
    return h, e


def energy_head16_bwd(ge, h, w0tf16, w2, H, mask=None):
    rows, C = h.shape
    gx = _new(h, rows, H)
    _call("energy_head16_bwd", "hermnet_energy_head16_bwd", P(ge), P(h), P(w0tf16), P(w2), P(mask), P(gx), rows, H, C)
    return gx


def pair_mean(x, vec, Te, P_, B, rows_out, backward=False):
    """HTNet: mean over a centre atom's P virtual target rows (backward=False: [Te*P*B, ...] -> [rows_out, ...], zero
    rows behind Te*B) or its gradient (backward=True: [rows_out, ...] -> [Te*P*B, ...])."""
    H = x.size(1)
    rows = Te * P_ * B if backward else rows_out
    xo, vo = _new(x, rows, H), _new(x, rows, 3, H)
    _call("pair_mean", "hermnet_pair_mean", 1 if backward else 0, P(x), P(vec), P(xo), P(vo), Te, P_, B, rows_out, H,
          1.0 / P_, 1.0 / P_, None, 0)
    return xo, vo


def pair_sum_accumulate(x, vec, x_acc, vec_acc, Te, P_, B, scale_x, scale_vec, ranges=None):
    """x_acc[c*B + i] += scale_x * sum_k x[(c*P + k)*B + i] (and vec likewise): the residual's gradient of HTNet's virtual
    target rows, one launch.  `ranges` = (device [k,2] int32, host list): only these rows of x_acc / vec_acc."""
    H = x.size(1)
    rd, nr = (None, 0) if ranges is None else (ranges[0], len(ranges[1]))
    _call("pair_sum", "hermnet_pair_mean", 2, P(x), P(vec), P(x_acc), P(vec_acc), Te, P_, B, x_acc.size(0), H, scale_x,
          scale_vec, P(rd), nr)


def halo_rows(mode, x, vec, idx, buf=None):
    """Packed halo rows [n, 4H] = [x | vec] of the rows `idx` (int64): mode 0 pack, 1 pack-and-clear, 2 unpack
    (see include/hermnet_hip.h).  Returns `buf` (allocated for the packing modes)."""
    n, H = int(idx.numel()), x.size(1)
    if buf is None:
        buf = _new(x, n, 4 * H)
    _call("halo_rows", "hermnet_halo_rows", mode, P(x), P(vec), P(idx), n, H, P(buf))
    return buf


def halo_accumulate(x, vec, plan, buf):
    """rows[plan.acc_rows[u]] += sum of the packed rows `buf[plan.acc_pos[q]]` of segment u, in list order
    (ordered sums: no float atomics anywhere on the path)."""
    rows, ptr, pos = plan.accumulate_lists()
    _call("halo_accumulate", "hermnet_halo_accumulate", P(x), P(vec), P(rows), P(ptr), P(pos), int(rows.numel()), x.size(1),
          P(buf))


def halo_proj_rows(mode, a, b, idx, buf=None):
    """The exchange of PROJECTED halo rows (csrc/node_kernels.hip: hermnet_halo_proj_rows): a packed row holds the S = a.size(0)
    blocks a[j][r] and one block  sum_s b[s][r]  (or b[r] when b has no slice axis), each W = a.size(2) floats.  Forward:
    a = xh [T, N, 3H], b = vec [N, 3, H]; backward: a = gxh, b = the per-relation partial sums of gvec [T, N, 3, H].
    mode 0 pack, 1 pack and clear every source, 2 unpack (b without a slice axis).  Returns `buf` [n, (S + 1) W]."""
    S, N, W = a.shape
    sliced = b.dim() == 4
    nsum = b.size(0) if sliced else 1
    n = int(idx.numel())
    if buf is None:
        buf = _new(a, n, (S + 1) * W)
    _call("halo_rows", "hermnet_halo_proj_rows", mode, P(a), N * W, S, P(b), N * W, nsum, P(idx), n, W, P(buf))
    return buf


def halo_proj_accumulate(a, b, plan, buf):
    """a[j][rows[u]] += the sum of block j of the returned rows of segment u, b[0][rows[u]] (or b[rows[u]]) += the sum of their
    last blocks, in list order (`plan.accumulate_lists()`): the owner's side of the gradient return, no atomics."""
    rows, ptr, pos = plan.accumulate_lists()
    S, N, W = a.shape
    _call("halo_accumulate", "hermnet_halo_proj_accumulate", P(a), N * W, S, P(b), P(rows), P(ptr), P(pos), int(rows.numel()),
          W, P(buf))


# ---- node chain kernels (csrc/node_chain.hip): one launch per chain on the fp32 matrix pipe ---------------------------
def chain_supported(H):
    """Widths the chain kernels are instantiated for: every multiple of 64 up to 512 (csrc/node_chain.hip for 64 / 128 /
    256, csrc/node_chain_wide.hip for the rest).  Anything else -- i.e. padded widths beyond 512 -- takes library GEMMs +
    the stage kernels above."""
    return bool(_lib.load().hermnet_node_chain_supported(int(H)))


def chain_tile_rows(H, update=False):
    """Rows per tile of the pre (or update) chain kernels at width H: the granularity of the row windows."""
    return int(_lib.load().hermnet_node_chain_tile_rows(int(H), 1 if update else 0))


def _bf16_planes(w):
    """w = p0 + p1 + p2 exactly (bf16 planes, each the round-to-nearest-even of what the planes before it leave): the three-way
    split behind the chain kernels' fp32 products on the bf16 matrix pipe (csrc/node_chain_common.h: split8).  Returned smallest
    first -- the order the kernels' weight streams hold them in."""
    w32 = w.float()
    p0 = w32.to(torch.bfloat16)
    r1 = w32 - p0.float()
    p1 = r1.to(torch.bfloat16)
    p2 = (r1 - p1.float()).to(torch.bfloat16)
    return [p2, p1, p0]


def weight_fragments(w):
    """nn.Linear weight [out, in] (or a stack [T, out, in]) -> the chain kernels' weight stream (include/hermnet_hip.h: frag(W);
    csrc/node_chain_common.h: mma_panel): per 32-row block cb of W and 16-deep k-group Q the three bf16 planes of the weights,
    smallest first, as v_mfma_f32_32x32x16_bf16 operands:
        frag(W)[((cb * K/16 + Q) * 3 + s) * 64 + l] = 8 bf16  W_(2-s)[32 cb + (l & 31)][16 Q + 8 (l >> 5) .. +7]
    out % 32 == 0, in % 16 == 0 -> float32 [..., out * in * 3 / 2] (6 bytes per weight, opaque)."""
    return _fragments(w, 32, 16)


def weight_fragments16(w):
    """The same for the 16-row kernels (csrc/node_chain16.hip: mma16_panel; include/hermnet_hip.h: frag16(W)): per 16-row block b
    and 32-deep k-group Q the three planes as v_mfma_f32_16x16x32_bf16 operands:
        frag16(W)[((b * K/32 + Q) * 3 + s) * 64 + l] = 8 bf16  W_(2-s)[16 b + (l & 15)][32 Q + 8 (l >> 4) .. +7]
    out % 16 == 0, in % 32 == 0 -> float32 [..., out * in * 3 / 2]."""
    return _fragments(w, 16, 32)


def _fragments(w, rows, depth):
    """Blocks of `rows` rows of W by k-groups of `depth`, lane l of an operand holding 8 consecutive k of row l % rows."""
    lead = w.shape[:-2]
    o, k = w.shape[-2:]
    n = len(lead)
    f = torch.stack(_bf16_planes(w), dim=n).reshape(*lead, 3, o // rows, rows, k // depth, depth // 8, 8)   # [s, b, m, Q, g, e]
    f = f.permute(*range(n), n + 1, n + 3, n, n + 4, n + 2, n + 5).contiguous()                             # [b, Q, s, g, m, e]
    return f.reshape(*lead, o * k * 3).view(torch.float32)


def update_tile_rows(graph, H):
    """16 or the default tile height: which form of the update kernels shortens the launch for this row layout
    (cached on the graph: it depends on the row counts only)."""
    return graph.derived("upd_tile", lambda: int(_lib.load().hermnet_node_update_tile_rows(
        _rowptr_host(graph), graph.N, graph.T, H)), key=H)


def update_stream(graph, H, w):
    """Which weight stream the update launches of this row layout read -> (tile_rows, (wvf, wx0f, wx2f) of the forward,
    (wx2tf, wx0tf, wvtf) of the backward): 16-row tiles on the frag16 copies where `update_tile_rows` picks them and the width
    has them, else tile_rows = 0 (the width's base tiles) on the frag copies.  The forward and the backward of a layer ask
    here, and so do `last_update_supported` and `fused_boundary_supported`, whose forms have 16-row kernels only."""
    if update_tile_rows(graph, H) == 16 and w.wvf16 is not None:
        return _stream16(w)
    return 0, (w.wvf, w.wx0f, w.wx2f), (w.wx2tf, w.wx0tf, w.wvtf)


def _stream16(w):
    return 16, (w.wvf16, w.wx0f16, w.wx2f16), (w.wx2tf16, w.wx0tf16, w.wvtf16)


def _rowptr_host(graph):
    return graph.derived("rowptr_c", lambda: (ctypes.c_int * len(graph.type_rowptr_host))(*graph.type_rowptr_host))


def _pre_outputs(x, T, zero_stats=False):
    """What a node projection of x [Ns,H] writes: (hb [T,Ns,H], xh [T,Ns,3H], mean [Ns], rstd [Ns])."""
    Ns, H = x.shape
    alloc = torch.zeros if zero_stats else torch.empty
    hb, xh = _new(x, T, Ns, H), _new(x, T, Ns, 3 * H)
    return hb, xh, alloc(Ns, dtype=x.dtype, device=x.device), alloc(Ns, dtype=x.dtype, device=x.device)


def node_pre_fwd(x, w, T, src_ranges=None, windows=None, mode=0, out=None):
    """x [Ns,H] -> (hb [T,Ns,H], xh [T,Ns,3H] incl. bias, mean [Ns], rstd [Ns])  (rmnet.py:52 for every relation).
    `src_ranges` [T,4] int32 (HTNet): the two source-row ranges a relation gathers from; other rows are skipped.
    `windows` [W,2] int32 + `mode` (atom shards): 1 = only the row tiles that touch a window, 2 = only the others;
    the second of the two calls passes the first one's result as `out`."""
    Ns, H = x.shape
    # (rows no relation wants keep (0, 0) statistics: finite)
    hb, xh, mean, rstd = out if out is not None else _pre_outputs(x, T, zero_stats=src_ranges is not None)
    nwin = 0 if windows is None else int(windows.size(0))
    _call("node_pre_fwd", "hermnet_node_pre_fwd", P(x), P(w.w1f), P(w.b1cat), P(w.w2f), P(w.b2), P(hb), P(xh), P(mean),
          P(rstd), P(src_ranges), Ns, T, H, w.h_real, 1e-5, P(windows), nwin, mode if windows is not None else 0)
    return hb, xh, mean, rstd


def species_table(emb, w, T):
    """The per-species table of `layer.SpeciesTable`: xh [T, V, 3H] of node_pre_fwd on the V embedding rows `emb` [V, H], by the
    same entry point and so the same kernel instance as the per-atom launch of this width.  A build, not a step's launch: no
    timer label (`_lib.call`)."""
    from .ops import _stream
    hb, xh, mean, rstd = _pre_outputs(emb, T)
    _lib.call("hermnet_node_pre_fwd", P(emb), P(w.w1f), P(w.b1cat), P(w.w2f), P(w.b2), P(hb), P(xh), P(mean), P(rstd), None,
              emb.size(0), T, emb.size(1), w.h_real, 1e-5, None, 0, 0, _stream())
    return xh


def species_expand(table, z_rows, Ns):
    """xh [T, Ns, 3H] = table[:, z_rows]: node_pre_fwd's xh for x = embedding[z_rows] (`z_rows` [Ns] int64), bit for bit, as one
    copy launch under node_pre_fwd's label (the layer's node projection, in its place among the launches)."""
    T, V, W = table.shape
    xh = _new(table, T, Ns, W)
    _call("node_pre_fwd", "hermnet_species_expand", P(table), P(z_rows), P(xh), Ns, T, V, W)
    return xh


def node_pre_bwd(gxh, hb, x, mean, rstd, w, add=None, src_ranges=None, windows=None, mode=0, out=None, parts_only=False):
    """Gradient of node_pre_fwd w.r.t. x (+ add).  `windows` / `mode` / `out` as in node_pre_fwd (`out` = (gx, parts) of
    the first call).  `parts_only`: no LayerNorm-backward launch -- returns the per-relation partial sums [T,Ns,H] for a
    consumer that runs it itself (node_update_bwd's `pending`)."""
    T, Ns, H = hb.shape
    if parts_only:          # (the LayerNorm backward's operands stay away, and with them the windows)
        x = mean = rstd = add = windows = out = None
    parts, gx = (out[1], out[0]) if out is not None else (_new(hb, T, Ns, H), None if parts_only else torch.empty_like(x))
    nwin = 0 if windows is None else int(windows.size(0))
    _call("node_pre_bwd", "hermnet_node_pre_bwd", P(gxh), P(hb), P(w.w2tf), P(w.w1tf), P(parts), P(x), P(mean), P(rstd),
          P(add), P(gx), P(src_ranges), Ns, T, H, w.h_real, P(windows), nwin, mode if windows is not None else 0)
    if parts_only:
        return parts
    return gx if out is None and windows is None else (gx, parts)


def _update_outputs(x1, vec_out=True):
    """What an update forward writes: the saved (vp [N,3,2H], h2b [N,H], q23 [N,2H], nrm [N,H]), x_out [N,H] and
    vec_out [N,3,H] (None for the form that leaves it out)."""
    N, H = x1.shape
    return (_new(x1, N, 3, 2 * H), _new(x1, N, H), _new(x1, N, 2 * H), _new(x1, N, H), _new(x1, N, H),
            _new(x1, N, 3, H) if vec_out else None)


def _update_fwd(form, x1, vec1, w, graph, w_next=None):
    """The update forward in one of its three forms -> (x_out, vec_out, vp, h2b, q23, nrm, pre_next):
      "general"  node_update_fwd on the stream `update_stream` picks;
      "last"     without vec_out (kernels of the 16-row tiles only; the layer asks `last_update_supported` first);
      "next"     with the next layer's node projection of x_out behind it (likewise; `fused_boundary_supported`)."""
    N, H = x1.shape
    tile, (wvf, wx0f, wx2f), _ = update_stream(graph, H, w) if form == "general" else _stream16(w)
    vp, h2b, q23, nrm, xo, vo = _update_outputs(x1, vec_out=form != "last")
    args = (P(x1), P(vec1), P(wvf), P(wx0f), P(w.bx0_s), P(wx2f), P(w.bx2_s), P(graph.row_active), P(graph.type_rowptr),
            _rowptr_host(graph), P(vp), P(h2b), P(q23), P(nrm), P(xo))
    pre = None
    if form == "general":
        _call("node_update_fwd", "hermnet_node_update_fwd", *args, P(vo), N, graph.T, H, tile)
    elif form == "last":
        _call("node_update_fwd", "hermnet_node_update_fwd_last", *args, N, graph.T, H)
    else:
        pre = _pre_outputs(xo, graph.T)
        _call("node_update_pre_fwd", "hermnet_node_update_pre_fwd", *args, P(vo), N, graph.T, H, P(w_next.w1f16),
              P(w_next.b1cat), P(w_next.w2f16), P(w_next.b2), *[P(t) for t in pre], graph.T, w_next.h_real, 1e-5)
    return xo, vo, vp, h2b, q23, nrm, pre


def _update_bwd(gxo, gvo, vp, h2b, q23, nrm, w, graph, pending=None, held=False):
    """The update backward -> (gx1, gvec1); gvo = None: the last-layer form (gvec_out = 0, 16-row tiles); `held`: the form that
    leaves gvo unwritten (`node_update_bwd_held`)."""
    N, H = gxo.shape
    tile, _, (wx2tf, wx0tf, wvtf) = update_stream(graph, H, w) if gvo is not None else _stream16(w)
    gx1 = torch.empty_like(gxo)
    gvec1 = _new(gxo, N, 3, H)
    saved = (P(vp), P(h2b), P(q23), P(nrm), P(wx2tf), P(wx0tf), P(wvtf), P(graph.row_active), P(graph.type_rowptr),
             _rowptr_host(graph), P(gx1), P(gvec1), N, graph.T, H)
    pend = None if pending is None else ctypes.byref(pending.struct)
    if held:
        _call("node_update_bwd", "hermnet_node_update_bwd_held", P(gxo), P(gvo), *saved, tile, pend)
    elif gvo is not None:
        _call("node_update_bwd", "hermnet_node_update_bwd", P(gxo), P(gvo), *saved, tile, pend)
    else:
        _call("node_update_bwd", "hermnet_node_update_bwd_last", P(gxo), *saved, pend)
    return gx1, gvec1


def node_update_fwd(x1, vec1, w, graph):
    """(x1, vec1) -> (x_out, vec_out) and the saved (vp [N,3,2H], h2b [N,H], q23 [N,2H], nrm [N,H])
    (rmnet.py:94-107, 29-31)."""
    return _update_fwd("general", x1, vec1, w, graph)[:6]


def last_update_supported(graph, H, w):
    """The update launches of the LAST layer without its vec output (csrc/node_chain16.hip: NOVEC / NOGV): width 128 on
    16-row update tiles."""
    return H == 128 and update_stream(graph, H, w)[0] == 16


def node_update_fwd_last(x1, vec1, w, graph):
    """node_update_fwd where nothing reads vec_out (the last layer in front of the read-out) -> (x_out, vp, h2b, q23, nrm);
    of q23 [N,2H] only the q half is written."""
    xo, _, vp, h2b, q23, nrm, _ = _update_fwd("last", x1, vec1, w, graph)
    return xo, vp, h2b, q23, nrm


def node_update_bwd_last(gxo, vp, h2b, q23, nrm, w, graph):
    """node_update_bwd for gvec_out = 0 (the saved tensors of node_update_fwd_last) -> (gx1, gvec1)."""
    return _update_bwd(gxo, None, vp, h2b, q23, nrm, w, graph)


class PendingGrads(object):
    """The gradients a layer's backward hands DOWN while they still sit in partial sums (hn_pending_grads): `gx` / `gvec`
    are the buffers the consumer -- the update backward of the layer below -- fills before it reads them.
    `chain` = (gxh, hb, w2tf16, w1tf16) (round 5, the fused form): the layer above has not even run its node_pre_bwd --
    the consumer runs that chain on its own tiles first; `gn_parts` is then None."""

    def __init__(self, gx, gvec, gn_parts, gvec_parts, x, mean, rstd, gx1, gvec1, h_real, chain=None):
        self.gx, self.gvec = gx, gvec
        self.tensors = (gn_parts, gvec_parts, x, mean, rstd, gx1, gvec1)        # (kept alive until consumed)
        self.chain = chain
        nparts = gvec_parts.size(0)
        extra = [None] * 4 if chain is None else [P(t) for t in chain]
        self.struct = _lib.PendingGrads(*[P(t) for t in self.tensors], nparts, h_real, *extra)


def fused_boundary_supported(graph, H, w, w_next=None):
    """The layer boundary as one node launch each way (csrc/node_chain16.hip): width 128, HVNet rows, and a row layout whose
    update kernels run on 16-row tiles (small grids: nodeops.update_tile_rows).  `w_next`: the next layer's weights (forward
    fusion: same width and relation count)."""
    if H != 128 or graph.num_src or graph.res_row is not None:
        return False
    if w_next is not None and (w_next.w1f16 is None or w_next.b1cat.numel() != graph.T * H):
        return False
    return update_stream(graph, H, w)[0] == 16


def node_update_pre_fwd(x1, vec1, w, graph, w_next):
    """node_update_fwd of this layer + node_pre_fwd of the NEXT layer (weights `w_next`) on the rows it produces, ONE launch:
    returns (x_out, vec_out, vp, h2b, q23, nrm, (hb, xh, mean, rstd))."""
    return _update_fwd("next", x1, vec1, w, graph, w_next)


def node_pre_fwd16(x, w, T):
    """node_pre_fwd on 16-row tiles (the second half of node_update_pre_fwd as a launch of its own: A/B, bit-for-bit check)."""
    Ns, H = x.shape
    pre = _pre_outputs(x, T)
    _call("node_pre_fwd16", "hermnet_node_pre_fwd16", P(x), P(w.w1f16), P(w.b1cat), P(w.w2f16), P(w.b2), *[P(t) for t in pre],
          Ns, T, H, w.h_real, 1e-5)
    return pre


def node_pre_bwd16(gxh, hb, w):
    """Per-relation partial sums gn [T,Ns,H] of node_pre_bwd on 16-row tiles (the first half of the fused update backward as
    a launch of its own)."""
    T, Ns, H = hb.shape
    parts = _new(hb, T, Ns, H)
    _call("node_pre_bwd16", "hermnet_node_pre_bwd16", P(gxh), P(hb), P(w.w2tf16), P(w.w1tf16), P(parts), Ns, T, H)
    return parts


def held_update_supported(graph, H, w):
    """`node_update_bwd_held` exists where the update launches of this row layout run 16-row tiles at width 128."""
    return H == 128 and update_stream(graph, H, w)[0] == 16


def node_update_bwd_held(gxo, gvo, vp, h2b, q23, nrm, w, graph, pending):
    """node_update_bwd with `pending` in its partial-sums form (`pending.chain is None`; `held_update_supported`) that keeps the
    gvec gradients it forms on chip: `gvo` is neither read nor written (same gx1 / gvec1 bits), `gxo` is workspace of the launch."""
    return _update_bwd(gxo, gvo, vp, h2b, q23, nrm, w, graph, pending, held=True)


def node_update_bwd(gxo, gvo, vp, h2b, q23, nrm, w, graph, pending=None):
    """Gradient of node_update_fwd w.r.t. (x1, vec1).  `pending` (PendingGrads whose gx / gvec ARE gxo / gvo): the kernel
    forms the incoming gradients from the partial sums of the layer above first."""
    return _update_bwd(gxo, gvo, vp, h2b, q23, nrm, w, graph, pending)
