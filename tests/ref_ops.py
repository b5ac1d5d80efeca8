"""Plain-PyTorch fp32/fp64 restatement of the two fused operators, in relation (row) order,
with DENSE radial basis (rmnet.py:168-172) -- used to localise kernel bugs op by op."""
import math

import torch


def geometry_ref(pos, graph, cell):
    j, i = graph.src_id.long(), graph.tgt_id.long()
    D = pos[j] - pos[i]
    if graph.shift is not None and cell is not None:
        c = cell.reshape(-1, 3, 3).to(pos.dtype)
        D = D + torch.einsum('ni,nij->nj', graph.shift.to(pos.dtype), c[graph.batch32.long()[j]])
    d = D.norm(dim=-1)
    d = torch.where(d.abs() <= 1e-6, torch.full_like(d, 1e-6), d)
    return torch.cat([D / d[:, None], d[:, None]], dim=1)


def envelope_ref(u, kind, p, factored=False):
    """rmnet.py:175-208.  `u` is masked BEFORE the expression as well as behind it: beyond the cutoff the expression is
    evaluated at 0, so the gradient there is exactly 0 (torch.where alone hands the NaN of exp(-u^2 / 0) or of inf * 0
    through its backward).  `factored`: the polynomial as 1 - u^p (1 + p w + p(p+1)/2 w^2), w = 1 - u -- the same
    polynomial (hermnet_math.h: hn_envelope) without the reference's left-to-right cancellation of terms of size ~p^2."""
    inside = u < 1
    us = torch.where(inside, u, torch.zeros_like(u))
    if kind == 0 and factored:
        w = 1 - us
        val = 1 - us ** p * (1 + p * w + (p * (p + 1) / 2) * w * w)
    elif kind == 0:
        a = -(p + 1) * (p + 2) / 2
        b = p * (p + 2)
        c = -p * (p + 1) / 2
        val = 1 + a * us ** p + b * us ** (p + 1) + c * us ** (p + 2)
    else:
        val = torch.exp(-(us ** 2) / ((1 - us) * (1 + us)))
    return torch.where(inside, val, torch.zeros_like(u))


def window_lo_ref(d, inv_rc, R):
    """hermnet_math.h: hn_window_lo in torch, on the fp32 distances the kernels see: lowest tap of the 12-tap window,
    in [-5, R] (taps outside [0, R) meet zero rows)."""
    u = d.float() * torch.tensor(inv_rc, dtype=torch.float32)
    t = (u * float(R - 1)).clamp(0.0, float(R + 5))
    return t.to(torch.int64) - 5


def message_scatter_ref(xh, vec, x, edge, wt, brbf, graph, rbf, factored=False, band=None, per_relation=False, residual=None):
    """Same contract as hermnet_message_scatter_fwd.  xh [T,Ns,3H]; wt [T,R,3H]; outputs in TARGET rows
    (graph.N; = source rows unless graph.num_src / graph.res_row are set: HTNet's virtual target rows).
    `factored`: envelope_ref's.  `band` = (lo [E] int64, taps): only the taps lo .. lo + taps - 1 of every edge (the
    kernels' banding, window_lo_ref) instead of all R.  `per_relation` (implied by `band`): the projection as one
    [E,R] x [R,3H] product per relation instead of one over a gathered [E,R,3H] weight -- the same sums.  `residual` =
    (x rows, vec rows or None) [N, ...]: the residual's operands where they are not to be x / vec (through res_row)
    themselves -- the kernels' backward contract with virtual target rows leaves the residual's identity term to the host."""
    T, _, H3 = xh.shape
    N = graph.N
    H = H3 // 3
    dt = x.dtype
    rowptr = graph.csr_rowptr.long()
    tgt_row = torch.repeat_interleave(torch.arange(N, device=x.device), rowptr[1:] - rowptr[:-1])
    src = graph.csr_src.long()
    trp = graph.type_rowptr.long()
    rel_row = torch.bucketize(torch.arange(N, device=x.device), trp[1:], right=True)  # T for unknown rows
    rel_e = rel_row[tgt_row]
    known = rel_e < T
    rhat, d = edge[:, :3], edge[:, 3]
    u = d * rbf.inv_rc
    env = envelope_ref(u, rbf.env_kind, rbf.env_p, factored)
    off = rbf.offset.to(dt)
    coeff = -0.5 / float(off[1] - off[0]) ** 2
    emb = env[:, None] * torch.exp(coeff * (u[:, None] - off[None, :]) ** 2)        # [E,R]
    re = rel_e.clamp(max=T - 1)
    if band is None and not per_relation:
        rb = torch.einsum('er,erc->ec', emb, wt[re]) + brbf[re]                      # [E,3H]
    else:
        if band is not None:
            lo, taps = band
            k = torch.arange(off.numel(), device=x.device)[None, :]
            emb = emb * ((k >= lo[:, None]) & (k < lo[:, None] + taps)).to(dt)
        onehot = torch.nn.functional.one_hot(re, T).to(dt)                           # [E,T]
        rb = sum(onehot[:, t:t + 1] * (emb @ wt[t]) for t in range(T)) + brbf[re]
    m = xh[re, src] * rb
    s, a, b = m[:, :H], m[:, H:2 * H], m[:, 2 * H:]
    mv = b[:, None, :] * rhat[:, :, None]
    if vec is not None:
        mv = mv + vec[src] * (a * (1 / math.sqrt(3.0)))[:, None, :]
    mv = mv * (1 / math.sqrt(H))
    kf = known.to(dt)
    dx = torch.zeros(N, H, dtype=dt, device=x.device).index_add_(0, tgt_row, s * kf[:, None])
    dv = torch.zeros(N, 3, H, dtype=dt, device=x.device).index_add_(0, tgt_row, mv * kf[:, None, None])
    rk = (rel_row < T).to(dt)
    res = getattr(graph, "res_row", None)
    xr = x if res is None else x[res.long()]
    v0 = torch.zeros_like(dv) if vec is None else (vec if res is None else vec[res.long()])
    if residual is not None:
        xr, v0 = residual[0], (torch.zeros_like(dv) if residual[1] is None else residual[1])
    x1 = (xr + dx) * (1 / math.sqrt(2.0)) * rk[:, None]
    vec1 = (v0 + dv) * rk[:, None, None]
    return x1, vec1


# ---------------------------------------------------------------------------------------------
# Plain-PyTorch versions of the node-level fused kernels (same contracts as hermnet_amd.nodeops)
# and of the message kernels' forward/backward entry points used by hermnet_amd.layer.
# ---------------------------------------------------------------------------------------------
def layernorm_fwd(x, eps=1e-5, h_real=0):
    Hr = h_real or x.size(-1)
    n, mean, rstd = torch.native_layer_norm(x[:, :Hr].contiguous(), [Hr], None, None, eps)
    if Hr < x.size(-1):
        n = torch.nn.functional.pad(n, (0, x.size(-1) - Hr))
    return n, mean.reshape(-1), rstd.reshape(-1)


def layernorm_bwd(g, x, mean, rstd, add=None, h_real=0):
    Hr = h_real or x.size(-1)
    gx = torch.ops.aten.native_layer_norm_backward(g[:, :Hr].contiguous(), x[:, :Hr].contiguous(), [Hr], mean.reshape(-1, 1),
                                                   rstd.reshape(-1, 1), None, None, [True, False, False])[0]
    if Hr < x.size(-1):
        gx = torch.nn.functional.pad(gx, (0, x.size(-1) - Hr))
    return gx if add is None else gx + add


def energy_head_fwd(h, w, b, mask=None):
    e = (torch.nn.functional.silu(h) / 0.6) @ w + (0 if b is None else b[0])
    return e if mask is None else e * mask


def energy_head_bwd(ge, h, w, mask=None):
    g = ge if mask is None else ge * mask
    return g[:, None] * w[None, :] * _dssilu(h)


def _with_bias(h, bias, rows_per_bias):
    """h [rows, cols] + bias [groups, cols] (group = row // rows_per_bias; <= 0: one row): the kernels'
    "bias convention" (include/hermnet_hip.h)."""
    if bias is None:
        return h
    b = bias.reshape(-1, h.size(-1))
    if rows_per_bias <= 0:
        return h + b[0]
    grp = torch.arange(h.size(0)) // rows_per_bias
    return h + b[grp]


def ssilu_fwd(h, bias=None, rows_per_bias=0):
    return torch.nn.functional.silu(_with_bias(h, bias, rows_per_bias)) / 0.6


def _dssilu(h):
    s = torch.sigmoid(h)
    return s * (1 + h * (1 - s)) / 0.6


def ssilu_bwd(g, h, N, T, C, gs_n, gs_t, bias=None, rows_per_bias=0):
    gg = torch.as_strided(g, (N, T, C), (gs_n, gs_t, 1))
    hb = _with_bias(h.reshape(-1)[:N * T * C].view(N, T * C), bias, rows_per_bias)
    return (gg * _dssilu(hb.view(N, T, C))).reshape(N, T * C)


def update_mid(vp, x1, rows, H):
    v1, v2 = vp[..., :H], vp[..., H:]
    vdot = torch.zeros(x1.size(0), H, dtype=x1.dtype)
    xin = torch.zeros(x1.size(0), 2 * H, dtype=x1.dtype)
    vdot[:rows] = (v1[:rows] * v2[:rows]).sum(1) / math.sqrt(H)
    xin[:rows, :H] = x1[:rows]
    xin[:rows, H:] = torch.sqrt((v2[:rows] ** 2).sum(1) + 1e-8)
    return vdot, xin


def _on(mask, N, nk):
    on = torch.arange(N) < nk
    if mask is not None:
        on = on & (mask != 0)
    return on


def _q_with_bias(q, qbias, rows_per_bias, nk):
    if qbias is None:
        return q
    q = q.clone()
    q[:nk] = _with_bias(q[:nk], qbias, rows_per_bias)
    return q


def update_out(q, vdot, vp, x1, vec1, mask, N, nk, H, qbias=None, rows_per_bias=0):
    on = _on(mask, N, nk)
    q = _q_with_bias(q, qbias, rows_per_bias, nk)
    q1, q2, q3 = q[:, :H], q[:, H:2 * H], q[:, 2 * H:]
    xo = x1 + (q1 + q2 * vdot) / math.sqrt(2.0)
    vo = vec1 + q3[:, None, :] * vp[..., :H]
    z = torch.zeros(())
    return torch.where(on[:, None], xo, z), torch.where(on[:, None, None], vo, z)


def update_out_bwd(gxo, gvo, q, vdot, vp, mask, N, nk, H, qbias=None, rows_per_bias=0):
    on = _on(mask, N, nk)
    q = _q_with_bias(q, qbias, rows_per_bias, nk)
    z = torch.zeros(())
    gx = torch.where(on[:, None], gxo, z)
    gv = torch.where(on[:, None, None], gvo, z)
    q2, q3 = q[:, H:2 * H], q[:, 2 * H:]
    s = 1 / math.sqrt(2.0)
    gq = torch.cat([gx * s, gx * vdot * s, (gv * vp[..., :H]).sum(1)], 1)
    gq = torch.where(on[:, None], gq, z)
    gvdot = torch.where(on[:, None], gx * q2 * s, z)
    gvp = torch.zeros(N, 3, 2 * H, dtype=gxo.dtype)
    gvp[..., :H] = torch.where(on[:, None, None], gv * q3[:, None, :], z)
    gvp[..., H:] = float("nan")          # the kernel leaves this half for update_mid_bwd
    gvp[nk:] = float("nan")
    return gq, gvdot, gvp, gx.clone(), gv.clone()


def update_mid_bwd(gvdot, gxin, vp, xin, gvp, gx1, rows, H):
    s = 1 / math.sqrt(H)
    v1, v2 = vp[:rows, :, :H], vp[:rows, :, H:]
    gd = gvdot[:rows, None, :]
    gnn = (gxin[:rows, H:] / xin[:rows, H:])[:, None, :]
    gx1[:rows] += gxin[:rows, :H]
    p = gvp[:rows, :, :H].clone()
    gvp[:rows, :, :H] = p + gd * s * v2
    gvp[:rows, :, H:] = gd * s * v1 + gnn * v2


# ---- node chain kernels (hermnet_amd.nodeops.node_*; csrc/node_chain.hip): same contracts, plain weights of `w` --------
def _tile_rows(Ns, H, windows, mode, device):
    """Rows of the tiles a windowed launch of the pre kernels runs (csrc/node_chain.hip: tile_selected)."""
    from hermnet_amd import nodeops
    TR = nodeops.chain_tile_rows(H)
    row0 = torch.arange(Ns, device=device) // TR * TR
    inside = torch.zeros(Ns, dtype=torch.bool, device=device)
    for lo, hi in windows.tolist():
        if hi > lo:
            inside |= (row0 < hi) & (row0 + TR > lo)
    return inside if mode == 1 else ~inside


def node_pre_fwd(x, w, T, src_ranges=None, windows=None, mode=0, out=None):
    Ns, H = x.shape
    dt = x.dtype
    n, mean, rstd = layernorm_fwd(x, 1e-5, h_real=w.h_real)
    hb = (n @ w.w1cat.to(dt).t() + w.b1cat.to(dt)).view(Ns, T, H).transpose(0, 1).contiguous()      # [T, Ns, H]
    a = torch.nn.functional.silu(hb) / 0.6
    xh = torch.bmm(a, w.w2t.to(dt)) + w.b2.to(dt)                                                    # [T, Ns, 3H]
    if windows is None or mode == 0:
        return hb, xh, mean, rstd
    # a windowed launch writes the rows of its tiles only (the rest: poison until the other launch fills it)
    rows = _tile_rows(Ns, H, windows, mode, x.device)
    if out is None:
        out = tuple(torch.full_like(t_, float("nan")) for t_ in (hb, xh, mean, rstd))
    out[0][:, rows], out[1][:, rows], out[2][rows], out[3][rows] = hb[:, rows], xh[:, rows], mean[rows], rstd[rows]
    return out


def node_pre_bwd(gxh, hb, x, mean, rstd, w, add=None, src_ranges=None, windows=None, mode=0, out=None, parts_only=False):
    T, Ns, H = hb.shape
    dt = x.dtype
    gh = torch.bmm(gxh, w.w2.to(dt)) * _dssilu(hb)                                                   # [T, Ns, H]
    gn = torch.bmm(gh, w.w1cat.to(dt).view(T, H, H))
    if parts_only:            # (hermnet_node_pre_bwd with gx = NULL: the per-relation partial sums only)
        return gn
    gn = gn.sum(0)
    gx = layernorm_bwd(gn, x, mean, rstd, add=add, h_real=w.h_real)
    if windows is None or mode == 0:
        return gx
    rows = _tile_rows(Ns, H, windows, mode, x.device)
    if out is None:
        out = (torch.full_like(gx, float("nan")), None)
    out[0][rows] = gx[rows]
    return out


def pair_mean(x, vec, Te, P, B, rows_out, backward=False):
    """csrc/node_kernels.hip: hermnet_pair_mean, modes 0 and 1.  Target rows are [Te][P][B] blocks of B rows.
    forward: [Te*P*B, ...] -> [rows_out, ...], row c*B + i = the mean over k of row (c*P + k)*B + i, zero rows behind Te*B;
    backward: [rows_out, ...] -> [Te*P*B, ...], row (c*P + k)*B + i = row c*B + i / P."""
    outs = []
    for t in (x, vec):
        tail = tuple(t.shape[1:])
        if backward:
            g = t[:Te * B].reshape((Te, 1, B) + tail).expand((Te, P, B) + tail)
            outs.append((g * (1.0 / P)).reshape((Te * P * B,) + tail))
        else:
            out = torch.zeros((rows_out,) + tail, dtype=t.dtype)
            out[:Te * B] = (t.view((Te, P, B) + tail).sum(1) * (1.0 / P)).reshape((Te * B,) + tail)
            outs.append(out)
    return tuple(outs)


def pair_sum_accumulate(x, vec, x_acc, vec_acc, Te, P, B, scale_x, scale_vec, ranges=None):
    """hermnet_pair_mean, mode 2 (in place): x_acc[c*B + i] += scale_x * sum_k x[(c*P + k)*B + i], vec likewise with
    scale_vec.  `ranges` = (tensor [k,2], host list of (lo, hi)): only the rows of x_acc / vec_acc inside one of them."""
    sel = torch.ones(Te * B, dtype=torch.bool) if ranges is None else _rows_of_ranges(
        [(lo, min(hi, Te * B)) for lo, hi in ranges[1]], Te * B)
    for t, acc, s in ((x, x_acc, scale_x), (vec, vec_acc, scale_vec)):
        tail = tuple(t.shape[1:])
        add = (t.view((Te, P, B) + tail).sum(1) * s).reshape((Te * B,) + tail)
        acc[:Te * B][sel] += add[sel]


def halo_rows(mode, x, vec, idx, buf=None):
    """csrc/node_kernels.hip: hermnet_halo_rows -- 0 pack, 1 pack-and-clear, 2 unpack (in place)."""
    H = x.size(1)
    if mode in (0, 1):
        buf = torch.cat([x.index_select(0, idx), vec.index_select(0, idx).reshape(-1, 3 * H)], dim=1)
        if mode == 1:
            x.index_fill_(0, idx, 0)
            vec.index_fill_(0, idx, 0)
        return buf
    assert mode == 2
    x.index_copy_(0, idx, buf[:, :H])
    vec.index_copy_(0, idx, buf[:, H:].reshape(-1, 3, H))
    return buf


def halo_proj_rows(mode, a, b, idx, buf=None):
    """csrc/node_kernels.hip: hermnet_halo_proj_rows -- packed row = [a[0][r] | ... | a[S-1][r] | sum_s b[s][r]]."""
    S, N, W = a.shape
    sliced = b.dim() == 4
    bv = b.reshape((b.size(0) if sliced else 1), N, W)
    if mode in (0, 1):
        buf = torch.cat([a.index_select(1, idx).permute(1, 0, 2).reshape(idx.numel(), S * W),
                         bv.index_select(1, idx).sum(0)], dim=1)
        if mode == 1:
            a.index_fill_(1, idx, 0)
            bv.index_fill_(1, idx, 0)
        return buf
    assert mode == 2 and not sliced
    a.index_copy_(1, idx, buf[:, :S * W].reshape(-1, S, W).permute(1, 0, 2))
    bv[0].index_copy_(0, idx, buf[:, S * W:])
    return buf


def halo_proj_accumulate(a, b, plan, buf):
    S, N, W = a.shape
    bv = b.reshape(-1, N, W)
    a.index_add_(1, plan.send_idx, buf[:, :S * W].reshape(-1, S, W).permute(1, 0, 2))
    bv[0].index_add_(0, plan.send_idx, buf[:, S * W:])


def halo_accumulate(x, vec, plan, buf):
    """hermnet_halo_accumulate: returned gradients summed per owned row in send-list order."""
    H = x.size(1)
    if buf.size(0) == 0:
        return
    rows, ptr, pos = plan.accumulate_lists()
    seg = torch.segment_reduce(buf.index_select(0, pos), "sum", lengths=ptr[1:] - ptr[:-1])
    x.index_add_(0, rows, seg[:, :H])
    vec.index_add_(0, rows, seg[:, H:].reshape(-1, 3, H))


def _update_parts(x1, vec1, w, graph):
    """Per relation block: (rows, v1, v2, vdot, norm, h2b, p, q, r) with autograd enabled inputs."""
    H = x1.size(1)
    dt = x1.dtype
    rp = graph.type_rowptr_host
    out = []
    for t in range(graph.T):
        lo, hi = rp[t], rp[t + 1]
        if hi <= lo:
            continue
        vp = vec1[lo:hi] @ w.wv[t].to(dt).t()                                   # [n, 3, 2H]
        v1, v2 = vp[..., :H], vp[..., H:]
        vdot = (v1 * v2).sum(1) / math.sqrt(H)
        norm = torch.sqrt((v2 ** 2).sum(1) + 1e-8)
        h2b = torch.cat([x1[lo:hi], norm], 1) @ w.wx0[t].to(dt).t() + w.bx0[t].to(dt)
        pqr = (torch.nn.functional.silu(h2b) / 0.6) @ w.wx2[t].to(dt).t() + w.bx2[t].to(dt)
        out.append((lo, hi, vp, v1, vdot, h2b, pqr))
    return out


def _node_update(x1, vec1, w, graph):
    N, H = x1.shape
    dt = x1.dtype
    act = torch.ones(N, dtype=dt) if graph.row_active is None else graph.row_active.to(dt)
    xo = torch.zeros(N, H, dtype=dt)
    vo = torch.zeros(N, 3, H, dtype=dt)
    vp_all = torch.zeros(N, 3, 2 * H, dtype=dt)
    h2b_all = torch.zeros(N, H, dtype=dt)
    q23 = torch.zeros(N, 2 * H, dtype=dt)
    nrm = torch.zeros(N, H, dtype=dt)
    xs, vs = [], []
    for lo, hi, vp, v1, vdot, h2b, pqr in _update_parts(x1, vec1, w, graph):
        p, q, r = pqr[:, :H], pqr[:, H:2 * H], pqr[:, 2 * H:]
        m = (act[lo:hi] != 0).to(dt)
        xs.append((lo, hi, (x1[lo:hi] + (p + q * vdot) / math.sqrt(2.0)) * m[:, None]))
        vs.append((lo, hi, (vec1[lo:hi] + r[:, None, :] * v1) * m[:, None, None]))
        vp_all[lo:hi], h2b_all[lo:hi], q23[lo:hi] = vp.detach(), h2b.detach(), pqr[:, H:].detach()
        nrm[lo:hi] = torch.sqrt((vp[..., H:].detach() ** 2).sum(1) + 1e-8)
    if xs:
        xo = torch.cat([torch.zeros(0, H, dtype=dt)] + _fill_rows(xs, N, (H,), dt))
        vo = torch.cat([torch.zeros(0, 3, H, dtype=dt)] + _fill_rows(vs, N, (3, H), dt))
    return xo, vo, vp_all, h2b_all, q23, nrm


def _fill_rows(parts, N, shape, dt):
    """Differentiable assembly of row blocks [(lo, hi, values)] into an N-row array (gaps = zero rows)."""
    out, at = [], 0
    for lo, hi, v in parts:
        if lo > at:
            out.append(torch.zeros((lo - at,) + shape, dtype=dt))
        out.append(v)
        at = hi
    if at < N:
        out.append(torch.zeros((N - at,) + shape, dtype=dt))
    return out


def node_update_fwd(x1, vec1, w, graph):
    with torch.no_grad():
        return _node_update(x1, vec1, w, graph)


def node_update_pre_fwd(x1, vec1, w, graph, w_next):
    """hermnet_node_update_pre_fwd: this layer's update and the NEXT layer's node projection of the rows it produces."""
    out = node_update_fwd(x1, vec1, w, graph)
    return tuple(out) + (node_pre_fwd(out[0], w_next, graph.T),)


def node_pre_fwd16(x, w, T):
    return node_pre_fwd(x, w, T)


def node_pre_bwd16(gxh, hb, w):
    T, Ns, H = hb.shape
    dt = hb.dtype
    gh = torch.bmm(gxh, w.w2.to(dt)) * _dssilu(hb)
    return torch.bmm(gh, w.w1cat.to(dt).view(T, H, H))


def node_update_bwd(gxo, gvo, vp, h2b, q23, nrm, w, graph, pending=None):
    """The kernel's backward formulas from the saved (vp, h2b, q23) (checked against autograd of the forward in
    tests/test_host_logic.py).  `pending` (hn_pending_grads): gxo / gvo are formed here first, from the partial sums of
    the layer above, and written into the caller's buffers."""
    N, H = gxo.shape
    dt = gxo.dtype
    if pending is not None:
        gn, gv, x, mean, rstd, gx1_up, gvec1_up = pending.tensors
        if pending.chain is not None:       # the fused form: the layer above's projection backward runs here, on gxh
            gn = node_pre_bwd16(pending.chain[0], pending.chain[1], pending.w_above)
        ident = (torch.arange(N) < graph.type_rowptr_host[-1]).to(dt)
        gxo.copy_(layernorm_bwd(gn.sum(0), x, mean, rstd, add=gx1_up * ident[:, None] / math.sqrt(2.0),
                                h_real=pending.struct.hidden_real))
        gvo.copy_(gv.sum(0) + gvec1_up * ident[:, None, None])
    act = torch.ones(N, dtype=dt) if graph.row_active is None else graph.row_active.to(dt)
    gx1 = torch.zeros(N, H, dtype=dt)
    gvec1 = torch.zeros(N, 3, H, dtype=dt)
    rp = graph.type_rowptr_host
    r2, rh = 1 / math.sqrt(2.0), 1 / math.sqrt(H)
    for t in range(graph.T):
        lo, hi = rp[t], rp[t + 1]
        if hi <= lo:
            continue
        m = (act[lo:hi] != 0).to(dt)
        gx, gv = gxo[lo:hi] * m[:, None], gvo[lo:hi] * m[:, None, None]
        v1, v2 = vp[lo:hi, :, :H], vp[lo:hi, :, H:]
        vdot = (v1 * v2).sum(1) * rh
        norm = nrm[lo:hi]
        q2, q3 = q23[lo:hi, :H], q23[lo:hi, H:]
        gq = torch.cat([gx * r2, gx * vdot * r2, (gv * v1).sum(1)], 1)
        gh2 = (gq @ w.wx2[t].to(dt)) * _dssilu(h2b[lo:hi])
        gxin = gh2 @ w.wx0[t].to(dt)
        gx1[lo:hi] = gx + gxin[:, :H]
        gnn = gxin[:, H:] / norm
        s_ = gx * q2 * (r2 * rh)
        gv1 = gv * q3[:, None, :] + s_[:, None, :] * v2
        gv2 = s_[:, None, :] * v1 + gnn[:, None, :] * v2
        gvec1[lo:hi] = gv + torch.cat([gv1, gv2], -1) @ w.wv[t].to(dt)
    return gx1, gvec1


def node_update_bwd_from_inputs(gxo, gvo, x1, vec1, w, graph):
    with torch.enable_grad():
        x1_ = x1.detach().requires_grad_(True)
        v_ = vec1.detach().requires_grad_(True)
        xo, vo = _node_update(x1_, v_, w, graph)[:2]
        return torch.autograd.grad([xo, vo], [x1_, v_], [gxo, gvo])


def _rows_of_ranges(ranges, n):
    sel = torch.zeros(n, dtype=torch.bool)
    for lo, hi in ranges:
        if hi > lo:
            sel[lo:hi] = True
    return sel


def msg_fwd(graph, rbf, H, xh, vec, x, w, edge, xh_bias=True, ranges=None, zero_unknown=True, out=None, range_rows=0):
    """`ranges` [T,2]: like the kernel, only these target rows are written (the rest keeps what `out` holds: poison
    when this call allocates it)."""
    edge = edge[0] if edge.dim() == 3 else edge
    x1, vec1 = message_scatter_ref(xh + w.b2 if xh_bias else xh, vec, x, edge, w.wt, w.brbf, graph, rbf)  # xh_bias = w.b2 [T,1,3H]
    if ranges is None:
        return x1, vec1
    sel = _rows_of_ranges(ranges.tolist(), x1.size(0))
    if zero_unknown:
        sel[int(graph.type_rowptr[-1]):] = True
    if out is None:
        out = (torch.full_like(x1, float("nan")), torch.full_like(vec1, float("nan")))
    out[0][sel], out[1][sel] = x1[sel], vec1[sel]
    return out


def msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, gedge, xh_bias=True, ranges=None, out=None, finish=True):
    """Backward contract of hermnet_message_scatter_bwd via autograd of the dense restatement;
    the edge gradient is Cartesian (w.r.t. D = rhat * d).  `ranges` = (tensor, [(lo, hi)]): only these SOURCE rows (and
    the edges leaving them) are written, the call returns its buffers (gxh, gvec, gx, None) for the complementary call.
    `finish=False` (gx = NULL in the C call): (gxh, per-relation partial sums of gvec WITHOUT the residual's identity term)."""
    if not finish:
        T = xh.size(0)
        scratch = gedge if ranges is None else torch.zeros_like(gedge)
        gxh, gv, _ = msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, scratch, xh_bias=xh_bias)
        part = None
        if gv is not None:
            ident = (torch.arange(graph.N) < int(graph.type_rowptr[T])).to(gv.dtype)
            part = torch.zeros((T,) + tuple(gv.shape), dtype=gv.dtype)
            part[0] = gv - gvec1 * ident[:, None, None]      # (the split over the relations is the kernel's own business)
        if ranges is None:
            return gxh, part
        # ranged launch without the finishing launch (the "proj" halo exchange): only these SOURCE rows are written
        sel = _rows_of_ranges(ranges[1], xh.size(1))
        if out is None:
            out = (torch.full_like(gxh, float("nan")), None if part is None else torch.full_like(part, float("nan")))
        out[0][:, sel] = gxh[:, sel]
        if part is not None:
            out[1][:, sel] = part[:, sel]
        esel = sel[graph.csr_src.long()]
        gedge[:, esel] = scratch[:, esel]
        return out
    with torch.enable_grad():
        xh_ = (xh + w.b2 if xh_bias else xh).detach().requires_grad_(True)
        x_ = torch.zeros(xh.size(1), H, dtype=xh.dtype).requires_grad_(True)
        v_ = vec.detach().requires_grad_(True) if vec is not None else None
        if edge.dim() == 3:          # per-layer handle of EdgeFanout: [H/64, E, 4] view of the same edge array
            edge = edge[0]
        D = (edge[:, :3] * edge[:, 3:4]).detach().requires_grad_(True)
        dn = D.norm(dim=-1)
        e_ = torch.cat([D / dn[:, None], dn[:, None]], 1)
        x1, vec1 = message_scatter_ref(xh_, v_, x_, e_, w.wt, w.brbf, graph, rbf)
        ins = [xh_, x_, D] + ([v_] if vec is not None else [])
        gr = torch.autograd.grad([x1, vec1], ins, [gx1, gvec1])
    gxh, gv, gx = gr[0], (gr[3] if vec is not None else None), gr[1]
    res = getattr(graph, "res_row", None)
    if res is not None:
        # kernel contract with virtual target rows: NO identity (residual) term in gx / gvec -- the host adds it
        T = xh.size(0)
        rk = (torch.arange(graph.N) < int(graph.type_rowptr[T])).to(xh.dtype)
        gx = gx - torch.zeros_like(gx).index_add_(0, res.long(), gx1 * rk[:, None] * (1 / math.sqrt(2.0)))
        if gv is not None:
            gv = gv - torch.zeros_like(gv).index_add_(0, res.long(), gvec1 * rk[:, None, None])
    if ranges is None:
        gedge.zero_()                    # (the caller may hand over uninitialised memory: the kernels write every slot)
        gedge[0, :, :3] = gr[2]          # all column blocks' contributions in slice 0, the others zero
        return gxh, gv, gx
    sel = _rows_of_ranges(ranges[1], xh.size(1))
    if out is None:
        nan = lambda t_: None if t_ is None else torch.full_like(t_, float("nan"))
        out = (nan(gxh), nan(gv), nan(gx), None)
    out[0][:, sel] = gxh[:, sel]
    if gv is not None:
        out[1][sel] = gv[sel]
    out[2][sel] = gx[sel]
    esel = sel[graph.csr_src.long()]                # the edges leaving the selected source rows
    gedge[:, esel] = 0
    gedge[0, esel, :3] = gr[2][esel]
    return out


# every kernel wrapper of hermnet_amd.nodeops that the fused layer calls on one device and has a restatement of its name here
NODEOPS = ("energy_head_fwd", "energy_head_bwd", "layernorm_fwd", "layernorm_bwd", "ssilu_fwd", "ssilu_bwd", "update_mid",
           "update_out", "update_out_bwd", "update_mid_bwd", "node_pre_fwd", "node_pre_bwd", "node_update_fwd", "node_update_bwd",
           "node_update_pre_fwd", "node_pre_fwd16", "node_pre_bwd16")


def install(put, extra=()):
    """Kernel wrappers -> their restatements: `put(object, name, value)` (monkeypatch.setattr, or setattr in a worker process)
    for NODEOPS and `extra` on hermnet_amd.nodeops, and for layer._msg_fwd / _msg_bwd."""
    import hermnet_amd.layer as lmod
    for fn in NODEOPS + tuple(extra):
        put(lmod.nodeops, fn, globals()[fn])
    put(lmod, "_msg_fwd", msg_fwd)
    put(lmod, "_msg_bwd", msg_bwd)


class RefEdgeGeometry(torch.autograd.Function):
    """Same contract as hermnet_amd.ops.EdgeGeometry: the incoming gradient is Cartesian (dE/dD)."""

    @staticmethod
    def forward(ctx, pos, cell, graph):
        ctx.graph = graph
        ctx.cell_shape = None if cell is None else tuple(cell.shape)
        return geometry_ref(pos.detach(), graph, None if cell is None else cell.detach())

    @staticmethod
    def backward(ctx, gedge):
        g = ctx.graph
        gp = torch.zeros(g.num_atoms, 3, dtype=gedge.dtype)
        gp.index_add_(0, g.src_id.long(), gedge[:, :3])
        gp.index_add_(0, g.tgt_id.long(), -gedge[:, :3])
        gcell = None
        if ctx.needs_input_grad[1] and g.shift is not None and ctx.cell_shape is not None:
            # D = ... + shift @ cell[batch[src]]  =>  dE/dcell[b] = sum_e shift_e (x) gD_e   (ops.EdgeGeometry)
            outer = g.shift.to(gedge.dtype)[:, :, None] * gedge[:, None, :3]
            nb = 1
            for v in ctx.cell_shape[:-2]:
                nb *= v
            b = g.batch32.long()[g.src_id.long()]
            gcell = torch.zeros(nb, 3, 3, dtype=gedge.dtype).index_add_(0, b, outer).reshape(ctx.cell_shape)
        return gp, gcell, None


# ---------------------------------------------------------------------------------------------
# The kernels of the TRAINING step (csrc/train_kernels.hip, train_node_kernels.hip, band_product.hip): the formulas of the
# kernels' header comments and of include/hermnet_hip.h, written out -- no autograd inside.  tests/test_train_reference.py
# checks each against float64 autograd of the torch expression to second order.  A cotangent that is None is zero.
# ---------------------------------------------------------------------------------------------
def _thirds(X):
    H = X.shape[-1] // 3
    return X[..., :H], X[..., H:2 * H], X[..., 2 * H:]


def _dot3(G, W):
    """sum_d G_d W_d over the Cartesian axis, in the kernels' order: G [E,3,H]; W [E,3] or [E,3,H]."""
    w = (lambda d: W[:, d, None]) if W.dim() == 2 else (lambda d: W[:, d])
    return G[:, 0] * w(0) + G[:, 1] * w(1) + G[:, 2] * w(2)


def _z(t, like):
    return torch.zeros_like(like) if t is None else t


def edge_message_fwd(X, R, V, U):
    """S = Xs Rs, M_d = (Xb Rb) U_d + V_d (Xa Ra)."""
    (xs, xa, xb), (rs, ra, rb) = _thirds(X), _thirds(R)
    M = (xb * rb)[:, None, :] * U[:, :, None]
    if V is not None:
        M = M + V * (xa * ra)[:, None, :]
    return xs * rs, M


def edge_message_bwd(GS, GM, X, R, V, U):
    """(GS, GM) -> gX, gR, gV (None with V), gU."""
    (xs, xa, xb), (rs, ra, rb) = _thirds(X), _thirds(R)
    gB = _dot3(GM, U)
    gXa = gRa = torch.zeros_like(xs)
    gV = None
    if V is not None:
        gA, A = _dot3(GM, V), xa * ra
        gXa, gRa, gV = gA * ra, gA * xa, GM * A[:, None, :]
    gX = torch.cat([GS * rs, gXa, gB * rb], 1)
    gR = torch.cat([GS * xs, gRa, gB * xb], 1)
    return gX, gR, gV, (GM * (xb * rb)[:, None, :]).sum(2)


def edge_message_bwd2(cX, cR, cV, cU, GS, GM, X, R, V, U):
    """Cotangents (cX, cR, cV, cU) of edge_message_bwd's outputs -> dGS, dGM, dX, dR, dV (None with V), dU."""
    (xs, xa, xb), (rs, ra, rb) = _thirds(X), _thirds(R)
    (cXs, cXa, cXb), (cRs, cRa, cRb) = _thirds(_z(cX, X)), _thirds(_z(cR, R))
    cU = _z(cU, U)
    tB, B = cXb * rb + cRb * xb, xb * rb
    gB, sU = _dot3(GM, U), _dot3(GM, cU)
    dGM = tB[:, None, :] * U[:, :, None] + B[:, None, :] * cU[:, :, None]
    dXa = dRa = torch.zeros_like(xs)
    dV = None
    if V is not None:
        cV = _z(cV, V)
        tA, A = cXa * ra + cRa * xa, xa * ra
        gA, sV = _dot3(GM, V), _dot3(GM, cV)
        dGM = dGM + (tA[:, None, :] * V + cV * A[:, None, :])
        dXa, dRa, dV = cRa * gA + ra * sV, cXa * gA + xa * sV, tA[:, None, :] * GM
    dX = torch.cat([cRs * GS, dXa, cRb * gB + rb * sU], 1)
    dR = torch.cat([cXs * GS, dRa, cXb * gB + xb * sU], 1)
    return cXs * rs + cRs * xs, dGM, dX, dR, dV, (GM * tB[:, None, :]).sum(2)


def _sum_rows(x, idx, n):
    return torch.zeros((n,) + tuple(x.shape[1:]), dtype=x.dtype).index_add_(0, idx, x)


def _r_of_edges(R, k):
    return R if k.r_rows is None else R.index_select(0, k.r_rows)


def _r_rows_out(gRe, R, k):
    """A per-edge gradient of R at the rows the edges read; rows no edge points to (padding) are zero."""
    if k.r_rows is None:
        return gRe
    return torch.zeros_like(R).index_copy_(0, k.r_rows, gRe)


def message_algebra_fwd(xh, vec, R, U, k):
    """trainops.MessageAlgebra: x_j = xh[k.xrow], vec_j = vec[k.src], R of edge e at row k.r_rows[e]; sums per target row."""
    V = None if vec is None else vec.index_select(0, k.src)
    S, M = edge_message_fwd(xh.index_select(0, k.xrow), _r_of_edges(R, k), V, U)
    return _sum_rows(S, k.tgt, k.n_tgt), _sum_rows(M, k.tgt, k.n_tgt)


def message_algebra_bwd(g_dx, g_dv, xh, vec, R, U, k):
    V = None if vec is None else vec.index_select(0, k.src)
    gX, gRe, gV, gU = edge_message_bwd(g_dx.index_select(0, k.tgt), g_dv.index_select(0, k.tgt), xh.index_select(0, k.xrow),
                                       _r_of_edges(R, k), V, U)
    return (_sum_rows(gX, k.xrow, xh.shape[0]), None if vec is None else _sum_rows(gV, k.src, vec.shape[0]),
            _r_rows_out(gRe, R, k), gU)


def message_algebra_bwd2(c_xh, cR, c_vec, cU, g_dx, g_dv, xh, vec, R, U, k):
    """-> (d g_dx, d g_dv, d xh, d vec (None with vec), dR, dU)."""
    sel = lambda t, i: None if t is None else t.index_select(0, i)
    V = sel(vec, k.src)
    dGS, dGM, dX, dRe, dV, dU = edge_message_bwd2(
        sel(c_xh, k.xrow), None if cR is None else _r_of_edges(cR, k), None if vec is None else sel(c_vec, k.src), cU,
        g_dx.index_select(0, k.tgt), g_dv.index_select(0, k.tgt), xh.index_select(0, k.xrow), _r_of_edges(R, k), V, U)
    return (_sum_rows(dGS, k.tgt, k.n_tgt), _sum_rows(dGM, k.tgt, k.n_tgt), _sum_rows(dX, k.xrow, xh.shape[0]),
            None if vec is None else _sum_rows(dV, k.src, vec.shape[0]), _r_rows_out(dRe, R, k), dU)


def segment_sum(x, idx, n_rows):
    """hermnet_segment_sum behind trainops.SumRows: out[r] = the sum of the rows k of x with idx[k] == r."""
    return _sum_rows(x, idx, n_rows)


def col_sum(g):
    """hermnet_col_sum behind trainops._col_sum_over_rows: [T,K,O] -> [T,O]."""
    return g.sum(1)


def edge_unit(order, D, gU=None, gd=None, C=None):
    """hermnet_edge_unit: U = D / d, d = max(|D|, 1e-6) and its two derivatives (csrc/train_kernels.hip's header):
    order 0 -> (U, d);  1 -> gD = (gU - U (U.gU)) / d + U gd;  2 -> (c_gU, c_gd, c_D) for the cotangent C of gD.
    On the floor d is a constant: no projection and no distance term."""
    n = torch.sqrt((D * D).sum(1))
    on = n <= 1.0e-6
    d = torch.where(on, torch.full_like(n, 1.0e-6), n)
    U = D / d[:, None]
    if order == 0:
        return U, d
    dot = lambda a, b: (a * b).sum(1)
    gU = _z(gU, D)
    gd = torch.where(on, torch.zeros_like(d), _z(gd, d))
    zero = torch.zeros_like(d)
    ug = torch.where(on, zero, dot(U, gU))
    if order == 1:
        return (gU - U * ug[:, None]) / d[:, None] + U * gd[:, None]
    uc = torch.where(on, zero, dot(U, C))
    pc, pg = C - U * uc[:, None], gU - U * ug[:, None]
    k = dot(gU, C) - uc * ug
    c_D = (gd[:, None] * pc - (k[:, None] * U + ug[:, None] * pc + uc[:, None] * pg) / d[:, None]) / d[:, None]
    return pc / d[:, None], uc, torch.where(on[:, None], torch.zeros_like(c_D), c_D)


def edge_unit_scale(order, D, gU=None, gd=None, C=None):
    """The same expressions with every term taken in magnitude (float64): the scale a cancelling gD / c_D is judged on."""
    D = D.double()
    U, d = edge_unit(0, D)
    a = lambda t: torch.zeros_like(D) if t is None else t.double().abs()
    one = lambda t: torch.zeros_like(d) if t is None else t.double().abs()
    Ua, inv = U.abs(), 1.0 / d
    dot = lambda p, q: (p * q).sum(1)
    off = (torch.sqrt((D * D).sum(1)) > 1.0e-6).double()          # on the floor c_gd and c_D are zero by definition
    if order == 1:
        return ((a(gU) + Ua * (off * dot(Ua, a(gU)))[:, None]) * inv[:, None] + Ua * (off * one(gd))[:, None]).amax(1)
    ug, uc = off * dot(Ua, a(gU)), off * dot(Ua, a(C))
    pc, pg = a(C) + Ua * uc[:, None], a(gU) + Ua * ug[:, None]
    k = dot(a(gU), a(C)) + uc * ug
    c_D = (one(gd)[:, None] * pc + (k[:, None] * Ua + ug[:, None] * pc + uc[:, None] * pg) * inv[:, None]) * inv[:, None]
    return (pc * inv[:, None]).amax(1), uc, c_D.amax(1) * off


def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def silu_bwd(gy, x):
    s = _sig(x)
    return gy * (s * (1.0 + x * (1.0 - s)))


def silu_bwd2(u, gy, x):
    """-> c_gy = u f'(x), c_x = u gy f''(x), f'' = s (1 - s) (2 + x (1 - 2 s))."""
    s = _sig(x)
    return u * (s * (1.0 + x * (1.0 - s))), u * gy * (s * (1.0 - s) * (2.0 + x * (1.0 - 2.0 * s)))


def _ln_row(x, eps):
    mu = x.mean(1, keepdim=True)
    y = x - mu
    r = 1.0 / torch.sqrt((y * y).mean(1, keepdim=True) + eps)
    return y * r, r


def ln_bwd(gy, x, eps):
    """gx = r (gy - mean(gy) - y mean(gy y))."""
    y, r = _ln_row(x, eps)
    m = lambda t: t.mean(1, keepdim=True)
    return (gy - m(gy) - y * m(gy * y)) * r


def ln_bwd2(v, gy, x, eps):
    """Cotangent v of gx -> c_gy = r (v - Vm - y Vy),  c_x = -r^2 [y P + b (v - Vm - y Vy) + Vy (gy - a - y b)]."""
    y, r = _ln_row(x, eps)
    m = lambda t: t.mean(1, keepdim=True)
    a, b, Vm, Vy = m(gy), m(gy * y), m(v), m(v * y)
    P = m(v * gy) - a * Vm - b * Vy
    t = v - Vm - y * Vy
    return t * r, (y * P + t * b + (gy - a - y * b) * Vy) * (-(r * r))


def mid_fwd(vp, xt, c0, c1):
    H = xt.shape[1]
    v1, v2 = vp[..., :H], vp[..., H:]
    return (v1 * v2).sum(1) * c0, torch.cat([xt, torch.sqrt((v2 * v2).sum(1) + c1)], 1)


def mid_bwd(g_vdot, g_xin, vp, c0, c1):
    H = g_vdot.shape[1]
    v1, v2 = vp[..., :H], vp[..., H:]
    ga, bn = (g_vdot * c0)[:, None, :], (g_xin[:, H:] / torch.sqrt((v2 * v2).sum(1) + c1))[:, None, :]
    return torch.cat([ga * v2, ga * v1 + bn * v2], 2), g_xin[:, :H].clone()


def mid_bwd2(u_vp, u_xt, g_vdot, g_xin, vp, c0, c1):
    """-> c_gvdot, c_gxin = (u_xt | S / n), c_vp = (c0 a u2 | c0 a u1 + b (u2 / n - v2 S / n^3))."""
    H = g_vdot.shape[1]
    v1, v2 = vp[..., :H], vp[..., H:]
    u_vp = _z(u_vp, vp)
    u1, u2 = u_vp[..., :H], u_vp[..., H:]
    ga, gb = (g_vdot * c0)[:, None, :], g_xin[:, H:]
    S = (u2 * v2).sum(1)
    rn = 1.0 / torch.sqrt((v2 * v2).sum(1) + c1)
    bn, bs = (gb * rn)[:, None, :], (gb * S * rn * rn * rn)[:, None, :]
    return ((u1 * v2 + u2 * v1).sum(1) * c0, torch.cat([_z(u_xt, g_vdot), S * rn], 1),
            torch.cat([ga * u2, ga * u1 + bn * u2 - bs * v2], 2))


def _m1(m, like):
    return torch.ones(like.shape[0], dtype=like.dtype) if m is None else m


def out_fwd(q, vdot, vp, xt, vt, m, c0):
    H = xt.shape[1]
    q1, q2, q3 = _thirds(q)
    mm = _m1(m, xt)
    return (xt + (q1 + q2 * vdot) * c0) * mm[:, None], (vt + q3[:, None, :] * vp[..., :H]) * mm[:, None, None]


def out_bwd(gx, gv, q, vdot, vp, m, c0, want_xt_vt=True):
    """-> g_q, g_vdot, g_vp = (m gv q3 | 0), g_xt = m gx, g_vt = m gv (the last two only on request: outputs nobody reads)."""
    H = gx.shape[1]
    q1, q2, q3 = _thirds(q)
    mm = _m1(m, gx)
    gx = gx * mm[:, None]
    gv = torch.zeros(gx.shape[0], 3, H, dtype=gx.dtype) if gv is None else gv * mm[:, None, None]
    g_q = torch.cat([gx * c0, gx * vdot * c0, (gv * vp[..., :H]).sum(1)], 1)
    first = (g_q, gx * q2 * c0, torch.cat([gv * q3[:, None, :], torch.zeros_like(gv)], 2))
    return first + (gx, gv) if want_xt_vt else first


def out_bwd2(c_gq, c_gvdot, c_gvp, c_gxt, c_gvt, gx, gv, q, vdot, vp, m, c0):
    """-> d_gx, d_gv, d_q = (0 | m gx c0 c_gvdot | m sum_d w1_d gv_d), d_vdot = m gx c0 k2, d_vp = (m gv k3 | 0)."""
    H = gx.shape[1]
    q1, q2, q3 = _thirds(q)
    mm = _m1(m, gx)
    k1, k2, k3 = _thirds(_z(c_gq, q))
    cvd, cxt = _z(c_gvdot, gx), _z(c_gxt, gx)
    z3 = torch.zeros(gx.shape[0], 3, H, dtype=gx.dtype)
    w1 = z3 if c_gvp is None else c_gvp[..., :H]
    cvt = z3 if c_gvt is None else c_gvt
    gx = gx * mm[:, None]
    gv = z3 if gv is None else gv * mm[:, None, None]
    v1 = vp[..., :H]
    d_gx = ((k1 + k2 * vdot + cvd * q2) * c0 + cxt) * mm[:, None]
    d_gv = (k3[:, None, :] * v1 + w1 * q3[:, None, :] + cvt) * mm[:, None, None]
    d_q = torch.cat([torch.zeros_like(gx), gx * cvd * c0, (w1 * gv).sum(1)], 1)
    return d_gx, d_gv, d_q, gx * k2 * c0, torch.cat([gv * k3[:, None, :], z3], 2)


def res_fwd(x, dx, v, dv, m, c0):
    mm = _m1(m, x)
    return (x + dx) * (mm * c0)[:, None], (dv if v is None else v + dv) * mm[:, None, None]


def mask_scale(g1, gv1, m, c0, rows, H):
    ref = g1 if g1 is not None else gv1
    mm = torch.ones(rows, dtype=ref.dtype) if m is None else m
    z1, z3 = torch.zeros(rows, H, dtype=ref.dtype), torch.zeros(rows, 3, H, dtype=ref.dtype)
    return _z(g1, z1) * (mm * c0)[:, None], _z(gv1, z3) * mm[:, None, None]


def band_product(A, B, bias):
    out = torch.bmm(A, B)
    return out if bias is None else out + bias[:, None, :]


def band_grad_a(g1, g2, B):
    return torch.bmm(g1 if g2 is None else g1 + g2, B.transpose(1, 2))


def band_grad_b(A, g1, g2):
    g = g1 if g2 is None else g1 + g2
    return torch.bmm(A.transpose(1, 2), g), g.sum(1)


def band_grads(A, B, g1, g2):
    """hermnet_band_product_grads: the three gradients from one pass over g1 (+ g2)."""
    return (band_grad_a(g1, g2, B),) + band_grad_b(A, g1, g2)
