"""Autograd wrappers around the C-ABI kernels (host side of the operator boundary,
SURVEY.md section 8(b)).  Tensors are allocated by PyTorch; the library only enqueues
kernels on the current stream.  CUDA(HIP) tensors only -- there is no CPU path.

The launch helper of the whole package lives here, beside the timer it serves: `_call(label, c_name, *args)` (this module,
`nodeops`, `trainops`); calls without a label take `_lib.call`."""
import ctypes
from types import SimpleNamespace

import torch

from . import _lib

P = _lib.ptr


class KernelTimer(object):
    """Optional per-launch timing with HIP events recorded on the launch stream (used by
    bench.py for the roofline figure).  Nothing is synchronised here; call `summary()` after
    the caller's own device synchronisation."""

    def __init__(self, prefix="message_scatter"):
        self.pairs = {}
        # only launches whose name starts with one of these are bracketed: an event pair costs ~15 us of host time
        self.prefix = (prefix,) if isinstance(prefix, str) else tuple(prefix)

    def launch(self, name, fn):
        if not name.startswith(self.prefix):
            return fn()
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        rc = fn()
        b.record()
        self.pairs.setdefault(name, []).append((a, b))
        return rc

    def summary(self):
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in self.pairs.items()}


_TIMER = None


def set_kernel_timer(timer):
    global _TIMER
    _TIMER = timer


def _launch(name, fn):
    return fn() if _TIMER is None else _TIMER.launch(name, fn)


def _stream():
    """hipStream_t of PyTorch's current stream as an integer (the raw getter: no Stream object per launch)."""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _call(label, c_name, *args):
    """One launch: the library's `c_name(*args, current stream)` under the timer label `label`; an error code raises.
    Without a timer installed the entry point is called directly: no closure per launch (profiles/train_refactor_ab.md)."""
    fn = getattr(_lib.load(), c_name)
    if _TIMER is None:
        rc = fn(*args, _stream())
    else:
        rc = _launch(label, lambda: fn(*args, _stream()))
    if rc != 0:
        _lib.check(rc, c_name)


def _require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError("hermnet_amd.%s: the hot path runs on MI355X only (got a %s tensor); "
                           "there is no CPU fallback" % (what, t.device))


class RbfDescriptor(object):
    """Host mirror of `hn_rbf_desc` (Gaussian basis * envelope, rmnet.py:156-193)."""

    def __init__(self, offset, rc, env_kind, env_p):
        self.offset = offset
        self.num_rbf = int(offset.numel())
        self.inv_rc = 1.0 / rc
        # GaussianSmearing: coeff = -0.5 / (offset[1] - offset[0]).item() ** 2
        self.coeff = None
        self.env_kind = env_kind
        self.env_p = env_p

    def struct(self):
        if self.coeff is None:
            o = self.offset.detach().float().cpu()
            self.coeff = -0.5 / float(o[1] - o[0]) ** 2
        return _lib.RbfDesc(self.offset.data_ptr(), self.num_rbf, self.inv_rc, self.coeff,
                            self.env_kind, self.env_p)


class AtomSink(object):
    """Per-evaluation request for per-atom outputs (`HVNet.forward` reads it from `data._hn_atom_props`; never stored on a
    cached graph).  `HVNet.forward` fills `energies` [N] (atom order, intensive models already divided by their graph's atom
    count); with `virials=True` the first position backward through `EdgeGeometry` fills `virials` [N,3,3] (atom order,
    W_i = -1/2 sum_{e touching i} D_e (x) dE/dD_e, include/hermnet_hip.h: hermnet_edge_geometry_bwd_virial).  Later backward
    passes through the same forward (the stress path's cell gradient) leave it as it is.
    `graph_virial=True` (stress.energy_forces_stress, the captured steps): the same backward also fills `graph_virial`
    [B,3,3] = the ordered per-graph sums of the W_i (hermnet_graph_virial); `energies=False` skips the per-atom energies."""

    def __init__(self, virials=True, graph_virial=False, energies=True):
        self.want_virials = bool(virials)
        self.want_graph_virial = bool(graph_virial)
        self.want_energies = bool(energies)
        self.energies = self.virials = self.graph_virial = None

    def reset(self):
        self.energies = self.virials = self.graph_virial = None
        return self


def graph_virial(vrows, graph):
    """[B,3,3] ordered per-graph sums of the per-atom virial rows `vrows` [rows,9] of `graph` (hermnet_graph_virial: two
    launches, no atomics, no host read)."""
    lib = _lib.load()
    B, n = int(graph.num_graphs), int(graph.num_atoms)
    if n == 0 or B == 0:
        return torch.zeros(B, 3, 3, dtype=torch.float32, device=vrows.device)
    out = torch.empty(B, 9, dtype=torch.float32, device=vrows.device)
    wbytes = lib.hermnet_graph_virial_workspace(n)
    work = torch.empty(wbytes, dtype=torch.uint8, device=vrows.device)
    _lib.call("hermnet_graph_virial", P(vrows), P(graph.row_of_node), P(graph.graph_perm), P(graph.batch32), n, B, P(work), wbytes,
              P(out), _stream())
    return out.view(B, 3, 3)


class EdgeGeometry(torch.autograd.Function):
    """`HVNet.with_edge` (hermnet.py:133-152) -> edge[E,4] = (rhat, d) in CSR order.  `sink` (optional `AtomSink`): the
    first backward also writes the per-atom virials into it."""

    @staticmethod
    def forward(ctx, pos, cell, graph, sink=None):
        _require_gpu(pos, "EdgeGeometry")
        pos_c = pos.detach().float().contiguous()
        edge = torch.empty(graph.E, 4, dtype=torch.float32, device=pos.device)
        cell_c = None
        if graph.shift is not None and cell is not None:
            cell_c = cell.detach().float().reshape(-1, 3, 3).contiguous()
        batch32 = graph.batch32
        _lib.call("hermnet_edge_geometry_fwd", P(pos_c), P(graph.src_id), P(graph.tgt_id),
                  P(graph.shift if cell_c is not None else None), P(cell_c), P(batch32), graph.E, P(edge), _stream())
        ctx.graph, ctx.sink = graph, sink
        ctx.keep = (pos_c, cell_c)
        ctx.cell_shape = None if cell is None else tuple(cell.shape)
        return edge

    @staticmethod
    def backward(ctx, gedge):
        graph = ctx.graph
        gD = gedge.float().contiguous()
        gpos_rows = torch.empty(graph.num_src or graph.N, 3, dtype=torch.float32, device=gD.device)
        if graph.num_src:
            # HTNet graph (virtual target rows): ordered segment sums, no atomics.  dE/dpos[i] = sum over the
            # edges leaving i of gD - sum over the edges entering i of gD.
            P_, B_, Te, TR = graph.triadic_pairs, graph.block, graph.T // graph.triadic_pairs, graph.T
            g3 = gD[:, :3].contiguous()
            rp_t, rp_s = graph.csr_rowptr.long(), graph.csc_rowptr.long()
            into = torch.segment_reduce(g3, "sum", lengths=rp_t[1:] - rp_t[:-1], unsafe=True)            # [Nt,3]
            outof = torch.segment_reduce(g3.index_select(0, graph.csc_pos.long()), "sum",
                                         lengths=rp_s[1:] - rp_s[:-1], unsafe=True)                      # [TR*Ns,3]
            gpos_rows = outof.view(TR, graph.num_src, 3).sum(0)
            gpos_rows[:Te * B_] -= into.view(Te, P_, B_, 3).sum(1).reshape(Te * B_, 3)
        elif ctx.sink is not None and ctx.sink.virials is None and ctx.sink.graph_virial is None:
            # virials wanted and not yet taken: the same position gradient (bit for bit) with W_i alongside
            pos_c, cell_c = ctx.keep
            csc = graph.out_rowptr is None
            vrows = torch.empty(graph.N, 9, dtype=torch.float32, device=gD.device)
            _lib.call("hermnet_edge_geometry_bwd_virial", P(gD), P(graph.csr_rowptr), P(graph.csc_rowptr if csc else None),
                      P(graph.csc_pos if csc else None), graph.T if csc else 0, P(None if csc else graph.out_rowptr),
                      P(None if csc else graph.out_edges), P(pos_c), P(graph.src_id), P(graph.tgt_id),
                      P(graph.shift if cell_c is not None else None), P(cell_c), P(graph.batch32), graph.N, P(gpos_rows),
                      P(vrows), _stream())
            if ctx.sink.want_virials:
                ctx.sink.virials = vrows.index_select(0, graph.row_of_node).view(-1, 3, 3)
            if ctx.sink.want_graph_virial:
                ctx.sink.graph_virial = graph_virial(vrows, graph)
        elif graph.out_rowptr is None:      # device-built graphs: out-edges from the CSC order (one sort fewer)
            _lib.call("hermnet_edge_geometry_bwd_csc", P(gD), P(graph.csr_rowptr), P(graph.csc_rowptr), P(graph.csc_pos),
                      graph.T, graph.N, P(gpos_rows), _stream())
        else:
            _lib.call("hermnet_edge_geometry_bwd", P(gD), P(graph.csr_rowptr), None, P(graph.out_rowptr), P(graph.out_edges),
                      graph.N, P(gpos_rows), _stream())
        gcell = None
        if ctx.needs_input_grad[1] and ctx.keep[1] is not None:
            # D = ... + shift @ cell[batch[src]]  =>  dE/dcell[b] = sum_{e in b} shift_e (x) gD_e
            # (what `virial_calc`, utils.py:153-155, differentiates for NPT runs)
            outer = graph.shift[:, :, None] * gD[:, None, :3]
            nb = ctx.keep[1].size(0)
            if nb == 1:
                gcell = outer.sum(0, keepdim=True)
            else:
                b = graph.batch32.long()[graph.src_id.long()]
                gcell = torch.zeros(nb, 3, 3, dtype=gD.dtype, device=gD.device).index_add_(0, b, outer)
            gcell = gcell.reshape(ctx.cell_shape)
        return gpos_rows.index_select(0, graph.row_of_node), gcell, None, None


class TrueEdgeGradient(torch.autograd.Function):
    """Identity on edge = (rhat, d) whose backward turns the TRUE gradient (dE/drhat, dE/dd), as produced
    by PyTorch autograd on the generic (optional radial basis) path, into the Cartesian dE/dD that
    `EdgeGeometry.backward` consumes:  gD = gd rhat + (gr - (gr.rhat) rhat) / d."""

    @staticmethod
    def forward(ctx, edge):
        ctx.save_for_backward(edge)
        return edge.clone()

    @staticmethod
    def backward(ctx, g):
        (edge,) = ctx.saved_tensors
        rh, d = edge[:, :3], edge[:, 3:4]
        gr, gd = g[:, :3], g[:, 3:4]
        gD = gd * rh + (gr - (gr * rh).sum(1, keepdim=True) * rh) / d
        return torch.cat([gD, torch.zeros_like(d)], dim=1)


def _msg_fwd(graph, rbf, H, xh, vec, x, w, edge, xh_bias=True, ranges=None, zero_unknown=True, out=None, range_rows=0):
    """`xh_bias=False`: xh already includes x_proj's bias (chain kernels).  `ranges` [T,2] int32 (device): only these
    target rows of every relation (atom shards: two launches over complementary ranges around the halo exchange;
    the second passes the first one's result as `out`); `range_rows`: how many rows they cover (host int)."""
    b2 = w.b2 if xh_bias else None
    if out is None:
        x1 = torch.empty(graph.N, H, dtype=x.dtype, device=x.device)          # target rows (= source rows unless HTNet)
        vec1 = torch.empty(graph.N, 3, H, dtype=x.dtype, device=x.device)
    else:
        x1, vec1 = out
    gs, rs = graph.as_struct(), rbf.struct()
    # (graph.fwd_taps: the step's per-edge tap records, or None -- the kernel then evaluates them itself; same bits)
    _call("message_scatter_fwd" + ("" if vec is not None else "_l0"), "hermnet_message_scatter_fwd_taps",
          ctypes.byref(gs), ctypes.byref(rs), H, P(xh), P(b2), P(vec), P(x), P(w.wt), P(w.brbf), P(edge),
          P(graph.fwd_taps), P(x1), P(vec1), P(ranges), 1 if zero_unknown else 0, int(range_rows))
    return x1, vec1


def _msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, gedge, xh_bias=True, ranges=None, out=None, finish=True):
    """`gedge` [H/64, E, 4] (zero-filled by the caller) receives the per-column-block Cartesian edge gradients.
    `ranges` = (device [k,2] int32, host list of (lo, hi)): only these SOURCE rows (atom shards: the halo rows first,
    the others while their gradients travel; the second call passes the first one's buffers as `out`).
    -> (gxh, gvec, gx), with `ranges` (gxh, gvec, gx, part): the buffers a second call takes as `out`.
    `finish=False` (only where `_bwd_sums_deferrable`): no finishing launch -- returns (gxh, per-relation partial sums of
    gvec [T,N,3,H] or None); the sums over the relations and the residual's identity terms are the consumer's."""
    b2 = w.b2 if xh_bias else None
    gvec = gx = None                   # (finish=False: the library leaves the finishing launch out when gx is NULL)
    if out is not None:
        gxh, gvec, gx, part = out if finish else (out[0], None, None, out[1])
    else:
        gxh = torch.empty_like(xh)
        if finish:
            gvec = None if vec is None else torch.empty_like(vec)
            gx = torch.empty(xh.size(1), H, dtype=gx1.dtype, device=gx1.device)   # source rows
        # per-relation partial sums of gvec: the result itself without the finishing launch, with it the workspace of the
        # channel-per-lane form
        part = None
        if vec is not None and (not finish or (graph.edge_table is not None and graph.T > 1)):
            part = torch.empty((graph.T,) + tuple(vec.shape), dtype=vec.dtype, device=vec.device)
    rd, rh, nr = None, None, 0
    if ranges is not None:
        rd, host = ranges
        nr = len(host)
        rh = (ctypes.c_int * (2 * nr))(*[v for lo_hi in host for v in lo_hi])
    gs, rs = graph.as_struct(), rbf.struct()
    _call("message_scatter_bwd" + ("" if vec is not None else "_l0"), "hermnet_message_scatter_bwd",
          ctypes.byref(gs), ctypes.byref(rs), H, P(xh), P(b2), P(vec), P(w.wt), P(w.brbf), P(edge), P(gx1), P(gvec1),
          P(gxh), P(gvec), P(gx), P(gedge), 0, P(graph.edge_table), P(part), P(rd), rh, nr)
    if not finish:
        return gxh, part
    if ranges is not None:
        return gxh, gvec, gx, part
    return gxh, gvec, gx


def _msg_bwd_gedge(graph, rbf, H, xh, w, edge, gx1, gvec1, gedge):
    """The message backward of a FIRST layer whose inputs carry no gradient (no vec rows; `_bwd_sums_deferrable`): only
    `gedge` is written -- no source-row sums, no gxh buffer."""
    gs, rs = graph.as_struct(), rbf.struct()
    _call("message_scatter_bwd_l0", "hermnet_message_scatter_bwd_gedge", ctypes.byref(gs), ctypes.byref(rs), H, P(xh),
          P(w.wt), P(w.brbf), P(edge), P(gx1), P(gvec1), P(gedge), P(graph.edge_table))


class MessageScatter(torch.autograd.Function):
    """rbf_proj + propagate + residual of one HeteroVertexConv layer, all relations
    (rmnet.py:24-26, 55-73; utils.py:11-24).  Returns (x1, vec1).

    The `edge` input carries (rhat, d); the gradient returned for it is the Cartesian
    gradient w.r.t. the edge vector D (what `EdgeGeometry.backward` consumes).
    First-order only: gradients w.r.t. rbf_proj weights are not produced (force path)."""

    @staticmethod
    def forward(ctx, xh, vec, x, edge, wt, brbf, graph, rbf):
        _require_gpu(x, "MessageScatter")
        H = x.size(1)
        xh = xh.contiguous()
        vec_c = None if vec is None else vec.contiguous()
        w = SimpleNamespace(wt=wt, brbf=brbf)        # (xh_bias=False: no b2)
        x1, vec1 = _msg_fwd(graph, rbf, H, xh, vec_c, x.contiguous(), w, edge, xh_bias=False)
        ctx.save_for_backward(xh, vec_c, edge, wt, brbf)
        ctx.graph, ctx.rbf, ctx.H = graph, rbf, H
        return x1, vec1

    @staticmethod
    def backward(ctx, gx1, gvec1):
        xh, vec, edge, wt, brbf = ctx.saved_tensors
        graph, rbf, H = ctx.graph, ctx.rbf, ctx.H
        gedge = torch.zeros(H // 64, graph.E, 4, dtype=torch.float32, device=gx1.device)
        gxh, gvec, gx = _msg_bwd(graph, rbf, H, xh, vec, SimpleNamespace(wt=wt, brbf=brbf), edge, gx1.contiguous(),
                                 gvec1.contiguous(), gedge, xh_bias=False)
        return gxh, gvec, gx, gedge.sum(0), None, None, None, None


def edge_radial_table(graph, rbf, edge):
    """[E+1,32] per-edge radial record (window start, 12 tap pairs, unit vector) in CSC order -- the order the
    channel-per-lane backward kernel walks --; ONE launch per step: geometry and radial basis are the same for every
    layer (`include/hermnet_hip.h`: hermnet_edge_radial_table)."""
    E = edge.size(0)
    table = torch.empty(E + 1, 32, dtype=torch.float32, device=edge.device)      # (+1: the stream reads one record ahead)
    gs, rs = graph.as_struct(), rbf.struct()
    _call("edge_radial_table", "hermnet_edge_radial_table", ctypes.byref(gs), ctypes.byref(rs), P(edge), P(table))
    return table


def edge_radial_tables(graph, rbf, edge):
    """`edge_radial_table` and, from the same launch, the forward's tap records [E,16] in CSR order (twelve raw taps, the
    envelope, the tile row of every edge: `include/hermnet_hip.h`: hermnet_edge_radial_tables), which the forward message
    kernel of every layer reads instead of evaluating them.  Returns (table, fwd_taps)."""
    E = edge.size(0)
    table = torch.empty(E + 1, 32, dtype=torch.float32, device=edge.device)
    taps = torch.empty(E, 16, dtype=torch.float32, device=edge.device)
    gs, rs = graph.as_struct(), rbf.struct()
    _call("edge_radial_table", "hermnet_edge_radial_tables", ctypes.byref(gs), ctypes.byref(rs), P(edge), P(table), P(taps))
    return table, taps
