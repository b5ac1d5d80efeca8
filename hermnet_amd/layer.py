"""One HeteroVertexConv layer (`HermNet/hermnet.py:37-65` + `rmnet.py:21-32`) as ONE autograd node with a hand-written
first-order backward.  `HeteroVertexConv.forward` picks between two Functions and decides the first one's `Route`:
  FusedRelationalLayer  the chain kernels (csrc/node_chain*.hip, widths up to 512), three launches each way: the node projection
                        of every relation (LayerNorm + x_proj), the message kernel, the update.  Projection and messages run
                        locally (`_local_*`) or, on an atom shard, around the exchange of the halo rows: "rows" (x | vec rows
                        travel, windowed node launches redo the halo tiles: `_halo_rows_*`) or "proj" (projected rows travel
                        forward, partial sums of gradients backward: `_halo_proj_*`).  `_update_fwd`: the fused layer boundaries.
  GemmRelationalLayer   switches.node_chain = False, and the only path for widths the chain kernels are not instantiated for:
                        the node-level linears through library GEMMs joined by the stage kernels (csrc/node_kernels.hip).
What the layers of one step hand to each other lives on that step's `StepState`.  Parameters are treated as constants
(energy/force evaluation; parameter gradients are not produced -- the training step runs through the differentiable
device-op path, `HVNet.forward` in train() mode).
"""
import torch

from . import _lib, nodeops, switches
from .ops import _launch, _msg_bwd, _msg_bwd_gedge, _msg_fwd
from .sharding import _all_to_all_rows_start, comm_wait


class LayerWeights(object):
    """Kernel-ready views of one HeteroVertexConv's parameters, rebuilt when they change.  Every copy is a declared field;
    a group that a width does not get is None in every field."""

    STATE = ("mods", "key", "builds", "_params", "h_real", "chain")
    # dense copies (transposed `t`, per-relation lists, stacked `_s`): the GEMM layer, the message kernels, tests/ref_ops.py
    DENSE = ("w1cat", "b1cat", "w1cat_t", "w2", "w2t", "b2", "wt", "brbf", "wv", "wvt", "wx0", "wx0t", "bx0", "wx2", "wx2t",
             "bx2", "wv_s", "wvt_s", "wx0_s", "wx0t_s", "bx0_s", "wx2_s", "wx2t_s", "bx2_s")
    # frag(W), frag(W^T) of the five weights (include/hermnet_hip.h): the 32/64-row and the wide chains (widths up to 512)
    FRAG = ("w1f", "w1tf", "w2f", "w2tf", "wvf", "wvtf", "wx0f", "wx0tf", "wx2f", "wx2tf")
    # frag16 of the same (width 128): the 16-row update, the last-layer forms, the boundary forms (the read-out: HeadWeights)
    FRAG16 = tuple(n + "16" for n in FRAG)
    __slots__ = STATE + DENSE + FRAG + FRAG16

    def __init__(self, mods):
        for n in self.__slots__:
            setattr(self, n, None)
        self.mods = list(mods)
        self.builds = 0               # how often the copies were (re)built (guard.ParamGuard stamps its fingerprints with it)
        # (owner module, name) of every parameter, collected once: walking `module.parameters()` on every
        # forward costs ~0.13 ms of host time per layer
        self._params = [(sub, name) for m in self.mods for sub in m.modules() for name in sub._parameters]

    @property
    def __dict__(self):
        """`vars(w)`: the declared fields by name (tests and tools move them to a device one by one)."""
        return {n: getattr(self, n) for n in self.__slots__}

    @staticmethod
    def _pad(w, dim, parts, H, Hp, scale=None):
        """Zero-pad `parts` consecutive blocks of H entries along `dim` to Hp entries each; `scale[k]` multiplies
        block k first."""
        if scale is not None:
            w = w.clone()
            for k, f in enumerate(scale):
                if f != 1.0:
                    w.narrow(dim, k * H, H).mul_(f)
        if Hp == H:
            return w
        shp = list(w.shape)
        shp[dim] = parts * Hp
        out = w.new_zeros(shp)
        for k in range(parts):
            out.narrow(dim, k * Hp, H).copy_(w.narrow(dim, k * H, H))
        return out

    @torch.no_grad()
    def refresh(self):
        """Widths that are not a multiple of 64 (the reference accepts any, hermnet.py:84-88): every channel axis is
        zero-padded to Hp = next multiple of 64, the column-block width of the message kernels.  Padded channels are
        exactly zero everywhere (zero weight rows/columns and biases; LayerNorm statistics over the real H,
        `h_real`), and the kernels' 1/sqrt(Hp) factors are turned back into 1/sqrt(H) by scaling the weights that
        feed them linearly by s = sqrt(Hp/H): the `a` and `b` thirds of x_proj[2] (message, rmnet.py:63-66) and the
        middle third of xvec_proj[2] (the factor of `vdot`, rmnet.py:97,104)."""
        key = _version_key(self._params)
        if key == self.key:
            return self
        ml = [m.message_layer for m in self.mods]
        ul = [m.update_layer for m in self.mods]
        H = ml[0].x_proj[0].weight.size(0)
        Hp = (H + 63) // 64 * 64
        s = (Hp / H) ** 0.5
        self.h_real = H if Hp != H else 0
        pad = lambda w, dim, parts, scale=None: self._pad(w, dim, parts, H, Hp, scale)
        st = lambda lst: torch.stack(lst, 0).contiguous()
        sab = None if Hp == H else (1.0, s, s)
        sq = None if Hp == H else (1.0, s, 1.0)
        # LayerNorm affine folded into the first Linear: (n*g + b) W1^T + b1 = n (W1*g)^T + (W1 b + b1)
        w1 = [pad(pad(m.x_proj[0].weight * m.x_layernorm.weight[None, :], 0, 1), 1, 1) for m in ml]
        b1 = [pad(m.x_proj[0].weight @ m.x_layernorm.bias + m.x_proj[0].bias, 0, 1) for m in ml]
        self.w1cat = torch.cat(w1, 0).contiguous()                                  # [T*H, H]
        self.b1cat = torch.cat(b1, 0).contiguous()                                  # [T*H]
        self.w1cat_t = self.w1cat.t().contiguous()                                  # [H, T*H]
        self.w2 = st([pad(pad(m.x_proj[2].weight, 0, 3, sab), 1, 1) for m in ml])   # [T, 3H, H]
        self.w2t = self.w2.transpose(1, 2).contiguous()                             # [T, H, 3H]
        self.b2 = torch.stack([pad(m.x_proj[2].bias, 0, 3, sab) for m in ml], 0)[:, None, :].contiguous()     # [T,1,3H]
        self.wt = st([pad(m.rbf_proj.weight.t(), 1, 3) for m in ml])                # [T, R, 3H]
        self.brbf = st([pad(m.rbf_proj.bias, 0, 3) for m in ml])                    # [T, 3H]
        # the update's three weights: per relation, transposed, and stacked for the uniform-block layout (one batched GEMM
        # per stage): wv [2H, H], wx0 [H, 2H], wx2 [3H, H]
        for name, ws in (("wv", [pad(pad(u.vec_proj.weight, 0, 2), 1, 1) for u in ul]),
                         ("wx0", [pad(pad(u.xvec_proj[0].weight, 0, 1), 1, 2) for u in ul]),
                         ("wx2", [pad(pad(u.xvec_proj[2].weight, 0, 3, sq), 1, 1) for u in ul])):
            ws = [w.contiguous() for w in ws]
            wts = [w.t().contiguous() for w in ws]
            for n, v in ((name, ws), (name + "t", wts), (name + "_s", st(ws)), (name + "t_s", st(wts))):
                setattr(self, n, v)
        self.bx0 = [pad(u.xvec_proj[0].bias, 0, 1) for u in ul]
        self.bx2 = [pad(u.xvec_proj[2].bias, 0, 3, sq) for u in ul]
        self.bx0_s, self.bx2_s = st(self.bx0)[:, None, :].contiguous(), st(self.bx2)[:, None, :].contiguous()
        # MFMA-operand-order copies of the five weights [T, out, in] and their transposes for the chain kernels
        self.chain = nodeops.chain_supported(Hp)
        if self.chain:
            w1s = self.w1cat.view(len(ml), Hp, Hp)
            five = (("w1", w1s, w1s.transpose(1, 2).contiguous()), ("w2", self.w2, self.w2t), ("wv", self.wv_s, self.wvt_s),
                    ("wx0", self.wx0_s, self.wx0t_s), ("wx2", self.wx2_s, self.wx2t_s))
            # (frag16: the 16-row kernels of csrc/node_chain16.hip exist at width 128 only)
            for sfx, fr in (("", nodeops.weight_fragments), ("16", nodeops.weight_fragments16))[:2 if Hp == 128 else 1]:
                for name, w, wt in five:
                    setattr(self, name + "f" + sfx, fr(w))
                    setattr(self, name + "tf" + sfx, fr(wt))
        self.key = key
        self.builds += 1
        return self


def _version_key(params):
    """Identity + version of the CURRENT parameter objects behind `params` = [(owner module, name)] (a replaced Parameter or
    an in-place update both change the key); data_ptr covers `.to(device)` / `.data = ...`."""
    key = []
    for sub, name in params:
        p = sub._parameters[name]
        if p is not None:               # e.g. vec_proj has bias=False
            key.append((id(p), p._version, p.data_ptr()))
    return tuple(key)


class HeadWeights(object):
    """The same for `out_energy` (EnergyHead): the copies the read-out kernels of this width read, owned by the model they
    were built from -- no other model can drop or evict them."""

    # w0 [C, H], b0 [C], w2v [C], b2 [1]: every form; w0t [H, C]: the fused form (nodeops.head_fused_supported);
    # w0f16, w0tf16 = frag16(w0), frag16(w0^T): the matrix-pipe form (nodeops.head16_supported, csrc/node_chain16.hip)
    __slots__ = ("lin0", "lin2", "key", "builds", "w0", "b0", "w2v", "b2", "w0t", "w0f16", "w0tf16")

    def __init__(self, out_energy=None):
        """`out_energy`: the model's nn.Sequential (`refresh`); None: copies of loose tensors, for one call (`build`)."""
        for n in self.__slots__:
            setattr(self, n, None)
        if out_energy is not None:
            self.lin0, self.lin2 = out_energy[0], out_energy[2]
        self.builds = 0

    @torch.no_grad()
    def refresh(self):
        key = _version_key([(m, n) for m in (self.lin0, self.lin2) for n in ("weight", "bias")])
        if key != self.key:
            self.build(self.lin0.weight.detach(), self.lin0.bias.detach(), self.lin2.weight.detach(), self.lin2.bias.detach())
            self.key = key
            self.builds += 1
        return self

    def build(self, w0, b0, w2, b2):
        """The copies of these four tensors; of (w0t | w0f16, w0tf16) what the read-out kernel of this width takes."""
        H, C = w0.size(1), w0.size(0)
        self.w0, self.b0, self.w2v, self.b2 = w0.contiguous(), b0, w2.reshape(-1).contiguous(), b2
        if nodeops.head16_supported(H, C):
            self.w0f16, self.w0tf16 = nodeops.weight_fragments16(self.w0), nodeops.weight_fragments16(self.w0.t().contiguous())
        elif nodeops.head_fused_supported(H, C):
            self.w0t = self.w0.t().contiguous()
        return self


class SpeciesTable(object):
    """Layer 0's node projection of every species, owned by the model beside its LayerWeights.  In an energy / force
    evaluation x of the first layer is the embedding gather (hermnet.py:123), so xh of a row depends on its species only:
    `table` [T, V, 3H] = xh of the V embedding rows, made by the `hermnet_node_pre_fwd` instance the per-atom launch of this
    width takes (same kernel family, tile height and width: a row's result does not depend on its tile's other rows, so the
    bits are the per-atom launch's), and `nodeops.species_expand` writes xh [T, N, 3H] from it.  Rebuilt when the embedding or
    layer 0's copies were; never inside a captured graph (`refresh` leaves `table` None there: the per-atom launch runs)."""

    __slots__ = ("embed", "key", "builds", "table")

    def __init__(self, embed):
        self.embed, self.key, self.builds, self.table = embed, None, 0, None

    @torch.no_grad()
    def refresh(self, w0):
        """Current for the embedding's weight and the build `w0.builds` of layer 0's LayerWeights -> self."""
        key = _version_key([(self.embed, "weight")]) + ((id(w0), w0.builds),)
        if key == self.key:
            return self
        emb = self.embed.weight.detach()
        self.table = None
        if not (w0.chain and emb.is_cuda and emb.dtype == torch.float32) or torch.cuda.is_current_stream_capturing():
            return self                 # (no key: a later refresh outside the capture builds it)
        Hp = w0.b2.size(-1) // 3
        if Hp != emb.size(1):           # (padded widths: the channels _prepare pads x with)
            emb = torch.nn.functional.pad(emb, (0, Hp - emb.size(1)))
        self.table = nodeops.species_table(emb.contiguous(), w0, len(w0.mods))
        self.key = key
        self.builds += 1
        return self


def _bwd_sums_deferrable(graph, H):
    """The message backward can leave its finishing launch to the consumer (hermnet_message_scatter_bwd with gx = NULL):
    channel-per-lane form, targets = sources (HVNet rows), 32-bit offsets.  Width 128 only: there the update backward
    keeps two or three workgroups per CU and forms the sums half a wave per row (measured, same job: 2.98 vs 3.01 ms at
    configs[1], 27.2 vs 27.6 ms at 100k atoms); the wide kernels (one workgroup per CU) lose more in their prologue than
    the two launches cost (H = 512: 22.5 vs 20.8 ms), so they keep the launches."""
    return (H == 128 and graph.edge_table is not None and not graph.num_src and graph.res_row is None
            and _lib.get_option("bwd_lanes16") == 0
            and graph.N * 3 * H * 4 < 2 ** 32 and switches.defer_sums())


def _virtual_residual(graph, gx1, gvec1, gx_in, gvec_in, H, ranges=None):
    """HTNet: the residual (rmnet.py:24-26) reads the atom's own row from each of its P virtual target rows; its gradient
    returns as the sum over those rows (the message backward adds no identity term with virtual targets).  `ranges`
    (device [k,2], host list): only these source rows (the ranged launches of the halo overlap)."""
    if not graph.num_src:
        return
    P_, B_, Te = graph.triadic_pairs, graph.block, graph.T // graph.triadic_pairs
    if gx_in.is_cuda and gvec_in is not None:
        nodeops.pair_sum_accumulate(gx1, gvec1, gx_in, gvec_in, Te, P_, B_, 0.5 ** 0.5, 1.0, ranges=ranges)
        return
    sel = slice(0, Te * B_)
    if ranges is not None:
        sel = torch.zeros(Te * B_, dtype=torch.bool)
        for lo, hi in ranges[1]:
            sel[lo:min(hi, Te * B_)] = True
    gx_in[:Te * B_][sel] += (gx1.view(Te, P_, B_, H).sum(1).reshape(Te * B_, H) * (0.5 ** 0.5))[sel]
    if gvec_in is not None:
        gvec_in[:Te * B_][sel] += gvec1.view(Te, P_, B_, 3, H).sum(1).reshape(Te * B_, 3, H)[sel]


class EdgeGradSink(object):
    """One buffer [layers, H/64, E, 4] for the edge gradients of a whole step: every layer's backward kernel
    writes its slice, and `EdgeFanout.backward` reduces all slices in ONE pass (instead of a zero-fill, a
    block sum and an autograd accumulation per layer)."""

    def __init__(self, layers, nblk, E, device, zero=True):
        """`zero=False`: every edge has a target of a known element, so every slot is written by the kernels and the
        69 MB (config 2) zero-fill can be skipped."""
        self.shape = (layers, nblk, E, 4)
        self.device = device
        self.zero = zero
        self.buf = None

    def slice(self, li):
        if self.buf is None:     # edges to targets of an unknown element are never written: zero once if there are any
            alloc = torch.zeros if self.zero else torch.empty
            self.buf = alloc(self.shape, dtype=torch.float32, device=self.device)
            if not self.zero and switches.debug_poison():
                self.buf.fill_(float("nan"))         # (tests: a slot the kernels did not write would poison the forces)
        return self.buf[li]


class EdgeFanout(torch.autograd.Function):
    """edge [E,4] -> one handle per layer, an [H/64, E, 4] stride-0 view of it (so that a layer can return its
    per-column-block gradient slices unreduced); backward = sum over every slice of every layer."""

    @staticmethod
    def forward(ctx, edge, sink):
        ctx.sink = sink
        L, nblk = sink.shape[0], sink.shape[1]
        return tuple(edge.unsqueeze(0).expand(nblk, *edge.shape) for _ in range(L))

    @staticmethod
    def backward(ctx, *grads):
        sink = ctx.sink
        buf, ctx.sink.buf = sink.buf, None            # the buffer belongs to this backward pass only
        if buf is not None and all(g is not None and g.data_ptr() == buf[i].data_ptr() for i, g in enumerate(grads)):
            L, nblk, E, _ = sink.shape
            return buf.view(L * nblk, E, 4).sum(0), None
        live = [g.sum(0) for g in grads if g is not None]     # partial graphs: plain accumulation
        return (torch.stack(live, 0).sum(0) if live else None), None


class StepState(object):
    """The context of ONE evaluation (`data._hn_step`): what `HVNet._prepare` leaves for the layers and what the layers hand to
    each other, indexed by layer.  Every forward creates its own, so no other step or model sees it; undeclared fields raise."""

    __slots__ = ("graph", "edge", "rbf", "edge_embed", "train", "fused", "whole", "weights", "head", "edge_sink",
                 "edge_handles", "layer", "last", "halo", "chain_node", "pending", "pre_next", "species")

    def __init__(self, graph=None, edge=None, rbf=None, edge_embed=None, train=False, fused=False, whole=True, weights=None,
                 head=None):
        self.graph = graph              # _prepare: relation-ordered graph of this neighbour list; every layer, the read-out
        self.edge = edge                # _prepare: edge geometry [E,4] = (rhat, d); layers that got no handle
        self.rbf = rbf                  # _prepare: the radial basis' descriptor for the kernels (None: materialised); layers
        self.edge_embed = edge_embed    # _prepare: the materialised basis of the optional bases / train(), else None; layers
        self.train = train              # _prepare: the differentiable device-op path; the read-out
        self.fused = fused              # _prepare: the basis is evaluated inside the kernels; the loop's `last`, the read-out
        self.whole = whole              # _prepare: no shard, or a lone world-1 plan (the unsharded forms); the loop, Route
        self.weights = weights          # _prepare: the list from `_refresh_weights` or None; layers; dropped behind the loop
        self.head = head                # _prepare: the model's HeadWeights, current, where EnergyHead runs; the read-out takes it
        self.edge_sink = None           # _prepare: EdgeGradSink of this step, where the edge gradients are wanted; backwards
        self.edge_handles = None        # _prepare: one handle per layer from `EdgeFanout`; layers; dropped behind the loop
        self.layer = 0                  # _run_layers: index of the layer that is running its forward; that layer
        self.last = False               # _run_layers: this layer may run short (the read-out takes its x only); that layer
        self.halo = None                # _run_layers: the exchange still due for the next layer; that layer takes it
        self.chain_node = None          # a chain layer: the autograd node of its outputs; the layer above takes it
        self.pending = {}               # consuming layer -> nodeops.PendingGrads, from one layer's backward to the next one's
        self.pre_next = {}              # layer -> (x, its node projection), left by the fused update launch of the layer below
        self.species = None             # _prepare: (the model's SpeciesTable.table, the x it gathered from the embedding); layer 0's Route


class Route(object):
    """How one layer runs on the chain kernels, decided once by `HeteroVertexConv.forward`.
    `exchange`, `halo` (atom shards; `sharding.HaloOverlap`): the exchange of the halo rows of (x, vec) is still due and runs
    inside the layer, in its "rows" or its "proj" form; None: nothing to exchange.
    `defer`: x and vec are the outputs of the chain layer below and of nothing else, so the backward may hand its input
    gradients down as partial sums (`_hand_down`) -- two small launches per layer boundary less, same bits.
    `pre`: the node projection of THIS x, already computed by the fused update launch of the layer below.
    `w_next`: the NEXT layer's weights, where its projection of the rows this layer produces may run inside this layer's
    update launch; `boundary`: switches.boundary_mode, read once (`_update_fwd`).
    `last`: the caller reads x_out only (HVNet's last layer in front of the read-out, energy / force evaluation): the layer
    returns (x_out, None) and its update launches leave out everything that only vec_out and its zero gradient need, where
    `nodeops.last_update_supported`; `first`: the first layer's message backward may skip the source rows' sums
    (switches.dead_ends, read once).
    `species`: (table [T, V, 3H], z_rows) where x is the embedding gather of an evaluation (the first layer, unsharded): the node
    projection is `nodeops.species_expand` of the model's `SpeciesTable` -- no hb / mean / rstd, nothing below takes a gradient;
    the layer drops it where somebody does want x's gradient."""

    def __init__(self, exchange=None, halo=None, defer=False, pre=None, w_next=None, last=False, species=None):
        self.exchange, self.halo, self.defer, self.pre, self.w_next = exchange, halo, defer, pre, w_next
        self.species = species if exchange is None and pre is None else None
        self.boundary = int(switches.boundary_mode)
        self.first = bool(switches.dead_ends)
        self.last = bool(last and switches.dead_ends and exchange is None and w_next is None)


def _local_fwd(x, vec, edge, graph, rbf, w, route):
    if route.pre is not None:
        pre = route.pre
    elif route.species is not None:     # xh from the per-species table; the saved tensors of a backward nobody runs: none
        pre = (None, nodeops.species_expand(route.species[0], route.species[1], x.size(0)), None, None)
    else:
        pre = nodeops.node_pre_fwd(x, w, graph.T, src_ranges=graph.src_ranges)
    x1, vec1 = _msg_fwd(graph, rbf, x.size(1), pre[1], vec, x, w, edge, xh_bias=False)
    return pre, x1, vec1


def _halo_rows_fwd(x, vec, edge, graph, rbf, w, route):
    """The exchange runs behind the node projection AND the message kernel of every target that reads no halo row (SURVEY
    8(e): "run interior edges while the halo is in flight"):
      pack -> start the all-to-all -> project every row (halo rows from stale inputs: redone below) -> messages into the
      early targets -> the STREAM waits -> unpack IN PLACE -> project the tiles that hold a halo row -> messages into the
      remaining targets."""
    halo, plan, H = route.halo, route.halo.plan, x.size(1)
    send = nodeops.halo_rows(0, x, vec, plan.send_idx)
    recv, work = _all_to_all_rows_start(send, plan.send_counts, plan.recv_counts, plan.group)
    if switches.debug_poison():     # (tests: nothing that runs before the unpack may depend on a halo row)
        nodeops.halo_rows(2, x, vec, plan.recv_idx, torch.full_like(recv, float("nan")))
    pre = nodeops.node_pre_fwd(x, w, graph.T, src_ranges=graph.src_ranges)
    out = _msg_fwd(graph, rbf, H, pre[1], vec, x, w, edge, xh_bias=False, ranges=halo.fwd_early, zero_unknown=True,
                   range_rows=halo.early_rows)
    comm_wait(work, "fwd", sum(plan.send_counts), sum(plan.recv_counts))
    if plan.recv_idx.numel() > 0:   # (a rank without halo atoms has nothing to redo)
        nodeops.halo_rows(2, x, vec, plan.recv_idx, recv)
        nodeops.node_pre_fwd(x, w, graph.T, src_ranges=graph.src_ranges, windows=halo.windows, mode=1, out=pre)
    if halo.late_rows > 0:
        _msg_fwd(graph, rbf, H, pre[1], vec, x, w, edge, xh_bias=False, ranges=halo.fwd_late, zero_unknown=False, out=out,
                 range_rows=halo.late_rows)
    return pre, out[0], out[1]


def _halo_proj_fwd(x, vec, edge, graph, rbf, w, route):
    """The halo rows travel as what the message kernel gathers -- xh[t] of every relation and vec, 12H floats per atom -- so
    no node kernel runs a second time on the halo tiles:
      project every row (halo rows from stale inputs: replaced below) -> pack (xh | vec) of the rows the peers need -> start
      the all-to-all -> messages into the targets that read no halo row -> the STREAM waits -> unpack IN PLACE -> messages
      into the remaining targets."""
    halo, plan, H = route.halo, route.halo.plan, x.size(1)
    pre = nodeops.node_pre_fwd(x, w, graph.T, src_ranges=graph.src_ranges)
    xh = pre[1]
    send = nodeops.halo_proj_rows(0, xh, vec, plan.send_idx)
    recv, work = _all_to_all_rows_start(send, plan.send_counts, plan.recv_counts, plan.group)
    if switches.debug_poison():     # (tests: nothing that runs before the unpack may depend on a halo row)
        nodeops.halo_proj_rows(2, xh, vec, plan.recv_idx, torch.full_like(recv, float("nan")))
    out = _msg_fwd(graph, rbf, H, xh, vec, x, w, edge, xh_bias=False, ranges=halo.fwd_early, zero_unknown=True,
                   range_rows=halo.early_rows)
    comm_wait(work, "fwd", sum(plan.send_counts), sum(plan.recv_counts))
    nodeops.halo_proj_rows(2, xh, vec, plan.recv_idx, recv)
    if halo.late_rows > 0:
        _msg_fwd(graph, rbf, H, xh, vec, x, w, edge, xh_bias=False, ranges=halo.fwd_late, zero_unknown=False, out=out,
                 range_rows=halo.late_rows)
    return pre, out[0], out[1]


def _update_fwd(x1, vec1, graph, w, step, li, route):
    """The update launch -> (x_out, vec_out, vp, h2b, q23, nrm).
    `switches.boundary_mode` -- how the node launches of a layer boundary are cut, where `nodeops.fused_boundary_supported`
    (width 128, 16-row update tiles, HVNet rows: csrc/node_chain16.hip):
      0 (default)  every phase a launch of its own: 64-row projection kernels + 16-row update kernels, the input gradients handed
                   down as partial sums (the round-4 form);
      4            the BACKWARD boundary as one launch: the projection's backward of layer l + 1 runs inside the update backward
                   of layer l (sums over the relations in registers, LayerNorm backward on the tile: no [T, N, H] partial sums in
                   memory);
      1            both boundaries as one launch each (the next layer's projection inside the update launch as well);
      3            only the forward boundary;
      2            the 16-row phases of mode 1 as launches of their own (the bit-for-bit check of the fused kernels).
    Measured in the model (configs[1], one box, three interleaved rounds).  With fp32 MFMAs (profiles/r05_boundary_ab.log):
    0: 2.944, 4: 2.945, 3: 2.971, 1: 2.988 ms per step.  Since the products run as bf16 splits (profiles/r05_boundary_ab_split.log):
    0: 2.80, 4: 2.82, 3: 2.87, 1: 2.89 -- with the matrix pipe 2.7 x cheaper a tile's time is its weight stream, and a 64-row
    projection tile streams a quarter of the bytes per row of a 16-row one: the fused forms lose what that gains.
    The forward boundary (1, 2, 3) leaves the next layer's projection in `step.pre_next`; the backward one: `_pre_bwd_parts`."""
    w_next = route.w_next
    if w_next is None or route.boundary not in (1, 2, 3) or not nodeops.fused_boundary_supported(graph, x1.size(1), w, w_next):
        return nodeops.node_update_fwd(x1, vec1, w, graph)
    if route.boundary != 2:
        x_out, vec_out, vp, h2b, q23, nrm, pre_next = nodeops.node_update_pre_fwd(x1, vec1, w, graph, w_next)
    else:
        x_out, vec_out, vp, h2b, q23, nrm = nodeops.node_update_fwd(x1, vec1, w, graph)
        pre_next = nodeops.node_pre_fwd16(x_out, w_next, graph.T)
    step.pre_next[li + 1] = (x_out, pre_next)
    return x_out, vec_out, vp, h2b, q23, nrm


def _edge_grad_slot(edge, graph, step, li, H, device):
    """Where the message backward writes the edge gradients [H/64, E, 4]: with a handle from `EdgeFanout`, the sink's slice."""
    if edge.dim() == 3 and step.edge_sink is not None:
        return step.edge_sink.slice(li)
    return torch.zeros(H // 64, graph.E, 4, dtype=torch.float32, device=device)


def _edge_grad(edge, gedge):
    """The gradient returned for `edge`: a handle from `EdgeFanout` gets the slices unreduced."""
    return gedge if edge.dim() == 3 else (gedge[0] if gedge.size(0) == 1 else gedge.sum(0))


def _hand_down(step, li, x, vec, gn_parts, gv_parts, mean, rstd, gx1, gvec1, w, chain=None):
    """The input gradients of layer `li` go down as partial sums: registered as `nodeops.PendingGrads` for the update backward
    of the layer below, which forms them in its own launch -> the (gx, gvec) buffers it will fill."""
    gx_total, gvec_in = torch.empty_like(x), torch.empty_like(vec)
    if switches.debug_poison():                # (tests: nothing reads them before that)
        gx_total.fill_(float("nan"))
        gvec_in.fill_(float("nan"))
    pend = step.pending[li - 1] = nodeops.PendingGrads(
        gx_total, gvec_in, gn_parts, gv_parts, x, mean, rstd, gx1, gvec1, w.h_real, chain=chain)
    pend.w_above = w            # (keeps the fragment copies alive; the CPU restatement of the tests reads it)
    return gx_total, gvec_in


def _pre_bwd_parts(ctx, gxh, hb, x, mean, rstd):
    """The projection's backward up to its per-relation partial sums -> (gn_parts, chain).  Boundary modes 1, 4: it runs inside
    the update backward of the layer below (`chain`, no launch here); 2: the same 16-row phase as a launch of its own."""
    graph, w = ctx.graph, ctx.w
    if ctx.route.boundary in (1, 2, 4) and nodeops.fused_boundary_supported(graph, x.size(1), w):
        if ctx.route.boundary != 2:
            return None, (gxh, hb, w.w2tf16, w.w1tf16)
        return nodeops.node_pre_bwd16(gxh, hb, w), None
    return nodeops.node_pre_bwd(gxh, hb, x, mean, rstd, w, src_ranges=graph.src_ranges, parts_only=True), None


def _local_bwd(ctx, x, mean, rstd, hb, xh, vec, edge, gx1, gvec1, gedge):
    graph, rbf, w, H = ctx.graph, ctx.rbf, ctx.w, x.size(1)
    if _bwd_sums_deferrable(graph, H):
        if ctx.route.defer and ctx.needs_input_grad[0]:
            gxh, gv_parts = _msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, gedge, xh_bias=False, finish=False)
            gn_parts, chain = _pre_bwd_parts(ctx, gxh, hb, x, mean, rstd)
            return _hand_down(ctx.step, ctx.li, x, vec, gn_parts, gv_parts, mean, rstd, gx1, gvec1, w, chain)
        if vec is None and not ctx.needs_input_grad[0]:     # the first layer: nothing below wants gx / gvec
            if ctx.route.first and x.is_cuda:               # ... nor the sums they would be formed from: gedge only
                _msg_bwd_gedge(graph, rbf, H, xh, w, edge, gx1, gvec1, gedge)
            else:
                _msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, gedge, xh_bias=False, finish=False)
            return None, None
    gxh, gvec_in, gx_in = _msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, gedge, xh_bias=False)
    _virtual_residual(graph, gx1, gvec1, gx_in, gvec_in, H)
    want_gx = ctx.needs_input_grad[0]
    return (nodeops.node_pre_bwd(gxh, hb, x, mean, rstd, w, add=gx_in, src_ranges=graph.src_ranges) if want_gx else None), gvec_in


def _halo_rows_bwd(ctx, x, mean, rstd, hb, xh, vec, edge, gx1, gvec1, gedge):
    """The gradients of the halo rows first: they travel to their owners while the other rows are computed."""
    graph, rbf, w, halo, plan, H = ctx.graph, ctx.rbf, ctx.w, ctx.route.halo, ctx.route.halo.plan, x.size(1)
    bufs = None
    if halo.bwd_first[1]:
        bufs = _msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, gedge, xh_bias=False, ranges=halo.bwd_first)
        gxh, gvec_in, gx_in, _ = bufs
        _virtual_residual(graph, gx1, gvec1, gx_in, gvec_in, H, halo.bwd_first)
        out = nodeops.node_pre_bwd(gxh, hb, x, mean, rstd, w, add=gx_in, src_ranges=graph.src_ranges,
                                   windows=halo.windows, mode=1)
        gsend = nodeops.halo_rows(1, out[0], gvec_in, plan.recv_idx)           # pack and clear: none stays here
    else:                                                                   # (a rank without halo atoms)
        out, gsend = None, x.new_empty(0, 4 * H)
    back, work = _all_to_all_rows_start(gsend, plan.recv_counts, plan.send_counts, plan.group)
    if halo.bwd_rest[1]:
        bufs = _msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, gedge, xh_bias=False, ranges=halo.bwd_rest, out=bufs)
        _virtual_residual(graph, gx1, gvec1, bufs[2], bufs[1], H, halo.bwd_rest)
    gxh, gvec_in, gx_in, _ = bufs
    gx_total = nodeops.node_pre_bwd(gxh, hb, x, mean, rstd, w, add=gx_in, src_ranges=graph.src_ranges,
                                    windows=halo.windows, mode=2, out=out)[0]
    comm_wait(work, "bwd", sum(plan.recv_counts), sum(plan.send_counts))
    nodeops.halo_accumulate(gx_total, gvec_in, plan, back)                  # gradients of my atoms used elsewhere
    return gx_total, gvec_in


def _halo_proj_bwd(ctx, x, mean, rstd, hb, xh, vec, edge, gx1, gvec1, gedge):
    """The gradients of the halo SOURCE rows first, as they stand behind the message backward -- gxh[t] of every relation and
    the per-relation partial sums of gvec, summed while they are packed; cleared here: the local halo rows were overwritten
    in the forward --; they travel to their owners while the other source rows are computed; the owners add them to their own
    gxh / partial sums in list order, and ONE node_pre_bwd over every row follows.  The input gradients go down as partial
    sums (`_hand_down`): no finishing launch, no windowed node launch, no LayerNorm backward."""
    graph, rbf, w, halo, plan, H = ctx.graph, ctx.rbf, ctx.w, ctx.route.halo, ctx.route.halo.plan, x.size(1)
    gxh = torch.empty_like(xh)
    gv_parts = torch.empty((graph.T,) + tuple(vec.shape), dtype=vec.dtype, device=vec.device)
    bufs = (gxh, gv_parts)
    if halo.bwd_first_rows[1]:
        _msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, gedge, xh_bias=False, ranges=halo.bwd_first_rows, out=bufs,
                 finish=False)
    gsend = nodeops.halo_proj_rows(1, gxh, gv_parts, plan.recv_idx)           # pack and clear: none stays here
    back, work = _all_to_all_rows_start(gsend, plan.recv_counts, plan.send_counts, plan.group)
    if halo.bwd_rest_rows[1]:
        _msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, gedge, xh_bias=False, ranges=halo.bwd_rest_rows, out=bufs,
                 finish=False)
    comm_wait(work, "bwd", sum(plan.recv_counts), sum(plan.send_counts))
    nodeops.halo_proj_accumulate(gxh, gv_parts, plan, back)                 # gradients of my atoms used elsewhere
    gn_parts = nodeops.node_pre_bwd(gxh, hb, x, mean, rstd, w, src_ranges=graph.src_ranges, parts_only=True)
    return _hand_down(ctx.step, ctx.li, x, vec, gn_parts, gv_parts, mean, rstd, gx1, gvec1, w)


_ROUTES = {None: (_local_fwd, _local_bwd), "rows": (_halo_rows_fwd, _halo_rows_bwd), "proj": (_halo_proj_fwd, _halo_proj_bwd)}


class FusedRelationalLayer(torch.autograd.Function):
    """(x, vec, edge) -> (x_out, vec_out) for one layer on the chain kernels, relation (row) order."""

    @staticmethod
    def forward(ctx, x, vec, edge, graph, rbf, w, step, route):
        """`edge`: [E,4], or this layer's handle from `EdgeFanout` ([H/64,E,4] stride-0 view; same memory).
        x / vec live in SOURCE rows, the outputs in TARGET rows; the two coincide for HVNet and differ for HTNet
        (`graph.num_src`: one target row per atom and pair relation, relations.build_triadic)."""
        x = x.contiguous()
        vec = None if vec is None else vec.contiguous()
        # (the proj form hands its input gradients down as partial sums: where the layer below cannot take them and somebody
        # wants them -- known only here --, the exchange takes the rows form)
        ctx.exchange = "rows" if (route.exchange == "proj" and not _bwd_sums_deferrable(graph, x.size(1))
                                  and (ctx.needs_input_grad[0] or ctx.needs_input_grad[2])) else route.exchange
        if route.species is not None and (ctx.needs_input_grad[0] or vec is not None or not x.is_cuda):
            route.species = None        # (x's gradient wanted -- known only here: the per-atom launch, which saves hb / mean / rstd)
        (hb, xh, mean, rstd), x1, vec1 = _ROUTES[ctx.exchange][0](x, vec, edge, graph, rbf, w, route)
        # (the last layer in front of a read-out of x: no vec output, and no zero gradient for it on the way back)
        # (the short forms are kernels of the device library only)
        ctx.short = route.last and x.is_cuda and ctx.exchange is None and nodeops.last_update_supported(graph, x.size(1), w)
        if ctx.short:
            x_out, vp, h2b, q23, nrm = nodeops.node_update_fwd_last(x1, vec1, w, graph)
            vec_out = None
        else:
            x_out, vec_out, vp, h2b, q23, nrm = _update_fwd(x1, vec1, graph, w, step, step.layer, route)
        ctx.save_for_backward(x, mean, rstd, hb, xh, vec, edge, vp, h2b, q23, nrm)
        ctx.graph, ctx.rbf, ctx.w, ctx.step, ctx.li, ctx.route = graph, rbf, w, step, step.layer, route
        return x_out, vec_out

    @staticmethod
    def backward(ctx, gxo, gvo):
        x, mean, rstd, hb, xh, vec, edge, vp, h2b, q23, nrm = ctx.saved_tensors
        pend = ctx.step.pending.pop(ctx.li, None)
        if ctx.short:
            if pend is not None:
                raise RuntimeError("hermnet_amd: gradients handed down to the last layer")
            gx1, gvec1 = nodeops.node_update_bwd_last(gxo.contiguous(), vp, h2b, q23, nrm, ctx.w, ctx.graph)
        else:
            gxo, gvo = gxo.contiguous(), gvo.contiguous()
            # (the layer above may have left its finishing launches to this one: the buffers arrive unfilled -- and they must
            # be the very buffers it registered: a copy made on the way would hold garbage, so that is refused loudly)
            if pend is not None and (pend.gx.data_ptr() != gxo.data_ptr() or pend.gvec.data_ptr() != gvo.data_ptr()):
                raise RuntimeError("hermnet_amd: the gradients handed down as partial sums (layer %d) did not arrive in the "
                                   "buffers they were registered with; set the environment variable named in "
                                   "hermnet_amd/switches.py: defer_sums to 0" % (ctx.li + 1))
            # (partial sums, 16-row tiles at width 128: gvo stays unwritten -- the kernel keeps what it forms of it on chip; a
            # form of the device library only)
            held = (pend is not None and pend.chain is None and switches.pending_on_chip and gxo.is_cuda
                    and nodeops.held_update_supported(ctx.graph, gxo.size(1), ctx.w))
            update_bwd = nodeops.node_update_bwd_held if held else nodeops.node_update_bwd
            gx1, gvec1 = update_bwd(gxo, gvo, vp, h2b, q23, nrm, ctx.w, ctx.graph, pending=pend)
        gedge = _edge_grad_slot(edge, ctx.graph, ctx.step, ctx.li, x.size(1), gx1.device)
        gx, gvec = _ROUTES[ctx.exchange][1](ctx, x, mean, rstd, hb, xh, vec, edge, gx1, gvec1, gedge)
        return (gx, gvec, _edge_grad(edge, gedge)) + (None,) * 5


def _relation_gemms(graph, a, w_s, w_t, out, bias=None, acc=False):
    """out[rows of t] = a[rows of t] @ W_t for every relation t, under `_launch("gemm", ...)`: ONE batched product over the
    stacked weights `w_s` where every relation owns `graph.block` rows (graph.uniform), else one product per non-empty
    relation with `w_t[t]`.  Operands [rows, 3, K] count as three rows each.  `bias`: added by the per-relation products
    only -- a bias that would be broadcast over a batched GEMM's rows is added by the consuming kernel on load instead
    (baddbmm with a broadcast bias first copies it over the whole output).  `acc`: the products are added to `out`."""
    rp = graph.type_rowptr_host
    nk, T, K, M = rp[-1], graph.T, a.size(-1), out.size(-1)
    if graph.uniform and nk > 0:
        av, ov = a[:nk].view(T, -1, K), out[:nk].view(T, -1, M)
        _launch("gemm", (lambda: torch.baddbmm(ov, av, w_s, out=ov)) if acc else (lambda: torch.bmm(av, w_s, out=ov)))
        return
    for t in range(T):
        lo, hi = rp[t], rp[t + 1]
        if hi > lo:
            av, ov = a[lo:hi].view(-1, K), out[lo:hi].view(-1, M)
            if acc:
                _launch("gemm", lambda: torch.addmm(ov, av, w_t[t], out=ov))
            elif bias is not None:
                _launch("gemm", lambda: torch.addmm(bias[t], av, w_t[t], out=ov))
            else:
                _launch("gemm", lambda: torch.mm(av, w_t[t], out=ov))


class GemmRelationalLayer(torch.autograd.Function):
    """The same layer with its node-level linears as library GEMMs joined by the stage kernels (csrc/node_kernels.hip):
    switches.node_chain = False, and every width the chain kernels are not instantiated for.  No exchange runs in here."""

    @staticmethod
    def forward(ctx, x, vec, edge, graph, rbf, w, step):
        Ns, H = x.shape
        N, T, B = graph.N, graph.T, graph.block
        nk = graph.type_rowptr_host[-1]
        uni = graph.uniform and nk > 0
        x = x.contiguous()
        vec = None if vec is None else vec.contiguous()
        # --- node projection of every relation: xh[t] = x_proj_t(LayerNorm_t(x))  (rmnet.py:52)
        n, mean, rstd = nodeops.layernorm_fwd(x, 1e-5, h_real=w.h_real)
        h = _launch("gemm", lambda: torch.addmm(w.b1cat, n, w.w1cat.t()))                                     # [Ns, T*H]
        a = nodeops.ssilu_fwd(h)
        xh = _launch("gemm", lambda: torch.bmm(a.view(Ns, T, H).transpose(0, 1), w.w2t))                      # [T, Ns, 3H], + b2 on load
        # --- fused edge part + residual (rmnet.py:55-73, 24-26)
        x1, vec1 = _msg_fwd(graph, rbf, H, xh, vec, x, w, edge)
        # --- PaiNNUpdate on the rows of each relation (rmnet.py:94-107)
        vp = torch.empty(N, 3, 2 * H, dtype=x.dtype, device=x.device)
        h2 = torch.empty(N, H, dtype=x.dtype, device=x.device)
        q = torch.empty(N, 3 * H, dtype=x.dtype, device=x.device)
        _relation_gemms(graph, vec1, w.wvt_s, w.wvt, vp)
        vdot, xin = nodeops.update_mid(vp, x1, nk, H)
        _relation_gemms(graph, xin, w.wx0t_s, w.wx0t, h2, bias=w.bx0)
        kb = dict(bias=w.bx0_s, rows_per_bias=B) if uni else {}
        a2 = nodeops.ssilu_fwd(h2[:nk], **kb) if nk > 0 else h2[:0]
        _relation_gemms(graph, a2, w.wx2t_s, w.wx2t, q, bias=w.bx2)
        qb = dict(qbias=w.bx2_s, rows_per_bias=B) if uni else {}
        x_out, vec_out = nodeops.update_out(q, vdot, vp, x1, vec1, graph.row_active, N, nk, H, **qb)
        ctx.save_for_backward(x, mean, rstd, h, xh, vec, edge, vp, vdot, xin, h2, q)
        ctx.graph, ctx.rbf, ctx.w, ctx.step, ctx.li, ctx.kb, ctx.qb = graph, rbf, w, step, step.layer, kb, qb
        return x_out, vec_out

    @staticmethod
    def backward(ctx, gxo, gvo):
        x, mean, rstd, h, xh, vec, edge, vp, vdot, xin, h2, q = ctx.saved_tensors
        graph, rbf, w, kb, qb = ctx.graph, ctx.rbf, ctx.w, ctx.kb, ctx.qb
        Ns, H = x.shape
        N, T, nk = graph.N, graph.T, graph.type_rowptr_host[-1]
        gq, gvdot, gvp, gx1, gvec1 = nodeops.update_out_bwd(gxo.contiguous(), gvo.contiguous(), q, vdot, vp, graph.row_active,
                                                            N, nk, H, **qb)
        gxin = torch.empty(N, 2 * H, dtype=x.dtype, device=x.device)
        ga2 = torch.empty(N, H, dtype=x.dtype, device=x.device)
        _relation_gemms(graph, gq, w.wx2_s, w.wx2, ga2)
        gh2 = nodeops.ssilu_bwd(ga2, h2, nk, 1, H, H, H, **kb) if nk > 0 else ga2[:0]
        _relation_gemms(graph, gh2, w.wx0_s, w.wx0, gxin)
        nodeops.update_mid_bwd(gvdot, gxin, vp, xin, gvp, gx1, nk, H)
        _relation_gemms(graph, gvp, w.wv_s, w.wv, gvec1, acc=True)
        gedge = _edge_grad_slot(edge, graph, ctx.step, ctx.li, H, gx1.device)
        gxh, gvec_in, gx_in = _msg_bwd(graph, rbf, H, xh, vec, w, edge, gx1, gvec1, gedge, xh_bias=True)
        _virtual_residual(graph, gx1, gvec1, gx_in, gvec_in, H)
        gx_total = None
        if ctx.needs_input_grad[0]:
            ga = _launch("gemm", lambda: torch.bmm(gxh, w.w2))                                                # [T, Ns, H]
            gh = nodeops.ssilu_bwd(ga, h, Ns, T, H, H, Ns * H)                   # [Ns, T*H]
            gn = _launch("gemm", lambda: torch.mm(gh, w.w1cat))                                               # [N, H]
            gx_total = nodeops.layernorm_bwd(gn, x, mean, rstd, add=gx_in, h_real=w.h_real)
        return (gx_total, gvec_in, _edge_grad(edge, gedge)) + (None,) * 4


class EnergyHead(torch.autograd.Function):
    """`out_energy` (hermnet.py:113-117,129) on relation-ordered rows: Linear (library GEMM, bias in the epilogue),
    then ScaledSiLU + the H/2 -> 1 Linear in one kernel; one autograd node with a hand-written backward.
    Parameters are constants here (eval() mode; train() mode runs the nn.Sequential)."""

    @staticmethod
    def forward(ctx, x, w0, b0, w2, b2, mask=None, head=None):
        """`mask` [N] (optional) multiplies the per-row energies: padding rows of the relation order -> 0.
        `head`: the model's HeadWeights of these four tensors (HVNet); without it the copies are built for this call."""
        hw = head if head is not None else HeadWeights().build(w0, b0, w2, b2)
        ctx.mask = mask
        ctx.mfma = x.is_cuda and hw.w0f16 is not None
        ctx.fused = ctx.mfma or (x.is_cuda and hw.w0t is not None)
        if ctx.mfma:       # the H -> C product on the matrix pipe (csrc/node_chain16.hip), one launch each way
            h, e = nodeops.energy_head16_fwd(x, hw.w0f16, hw.b0, hw.w2v, hw.b2, mask)
            ctx.save_for_backward(h, hw.w0tf16, hw.w2v)
            ctx.H = x.size(1)
            return e
        if ctx.fused:      # one launch each way, no library GEMM (csrc/node_kernels.hip: energy_head_fused_kernel)
            h, e = nodeops.energy_head_fused_fwd(x, hw.w0t, hw.b0, hw.w2v, hw.b2, mask)
        else:
            h = _launch("gemm", lambda: torch.addmm(hw.b0, x, hw.w0.t()))             # [N, H/2]
            e = nodeops.energy_head_fwd(h, hw.w2v, hw.b2, mask)                       # [N]
        ctx.save_for_backward(h, hw.w0, hw.w2v)
        return e

    @staticmethod
    def backward(ctx, ge):
        h, w0, w2v = ctx.saved_tensors
        if ctx.mfma:
            gx = nodeops.energy_head16_bwd(ge.contiguous(), h, w0, w2v, ctx.H, ctx.mask)
        elif ctx.fused:
            gx = nodeops.energy_head_fused_bwd(ge.contiguous(), h, w0, w2v, ctx.mask)
        else:
            gh = nodeops.energy_head_bwd(ge.contiguous(), h, w2v, ctx.mask)
            gx = _launch("gemm", lambda: torch.mm(gh, w0))
        return (gx,) + (None,) * 6
