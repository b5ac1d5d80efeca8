"""GPU: the update chain kernels of the 16-row tiles (csrc/node_chain16.hip) that keep tile rows on chip.

  backward  node_update_bwd16_kernel<128, false, false>: gradients that arrive as partial sums (hn_pending_grads, gn_parts
            form) are formed in registers and handed to the elementwise pass there; gv[d] waits in LDS tiles for the last three
            products, for pending sums and for a gvec_out loaded from memory alike.  hermnet_node_update_bwd still fills
            gx_out / gvec_out; hermnet_node_update_bwd_held leaves gvec_out alone.
  forward   node_update_fwd16_kernel<128, false, false>: vec1 stays in its LDS tiles and v1 in a wave-private park for the
            residual vec_out = vec1 + r v1.

The backward's reference is NOT the pending kernel: gx_out / gvec_out come from the library's finishing launches
(message_bwd_finish_kernel behind hermnet_message_scatter_bwd, layernorm_bwd_parts_kernel behind hermnet_node_pre_bwd: what
HERMNET_DEFER_SUMS=0 runs), fed to hermnet_node_update_bwd without `pending`; everything is compared bit for bit (int32 views:
the signs of zeros count).  The forward's reference is the float64 restatement (tests/ref_ops.py) under the row rule of
helpers.judge_rows, floor 2e-6, for the 16-row kernel and for the 32-row base kernel of node_chain.hip beside it.

Row layouts (H = 128, T = 3): 333 atoms of random species including an unknown element; relation blocks of 17, 16 and 1 rows
plus 5 rows of an unknown element (a ragged last tile, an exactly full one, a one-row tile, the zero tiles behind
type_rowptr[T]); an empty relation; a row_active with zeros inside tiles and one whole inactive tile; uniform equal blocks
with inert padding rows.  Operands: unit normal, plus a LayerNorm row of 1e3 + noise, a row at 1e-20 and a constant row.
Every output buffer and both handed-down buffers start as NaN."""
import copy
import ctypes
import math

import pytest
import torch

from hermnet_amd import _lib, nodeops, ops, switches
from hermnet_amd.ops import RbfDescriptor, edge_radial_tables, _stream
from hermnet_amd.relations import RelationalGraph
from helpers import Golden, judge_rows, row_err
import ref_ops

pytestmark = pytest.mark.gpu
P = _lib.ptr
H, T, R, RC = 128, 3, 128, 5.0
Z_LIST = [13, 28, 29]
LAYOUTS = ["n333", "ragged", "empty", "inactive", "uniform"]
FWD_FLOOR = 2e-6
BAD_ARG = 1
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _species(kind, gen):
    if kind == "n333":
        return torch.tensor(Z_LIST + [1])[torch.randint(0, T + 1, (333,), generator=gen)]
    counts, unknown = {"ragged": ((17, 16, 1), 5), "empty": ((20, 0, 9), 0), "inactive": ((40, 20, 7), 2),
                       "uniform": ((20, 13, 9), 3)}[kind]
    z = torch.cat([torch.full((c,), Z_LIST[t]) for t, c in enumerate(counts)] + [torch.full((unknown,), 1)])
    return z[torch.randperm(z.numel(), generator=gen)]


def _layout(kind, dev):
    """-> (device graph, its CPU mirror for the restatements).  In-degrees 0 .. 8, edges in random order."""
    if kind not in _CACHE:
        gen = torch.Generator().manual_seed(LAYOUTS.index(kind) + 40)
        z = _species(kind, gen)
        n = z.numel()
        ei = torch.stack([torch.randint(0, n, (4 * n,), generator=gen), torch.randint(0, n, (4 * n,), generator=gen)])
        g = RelationalGraph.build(z.to(dev), ei.to(dev), Z_LIST, uniform={"uniform": True, "n333": None}.get(kind, False))
        rp = list(g.type_rowptr_host)
        if kind == "ragged":
            assert [rp[t + 1] - rp[t] for t in range(T)] == [17, 16, 1] and g.N - rp[T] == 5 and not g.uniform
        if kind == "empty":
            assert rp[1] == rp[2]
        if kind == "inactive":        # zeros inside the first and the last tile of relation 0, its middle tile entirely off
            g.row_active[[3, 35, 41]] = 0.0
            g.row_active[16:32] = 0.0
        if kind == "uniform":
            assert g.uniform and g.block == 20 and int((g.row_active[:rp[T]] == 0).sum()) >= 18
        gc = copy.copy(g)
        gc.row_active = g.row_active.cpu()
        _CACHE[kind] = (g, gc)
    return _CACHE[kind]


def _weights(dev):
    """LayerWeights of three randomly initialised PaiNNModules -> (CPU, for the restatements; the same on the device)."""
    if "w" not in _CACHE:
        from hermnet_amd.layer import LayerWeights
        from hermnet_amd.rmnet import PaiNNModule
        torch.manual_seed(7)
        mods = [PaiNNModule(hidden_channels=H, num_rbf=16) for _ in range(T)]
        for m in mods:
            for p in m.parameters():
                p.data.normal_(0, 0.3)
        w = LayerWeights(mods).refresh()
        w.h_real = 0
        wd = copy.copy(w)
        for k, v in vars(w).items():
            if torch.is_tensor(v):
                setattr(wd, k, v.to(dev))
        _CACHE["w"] = (w, wd)
    return _CACHE["w"]


def _rowptr(graph):
    vals = list(graph.type_rowptr_host)
    return (ctypes.c_int * len(vals))(*vals)


def _hostile_rows(t, gen):
    """Rows 2, 9 and 20 of a unit-normal [N, ...] operand: 1e3 + noise, 1e-20 x noise, a constant."""
    t[2] = 1.0e3 + torch.randn(t[2].shape, generator=gen)
    t[9] = 1.0e-20 * torch.randn(t[9].shape, generator=gen)
    t[20] = 0.37
    return t


# ---- forward --------------------------------------------------------------------------------------------------------------------
def _update_fwd(graph, wd, x1, vec1, tile):
    N, dev = graph.N, x1.device
    o = dict(vp=_nan(dev, N, 3, 2 * H), h2b=_nan(dev, N, H), q23=_nan(dev, N, 2 * H), nrm=_nan(dev, N, H), xo=_nan(dev, N, H),
             vo=_nan(dev, N, 3, H))
    ws = (wd.wvf16, wd.wx0f16, wd.wx2f16) if tile == 16 else (wd.wvf, wd.wx0f, wd.wx2f)
    rc = _lib.load().hermnet_node_update_fwd(P(x1), P(vec1), P(ws[0]), P(ws[1]), P(wd.bx0_s), P(ws[2]), P(wd.bx2_s),
                                             P(graph.row_active), P(graph.type_rowptr), _rowptr(graph), P(o["vp"]), P(o["h2b"]),
                                             P(o["q23"]), P(o["nrm"]), P(o["xo"]), P(o["vo"]), N, graph.T, H, tile, _stream())
    assert rc == 0
    return o


def _fwd_inputs(graph, seed):
    gen = torch.Generator().manual_seed(seed)
    return _hostile_rows(torch.randn(graph.N, H, generator=gen), gen), _hostile_rows(torch.randn(graph.N, 3, H, generator=gen), gen)


@pytest.mark.parametrize("kind", LAYOUTS)
def test_update_forward_with_rows_on_chip_against_fp64(kind):
    """hermnet_node_update_fwd at tile_rows = 16 (vec1 / v1 of the residual from LDS) and at tile_rows = 0 (the 32-row base
    kernel, which re-reads them from memory), each against the float64 restatement: x_out, vec_out on every row (rows of an
    unknown element and inactive rows exactly zero), vp, h2b, q23, nrm on the active rows of known elements."""
    dev = _dev()
    g, gc = _layout(kind, dev)
    w, wd = _weights(dev)
    x1, vec1 = _fwd_inputs(g, 51)
    r64, r32 = ref_ops.node_update_fwd(x1.double(), vec1.double(), w, gc), ref_ops.node_update_fwd(x1, vec1, w, gc)
    nk = g.type_rowptr_host[T]
    live = gc.row_active[:nk] != 0
    outs = {tile: _update_fwd(g, wd, x1.to(dev), vec1.to(dev), tile) for tile in (16, 0)}
    for tile, o in outs.items():
        for k, name in enumerate(("xo", "vo", "vp", "h2b", "q23", "nrm")):
            got, a, b = o[name], r64[k], r32[k]
            if k >= 2:          # saved tensors: defined where the backward reads them
                got, a, b = got[:nk][live.to(dev)], a[:nk][live], b[:nk][live]
            share, worst = judge_rows(got, a, b, FWD_FLOOR, "update_fwd tile %d %s %s" % (tile, kind, name))
            print("update_fwd %-8s tile %2d %-3s worst err/bound %.3f  deciding share %.3f" % (kind, tile, name, worst, share))
    for name in ("xo", "vo"):
        print("update_fwd %-8s %-3s tile 16 against tile 0: worst row err %.2e"
              % (kind, name, float(row_err(outs[16][name], outs[0][name]).max())))
        dead = torch.ones(g.N, dtype=torch.bool)
        dead[:nk] = ~live
        if bool(dead.any()):
            assert float(outs[16][name][dead.to(dev)].abs().max()) == 0.0


# ---- backward -------------------------------------------------------------------------------------------------------------------
def _case(kind, dev):
    """One layer boundary on this layout: the layer above's message backward and projection backward run twice -- leaving
    partial sums, and with their finishing launches -- over the same operands; the update backward below them on saved tensors
    of a real forward.  Computed once per layout, never modified."""
    key = ("bwd", kind)
    if key in _CACHE:
        return _CACHE[key]
    g, gc = _layout(kind, dev)
    w, wd = _weights(dev)
    N = g.N
    gen = torch.Generator().manual_seed(60 + LAYOUTS.index(kind))
    rnd = lambda *s: torch.randn(*s, generator=gen)
    lib = _lib.load()
    # the layer above: its LayerNorm input x, saved pre-activations, vec rows, message weights, edges, and the results of its own
    # update backward (gx1a, gvec1a: the residual's identity terms)
    x = _hostile_rows(rnd(N, H), gen).to(dev)
    mean = x.double().mean(1).float()
    rstd = (1.0 / (x.double().var(1, unbiased=False) + 1e-5).sqrt()).float()
    hb, xh, vec = rnd(T, N, H).to(dev), rnd(T, N, 3 * H).to(dev), rnd(N, 3, H).to(dev)
    wt, brbf = (rnd(T, R, 3 * H) / math.sqrt(R)).contiguous().to(dev), (0.1 * rnd(T, 3 * H)).contiguous().to(dev)
    gx1a, gvec1a = _hostile_rows(rnd(N, H), gen).to(dev), _hostile_rows(rnd(N, 3, H), gen).to(dev)
    rhat = torch.nn.functional.normalize(rnd(g.E, 3), dim=1)
    edge = torch.cat([rhat, (RC * (0.02 + 0.97 * torch.rand(g.E, generator=gen)))[:, None]], 1).float().contiguous().to(dev)
    rbf = RbfDescriptor(torch.linspace(0, 1, R, device=dev), RC, 0, 5)
    table, _ = edge_radial_tables(g, rbf, edge)
    gs, rs = g.as_struct(), rbf.struct()

    def message_bwd(finish):
        gxh, part = _nan(dev, T, N, 3 * H), _nan(dev, T, N, 3, H)
        gvec, gx = (_nan(dev, N, 3, H), _nan(dev, N, H)) if finish else (None, None)
        gedge = torch.zeros(H // 64, g.E, 4, device=dev)
        assert lib.hermnet_message_scatter_bwd(ctypes.byref(gs), ctypes.byref(rs), H, P(xh), None, P(vec), P(wt), P(brbf), P(edge),
                                               P(gx1a), P(gvec1a), P(gxh), P(gvec), P(gx), P(gedge), 0, P(table), P(part), None,
                                               None, 0, _stream()) == 0
        return gxh, part, gvec, gx

    gxh, gv_parts, _, _ = message_bwd(False)
    gxh_f, gv_parts_f, gvo_ref, gx_add = message_bwd(True)
    assert _same_bits(gxh, gxh_f) and _same_bits(gv_parts, gv_parts_f)
    gn_parts = nodeops.node_pre_bwd(gxh, hb, x, mean, rstd, wd, parts_only=True)
    gxo_ref = nodeops.node_pre_bwd(gxh, hb, x, mean, rstd, wd, add=gx_add)
    # the layer below: saved tensors of its update forward
    x1, vec1 = _fwd_inputs(g, 70 + LAYOUTS.index(kind))
    saved = _update_fwd(g, wd, x1.to(dev), vec1.to(dev), 16)
    c = dict(g=g, wd=wd, saved=saved, gn_parts=gn_parts, gv_parts=gv_parts, x=x, mean=mean, rstd=rstd, gx1a=gx1a, gvec1a=gvec1a,
             gxo_ref=gxo_ref, gvo_ref=gvo_ref)
    rc, c["gx1"], c["gvec1"] = _update_bwd(c, "hermnet_node_update_bwd", gxo_ref.clone(), gvo_ref.clone(), None)
    assert rc == 0
    nk = g.type_rowptr_host[T]
    assert torch.isfinite(gxo_ref).all() and torch.isfinite(gvo_ref).all()
    assert torch.isfinite(c["gx1"]).all() and torch.isfinite(c["gvec1"]).all() and float(c["gvec1"][:nk].abs().max()) > 1e-3
    _CACHE[key] = c
    return c


def _pending(c, **override):
    f = dict(gn_parts=c["gn_parts"], gvec_parts=c["gv_parts"], x=c["x"], mean=c["mean"], rstd=c["rstd"], gx1=c["gx1a"],
             gvec1=c["gvec1a"])
    f.update(override)
    return _lib.PendingGrads(*[P(f[k]) for k in ("gn_parts", "gvec_parts", "x", "mean", "rstd", "gx1", "gvec1")], T, 0,
                             P(override.get("gxh")), None, None, None)


def _update_bwd(c, entry, gxo, gvo, pend, tile=16, hidden=H, null=()):
    """-> (return code, gx1, gvec1), both NaN-filled before the call; `null`: arguments passed as NULL."""
    g, wd, s = c["g"], c["wd"], c["saved"]
    dev = gxo.device
    gx1, gvec1 = _nan(dev, g.N, H), _nan(dev, g.N, 3, H)
    a = dict(gxo=gxo, gvo=gvo, vp=s["vp"], h2b=s["h2b"], q23=s["q23"], nrm=s["nrm"], wx2t=wd.wx2tf16, wx0t=wd.wx0tf16,
             wvt=wd.wvtf16, act=g.row_active, rp=g.type_rowptr, gx1=gx1, gvec1=gvec1)
    for k in null:
        a[k] = None
    rc = getattr(_lib.load(), entry)(P(a["gxo"]), P(a["gvo"]), P(a["vp"]), P(a["h2b"]), P(a["q23"]), P(a["nrm"]), P(a["wx2t"]),
                                     P(a["wx0t"]), P(a["wvt"]), P(a["act"]), P(a["rp"]), _rowptr(g), P(a["gx1"]), P(a["gvec1"]),
                                     g.N, g.T, hidden, tile, None if pend is None else ctypes.byref(pend), _stream())
    return rc, gx1, gvec1


@pytest.mark.parametrize("kind", LAYOUTS)
def test_pending_sums_formed_in_registers_fill_both_buffers(kind):
    """(i) hermnet_node_update_bwd with `pending`: gx1 / gvec1 are the bits the finishing launches' gradients give, and
    gx_out / gvec_out are filled with those launches' bits on the rows below type_rowptr[T]."""
    dev = _dev()
    c = _case(kind, dev)
    N, nk = c["g"].N, c["g"].type_rowptr_host[T]
    bx, bv = _nan(dev, N, H), _nan(dev, N, 3, H)
    rc, gx1, gvec1 = _update_bwd(c, "hermnet_node_update_bwd", bx, bv, _pending(c))
    assert rc == 0
    assert _same_bits(gx1, c["gx1"]) and _same_bits(gvec1, c["gvec1"])
    assert _same_bits(bx[:nk], c["gxo_ref"][:nk]) and _same_bits(bv[:nk], c["gvo_ref"][:nk])


@pytest.mark.parametrize("kind", LAYOUTS)
def test_held_form_returns_the_same_bits_and_leaves_gvec_out_alone(kind):
    """(ii) hermnet_node_update_bwd_held: the same gx1 / gvec1 bits; a NaN-filled gvec_out stays NaN everywhere; gvec_out may be
    NULL."""
    dev = _dev()
    c = _case(kind, dev)
    N = c["g"].N
    for with_buffer in (True, False):
        bx, bv = _nan(dev, N, H), (_nan(dev, N, 3, H) if with_buffer else None)
        rc, gx1, gvec1 = _update_bwd(c, "hermnet_node_update_bwd_held", bx, bv, _pending(c))
        assert rc == 0
        assert _same_bits(gx1, c["gx1"]) and _same_bits(gvec1, c["gvec1"])
        if with_buffer:
            assert bool(torch.isnan(bv).all())


def test_gvec_out_from_memory_takes_the_same_path():
    """Nothing pending: gv[d] loaded from gvec_out is parked in the LDS tiles too.  Against the float64 restatement by the row
    rule (floor 5e-6), on the layout with inactive rows."""
    dev = _dev()
    c = _case("inactive", dev)
    g, gc = _layout("inactive", dev)
    w, _ = _weights(dev)
    s = c["saved"]
    cpu = lambda t, dt: t.cpu().to(dt)
    refs = [ref_ops.node_update_bwd(cpu(c["gxo_ref"], dt), cpu(c["gvo_ref"], dt), cpu(s["vp"], dt), cpu(s["h2b"], dt),
                                    cpu(s["q23"], dt), cpu(s["nrm"], dt), w, gc) for dt in (torch.float64, torch.float32)]
    nk = g.type_rowptr_host[T]
    for k, (name, got) in enumerate((("gx1", c["gx1"]), ("gvec1", c["gvec1"]))):
        share, worst = judge_rows(got, refs[0][k], refs[1][k], 5e-6, "update_bwd " + name, slice(0, nk))
        print("update_bwd inactive %-5s worst err/bound %.3f  deciding share %.3f" % (name, worst, share))
        assert float(got[nk:].abs().max()) == 0.0


def test_held_form_refuses_before_any_launch():
    """(iii) HN_ERR_BAD_ARG and untouched (NaN) outputs: no pending record, the fused form (pending->gxh), tile_rows 0 / 32,
    widths 64 / 192 / 256, each required argument and each field of the record NULL."""
    dev = _dev()
    c = _case("ragged", dev)
    N = c["g"].N
    entry = "hermnet_node_update_bwd_held"
    bx, bv = _nan(dev, N, H), _nan(dev, N, 3, H)
    runs = [_update_bwd(c, entry, bx, bv, None), _update_bwd(c, entry, bx, bv, _pending(c, gxh=c["gn_parts"]))]
    runs += [_update_bwd(c, entry, bx, bv, _pending(c), tile=tile) for tile in (0, 32)]
    runs += [_update_bwd(c, entry, bx, bv, _pending(c), hidden=width) for width in (64, 192, 256)]
    runs += [_update_bwd(c, entry, bx, bv, _pending(c), null=(k,))
             for k in ("gxo", "vp", "h2b", "q23", "nrm", "wx2t", "wx0t", "wvt", "rp", "gx1", "gvec1")]
    runs += [_update_bwd(c, entry, bx, bv, _pending(c, **{k: None}))
             for k in ("gn_parts", "gvec_parts", "x", "mean", "rstd", "gx1", "gvec1")]
    torch.cuda.synchronize()
    for k, (rc, gx1, gvec1) in enumerate(runs):
        assert rc == BAD_ARG, k
        # (an argument passed as NULL has no buffer to look at)
        assert bool(torch.isnan(gx1).all()) and bool(torch.isnan(gvec1).all()), k
    assert bool(torch.isnan(bx).all()) and bool(torch.isnan(bv).all())


# ---- model level ----------------------------------------------------------------------------------------------------------------
class _LaunchCounter(object):
    def __init__(self):
        self.names = []

    def launch(self, name, fn):
        self.names.append(name)
        return fn()


def _energy_forces(model, data, dev):
    d = data.to(dev)
    d.pos.requires_grad_(True)
    cnt = _LaunchCounter()
    ops.set_kernel_timer(cnt)
    try:
        e = model(d)
        f = -torch.autograd.grad(e.sum(), d.pos)[0]
    finally:
        ops.set_kernel_timer(None)
    torch.cuda.synchronize()
    assert not d._hn_step.pending           # every handed-down gradient was picked up
    return e.detach().clone(), f.clone(), cnt.names


def _model(name, dev):
    g = Golden(name)
    model = g.model().to(dev)
    for prm in model.parameters():
        prm.requires_grad_(False)
    return g, model


@pytest.mark.parametrize("name", ["alloy108", "alloy108_unknown_type", "mol16"])
def test_model_with_and_without_pending_on_chip_gives_the_same_bits(name, monkeypatch):
    """switches.pending_on_chip True against False: energy and forces bit for bit, as many library calls, nothing left in
    step.pending; the same bits from a replayed GraphedStep (two replays); poisoned hand-down buffers throughout."""
    from hermnet_amd.graph import GraphedStep
    dev = _dev()
    monkeypatch.setenv("HERMNET_DEBUG_POISON", "1")
    g, model = _model(name, dev)
    held = []
    monkeypatch.setattr(nodeops, "node_update_bwd_held",
                        lambda *a, _f=nodeops.node_update_bwd_held, **k: (held.append(1), _f(*a, **k))[1])
    e1, f1, n1 = _energy_forces(model, g.data(), dev)
    layers = g.model_kw["num_layers"]
    assert len(held) == layers - 1 and layers >= 2              # (every update backward but the last layer's takes a hand-down)
    step = GraphedStep(model, g.data().to(dev), warmup=2)
    for _ in range(2):
        eg, fg = step()
        assert _same_bits(eg, e1) and _same_bits(fg, f1)
    del held[:]
    monkeypatch.setattr(switches, "pending_on_chip", False)
    e0, f0, n0 = _energy_forces(model, g.data(), dev)
    assert held == [] and len(n0) == len(n1)
    assert torch.isfinite(f1).all() and float(f1.abs().max()) > 1e-4
    assert _same_bits(e1, e0) and _same_bits(f1, f0)


def test_model_with_finishing_launches_gives_the_same_bits(monkeypatch):
    """HERMNET_DEFER_SUMS=0: nothing is pending, the update backward loads gvec_out from memory and parks gv[d] in LDS all the
    same -- the bits of the deferred path (the projection's backward in the same form on both sides: boundary_mode 0)."""
    dev = _dev()
    monkeypatch.setattr(switches, "boundary_mode", 0)
    g, model = _model("alloy108", dev)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("HERMNET_DEFER_SUMS", flag)
        res[flag] = _energy_forces(model, g.data(), dev)
    assert len(res["0"][2]) == len(res["1"][2])
    assert _same_bits(res["0"][0], res["1"][0]) and _same_bits(res["0"][1], res["1"][1])
