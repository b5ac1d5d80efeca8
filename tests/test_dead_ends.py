"""GPU: the kernel forms without the dead work at the two ends of the layer stack, against the general forms, bit for bit.

  last layer   hermnet_node_update_fwd_last / _bwd_last (csrc/node_chain16.hip: NOVEC / NOGV): the read-out takes x only, so
               vec_out feeds nothing and its gradient is identically zero;
  first layer  hermnet_message_scatter_bwd_gedge (csrc/message_bwd_cl.hip: NEED_GXH = false): x of the first layer is the
               species embedding, so only gedge is a result of its message backward.

Shapes: 53 atoms of three elements (28 / 22 / 3: no count is a multiple of the 16-row tile, one element has very few atoms),
H = 128 (two column blocks), num_rbf = 128 and 256 (the windowed launches); the graph kinds add atoms of an unknown element
(rows past type_rowptr[T]), an element without any atom (an empty relation) and the NULL edges of a padded list.
"Bit for bit" compares the int32 views: torch.equal on floats would let a flipped sign of zero through."""
import ctypes
import math

import numpy as np
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import _lib, nodeops, switches, synth
from hermnet_amd.layer import LayerWeights
from hermnet_amd.ops import RbfDescriptor, edge_radial_tables, _stream
from hermnet_amd.relations import RelationalGraph
from helpers import Golden, rel_err

pytestmark = pytest.mark.gpu
P = _lib.ptr
RC = 5.0
ELEMS = ["Al", "Ni", "Cu"]
Z_LIST = [13, 28, 29]
H = 128
KINDS = ["plain", "unknown", "empty", "padded"]
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _species(kind):
    z = torch.tensor([13] * 28 + [28] * 22 + [29] * 3)
    if kind == "unknown":
        z[[5, 30, 40, 52]] = 1          # four atoms of an element the model does not know
    if kind == "empty":
        z[50:] = 28                     # no Cu atom at all: its relation is empty
    return z[torch.randperm(53, generator=torch.Generator().manual_seed(2))]


def _graph(kind, dev):
    """53 atoms; in-degrees 0, 1, 3, 5 and 70 on the first atoms, 2..9 elsewhere; "padded": 21 NULL edges behind the real ones."""
    if kind not in _CACHE:
        gen = torch.Generator().manual_seed(17)
        z = _species(kind)
        n = z.numel()
        deg = torch.randint(2, 10, (n,), generator=gen)
        deg[:5] = torch.tensor([0, 1, 3, 5, 70])
        tgt = torch.repeat_interleave(torch.arange(n), deg)
        src = torch.randint(0, n, (tgt.numel(),), generator=gen)
        perm = torch.randperm(tgt.numel(), generator=gen)
        ei = torch.stack([src[perm], tgt[perm]])
        if kind == "padded":
            ei = torch.cat([ei, torch.full((2, 21), -1, dtype=ei.dtype)], 1)
        _CACHE[kind] = RelationalGraph.build(z.to(dev), ei.to(dev), Z_LIST)
    return _CACHE[kind]


def _edges(E, R, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    rhat = torch.nn.functional.normalize(torch.randn(E, 3, generator=gen), dim=1)
    d = RC * (0.02 + 0.97 * torch.rand(E, generator=gen))
    special = [1e-4, 0.01, RC * 0.9999, RC, RC * 1.3]
    pick = torch.randint(0, 4 * len(special), (E,), generator=gen)
    for k, v in enumerate(special):
        d[pick == k] = v
    return torch.cat([rhat, d[:, None]], 1).float().contiguous().to(dev)


def _weights(dev):
    """Kernel-ready weights of one layer with the three elements' update networks (random parameters)."""
    if "w" not in _CACHE:
        model = hn.HVNet(ELEMS, rc=RC, num_layers=1, hidden_channels=H, num_rbf=128).eval()
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 3))
        model = model.to(dev)
        _CACHE["w"] = (model, LayerWeights(model.hermconvs[0].mods.values()).refresh())
    return _CACHE["w"][1]


def _rowptr(graph):
    vals = list(graph.type_rowptr_host)
    return (ctypes.c_int * len(vals))(*vals)


def _update_fwd(graph, w, x1, vec1, short):
    """-> dict of the outputs, every buffer pre-filled with NaN."""
    N, dev = graph.N, x1.device
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    o = dict(vp=nan(N, 3, 2 * H), h2b=nan(N, H), q23=nan(N, 2 * H), nrm=nan(N, H), xo=nan(N, H))
    lib = _lib.load()
    head = (P(x1), P(vec1), P(w.wvf16), P(w.wx0f16), P(w.bx0_s), P(w.wx2f16), P(w.bx2_s), P(graph.row_active),
            P(graph.type_rowptr), _rowptr(graph), P(o["vp"]), P(o["h2b"]), P(o["q23"]), P(o["nrm"]), P(o["xo"]))
    if short:
        rc = lib.hermnet_node_update_fwd_last(*head, N, graph.T, H, _stream())
    else:
        o["vo"] = nan(N, 3, H)
        rc = lib.hermnet_node_update_fwd(*head, P(o["vo"]), N, graph.T, H, 16, _stream())
    assert rc == 0
    return o


def _update_inputs(graph, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(graph.N, H, generator=gen).to(dev), torch.randn(graph.N, 3, H, generator=gen).to(dev)


@pytest.mark.parametrize("kind", KINDS)
def test_update_forward_without_vec_out_is_bit_identical(kind):
    """x_out and every saved tensor the short backward reads (vp, h2b, nrm, the q half of q23): the general form's bits, and
    nothing of them left unwritten (the buffers start as NaN)."""
    dev = _dev()
    graph, w = _graph(kind, dev), _weights(dev)
    x1, vec1 = _update_inputs(graph, dev, 31)
    a, b = _update_fwd(graph, w, x1, vec1, False), _update_fwd(graph, w, x1, vec1, True)
    nk = graph.type_rowptr_host[graph.T]
    assert (nk < graph.N) == (kind == "unknown")
    assert torch.isfinite(b["xo"]).all() and _same_bits(a["xo"], b["xo"])
    for name in ("vp", "h2b", "nrm"):
        assert torch.isfinite(b[name][:nk]).all(), name
        assert _same_bits(a[name][:nk], b[name][:nk]), name
    assert torch.isfinite(b["q23"][:nk, :H]).all() and _same_bits(a["q23"][:nk, :H], b["q23"][:nk, :H])
    assert torch.isfinite(a["vo"]).all() and float(a["vo"].abs().max()) > 0.1      # (the general form did run)


def _update_bwd(graph, w, gxo, saved, short, pending=None):
    N, dev = graph.N, gxo.device
    gx1, gvec1 = torch.full((N, H), float("nan"), device=dev), torch.full((N, 3, H), float("nan"), device=dev)
    lib = _lib.load()
    tail = (P(saved["vp"]), P(saved["h2b"]), P(saved["q23"]), P(saved["nrm"]), P(w.wx2tf16), P(w.wx0tf16), P(w.wvtf16),
            P(graph.row_active), P(graph.type_rowptr), _rowptr(graph), P(gx1), P(gvec1), N, graph.T, H)
    if short:
        rc = lib.hermnet_node_update_bwd_last(P(gxo), *tail, pending, _stream())
    else:
        gvo = torch.zeros(N, 3, H, device=dev)
        rc = lib.hermnet_node_update_bwd(P(gxo), P(gvo), *tail, 16, pending, _stream())
    return rc, gx1, gvec1


@pytest.mark.parametrize("kind", KINDS)
def test_update_backward_for_a_zero_vec_gradient_is_bit_identical(kind):
    """The short form against the general form fed gvo = 0, signs of zeros included.  gxo carries what makes zeros of either
    sign inside the chain: all-zero rows, rows of -0, single zeros and -0 entries, a row of tiny values next to large ones."""
    dev = _dev()
    graph, w = _graph(kind, dev), _weights(dev)
    x1, vec1 = _update_inputs(graph, dev, 32)
    saved = _update_fwd(graph, w, x1, vec1, False)
    short_saved = _update_fwd(graph, w, x1, vec1, True)          # (its q23 has no r half: the short backward must not need it)
    gen = torch.Generator().manual_seed(33)
    gxo = torch.randn(graph.N, H, generator=gen)
    gxo[3] = 0.0
    gxo[17] = 0.0
    gxo[21] = -0.0
    gxo[40, ::2] = 0.0
    gxo[41, 1::3] = -0.0
    gxo[45] *= 1e-30
    gxo[46, :64] *= 1e30
    gxo = gxo.to(dev)
    rc_a, gx_a, gv_a = _update_bwd(graph, w, gxo, saved, False)
    rc_b, gx_b, gv_b = _update_bwd(graph, w, gxo, short_saved, True)
    assert rc_a == 0 and rc_b == 0
    assert torch.isfinite(gx_b).all() and torch.isfinite(gv_b).all()
    assert float(gv_a.abs().max()) > 1e-3
    assert _same_bits(gx_a, gx_b)
    assert _same_bits(gv_a, gv_b)


def _msg_inputs(graph, R, dev, seed=3):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    T, N = graph.T, graph.N
    xh = rnd(T, N, 3 * H)
    wt = (rnd(T, R, 3 * H) / math.sqrt(R)).contiguous()
    brbf = (0.1 * rnd(T, 3 * H)).contiguous()
    return xh, wt, brbf, rnd(N, H), rnd(N, 3, H)


@pytest.mark.parametrize("R", [128, 256], ids=["whole_tile", "windowed"])
@pytest.mark.parametrize("kind", KINDS)
def test_layer0_message_backward_without_source_sums_is_bit_identical(kind, R):
    """gedge of NEED_GXH = false (no gxh buffer at all) against the general layer-0 form; num_rbf = 256 takes the two launches
    over tap-row windows.  Slots no kernel writes (edges into rows of an unknown element, NULL edges) keep the fill."""
    dev = _dev()
    graph = _graph(kind, dev)
    rbf = RbfDescriptor(torch.linspace(0, 1, R, device=dev), RC, 0, 5)
    edge = _edges(graph.E, R, 5, dev)
    xh, wt, brbf, gx1, gv1 = _msg_inputs(graph, R, dev)
    table, _ = edge_radial_tables(graph, rbf, edge)
    lib = _lib.load()
    gs, rs = graph.as_struct(), rbf.struct()
    ge_a = torch.full((H // 64, graph.E, 4), 7.0, device=dev)
    ge_b = torch.full((H // 64, graph.E, 4), 7.0, device=dev)
    gxh = torch.full_like(xh, float("nan"))
    assert lib.hermnet_message_scatter_bwd(ctypes.byref(gs), ctypes.byref(rs), H, P(xh), None, None, P(wt), P(brbf), P(edge),
                                           P(gx1), P(gv1), P(gxh), None, None, P(ge_a), 0, P(table), None, None, None, 0,
                                           _stream()) == 0
    assert lib.hermnet_message_scatter_bwd_gedge(ctypes.byref(gs), ctypes.byref(rs), H, P(xh), P(wt), P(brbf),
                                                 P(edge), P(gx1), P(gv1), P(ge_b), P(table), _stream()) == 0
    assert torch.isfinite(gxh).all()                        # (the general form did write its source-row sums)
    assert torch.isfinite(ge_b).all() and float((ge_b != 7.0).float().mean()) > 0.5
    assert _same_bits(ge_a, ge_b)


def test_refusals():
    """HN_ERR_BAD_ARG before any launch: the short update backward with gradients pending from a layer above, the gedge-only
    message backward without the edge table, the kernel with vec rows without a gxh buffer (hermnet_message_scatter_bwd's
    own argument check, which is what keeps a null gxh away from the HAS_VEC instances)."""
    dev = _dev()
    graph, w = _graph("plain", dev), _weights(dev)
    x1, vec1 = _update_inputs(graph, dev, 34)
    saved = _update_fwd(graph, w, x1, vec1, True)
    buf = torch.zeros(graph.T * graph.N * 3 * H, device=dev)
    pend = _lib.PendingGrads(P(buf), P(buf), P(buf), P(buf), P(buf), P(buf), P(buf), 1, 0, None, None, None, None)
    rc, gx1, gvec1 = _update_bwd(graph, w, x1, saved, True, pending=ctypes.byref(pend))
    assert rc == 1
    assert torch.isnan(gx1).all() and torch.isnan(gvec1).all()          # nothing ran
    R = 128
    rbf = RbfDescriptor(torch.linspace(0, 1, R, device=dev), RC, 0, 5)
    edge = _edges(graph.E, R, 5, dev)
    xh, wt, brbf, g1, gv1 = _msg_inputs(graph, R, dev)
    table, _ = edge_radial_tables(graph, rbf, edge)
    lib = _lib.load()
    gs, rs = graph.as_struct(), rbf.struct()
    gedge = torch.full((H // 64, graph.E, 4), 7.0, device=dev)
    part = torch.empty(graph.T, graph.N, 3, H, device=dev)
    # (the gedge-only export has no vec argument; without the edge table it has no kernel form to run)
    assert lib.hermnet_message_scatter_bwd_gedge(ctypes.byref(gs), ctypes.byref(rs), H, P(xh), P(wt), P(brbf),
                                                 P(edge), P(g1), P(gv1), P(gedge), None, _stream()) == 1
    assert lib.hermnet_message_scatter_bwd(ctypes.byref(gs), ctypes.byref(rs), H, P(xh), None, P(vec1), P(wt), P(brbf), P(edge),
                                           P(g1), P(gv1), None, None, None, P(gedge), 0, P(table), P(part), None, None, 0,
                                           _stream()) == 1
    torch.cuda.synchronize()
    assert bool((gedge == 7.0).all())


def _alloy53(kind):
    """53 atoms of a jittered fcc cell (7.2 x 7.2 x 14.4 A, periodic), species as in `_species`; cutoff 3 A."""
    pos, cell, _ = synth.fcc_alloy_atoms(reps=(2, 2, 4), seed=4)
    return synth.periodic_data(pos[:53], cell, _species(kind).numpy().astype(np.int64), 3.0)


def _energy_forces(model, data, dev):
    d = data.to(dev)
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    return e.detach().clone(), f.clone(), d


@pytest.mark.parametrize("layers,kind", [(1, "plain"), (2, "unknown"), (5, "plain"), (2, "empty")])
def test_model_with_and_without_the_short_forms_gives_the_same_bits(layers, kind, monkeypatch):
    """HVNet with 1 (first = last layer), 2 and 5 layers: switches.dead_ends on against off."""
    import hermnet_amd.layer as lmod
    dev = _dev()
    model = hn.HVNet(ELEMS, rc=3.0, num_layers=layers, hidden_channels=H, num_rbf=128).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 7))
    model = model.to(dev)
    for prm in model.parameters():
        prm.requires_grad_(False)
    calls = []
    for mod, name in ((nodeops, "node_update_fwd_last"), (nodeops, "node_update_bwd_last"), (lmod, "_msg_bwd_gedge")):
        def wrap(*a, _f=getattr(mod, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(mod, name, wrap)
    e1, f1, d1 = _energy_forces(model, _alloy53(kind), dev)
    assert sorted(calls) == ["_msg_bwd_gedge", "node_update_bwd_last", "node_update_fwd_last"]
    assert d1.vec is None
    del calls[:]
    monkeypatch.setattr(switches, "dead_ends", False)
    e0, f0, d0 = _energy_forces(model, _alloy53(kind), dev)
    assert calls == [] and d0.vec is not None
    assert float(f0.abs().max()) > 1e-4
    assert _same_bits(e1, e0) and _same_bits(f1, f0)


def test_golden_through_the_short_forms_and_the_replayed_step():
    """alloy108 (the reference's own outputs, its committed tolerance) through the default path, which takes the short forms;
    the same step replayed from a captured graph gives the eager bits."""
    from hermnet_amd.graph import GraphedStep
    dev = _dev()
    g = Golden("alloy108")
    model = g.model().to(dev)
    for prm in model.parameters():
        prm.requires_grad_(False)
    e, f, d = _energy_forces(model, g.data(), dev)
    assert d.vec is None                                     # (the last layer ran without its vec output)
    assert rel_err(e.cpu(), g.energy) < 1e-5 and rel_err(f.cpu(), g.forces) < 1e-5
    d2 = g.data().to(dev)
    step = GraphedStep(model, d2, warmup=2)
    eg, fg = step()
    assert _same_bits(eg, e) and _same_bits(fg, f)
