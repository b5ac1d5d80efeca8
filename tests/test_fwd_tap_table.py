"""GPU: the forward message kernel fed from the once-per-step tap records (hermnet_edge_radial_tables ->
hermnet_message_scatter_fwd_taps) against the form that evaluates taps, envelope and tile row in its edge loop
(hermnet_message_scatter_fwd).  The records hold exactly what the loop computes, so every comparison here is bit for bit.

Synthetic inputs, fixed seeds, ~200 atoms: the `edge` array (rhat, d) is handed to the kernels directly, so the distances
that matter are placed by hand -- d near 0 (window running into the zero rows below tap 0), d just under rc (window running
past tap R-1), d >= rc (the bias-only message) -- and the target rows have 0, 1, 3, 5 and 70 edges (padding slots of a group
of four, the empty row, the 64-edge batch boundary).  Atoms of an unknown element and the NULL edges of a padded list are in
every graph."""
import ctypes
import math

import pytest
import torch

from hermnet_amd import _lib
from hermnet_amd.ops import RbfDescriptor, edge_radial_tables, _stream
from hermnet_amd.relations import RelationalGraph

pytestmark = pytest.mark.gpu
P = _lib.ptr
RC = 5.0
Z_LIST = [13, 28, 29]
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _edge_list(seed):
    """(atomic_number [200], edge_index [2,E]) with in-degrees 0, 1, 3, 5, 70 on the first atoms of every element, small
    random degrees elsewhere, ten atoms of an unknown element (sources and targets of edges) and 37 NULL edges."""
    gen = torch.Generator().manual_seed(seed)
    n = 200
    z = torch.tensor([Z_LIST[i % 3] for i in range(n)])
    z[190:] = 1                                         # unknown element
    deg = torch.randint(2, 10, (n,), generator=gen)
    for k, dg in enumerate([0, 1, 3, 5, 70, 64, 65, 4, 8]):
        deg[3 * k:3 * k + 3] = dg                       # one such row per element
    tgt = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (tgt.numel(),), generator=gen)
    perm = torch.randperm(tgt.numel(), generator=gen)
    ei = torch.stack([src[perm], tgt[perm]])
    null = torch.full((2, 37), -1, dtype=ei.dtype)
    return z, torch.cat([ei, null], 1)


def _edges(E, R, seed, dev):
    """[E,4] (rhat, d): random directions; distances mostly inside the cutoff, with the special ones sprinkled over them."""
    gen = torch.Generator().manual_seed(seed)
    rhat = torch.nn.functional.normalize(torch.randn(E, 3, generator=gen), dim=1)
    d = RC * (0.02 + 0.97 * torch.rand(E, generator=gen))
    special = [1e-4, 0.01, RC * 2.5 / (R - 1), RC * 0.9999, RC * (1 - 1.5 / (R - 1)), RC, RC * 1.3, 1e4]
    pick = torch.randint(0, 3 * len(special), (E,), generator=gen)      # a third of the edges take a special distance
    for k, v in enumerate(special):
        d[pick == k] = v
    return torch.cat([rhat, d[:, None]], 1).float().contiguous().to(dev)


def _graph(kind, dev):
    if kind not in _CACHE:
        z, ei = _edge_list(11)
        if kind == "triadic":
            z = torch.where(z != 29, z, torch.ones_like(z))    # two elements: T = 2 * 3 pair relations
            ei = ei[:, ei[0] >= 0]                             # (padded lists are HVNet's)
            _CACHE[kind] = RelationalGraph.build_triadic(z.to(dev), ei.to(dev), Z_LIST[:2])
        else:
            _CACHE[kind] = RelationalGraph.build(z.to(dev), ei.to(dev), Z_LIST)
    return _CACHE[kind]


def _rbf(R, dev, env_kind=0, env_p=5):
    return RbfDescriptor(torch.linspace(0, 1, R, device=dev), RC, env_kind, env_p)


def _inputs(graph, H, R, has_vec, dev, seed=3):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    T, Ns = graph.T, graph.num_src or graph.N
    xh, x = rnd(T, Ns, 3 * H), rnd(Ns, H)
    vec = rnd(Ns, 3, H) if has_vec else None
    wt = (rnd(T, R, 3 * H) / math.sqrt(R)).contiguous()
    brbf, xb = (0.1 * rnd(T, 3 * H)).contiguous(), (0.1 * rnd(T, 3 * H)).contiguous()
    return xh, xb, vec, x, wt, brbf


def _fwd(graph, rbf, H, ins, edge, taps, out=None, ranges=None, zero_unknown=1, range_rows=0):
    lib = _lib.load()
    xh, xb, vec, x, wt, brbf = ins
    if out is None:       # (a fill no kernel produces: a row left unwritten by one form only would show)
        out = (torch.full((graph.N, H), 7.0, device=edge.device), torch.full((graph.N, 3, H), 7.0, device=edge.device))
    gs, rs = graph.as_struct(), rbf.struct()
    if taps is None:
        rc = lib.hermnet_message_scatter_fwd(ctypes.byref(gs), ctypes.byref(rs), H, P(xh), P(xb), P(vec), P(x), P(wt), P(brbf),
                                             P(edge), P(out[0]), P(out[1]), P(ranges), zero_unknown, range_rows, _stream())
    else:
        rc = lib.hermnet_message_scatter_fwd_taps(ctypes.byref(gs), ctypes.byref(rs), H, P(xh), P(xb), P(vec), P(x), P(wt),
                                                  P(brbf), P(edge), P(taps), P(out[0]), P(out[1]), P(ranges), zero_unknown,
                                                  range_rows, _stream())
    assert rc == 0
    return out


def test_the_synthetic_graph_has_the_rows_the_cases_need():
    graph = _graph("hvnet", _dev())
    deg = (graph.csr_rowptr[1:] - graph.csr_rowptr[:-1]).cpu()
    known = deg[:graph.type_rowptr_host[graph.T]].tolist()
    for want in (0, 1, 3, 5, 64, 65, 70):
        assert want in known, want
    assert graph.N > graph.type_rowptr_host[graph.T]          # rows of the unknown element


@pytest.mark.parametrize("has_vec", [True, False], ids=["vec", "layer0"])
@pytest.mark.parametrize("H,R", [(128, 128), (64, 128), (128, 200), (64, 200)])
def test_table_fed_forward_is_bit_identical(H, R, has_vec):
    """One and two column blocks; one launch (num_rbf = 128) and the two windowed launches with accumulate (200); 8 waves
    with vec rows, 16 without."""
    dev = _dev()
    graph = _graph("hvnet", dev)
    rbf = _rbf(R, dev)
    edge = _edges(graph.E, R, 5, dev)
    ins = _inputs(graph, H, R, has_vec, dev)
    _, taps = edge_radial_tables(graph, rbf, edge)
    x1, vec1 = _fwd(graph, rbf, H, ins, edge, None)
    y1, wec1 = _fwd(graph, rbf, H, ins, edge, taps)
    assert torch.isfinite(x1).all() and torch.isfinite(vec1).all()
    assert not bool((x1 == 7.0).any())                         # every row written
    assert torch.equal(x1, y1) and torch.equal(vec1, wec1)


def test_table_fed_forward_with_the_exponential_envelope_is_bit_identical():
    dev = _dev()
    graph = _graph("hvnet", dev)
    rbf = _rbf(128, dev, env_kind=1, env_p=0)
    edge = _edges(graph.E, 128, 6, dev)
    ins = _inputs(graph, 128, 128, True, dev)
    _, taps = edge_radial_tables(graph, rbf, edge)
    a, b = _fwd(graph, rbf, 128, ins, edge, None), _fwd(graph, rbf, 128, ins, edge, taps)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("R", [128, 200])
def test_table_fed_forward_over_complementary_ranges_is_bit_identical(R):
    """The sharded step's form: two launches over complementary target ranges into one output."""
    dev = _dev()
    graph = _graph("hvnet", dev)
    H, T = 128, graph.T
    rbf = _rbf(R, dev)
    edge = _edges(graph.E, R, 7, dev)
    ins = _inputs(graph, H, R, True, dev)
    _, taps = edge_radial_tables(graph, rbf, edge)
    whole = _fwd(graph, rbf, H, ins, edge, None)
    rp = list(graph.type_rowptr_host)
    cuts = [[rp[t], rp[t] + (rp[t + 1] - rp[t]) * k // 3, rp[t + 1]] for t, k in zip(range(T), [1, 0, 3])]
    early = torch.tensor([[c[0], c[1]] for c in cuts], dtype=torch.int32, device=dev)
    late = torch.tensor([[c[1], c[2]] for c in cuts], dtype=torch.int32, device=dev)
    n_early = sum(c[1] - c[0] for c in cuts)
    out = _fwd(graph, rbf, H, ins, edge, taps, ranges=early, zero_unknown=1, range_rows=n_early)
    out = _fwd(graph, rbf, H, ins, edge, taps, out=out, ranges=late, zero_unknown=0, range_rows=rp[T] - n_early)
    assert torch.equal(out[0], whole[0]) and torch.equal(out[1], whole[1])


def test_table_fed_forward_on_a_triadic_graph_is_bit_identical():
    """HTNet rows: num_src != N, the residual through res_row."""
    dev = _dev()
    graph = _graph("triadic", dev)
    assert graph.num_src and graph.num_src != graph.N
    H, R = 128, 128
    rbf = _rbf(R, dev)
    edge = _edges(graph.E, R, 8, dev)
    ins = _inputs(graph, H, R, True, dev)
    _, taps = edge_radial_tables(graph, rbf, edge)
    a, b = _fwd(graph, rbf, H, ins, edge, None), _fwd(graph, rbf, H, ins, edge, taps)
    assert torch.isfinite(a[0]).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _fma32(a, b, c):
    """fp32 fused multiply-add of fp32 tensors: the product of two fp32 values is exact in fp64."""
    return (a.double() * b.double() + c.double()).float()


def test_record_contents():
    """Tile row: exact against a plain torch restatement of hn_window_lo.  env: exact against the restatement of
    hn_envelope's polynomial form with the roundings the forward kernels give it (FMA, multiply, add, FMA; an fp32 FMA is
    restated through the exact fp64 product).
    Taps: exact against the IN-KERNEL values, read back through a graph with one edge per target row and weights
    W[k][c] = delta(k, c), x_proj part s = 1, no bias: the table-free kernel then returns x1[r][lo + m] = fl(fl(env g_m) / sqrt2),
    which two fp32 multiplications of the record's words must reproduce bit for bit.  (The fallback of the issue --
    torch.exp at a relative tolerance -- was not needed.)"""
    dev = _dev()
    H = R = 128
    n = 192
    z = torch.tensor([Z_LIST[i % 3] for i in range(n)])
    gen = torch.Generator().manual_seed(21)
    ei = torch.stack([torch.randint(0, n, (n,), generator=gen), torch.arange(n)])       # one edge into every atom
    graph = RelationalGraph.build(z.to(dev), ei.to(dev), Z_LIST)
    E, T, N = graph.E, graph.T, graph.N
    assert E == n and int((graph.csr_rowptr[1:] - graph.csr_rowptr[:-1]).max()) == 1
    rbf = _rbf(R, dev)
    edge = _edges(E, R, 22, dev)
    _, taps = edge_radial_tables(graph, rbf, edge)
    torch.cuda.synchronize()

    # --- tile row and envelope against torch
    u = edge[:, 3] * torch.tensor(rbf.inv_rc, dtype=torch.float32, device=dev)
    t = (u * float(R - 1)).clamp(0.0, float(R + 5))
    row = t.to(torch.int32) - 5 + 11
    assert torch.equal(taps[:, 13].contiguous().view(torch.int32), row)
    assert int(row.min()) < 11 and int(row.max()) + 12 > R + 11          # windows past both ends of the taps are present
    p = 5.0
    up1 = u * u * u * u                                                  # ((1 u) u) u) u ... : u^(p-1), left to right
    up = up1 * u
    w = 1.0 - u
    one, fp = torch.ones_like(u), torch.full_like(u, p)
    k2 = torch.full_like(u, 0.5 * p * (p + 1.0))
    env = _fma32(-(1.0 + w * _fma32(k2, w, fp)), up, one)
    env = torch.where(u < 1.0, env, torch.zeros_like(env))
    print("env: max |record - restatement| = %.3e, mismatches %d of %d"
          % (float((taps[:, 12] - env).abs().max()), int((taps[:, 12] != env).sum()), E))
    assert torch.equal(taps[:, 12], env)
    assert not bool(taps[:, 14:].any())

    # --- taps x envelope against the in-kernel values
    wt = torch.zeros(T, R, 3 * H, device=dev)
    wt[:, torch.arange(R), torch.arange(R)] = 1.0                        # part s: W[k][c] = delta(k, c)
    xh = torch.zeros(T, N, 3 * H, device=dev)
    xh[:, :, :H] = 1.0
    ins = (xh, None, None, torch.zeros(N, H, device=dev), wt, torch.zeros(T, 3 * H, device=dev))
    x1, _ = _fwd(graph, rbf, H, ins, edge, None)
    has_edge = (graph.csr_rowptr[1:] - graph.csr_rowptr[:-1]) == 1
    rows = torch.nonzero(has_edge).flatten()
    e_of_row = graph.csr_rowptr[:-1][rows].long()
    assert rows.numel() == E
    k = (row[e_of_row].long() - 11)[:, None] + torch.arange(12, device=dev)[None, :]     # tap index of word m
    ok = (k >= 0) & (k < R)
    want = torch.zeros(E, R, device=dev)
    val = (taps[e_of_row, 12:13] * taps[e_of_row, :12]) * 0.70710678118654752
    for m in range(12):                                                  # (taps outside [0, R) meet zero rows)
        sel = ok[:, m]
        want[sel, k[sel, m]] = val[sel, m]
    assert torch.equal(x1[rows], want)
    assert float(want.abs().max()) > 0.1


def test_model_energy_and_forces_do_not_depend_on_the_records(monkeypatch):
    """alloy108: eager with the records, eager with them withheld, and the replayed step -- the same bits."""
    import hermnet_amd.hermnet as hmod
    from hermnet_amd.graph import GraphedStep
    from helpers import Golden
    dev = _dev()
    g = Golden("alloy108")
    model = g.model().to(dev)
    for prm in model.parameters():
        prm.requires_grad_(False)

    used = []

    def run(withhold):
        d = g.data().to(dev)
        d.pos.requires_grad_(True)
        if withhold:
            monkeypatch.setattr(hmod, "edge_radial_tables", lambda *a: (edge_radial_tables(*a)[0], None))
        e = model(d)
        used.append(d._hn_graph.fwd_taps is not None)
        f = -torch.autograd.grad(e.sum(), d.pos)[0]
        monkeypatch.undo()
        return e.detach().clone(), f.clone()

    e1, f1 = run(False)
    e0, f0 = run(True)
    assert used == [True, False]
    assert torch.equal(e1, e0) and torch.equal(f1, f0)
    d = g.data().to(dev)
    step = GraphedStep(model, d, warmup=2)
    eg, fg = step()
    assert d._hn_graph.fwd_taps is not None
    assert torch.equal(eg, e1) and torch.equal(fg, f1)
