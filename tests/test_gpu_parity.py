"""GPU parity tests proper (-m gpu): the HIP path, called through the C ABI, against
(a) a plain PyTorch restatement of each fused operator (op-level, localises bugs),
(b) the golden vectors of the reference, and (c) the CPU oracle on the same seeded inputs.

Tolerance (BASELINE.json north_star): energies and forces within 1e-5 relative
(forces relative to max|F|); neighbour indices bit-exact."""
import math
import os

import numpy as np

import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import synth
from hermnet_amd.ops import EdgeGeometry, MessageScatter
from hermnet_amd.relations import RelationalGraph
from hermnet_amd.elements import atomic_numbers
from helpers import Golden, SMALL_CASES, NONGAUSS_CASES, rel_err, judge_rows, row_err, FLT_MIN
import ref_ops

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _graph(g, dev):
    d = g.data().to(dev)
    zl = [atomic_numbers[e] for e in g.elems]
    graph = RelationalGraph.build(d.atomic_number, d.edge_index, zl,
                                  edge_shift=d.get("edge_shift") if d.get("cell") is not None else None,
                                  batch=d.batch)
    return d, graph


@pytest.mark.parametrize("name", ["c1_si64", "c1_si64_refcompat", "alloy108", "mol16"])
def test_edge_geometry_fwd_bwd(name):
    dev = _dev()
    g = Golden(name)
    d, graph = _graph(g, dev)
    pos = d.pos.clone().requires_grad_(True)
    edge = EdgeGeometry.apply(pos, d.get("cell"), graph)
    pos_r = d.pos.clone().requires_grad_(True)
    edge_r = ref_ops.geometry_ref(pos_r, graph, d.get("cell"))
    assert rel_err(edge[:, 3], edge_r[:, 3]) < 1e-6
    assert float((edge[:, :3] - edge_r[:, :3]).abs().max()) < 1e-6
    # backward contract: incoming gradient is dE/dD (Cartesian); check against index_add
    gD = torch.randn(graph.E, 4, device=dev)
    (gp,) = torch.autograd.grad(edge, pos, gD)
    ref = torch.zeros_like(d.pos).index_add_(0, graph.src_id.long(), gD[:, :3]).index_add_(0, graph.tgt_id.long(), -gD[:, :3])
    assert rel_err(gp, ref) < 1e-5


@pytest.mark.parametrize("bwd_form", ["channel-per-lane", "vw"])
@pytest.mark.parametrize("name,has_vec", [("c1_si64", True), ("c1_si64", False), ("c1_si64_refcompat", True),
                                          ("alloy108", True), ("alloy108_unknown_type", True),
                                          ("alloy108_h64", True), ("alloy32_h256", True), ("mol16", True)])
def test_message_scatter_op(name, has_vec, bwd_form):
    """Forward and backward of the fused operator vs the dense PyTorch restatement (fp64 reference); both forms of
    the backward kernel (with the per-edge radial table: one edge per wave, taps in SGPRs; without: 16 lanes per edge)."""
    from hermnet_amd.ops import edge_radial_table
    dev = _dev()
    g = Golden(name)
    d, graph = _graph(g, dev)
    model = g.model().to(dev)
    rbf = model.radial_basis.descriptor()
    H, R, T, N = model.hidden_channels, rbf.num_rbf, graph.T, graph.N
    gen = torch.Generator(device="cpu").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    xh, x = rnd(T, N, 3 * H), rnd(N, H)
    vec = rnd(N, 3, H) if has_vec else None
    wt = (rnd(T, R, 3 * H) / math.sqrt(R)).contiguous()
    brbf = (0.1 * rnd(T, 3 * H)).contiguous()
    edge = EdgeGeometry.apply(d.pos, d.get("cell"), graph)
    graph.edge_table = edge_radial_table(graph, rbf, edge) if bwd_form == "channel-per-lane" else None

    xh.requires_grad_(True); x.requires_grad_(True)
    if has_vec:
        vec.requires_grad_(True)
    edge_in = edge.detach().clone().requires_grad_(True)
    x1, vec1 = MessageScatter.apply(xh, vec, x, edge_in, wt, brbf, graph, rbf)

    # fp64 reference on the same inputs; edge enters as (rhat, d) = (D/|D|, |D|) of a free vector D
    D64 = (edge[:, :3] * edge[:, 3:4]).double().detach().requires_grad_(True)
    dn = D64.norm(dim=-1)
    e64 = torch.cat([D64 / dn[:, None], dn[:, None]], 1)
    xh64 = xh.detach().double().requires_grad_(True)
    x64 = x.detach().double().requires_grad_(True)
    v64 = vec.detach().double().requires_grad_(True) if has_vec else None

    class R64:  # rbf descriptor in fp64
        inv_rc, env_kind, env_p, offset = rbf.inv_rc, rbf.env_kind, rbf.env_p, rbf.offset.double()
    x1r, vec1r = ref_ops.message_scatter_ref(xh64, v64, x64, e64, wt.double(), brbf.double(), graph, R64)
    assert rel_err(x1.double(), x1r) < TOL, "x1"
    assert rel_err(vec1.double(), vec1r) < TOL, "vec1"

    gx1, gv1 = rnd(N, H), rnd(N, 3, H)
    ins = [xh, x, edge_in] + ([vec] if has_vec else [])
    grads = torch.autograd.grad([x1, vec1], ins, [gx1, gv1])
    ins_r = [xh64, x64, D64] + ([v64] if has_vec else [])
    grads_r = torch.autograd.grad([x1r, vec1r], ins_r, [gx1.double(), gv1.double()])
    names = ["gxh", "gx", "gD"] + (["gvec"] if has_vec else [])
    for nm, a, b in zip(names, grads, grads_r):
        a = a[:, :3] if nm == "gD" else a
        assert rel_err(a.double(), b) < 2 * TOL, nm


@pytest.mark.parametrize("name,has_vec", [("alloy108", True), ("alloy108_unknown_type", True), ("alloy108_h64", False),
                                          ("alloy32_h256", True), ("mol16", True)])
def test_message_kernels_over_complementary_row_ranges_are_bit_identical(name, has_vec):
    """Atom shards run the message kernels in two launches around the halo exchange ("run interior edges
    while the halo is in flight"): forward over complementary TARGET row ranges of every relation, backward over
    complementary SOURCE row ranges.  Poisoned buffers in between; together they must give bit for bit what one launch
    gives -- ragged, empty and whole-block ranges."""
    from hermnet_amd import layer as L
    from hermnet_amd.ops import edge_radial_table
    from test_host_logic import _layer_weights_and_graph
    dev = _dev()
    g = Golden(name)
    d, graph = _graph(g, dev)
    model = g.model().to(dev)
    rbf = model.radial_basis.descriptor()
    H, R, T, N = model.hidden_channels, rbf.num_rbf, graph.T, graph.N
    gen = torch.Generator(device="cpu").manual_seed(4)
    rnd = lambda *s_: torch.randn(*s_, generator=gen).to(dev)
    xh, x = rnd(T, N, 3 * H), rnd(N, H)
    vec = rnd(N, 3, H) if has_vec else None

    class W:          # what layer._msg_fwd / _msg_bwd read of LayerWeights
        wt = (rnd(T, R, 3 * H) / math.sqrt(R)).contiguous()
        brbf = (0.1 * rnd(T, 3 * H)).contiguous()
        b2 = None
    edge = EdgeGeometry.apply(d.pos, d.get("cell"), graph).detach()
    graph.edge_table = edge_radial_table(graph, rbf, edge)
    rp = list(graph.type_rowptr_host)
    x1, vec1 = L._msg_fwd(graph, rbf, H, xh, vec, x, W, edge, xh_bias=False)
    cuts = [[rp[t], rp[t] + (rp[t + 1] - rp[t]) * k // 3, rp[t + 1]] for t, k in zip(range(T), [1, 0, 3, 2])]
    early = torch.tensor([[c[0], c[1]] for c in cuts], dtype=torch.int32, device=dev)
    late = torch.tensor([[c[1], c[2]] for c in cuts], dtype=torch.int32, device=dev)
    nan = lambda t_: torch.full_like(t_, float("nan"))
    n_early = sum(c[1] - c[0] for c in cuts)
    part = L._msg_fwd(graph, rbf, H, xh, vec, x, W, edge, xh_bias=False, ranges=early, zero_unknown=True, out=(nan(x1), nan(vec1)),
                      range_rows=n_early)
    esel = torch.zeros(N, dtype=torch.bool, device=dev)
    for c in cuts:
        esel[c[0]:c[1]] = True
    esel[rp[-1]:] = True
    assert torch.equal(part[0][esel], x1[esel]) and bool(torch.isnan(part[0][~esel]).all())
    both = L._msg_fwd(graph, rbf, H, xh, vec, x, W, edge, xh_bias=False, ranges=late, zero_unknown=False, out=part,
                      range_rows=rp[T] - n_early)
    assert torch.equal(both[0], x1) and torch.equal(both[1], vec1)

    gx1, gv1 = rnd(N, H), rnd(N, 3, H)
    ge = torch.full((H // 64, graph.E, 4), float("nan"), device=dev)     # (edges into unknown-element rows stay unwritten)
    gxh, gvec, gx = L._msg_bwd(graph, rbf, H, xh, vec, W, edge, gx1, gv1, ge, xh_bias=False)
    same = lambda p_, q_: bool(((p_ == q_) | (torch.isnan(p_) & torch.isnan(q_))).all())
    a, b, c_ = N // 5, min(N // 5 + 37, N - 5), N - 3
    for first, rest in [([(a, b), (c_, N)], [(0, a), (b, c_)]), ([(0, N)], []), ([(0, 1)], [(1, N)])]:
        ge2 = nan(ge)
        dv = lambda r: torch.tensor(r, dtype=torch.int32, device=dev).reshape(-1, 2)
        bufs = L._msg_bwd(graph, rbf, H, xh, vec, W, edge, gx1, gv1, ge2, xh_bias=False, ranges=(dv(first), first),
                          out=(nan(gxh), None if gvec is None else nan(gvec), nan(gx),
                               None if (vec is None or T == 1) else torch.full((T,) + tuple(vec.shape), float("nan"), device=dev)))
        fsel = torch.zeros(N, dtype=torch.bool, device=dev)
        for lo, hi in first:
            fsel[lo:hi] = True
        assert torch.equal(bufs[0][:, fsel], gxh[:, fsel]) and torch.equal(bufs[2][fsel], gx[fsel])
        assert bool(torch.isnan(bufs[2][~fsel]).all())
        if rest:
            bufs = L._msg_bwd(graph, rbf, H, xh, vec, W, edge, gx1, gv1, ge2, xh_bias=False, ranges=(dv(rest), rest), out=bufs)
        assert torch.equal(bufs[0], gxh) and torch.equal(bufs[2], gx) and same(ge2, ge)
        if gvec is not None:
            assert torch.equal(bufs[1], gvec)


@pytest.mark.parametrize("name", SMALL_CASES + NONGAUSS_CASES)
def test_hvnet_matches_reference_golden(name):
    """Energy + forces of the HIP path vs the reference's own outputs (golden fixtures)."""
    dev = _dev()
    g = Golden(name)
    model = g.model().to(dev)
    d = g.data().to(dev)
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    assert rel_err(e.detach().cpu(), g.energy) < TOL, (e, g.energy)
    assert rel_err(f.cpu(), g.forces) < TOL


@pytest.mark.parametrize("name", ["c1_si64", "alloy108"])
def test_hvnet_layer_intermediates(name):
    dev = _dev()
    g = Golden(name)
    model = g.model().to(dev)
    d = g.data().to(dev)
    outs = []
    hooks = [c.register_forward_hook(lambda m, i, o: outs.append((o.x.detach().clone(), o.vec.detach().clone())))
             for c in model.hermconvs]
    with torch.no_grad():
        model(d)
    order = d._hn_graph.row_of_node
    for l, (x, v) in enumerate(outs):
        xr = torch.from_numpy(g.arrays["x_l%d" % l])
        vr = torch.from_numpy(g.arrays["vec_l%d" % l])
        assert rel_err(x[order].cpu(), xr) < TOL, "x layer %d" % l
        assert rel_err(v[order].cpu(), vr) < TOL, "vec layer %d" % l
    for h in hooks:
        h.remove()


def test_config2_10k_atoms_matches_reference_golden():
    """BASELINE.json configs[1] at full size against the reference's forces (golden, 10k atoms)."""
    dev = _dev()
    g = Golden("c2_alloy10k")
    model = g.model().to(dev)
    d = g.data(regenerate_graph=lambda: synth.fcc_alloy()).to(dev)
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    assert rel_err(e.detach().cpu(), g.energy) < TOL, (e, g.energy)
    assert rel_err(f.cpu(), g.forces) < TOL
    # size-independent properties: momentum conservation and run-to-run bit reproducibility
    assert float(f.sum(0).abs().max()) < 1e-3
    d2 = g.data(regenerate_graph=lambda: synth.fcc_alloy()).to(dev)
    d2.pos.requires_grad_(True)
    e2 = model(d2)
    f2 = -torch.autograd.grad(e2.sum(), d2.pos)[0]
    assert torch.equal(e, e2) and torch.equal(f, f2), "segmented sums must be deterministic"


def _batch_periodic(parts):
    """Concatenate periodic single-cell `Data` objects into one batch (cell [B,3,3], per-graph `batch`)."""
    off, pos, z, ei, sh, cell, b = 0, [], [], [], [], [], []
    for g, d in enumerate(parts):
        pos.append(d.pos); z.append(d.atomic_number); ei.append(d.edge_index + off); sh.append(d.edge_shift)
        cell.append(d.cell.reshape(1, 3, 3)); b.append(torch.full((d.pos.size(0),), g, dtype=torch.long))
        off += d.pos.size(0)
    return hn.Data(pos=torch.cat(pos), atomic_number=torch.cat(z), edge_index=torch.cat(ei, 1), edge_shift=torch.cat(sh),
                   cell=torch.cat(cell), batch=torch.cat(b))


@pytest.mark.parametrize("intensive", [False, True])
def test_batch_of_different_periodic_cells_matches_oracle(intensive):
    """`edge_shift @ cell[batch[j]]` (hermnet.py:139) with a different cell per graph, per-graph read-out, and the
    cell gradient (virial path) per graph."""
    from oracle import hermnet_oracle as orc
    dev = _dev()
    data = _batch_periodic([synth.si_diamond(), synth.fcc_alloy(reps=(2, 2, 3), rc=5.0), synth.si_diamond(reps=(1, 1, 2), seed=3)])
    elems = ["Si", "Al", "Ni", "Cu"]
    kw = dict(rc=5.0, num_layers=3, hidden_channels=128, num_rbf=64, intensive=intensive)
    model = hn.HVNet(elems, **kw).eval()
    sd = synth.synth_state_dict(model.state_dict(), 21)
    model.load_state_dict(sd)
    e_ref, f_ref = orc.energy_and_forces(sd, elems, data, **kw)
    # oracle's cell gradient (fp32 autograd on the CPU)
    cell_r = data.cell.clone().requires_grad_(True)
    e_c = orc.hvnet_energy(sd, elems, data.pos, data.atomic_number, data.edge_index, data.batch, data.edge_shift, cell_r, **kw)
    gcell_ref = torch.autograd.grad(e_c.sum(), cell_r)[0]
    model = model.to(dev)
    d = data.to(dev)
    d.pos.requires_grad_(True)
    d.cell.requires_grad_(True)
    e = model(d)
    f, gcell = torch.autograd.grad(e.sum(), [d.pos, d.cell])
    assert e.shape == (3,)
    assert rel_err(e.detach().cpu(), e_ref) < TOL and rel_err(-f.cpu(), f_ref) < TOL
    assert rel_err(gcell.cpu(), gcell_ref) < 5 * TOL


def test_cpu_tensor_is_refused():
    g = Golden("c1_si64")
    model = g.model()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(g.data())


def test_node_kernels_match_pytorch_restatement():
    """Each fused node-level kernel (csrc/node_kernels.hip) vs tests/ref_ops.py, fp32, incl. zero rows."""
    from hermnet_amd import nodeops
    dev = _dev()
    gen = torch.Generator().manual_seed(5)
    N, nk, H, T = 37, 30, 128, 3
    rnd = lambda *s: torch.randn(*s, generator=gen)
    c = lambda t: None if t is None else t.to(dev)
    h = rnd(N, T * H)
    assert rel_err(nodeops.ssilu_fwd(c(h)).cpu(), ref_ops.ssilu_fwd(h)) < 1e-6
    g_tn = rnd(T, N, H)
    out = nodeops.ssilu_bwd(c(g_tn), c(h), N, T, H, H, N * H).cpu()
    assert rel_err(out, ref_ops.ssilu_bwd(g_tn, h, N, T, H, H, N * H)) < 1e-6
    vp, x1, vec1, q = rnd(N, 3, 2 * H), rnd(N, H), rnd(N, 3, H), rnd(N, 3 * H)
    mask = (torch.arange(N) % 5 != 0).float()
    vd, xin = nodeops.update_mid(c(vp), c(x1), nk, H)
    vd_r, xin_r = ref_ops.update_mid(vp, x1, nk, H)
    assert rel_err(vd.cpu()[:nk], vd_r[:nk]) < 1e-6 and rel_err(xin.cpu()[:nk], xin_r[:nk]) < 1e-6
    for m in (None, mask):
        xo, vo = nodeops.update_out(c(q), c(vd_r), c(vp), c(x1), c(vec1), c(m), N, nk, H)
        xo_r, vo_r = ref_ops.update_out(q, vd_r, vp, x1, vec1, m, N, nk, H)
        assert rel_err(xo.cpu(), xo_r) < 1e-6 and rel_err(vo.cpu(), vo_r) < 1e-6
        gxo, gvo = rnd(N, H), rnd(N, 3, H)
        outs = nodeops.update_out_bwd(c(gxo), c(gvo), c(q), c(vd_r), c(vp), c(m), N, nk, H)
        refs = ref_ops.update_out_bwd(gxo, gvo, q, vd_r, vp, m, N, nk, H)
        for k, (a, b) in enumerate(zip(outs, refs)):
            a = a.cpu()
            if k == 2:      # gvp: only the v1 half of the known rows is defined at this point
                a, b = a[:nk, :, :H], b[:nk, :, :H]
            elif k in (0, 1):
                a, b = a[:nk], b[:nk]
            assert rel_err(a, b) < 1e-6, k
        gq, gvdot, gvp, gx1, gvec1 = refs
        gxin = rnd(N, 2 * H)
        gvp_d, gx1_d = c(gvp.clone()), c(gx1.clone())
        nodeops.update_mid_bwd(c(gvdot), c(gxin), c(vp), c(xin_r), gvp_d, gx1_d, nk, H)
        ref_ops.update_mid_bwd(gvdot, gxin, vp, xin_r, gvp, gx1, nk, H)
        assert rel_err(gvp_d.cpu()[:nk], gvp[:nk]) < 1e-6 and rel_err(gx1_d.cpu(), gx1) < 1e-6


@pytest.mark.parametrize("H,T,counts,uniform,hr", [(128, 3, (70, 91, 45), None, 0), (128, 3, (130, 3, 61), False, 0),
                                                   (64, 2, (100, 77), None, 50), (256, 3, (40, 33, 50), None, 0),
                                                   (128, 1, (300,), None, 0), (128, 3, (4000, 3900, 4100), None, 0),
                                                   (128, 3, (7000, 7100, 6900), None, 0),
                                                   # every other multiple of 64 up to the reference's default width
                                                   # (csrc/node_chain_wide.hip; odd multiples leave a round half empty)
                                                   (192, 3, (40, 33, 50), None, 0), (320, 2, (70, 29), None, 0),
                                                   (384, 3, (33, 64, 31), False, 0), (448, 2, (50, 41), None, 0),
                                                   (512, 3, (40, 33, 50), None, 0), (512, 1, (700,), None, 0),
                                                   # a padded width whose second column block is partly empty: 100 -> 128
                                                   (128, 3, (70, 91, 45), None, 100)])
def test_node_chain_kernels_match_restatement(H, T, counts, uniform, hr):
    _node_chain_case(H, T, counts, uniform, hr)


@pytest.mark.parametrize("H,T,counts,uniform", [(128, 3, (70, 91, 45), None), (128, 3, (130, 3, 61), False), (128, 1, (300,), None),
                                                (128, 3, (3300, 3400, 3341), None)])
def test_update_chain_on_16_row_tiles_matches_restatement(H, T, counts, uniform, monkeypatch):
    """csrc/node_chain16.hip: the PaiNNUpdate chain and its backward on 16-row tiles (v_mfma_f32_16x16x4_f32, frag16
    weight copies) -- the form the library picks for grids that 32-row tiles quantise badly (10,041 rows: 314 tiles on 256
    CUs) -- forced here for every layout, vs the fp64 restatement; and the library's own choice for configs[1]'s row counts."""
    from hermnet_amd import nodeops, _lib
    monkeypatch.setattr(nodeops, "update_tile_rows", lambda graph, H_: 16)
    _node_chain_case(H, T, counts, uniform, 0)
    monkeypatch.undo()
    import ctypes
    rp = (ctypes.c_int * 4)(0, 3347, 6694, 10041)
    assert _lib.load().hermnet_node_update_tile_rows(rp, 10041, 3, 128) == 16       # configs[1]
    rp = (ctypes.c_int * 4)(0, 33800, 67600, 101397)
    assert _lib.load().hermnet_node_update_tile_rows(rp, 101397, 3, 128) == 32      # configs[3]: weight traffic wins


@pytest.mark.parametrize("T,counts,uniform", [(3, (70, 91, 45), None), (3, (130, 3, 61), False), (1, (300,), None),
                                              (3, (3300, 3400, 3341), None)])
def test_layer_boundary_as_one_node_launch_each_way(T, counts, uniform, monkeypatch):
    """Round 5 (rmnet.py:29-31, 94-107 then :52 of the next layer): csrc/node_chain16.hip.
    (i)  The node projection and its backward on 16-row tiles (`hermnet_node_pre_fwd16` / `_bwd16`) vs the fp64 restatement.
    (ii) `hermnet_node_update_pre_fwd` -- a tile's update and the NEXT layer's projection of the rows it has just produced in
         ONE launch -- equals update (16-row form) + pre_fwd16 bit for bit, every output buffer NaN-poisoned beforehand; rows
         of unknown elements and of an inactive relation included (their projection runs on x = 0).
    (iii) `hermnet_node_update_bwd` with `pending->gxh` -- the projection's backward of the layer above inside the update
         backward, sums over the relations in registers, LayerNorm backward on the tile -- equals pre_bwd16 + the `gn_parts`
         form bit for bit (poisoned gx_out / gvec_out), and the fp64 restatement to rounding."""
    from test_host_logic import _layer_weights_and_graph
    from hermnet_amd import nodeops
    import copy
    H = 128
    dev = _dev()
    monkeypatch.setattr(nodeops, "update_tile_rows", lambda graph, H_: 16)
    w, g = _layer_weights_and_graph(H, T, counts, uniform=uniform, unknown=5)
    w2_, _ = _layer_weights_and_graph(H, T, counts, seed=7, uniform=uniform, unknown=5)      # the next layer's weights
    gen = torch.Generator().manual_seed(3)
    N = g.N
    rnd = lambda *s_: torch.randn(*s_, generator=gen)
    x1, vec1 = rnd(N, H), rnd(N, 3, H)

    def on_dev(w_):
        wd_ = copy.copy(w_)
        for k, v in vars(w_).items():
            if torch.is_tensor(v):
                setattr(wd_, k, v.to(dev))
        return wd_
    wd, wn = on_dev(w), on_dev(w2_)
    gd = copy.copy(g)
    gd.row_active, gd.type_rowptr = g.row_active.to(dev), g.type_rowptr.to(dev)
    gd._rowptr_c = None
    c = lambda t: t.to(dev)
    d64 = lambda t: t.double()
    assert nodeops.fused_boundary_supported(gd, H, wd, wn)
    # ---- (i) the projection phases as kernels of their own
    x = rnd(N, H)
    hb, xh, mean, rstd = nodeops.node_pre_fwd16(c(x), wn, T)
    hb_r, xh_r, mean_r, rstd_r = ref_ops.node_pre_fwd(d64(x), w2_, T)
    assert rel_err(hb.cpu().double(), hb_r) < 2e-6 and rel_err(xh.cpu().double(), xh_r) < 2e-6
    assert rel_err(mean.cpu().double(), mean_r) < 2e-6 and rel_err(rstd.cpu().double(), rstd_r) < 2e-6
    gxh = rnd(T, N, 3 * H) * 0.3
    parts = nodeops.node_pre_bwd16(c(gxh), hb, wn)
    parts_r = ref_ops.node_pre_bwd(d64(gxh), hb_r, d64(x), mean_r, rstd_r, w2_, parts_only=True)
    assert rel_err(parts.cpu().double(), parts_r) < 5e-6
    # ---- (ii) forward: fused == update + projection, bit for bit
    xo, vo, vp, h2b, q23, nrm = nodeops.node_update_fwd(c(x1), c(vec1), wd, gd)
    pre_u = nodeops.node_pre_fwd16(xo, wn, T)
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real_empty(*a, **k).fill_(float("nan"))
                        if k.get("dtype", torch.float32).is_floating_point else real_empty(*a, **k))
    fused = nodeops.node_update_pre_fwd(c(x1), c(vec1), wd, gd, wn)
    monkeypatch.setattr(torch, "empty", real_empty)
    nk = g.type_rowptr_host[-1]
    for k_, (a, b) in enumerate(zip(fused[:6], (xo, vo, vp, h2b, q23, nrm))):
        if k_ >= 2:                     # saved tensors: defined on the rows of known elements
            a, b = a[:nk], b[:nk]
        assert torch.equal(a, b), k_
    for a, b in zip(fused[6], pre_u):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # (and against the restatement through both stages)
    refs = ref_ops.node_update_fwd(d64(x1), d64(vec1), w, g)
    pre_r = ref_ops.node_pre_fwd(refs[0], w2_, T)
    assert rel_err(fused[6][1].cpu().double(), pre_r[1]) < 5e-6
    # ---- (iii) backward: fused == pre_bwd16 + the partial-sum form, bit for bit
    hb2, xh2, mean2, rstd2 = fused[6]
    gv_parts, gx1_up, gvec1_up = c(rnd(T, N, 3, H)), c(rnd(N, H)), c(rnd(N, 3, H))
    gxh_d = c(gxh)
    gn_parts = nodeops.node_pre_bwd16(gxh_d, hb2, wn)
    nan = lambda *s_: torch.full(s_, float("nan"), device=dev)
    bx, bv = nan(N, H), nan(N, 3, H)
    want = nodeops.node_update_bwd(bx, bv, vp, h2b, q23, nrm, wd, gd,
                                   pending=nodeops.PendingGrads(bx, bv, gn_parts, gv_parts, xo, mean2, rstd2, gx1_up, gvec1_up, 0))
    fx, fv = nan(N, H), nan(N, 3, H)
    got = nodeops.node_update_bwd(fx, fv, vp, h2b, q23, nrm, wd, gd,
                                  pending=nodeops.PendingGrads(fx, fv, None, gv_parts, xo, mean2, rstd2, gx1_up, gvec1_up, 0,
                                                               chain=(gxh_d, hb2, wn.w2tf16, wn.w1tf16)))
    assert torch.equal(fx[:nk], bx[:nk]) and torch.equal(fv[:nk], bv[:nk])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    # restatement: LayerNorm backward over the summed parts + the residual's identity term, then the update backward
    ident = (torch.arange(N) < nk).double()
    gn_r = ref_ops.node_pre_bwd(d64(gxh), pre_r[0], refs[0], pre_r[2], pre_r[3], w2_, parts_only=True).sum(0)
    gxo_r = ref_ops.layernorm_bwd(gn_r, refs[0], pre_r[2], pre_r[3], add=gx1_up.cpu().double() * ident[:, None] / math.sqrt(2.0))
    gvo_r = gv_parts.cpu().double().sum(0) + gvec1_up.cpu().double() * ident[:, None, None]
    gx1_r, gvec1_r = ref_ops.node_update_bwd(gxo_r, gvo_r, refs[2], refs[3], refs[4], refs[5], w, g)
    assert rel_err(got[0].cpu().double(), gx1_r) < 1e-5 and rel_err(got[1].cpu().double(), gvec1_r) < 1e-5


@pytest.mark.parametrize("name", ["alloy108", "c1_si64", "alloy108_unknown_type", "mol16"])
def test_fused_layer_boundary_changes_no_bit_of_the_model(name, monkeypatch):
    """Model level: `switches.boundary_mode` = 1 (one node launch per layer boundary each way) gives bit for bit the
    energies and forces of the same 16-row phases run as separate launches (= 2), with every buffer the consuming launches
    must fill NaN-poisoned; the default form (= 0: 64-row projection kernels, another summation order) agrees to rounding;
    all three meet the reference's golden."""
    from hermnet_amd import switches
    dev = _dev()
    g = Golden(name)
    model = g.model().to(dev)
    out = {}
    monkeypatch.setenv("HERMNET_DEBUG_POISON", "1")
    for mode in ("1", "2", "0"):
        monkeypatch.setattr(switches, "boundary_mode", int(mode))
        d = g.data().to(dev)
        d.pos.requires_grad_(True)
        e = model(d)
        f = -torch.autograd.grad(e.sum(), d.pos)[0]
        out[mode] = (e.detach().clone(), f.clone())
        assert rel_err(e.detach().cpu(), g.energy) < TOL and rel_err(f.cpu(), g.forces) < TOL, mode
    assert torch.equal(out["1"][0], out["2"][0]) and torch.equal(out["1"][1], out["2"][1])
    assert rel_err(out["1"][0], out["0"][0]) < 2e-6 and rel_err(out["1"][1], out["0"][1]) < 5e-6


@pytest.mark.parametrize("rows", [1, 16, 333, 10041])
def test_read_out_on_the_matrix_pipe_matches_the_staged_weight_form(rows, monkeypatch):
    """hermnet_energy_head16_fwd / _bwd (hermnet.py:112-116,129 with its 128 -> 64 product on v_mfma_f32_16x16x4_f32) vs the
    round-3 kernels (weights staged in LDS, VALU) and vs the fp64 torch expression: per-row energies, saved pre-activations,
    the gradient w.r.t. x; a row mask; row counts that leave the last tile ragged."""
    from hermnet_amd.layer import EnergyHead
    dev = _dev()
    gen = torch.Generator().manual_seed(rows)
    H, C = 128, 64
    x = torch.randn(rows, H, generator=gen)
    w0, b0 = torch.randn(C, H, generator=gen) * 0.2, torch.randn(C, generator=gen) * 0.2
    w2, b2 = torch.randn(1, C, generator=gen) * 0.3, torch.randn(1, generator=gen)
    mask = (torch.rand(rows, generator=gen) > 0.2).float()
    ge = torch.randn(rows, generator=gen)
    xd = x.double().requires_grad_(True)
    hr = xd @ w0.double().t() + b0.double()
    er = ((torch.nn.functional.silu(hr) / 0.6) @ w2.double().t()).squeeze(1) + b2.double()
    er = er * mask.double()
    (gr,) = torch.autograd.grad(er, xd, ge.double())
    out = {}
    from hermnet_amd import nodeops
    for flag in ("1", "0"):
        if flag == "0":       # (the staged-weight VALU form: what widths without the 16-row read-out take)
            monkeypatch.setattr(nodeops, "head16_supported", lambda H_, C_: False)
        xg = x.to(dev).requires_grad_(True)
        e = EnergyHead.apply(xg, w0.to(dev), b0.to(dev), w2.to(dev), b2.to(dev), mask.to(dev))
        (g,) = torch.autograd.grad(e, xg, ge.to(dev))
        out[flag] = (e.detach().cpu(), g.cpu())
        assert rel_err(e.detach().cpu().double(), er.detach()) < 2e-6 and rel_err(g.cpu().double(), gr) < 2e-6, flag
    assert rel_err(out["1"][0], out["0"][0]) < 2e-6 and rel_err(out["1"][1], out["0"][1]) < 2e-6


def _node_chain_case(H, T, counts, uniform, hr):
    """csrc/node_chain.hip (LayerNorm + x_proj chain, PaiNNUpdate chain and their backward kernels on the fp32 matrix
    pipe) vs the fp64 PyTorch restatement of tests/ref_ops.py: ragged relation blocks, an inactive relation, rows of
    unknown elements, zero-padded channels (hidden_real).  Through the nodeops wrappers, so the library picks the instances: at
    H = 128 the 64-row projection kernels and the 32-row update kernels (16-row ones where test_update_chain_on_16_row_tiles
    forces them) -- NOT the 64-row update instances node_update_fwd / _bwd_kernel<128, 64, 1>, which run only above option
    update_tile64_max = 0; tests/test_chain_rows.py runs those, and every other compiled instance, by name."""
    from test_host_logic import _layer_weights_and_graph
    from hermnet_amd import nodeops
    dev = _dev()
    # hr: modules of hidden_channels = hr, which layer.LayerWeights.refresh pads to H itself (zero rows / columns in every
    # weight, h_real = hr for the LayerNorm statistics); the operands carry zeros in the padded channels
    w, g = _layer_weights_and_graph(hr or H, T, counts, uniform=uniform, unknown=5)
    assert w.h_real == hr and w.w1cat.size(1) == H
    gen = torch.Generator().manual_seed(2)
    N = g.N
    chan = torch.zeros(H)
    chan[:hr or H] = 1.0
    rnd = lambda *s_: torch.randn(*s_, generator=gen) * chan.repeat(s_[-1] // H)
    x, x1, vec1 = rnd(N, H), rnd(N, H), rnd(N, 3, H)
    gxh, gxo, gvo, add = rnd(T, N, 3 * H) * 0.3, rnd(N, H), rnd(N, 3, H), rnd(N, H)
    pad = chan == 0

    def padded_channels_are_zero(*outs):
        """Padded channels are exactly zero in everything the kernels hand on ([.., parts * H] arrays part by part)."""
        for t_ in outs:
            assert not bool(t_.reshape(-1, H)[:, pad.to(t_.device)].any())
    # device copies of the weights and the graph
    import copy
    wd = copy.copy(w)
    for k, v in vars(w).items():
        if torch.is_tensor(v):
            setattr(wd, k, v.to(dev))
    gd = copy.copy(g)
    gd.row_active, gd.type_rowptr = g.row_active.to(dev), g.type_rowptr.to(dev)
    gd._rowptr_c = None
    c = lambda t: t.to(dev)
    d64 = lambda t: t.double()
    hb, xh, mean, rstd = nodeops.node_pre_fwd(c(x), wd, T)
    hb_r, xh_r, mean_r, rstd_r = ref_ops.node_pre_fwd(d64(x), w, T)
    assert rel_err(hb.cpu().double(), hb_r) < 2e-6 and rel_err(xh.cpu().double(), xh_r) < 2e-6
    assert rel_err(mean.cpu().double(), mean_r) < 2e-6 and rel_err(rstd.cpu().double(), rstd_r) < 2e-6
    padded_channels_are_zero(hb, xh)
    for a in (None, add):
        gx = nodeops.node_pre_bwd(c(gxh), hb, c(x), mean, rstd, wd, add=None if a is None else c(a))
        gx_r = ref_ops.node_pre_bwd(d64(gxh), hb_r, d64(x), mean_r, rstd_r, w, add=None if a is None else d64(a))
        assert rel_err(gx.cpu().double(), gx_r) < 5e-6
        padded_channels_are_zero(gx)
    # row windows (atom shards: the halo exchange sits between two launches that partition the row tiles): the tiles
    # outside the windows, then the tiles that touch one, give bit for bit what one launch gives -- poisoned buffers
    # in between, windows that are empty, ragged and straddling a tile border
    win = torch.tensor([[0, 0], [N // 3 - 5, N // 3 + 9], [N - 3, N]], dtype=torch.int32, device=dev)
    sel = ref_ops._tile_rows(N, H, win.cpu(), 1, torch.device("cpu"))
    assert bool(sel.any()) and (N <= 128 or not bool(sel.all()))
    part = nodeops.node_pre_fwd(c(x), wd, T, windows=win, mode=2, out=tuple(torch.full_like(t_, float("nan")) for t_ in (hb, xh, mean, rstd)))
    assert bool(torch.isnan(part[1][:, sel.to(dev)]).all()) and bool(torch.equal(part[1][:, ~sel.to(dev)], xh[:, ~sel.to(dev)]))
    full = nodeops.node_pre_fwd(c(x), wd, T, windows=win, mode=1, out=part)
    for a, b in zip(full, (hb, xh, mean, rstd)):
        assert torch.equal(a, b)
    poison = (torch.full_like(gx, float("nan")), torch.full((T, N, H), float("nan"), device=dev))
    first = nodeops.node_pre_bwd(c(gxh), hb, c(x), mean, rstd, wd, add=c(add), windows=win, mode=1, out=poison)
    assert bool(torch.equal(first[0][sel.to(dev)], gx[sel.to(dev)])) and bool(torch.isnan(first[0][~sel.to(dev)]).all())
    both = nodeops.node_pre_bwd(c(gxh), hb, c(x), mean, rstd, wd, add=c(add), windows=win, mode=2, out=first)
    assert torch.equal(both[0], gx)
    xo, vo, vp, h2b, q23, nrm = nodeops.node_update_fwd(c(x1), c(vec1), wd, gd)
    refs = ref_ops.node_update_fwd(d64(x1), d64(vec1), w, g)
    nk = g.type_rowptr_host[-1]
    for k, (a, b) in enumerate(zip((xo, vo, vp, h2b, q23, nrm), refs)):
        a = a.cpu().double()
        if k >= 2:                      # saved tensors: defined on the rows of known elements
            a, b = a[:nk], b[:nk]
            real = (g.row_real[:nk] != 0) if g.row_real is not None else slice(None)
            a, b = a[real], b[real]
        assert rel_err(a, b) < 3e-6, k
    # (nrm = sqrt(|v2|^2 + 1e-8) is 1e-4 in a padded channel, in the kernel as in the restatement: the zero columns of
    # xvec_proj[0] take it out of everything behind it)
    rows = real.to(dev) if torch.is_tensor(real) else real
    padded_channels_are_zero(xo, vo, *(t_[:nk][rows] for t_ in (vp, h2b, q23)))   # (saved tensors: rows of known elements)
    gx1, gvec1 = nodeops.node_update_bwd(c(gxo), c(gvo), vp, h2b, q23, nrm, wd, gd)
    gx1_r, gvec1_r = ref_ops.node_update_bwd(d64(gxo), d64(gvo), refs[2], refs[3], refs[4], refs[5], w, g)
    assert rel_err(gx1.cpu().double(), gx1_r) < 5e-6 and rel_err(gvec1.cpu().double(), gvec1_r) < 5e-6
    assert torch.isfinite(gx1).all() and torch.isfinite(gvec1).all()
    padded_channels_are_zero(gx1, gvec1)


# ---- parity MARGIN: the goldens assert < 1e-5; these fail at HALF of it, so a precision trade (a trimmed
# tap, a reordered sum, a dropped partial product) turns a margin test red long before it turns a golden red
MARGIN_ENERGY, MARGIN_FORCES = 2.5e-6, 5.0e-6


@pytest.mark.parametrize("name", SMALL_CASES + ["c2_alloy10k"])
def test_parity_margin_against_reference_goldens(name):
    """Every golden of the reference's own code (tests/golden/*.npz, incl. configs[1] at full size): energy within 2.5e-6,
    forces within 5e-6 of max |F| -- half of BASELINE.json's 1e-5.  Round 5 measured 1.8e-6 / 4.2e-6 at worst
    (profiles/r05_parity_margin.log)."""
    dev = _dev()
    g = Golden(name)
    model = g.model().to(dev)
    d = (g.data(regenerate_graph=lambda: synth.fcc_alloy()) if name == "c2_alloy10k" else g.data()).to(dev)
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    ee, fe = rel_err(e.detach().cpu(), g.energy), rel_err(f.cpu(), g.forces)
    print("parity margin %-24s energy %.2e forces %.2e" % (name, ee, fe))
    assert ee < MARGIN_ENERGY, (name, ee)
    assert fe < MARGIN_FORCES, (name, fe)


@pytest.mark.parametrize("H,T,counts,tile16", [(128, 3, (70, 91, 45), False), (128, 3, (70, 91, 45), True), (256, 2, (60, 45), False),
                                               (512, 2, (40, 33), False)])
def test_node_chain_kernels_on_adversarial_operands(H, T, counts, tile16, monkeypatch):
    """The node chain kernels run every product as a three-way bf16 split on the bf16 matrix pipe (csrc/node_chain_common.h:
    split8, mma_panel; node_chain16.hip: mma16_panel) and claim fp32-equivalent results.  Operands chosen to break a sloppier
    scheme, every ROW judged on its own scale (`helpers.row_err`) against the fp64 restatement:
      * per-row scales from 1e-12 to 1e+12 (x: LayerNorm input; gradients) and 1e-6 ... 1e+6 (vec: its square enters vdot),
      * cancelling rows: a constant offset of 1e3 under unit noise (LayerNorm's mean removal), vec rows whose channels
        alternate in sign so that the vec_proj sums cancel,
      * rows of the linear backward chain at 1e-30 (the third bf16 plane of such a value sits at 1e-35, just above the bf16
        denormals: below ~1e-33 the residual planes flush and a row keeps >= 8 significant bits -- documented, not tested).
    Bound per row: the kernels' usual 5e-6 (2e-6 forward), or 8 x the error a plain fp32 evaluation of the same chain makes on
    that row, whichever is larger -- cancellation costs fp32 itself digits (and how many depends on the order of a sum: the
    kernels' LayerNorm and torch's reduce a row in different trees); the split products must not cost more.
    Behind them, as further rows of the update chain: the tail of ScaledSiLU (`_chain_tail_rows`; measured on the MI355X:
    worst row 6.3e-7 at H = 128, 6.4e-7 at 256, 9.4e-7 at 512, against a derived bound of 1.25e-5)."""
    from test_host_logic import _layer_weights_and_graph
    from hermnet_amd import nodeops
    import copy
    dev = _dev()
    if tile16:
        monkeypatch.setattr(nodeops, "update_tile_rows", lambda graph, H_: 16)
    w, g = _layer_weights_and_graph(H, T, counts, uniform=None, unknown=5)
    w.h_real = 0
    gen = torch.Generator().manual_seed(11)
    N = g.N
    rnd = lambda *s_: torch.randn(*s_, generator=gen)
    scale = lambda n, lo, hi: 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen))
    x = rnd(N, H) * scale(N, -12, 12)[:, None]
    x[::7] = 1.0e3 + rnd(x[::7].shape[0], H)                                   # LayerNorm removes 1e3 under unit noise
    x1 = rnd(N, H) * scale(N, -6, 6)[:, None]
    alt = torch.tensor([1.0, -1.0]).repeat(H // 2)
    vec1 = rnd(N, 3, H) * scale(N, -6, 6)[:, None, None]
    vec1[::5] = (alt[None, None, :] + 1e-3 * rnd(vec1[::5].shape[0], 3, H)) * scale(vec1[::5].shape[0], -3, 3)[:, None, None]
    gxh = rnd(T, N, 3 * H) * scale(N, -12, 12)[None, :, None]
    gxh[:, ::9] = rnd(T, gxh[:, ::9].shape[1], 3 * H) * 1.0e-30
    gxo, gvo = rnd(N, H) * scale(N, -6, 6)[:, None], rnd(N, 3, H) * scale(N, -6, 6)[:, None, None]
    wd = copy.copy(w)
    for k, v in vars(w).items():
        if torch.is_tensor(v):
            setattr(wd, k, v.to(dev))
    gd = copy.copy(g)
    gd.row_active, gd.type_rowptr = g.row_active.to(dev), g.type_rowptr.to(dev)
    gd._rowptr_c = None
    c = lambda t: t.to(dev)
    d64 = lambda t: t.double()
    nk = g.type_rowptr_host[-1]

    judge = judge_rows          # (helpers.py: every row on its own scale, `row_err`)

    # the node projection: LayerNorm -> [H -> H] -> ScaledSiLU -> [H -> 3H]; rows of [T, N, .] arrays judged per (t, row)
    hb, xh, mean, rstd = nodeops.node_pre_fwd(c(x), wd, T)
    r64, r32 = ref_ops.node_pre_fwd(d64(x), w, T), ref_ops.node_pre_fwd(x, w, T)
    for k, nm in ((0, "hb"), (1, "xh")):
        judge((hb, xh)[k].reshape(T * N, -1), r64[k].reshape(T * N, -1), r32[k].reshape(T * N, -1), 2e-6, "pre_fwd " + nm)
    # its backward down to the per-relation partial sums: LINEAR in gxh -- the split products alone, rows at 1e-30 included
    parts = nodeops.node_pre_bwd(c(gxh), hb, c(x), mean, rstd, wd, parts_only=True)
    p64 = ref_ops.node_pre_bwd(d64(gxh), r64[0], d64(x), r64[2], r64[3], w, parts_only=True)
    p32 = ref_ops.node_pre_bwd(gxh, r32[0], x, r32[2], r32[3], w, parts_only=True)
    judge(parts.reshape(T * N, -1), p64.reshape(T * N, -1), p32.reshape(T * N, -1), 5e-6, "pre_bwd parts")
    # PaiNNUpdate and its backward
    outs = nodeops.node_update_fwd(c(x1), c(vec1), wd, gd)
    u64, u32 = ref_ops.node_update_fwd(d64(x1), d64(vec1), w, g), ref_ops.node_update_fwd(x1, vec1, w, g)
    known = slice(0, nk)
    judge(outs[0], u64[0], u32[0], 3e-6, "update_fwd x", known)
    judge(outs[1], u64[1], u32[1], 3e-6, "update_fwd vec", known)
    gx1, gvec1 = nodeops.node_update_bwd(c(gxo), c(gvo), outs[2], outs[3], outs[4], outs[5], wd, gd)
    b64 = ref_ops.node_update_bwd(d64(gxo), d64(gvo), u64[2], u64[3], u64[4], u64[5], w, g)
    b32 = ref_ops.node_update_bwd(gxo.clone(), gvo.clone(), u32[2], u32[3], u32[4], u32[5], w, g)
    judge(gx1, b64[0], b32[0], 5e-6, "update_bwd gx1", known)
    judge(gvec1, b64[1], b32[1], 5e-6, "update_bwd gvec1", known)
    _chain_tail_rows(w, wd, g, gd, H, gen)


def _chain_tail_rows(w, wd, g, gd, H, gen):
    """The tail rows of tests/test_stage_reference.py as further rows of x1 for the update chain (sigmoid_ of
    csrc/node_chain_common.h: the fast exponential and the hardware reciprocal), on a copy of the weights in which the x half
    of Wx0 is the identity and bx0 = bx2 = 0: with vec1 = 0 the pre-activations are then h2b = x1 itself -- rows whose every
    entry lies in [-80, -20], and rows at +-100 and +-1e6, in turn -- and q23 = ScaledSiLU(h2b) Wx2[H:] shows the tail: such a
    row within floor + 2 |h|max 2^-24 of float64 (or 8 x the fp32 restatement's error), the rows at -100 and -1e6 below
    FLT_MIN x H, those at +100 and +1e6 by the row rule; everything finite, backward included."""
    import copy
    from hermnet_amd import nodeops
    from test_stage_reference import TAIL_SATURATED
    dev = _dev()
    N, T, nk = g.N, g.T, g.type_rowptr_host[-1]
    eye = torch.cat([torch.eye(H), torch.zeros(H, H)], 1)                  # [H, 2H]: h2 = x1 (the |v2| half unread)
    eye_s = eye.expand(T, H, 2 * H).contiguous().to(dev)
    w0, wd0 = copy.copy(w), copy.copy(wd)
    w0.wx0, w0.bx0, w0.bx2 = [eye] * T, [torch.zeros(H)] * T, [torch.zeros_like(b) for b in w.bx2]
    wd0.bx0_s, wd0.bx2_s = torch.zeros_like(wd.bx0_s), torch.zeros_like(wd.bx2_s)
    wd0.wx0f, wd0.wx0tf = nodeops.weight_fragments(eye_s), nodeops.weight_fragments(eye_s.transpose(1, 2).contiguous())
    if wd.wx0f16 is not None:
        wd0.wx0f16 = nodeops.weight_fragments16(eye_s)
        wd0.wx0tf16 = nodeops.weight_fragments16(eye_s.transpose(1, 2).contiguous())
    kind = torch.arange(N) % (1 + len(TAIL_SATURATED))              # 0: a row in the tail; k: TAIL_SATURATED[k - 1]
    x1 = -20.0 - 60.0 * torch.rand(N, H, generator=gen)
    x1[:, 0], x1[:, 1] = -20.0, -80.0
    for k, v in enumerate(TAIL_SATURATED):
        x1[kind == k + 1] = v
    vec1 = torch.zeros(N, 3, H)
    outs = nodeops.node_update_fwd(x1.to(dev), vec1.to(dev), wd0, gd)
    u64, u32 = ref_ops.node_update_fwd(x1.double(), vec1.double(), w0, g), ref_ops.node_update_fwd(x1, vec1, w0, g)
    rows = torch.arange(N) < nk
    if g.row_real is not None:
        rows &= g.row_real.cpu() != 0
    if g.row_active is not None:
        rows &= g.row_active.cpu() != 0
    h2b = u64[3]
    tail = rows & (kind == 0)
    assert int(tail.sum()) >= 5 and float(h2b[tail].max()) == -20.0 and float(h2b[tail].min()) == -80.0
    for t_ in outs:
        assert bool(torch.isfinite(t_[:nk][rows[:nk].to(dev)]).all())
    judge_rows(outs[0], u64[0], u32[0], 3e-6, "tail rows update_fwd x", slice(0, nk))
    q, q64, q32 = outs[4].cpu().double(), u64[4], u32[4]
    err, base = row_err(q[tail], q64[tail]), row_err(q32[tail], q64[tail])
    bound = torch.maximum(3e-6 + 2.0 * h2b[tail].abs().amax(1) * 2.0 ** -24, 8.0 * base)
    print("chain tail rows H=%d: worst q23 row err %.2e, its bound %.2e" % (H, float(err.max()), float(bound[err.argmax()])))
    assert bool((err <= bound).all()), float((err / bound).max())
    for k, v in enumerate(TAIL_SATURATED):
        sel = rows & (kind == k + 1)
        assert bool(sel.any())
        if v > 0:
            judge_rows(q[sel], q64[sel], q32[sel], 3e-6, "tail rows q23 at %g" % v)
        else:
            assert float(q[sel].abs().max()) < FLT_MIN * H, v
    gen2 = torch.Generator().manual_seed(13)
    gx1, gvec1 = nodeops.node_update_bwd(torch.randn(N, H, generator=gen2).to(dev), torch.randn(N, 3, H, generator=gen2).to(dev),
                                         outs[2], outs[3], outs[4], outs[5], wd0, gd)
    assert bool(torch.isfinite(gx1).all()) and bool(torch.isfinite(gvec1).all())


@pytest.mark.parametrize("E,H,has_v", [(1000, 128, True), (777, 128, False), (301, 100, True), (50, 512, True), (5, 4, True),
                                       (130, 36, False)])
def test_edge_message_kernels_match_autograd_to_second_order(E, H, has_v):
    """csrc/train_kernels.hip (the training step's per-edge message algebra: forward, backward, backward of the backward)
    vs PyTorch autograd on the torch expression of the same map in float64: outputs, first-order gradients taken with
    create_graph=True, and the gradients of a functional of those w.r.t. every input AND the first cotangents."""
    from hermnet_amd import rmnet, trainops
    dev = _dev()
    gen = torch.Generator().manual_seed(E + H)
    rnd = lambda *s_: torch.randn(*s_, generator=gen)
    base = dict(X=rnd(E, 3 * H), R=rnd(E, 3 * H), V=rnd(E, 3, H) if has_v else None, U=rnd(E, 3),
                ws=rnd(E, H), wm=rnd(E, 3, H))
    wg = dict(X=rnd(E, 3 * H), R=rnd(E, 3 * H), V=rnd(E, 3, H), U=rnd(E, 3))

    def run(fn, device, dtype):
        t = {k: (None if v is None else v.to(device=device, dtype=dtype).requires_grad_(True)) for k, v in base.items()}
        S, M = fn(t["X"], t["R"], t["V"], t["U"])
        L1 = (S * t["ws"]).sum() + (M * t["wm"]).sum()
        names = [k for k in ("X", "R", "V", "U") if t[k] is not None]
        first = torch.autograd.grad(L1, [t[k] for k in names], create_graph=True)
        L2 = sum((g * wg[k].to(device=device, dtype=dtype)).sum() for k, g in zip(names, first))
        leaves = names + ["ws", "wm"]
        second = torch.autograd.grad(L2, [t[k] for k in leaves], allow_unused=True)
        out = {"S": S, "M": M}
        out.update({"g" + k: g for k, g in zip(names, first)})
        out.update({"d" + k: g for k, g in zip(leaves, second)})
        return {k: (None if v is None else v.detach().double().cpu()) for k, v in out.items()}

    got = run(trainops.EdgeMessage.apply, dev, torch.float32)
    ref = run(trainops._edge_message_torch, torch.device("cpu"), torch.float64)
    assert set(got) == set(ref)
    for k in ref:
        assert (got[k] is None) == (ref[k] is None), k
        if ref[k] is not None:
            assert rel_err(got[k], ref[k]) < 1e-5, (k, rel_err(got[k], ref[k]))


def test_training_step_is_bit_reproducible_run_to_run():
    """No float atomics with colliding addresses are left on the training path (segmented sums for every scatter, ordered
    sums for the weight windows of the bucketed basis): loss, energies, forces and EVERY parameter gradient of a step repeat
    bit for bit.  (The reference's own step does not: torch_scatter / index_add accumulate in arrival order.)"""
    import torch.nn.functional as F
    import hermnet_amd as hn
    from hermnet_amd import synth
    dev = _dev()
    d = synth.molecule_batch(num_graphs=96).to(dev)
    model = hn.HVNet(["H", "C", "O"], rc=5.0, num_layers=3, hidden_channels=128, num_rbf=64)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 12))
    model = model.to(dev).train()
    gen = torch.Generator().manual_seed(0)
    y = torch.randn(96, generator=gen).to(dev)
    ft = (0.5 * torch.randn(d.pos.shape, generator=gen)).to(dev)
    runs = []
    for _ in range(3):
        model.zero_grad()
        d.pos.requires_grad_(True)
        e = model(d)
        f = -torch.autograd.grad(e.sum(), d.pos, create_graph=True)[0]
        loss = 0.2 * F.mse_loss(e, y) + 0.8 * F.mse_loss(f, ft)
        loss.backward()
        runs.append((loss.detach().clone(), e.detach().clone(), f.detach().clone(),
                     {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    for other in runs[1:]:
        assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1]) and torch.equal(runs[0][2], other[2])
        assert len(other[3]) == len(runs[0][3]) > 0
        assert [n for n in runs[0][3] if not torch.equal(runs[0][3][n], other[3][n])] == []


def test_message_algebra_with_row_sums_inside_equals_the_per_edge_kernels(monkeypatch):
    """hermnet_edge_message_{fwd,bwd,bwd2}_rows (sums over a row's edges kept in registers) vs the per-edge kernels followed by
    segmented sums, through a whole training step: loss, energies, forces and every parameter gradient (HVNet with an
    unknown element in the batch, and HTNet: two row spaces)."""
    import torch.nn.functional as F
    import hermnet_amd as hn
    from hermnet_amd import synth
    dev = _dev()
    # (widths: 64 = 16 lanes per row group; 320 and 512 = a whole wave per group and TWO passes over the channel quads, the
    # second one partly empty at 320: the per-edge channel sums are then accumulated across the passes)
    for cls, elems, width in ((hn.HVNet, ["H", "C", "O"], 64), (hn.HVNet, ["H", "C"], 64), (hn.HTNet, ["H", "C", "O"], 64),
                              (hn.HVNet, ["H", "C", "O"], 320), (hn.HVNet, ["H", "C", "O"], 512)):
        torch.manual_seed(3)
        d = synth.molecule_batch(num_graphs=24 if width == 64 else 8).to(dev)
        model = cls(elems, rc=5.0, num_layers=3 if width == 64 else 2, hidden_channels=width, num_rbf=32)
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 12))
        model = model.to(dev).train()
        gen = torch.Generator().manual_seed(0)
        y = torch.randn(int(d.batch.max()) + 1, generator=gen).to(dev)
        ft = (0.5 * torch.randn(d.pos.shape, generator=gen)).to(dev)
        res = []
        from hermnet_amd import switches
        for flag in ("0", "1"):
            monkeypatch.setattr(switches, "train_row_sums", flag == "1")
            model.zero_grad()
            d.pos.requires_grad_(True)
            e = model(d)
            f = -torch.autograd.grad(e.sum(), d.pos, create_graph=True)[0]
            loss = 0.2 * F.mse_loss(e, y) + 0.8 * F.mse_loss(f, ft)
            loss.backward()
            res.append((e.detach().clone(), f.detach().clone(),
                        {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
        assert rel_err(res[1][0], res[0][0]) < 2e-6 and rel_err(res[1][1], res[0][1]) < 5e-6
        assert set(res[0][2]) == set(res[1][2]) and len(res[0][2]) > 0
        for n in res[0][2]:
            assert rel_err(res[1][2][n], res[0][2][n]) < 2e-5, n


@pytest.mark.parametrize("name", ["alloy108", "alloy108_unknown_type", "mol16"])
def test_edge_difference_and_its_adjoint_match_indexing_to_second_order(name):
    """trainops.EdgeDiff (D = pos[source] - pos[target] with a sort-free, atomics-free adjoint built from the CSR / CSC
    segments) vs plain tensor indexing: values, gradient, gradient of a functional of the gradient."""
    from hermnet_amd import trainops
    from hermnet_amd.elements import atomic_numbers
    dev = _dev()
    g = Golden(name)
    d = g.data().to(dev)
    graph = RelationalGraph.build(d.atomic_number, d.edge_index, [atomic_numbers[e] for e in g.elems],
                                  d.get("edge_shift") if d.get("cell") is not None else None, d.batch)
    src, tgt = graph.src_id.long(), graph.tgt_id.long()
    gen = torch.Generator().manual_seed(1)
    w1 = torch.randn(graph.E, 3, generator=gen).to(dev)
    w2 = torch.randn(d.pos.shape, generator=gen).to(dev)
    T = graph.T
    known = (torch.arange(graph.E, device=dev) < int(graph.csr_rowptr[int(graph.type_rowptr_host[-1])])).float()[:, None]
    res = []
    for fn in (lambda p: trainops.EdgeDiff.apply(p, graph), lambda p: p[src] - p[tgt]):
        p = d.pos.clone().requires_grad_(True)
        D = fn(p)
        # (edges into atoms of an unknown element carry no gradient in the model: the adjoint leaves them out on purpose)
        (g1,) = torch.autograd.grad(((D ** 2) * w1 * known).sum(), p, create_graph=True)
        (g2,) = torch.autograd.grad((g1 * w2).sum(), p)
        res.append((D.detach(), g1.detach(), g2))
    assert torch.equal(res[0][0], res[1][0])
    assert rel_err(res[0][1], res[1][1]) < 1e-5 and rel_err(res[0][2], res[1][2]) < 1e-5


def _second_order_vs_float64(fn_gpu, fn_ref, inputs, dev, tol=2e-5):
    """outputs, first-order gradients (create_graph=True) and the gradients of a functional of those w.r.t. every input and
    every first cotangent: a float32 GPU function against its torch expression in float64 on the host."""
    gen = torch.Generator().manual_seed(7)

    def run(fn, device, dtype):
        g = torch.Generator().manual_seed(11)
        t = [None if v is None else v.to(device=device, dtype=dtype).requires_grad_(v.is_floating_point() and v.dim() > 1)
             for v in inputs]
        outs = fn(*t)
        outs = outs if isinstance(outs, tuple) else (outs,)
        w1 = [torch.randn(o.shape, generator=g).to(device=device, dtype=dtype).requires_grad_(True) for o in outs]
        leaves = [v for v in t if v is not None and v.requires_grad]
        L1 = sum((o * w).sum() for o, w in zip(outs, w1))
        first = torch.autograd.grad(L1, leaves, create_graph=True)
        w2 = [torch.randn(f.shape, generator=g).to(device=device, dtype=dtype) for f in first]
        L2 = sum((f * w).sum() for f, w in zip(first, w2))
        second = torch.autograd.grad(L2, leaves + w1, allow_unused=True)
        res = list(outs) + list(first) + list(second)
        return [None if v is None else v.detach().double().cpu() for v in res]

    got, ref = run(fn_gpu, dev, torch.float32), run(fn_ref, torch.device("cpu"), torch.float64)
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        if b is None or float(b.abs().max()) == 0.0:
            assert a is None or float(a.abs().max()) < 1e-6, k
        else:
            assert a is not None and rel_err(a, b) < tol, (k, rel_err(a, b))


@pytest.mark.parametrize("T,K,O", [(3, 20172, 384), (1, 257, 4), (12, 1681, 128), (2, 300, 1024), (3, 6724, 96)])
def test_col_sum_kernel_matches_fp64_and_repeats(T, K, O):
    """`hermnet_col_sum` behind trainops._col_sum_over_rows (the bias gradients of the training step's node linears): against the
    fp64 sum, bit-identical from run to run, and differentiable (a broadcast)."""
    from hermnet_amd import trainops
    dev = _dev()
    gen = torch.Generator().manual_seed(T + K + O)
    g = torch.randn(T, K, O, generator=gen)
    gd = g.to(dev).requires_grad_(True)
    out = trainops._col_sum_over_rows(gd)
    ref = g.double().sum(1)
    assert out.shape == (T, O) and float((out.detach().cpu().double() - ref).abs().max()) < 3e-6 * K ** 0.5 * 4
    assert torch.equal(out, trainops._col_sum_over_rows(gd))
    w = torch.randn(T, O, generator=gen).to(dev)
    (gg,) = torch.autograd.grad((out * w).sum(), gd)
    assert torch.equal(gg, w[:, None, :].expand(T, K, O))


@pytest.mark.parametrize("E", [5000, 3, 0])
def test_edge_unit_vectors_match_autograd_to_second_order(E):
    """trainops.EdgeUnit (`hermnet_edge_unit`: U = D / d, d = max(|D|, 1e-6); /root/reference/HermNet/hermnet.py:144-152) vs float64
    autograd of the torch expression: values, first-order gradients with create_graph=True and the gradients of a functional
    of those w.r.t. D and both cotangents; one edge sits on the distance floor."""
    from hermnet_amd import trainops
    dev = _dev()
    gen = torch.Generator().manual_seed(E + 1)
    D = torch.randn(E, 3, generator=gen) * 2.0
    if E > 3:
        D[2] = torch.tensor([3.0e-7, -2.0e-7, 0.0])                      # on the floor: d = 1e-6 (at exactly 0 torch's norm has a NaN gradient)

    def ref(D):
        d = D.norm(dim=-1)
        d = torch.where(d.abs() <= 1.0e-6, torch.full_like(d, 1.0e-6), d)
        return D / d[:, None], d

    if E == 0:
        U, d = trainops.EdgeUnit.apply(D.to(dev).requires_grad_(True))
        assert U.shape == (0, 3) and d.shape == (0,)
        return
    _second_order_vs_float64(lambda D: trainops.EdgeUnit.apply(D), ref, [D], dev)


@pytest.mark.parametrize("R,H", [(700, 128), (33, 36), (5, 512)])
def test_training_node_stage_kernels_match_autograd_to_second_order(R, H):
    """csrc/train_node_kernels.hip behind trainops.{LayerNorm2, SiLU2, UpdateMid, UpdateOut} (the node-level stages of the
    training step, one launch per order of differentiation) vs float64 autograd of the torch expressions of rmnet.py:52,
    94-107, 110-117."""
    import math
    import torch.nn.functional as F
    from hermnet_amd import trainops
    dev = _dev()
    gen = torch.Generator().manual_seed(R + H)
    rnd = lambda *s_: torch.randn(*s_, generator=gen)
    c, s2 = 1.0 / math.sqrt(H), 1.0 / math.sqrt(2.0)
    _second_order_vs_float64(lambda x: trainops.LayerNorm2.apply(x, 1e-5), lambda x: F.layer_norm(x, (H,), eps=1e-5),
                             [rnd(R, H) * 2 + 0.3], dev, tol=1e-4)
    _second_order_vs_float64(trainops.SiLU2.apply, F.silu, [rnd(R, H) * 2], dev)

    def mid_ref(vp, xt):
        v1, v2 = vp[..., :H], vp[..., H:]
        return (v1 * v2).sum(1) * c, torch.cat([xt, torch.sqrt((v2 ** 2).sum(1) + 1e-8)], -1)

    _second_order_vs_float64(lambda vp, xt: trainops.UpdateMid.apply(vp, xt, c, 1e-8), mid_ref, [rnd(R, 3, 2 * H), rnd(R, H)], dev)
    for mask in (None, (torch.rand(R, generator=gen) > 0.3).float()):
        def out_ref(q, vdot, vp, xt, vt, m=mask):
            q1, q2, q3 = q[:, :H], q[:, H:2 * H], q[:, 2 * H:]
            xo, vo = xt + (q1 + q2 * vdot) * s2, vt + q3[:, None, :] * vp[..., :H]
            if m is not None:
                mm = m.to(device=q.device, dtype=q.dtype)
                xo, vo = xo * mm[:, None], vo * mm[:, None, None]
            return xo, vo

        mg = None if mask is None else mask.to(dev)
        _second_order_vs_float64(lambda q, vdot, vp, xt, vt: trainops.UpdateOut.apply(q, vdot, vp, xt, vt, mg, s2), out_ref,
                                 [rnd(R, 3 * H), rnd(R, H), rnd(R, 3, 2 * H), rnd(R, H), rnd(R, 3, H)], dev)
        for has_vec in (True, False):
            def res_ref(x, dx, v, dv, m=mask):
                x1, v1 = (x + dx) * s2, (dv if v is None else v + dv)
                if m is not None:
                    mm = m.to(device=x.device, dtype=x.dtype)
                    x1, v1 = x1 * mm[:, None], v1 * mm[:, None, None]
                return x1, v1

            _second_order_vs_float64(lambda x, dx, v, dv: trainops.Residual.apply(x, dx, v, dv, mg, s2), res_ref,
                                     [rnd(R, H), rnd(R, H), rnd(R, 3, H) if has_vec else None, rnd(R, 3, H)], dev)


@pytest.mark.parametrize("E,H,R,T,env", [(6000, 128, 128, 3, "polynomial"), (900, 64, 50, 2, "polynomial"), (700, 32, 20, 1, "exponential")])
def test_bucketed_basis_projection_matches_dense_to_second_order(E, H, R, T, env):
    """`trainops.BucketedBasis` (edges sorted by (relation, distance bucket), 32-centre windows, one batched product) vs the
    dense Gaussian basis + nn.Linear per relation in float64: values in the edges' own order, first-order gradients
    w.r.t. distances, weights and biases with create_graph=True, and the gradients of a functional of those.
    Distances run past the cutoff and to both ends of the centre range."""
    from hermnet_amd import rmnet, trainops
    dev = _dev()
    gen = torch.Generator().manual_seed(E + R)
    rc = 5.0
    rb = rmnet.RadialBasis(R, rc, envelope={"name": env} if env == "exponential" else {"name": "polynomial", "exponent": 5})
    # (the exponential envelope's masked branch overflows within ~1e-3 of the cutoff from above -- in the reference as
    # well, rmnet.py:196-208 --, so that case keeps its random distances inside the cutoff)
    d0 = torch.rand(E, generator=gen) * (1.12 if env == "polynomial" else 0.99) * rc
    d0[:4] = torch.tensor([1e-3, 0.97 * rc, (1.0 if env == "polynomial" else 0.985) * rc, 1.1 * rc])
    cuts = sorted(torch.randint(0, E, (T - 1,), generator=gen).tolist())
    bounds = [0] + cuts + [E - 7]                                  # the last 7 edges: targets of unknown elements
    W0 = [torch.randn(3 * H, R, generator=gen) * 0.3 for _ in range(T)]
    b0 = [torch.randn(3 * H, generator=gen) for _ in range(T)]
    sc0 = torch.rand(3 * H, generator=gen) + 0.5
    c0, wd = torch.randn(bounds[T], 3 * H, generator=gen), torch.randn(E, generator=gen)

    def run(bucketed, device, dtype):
        m = rb.to(device=device, dtype=dtype)
        t = lambda v: v.to(device=device, dtype=dtype)
        d = t(d0).requires_grad_(True)
        W = [t(w).requires_grad_(True) for w in W0]
        b = [t(v).requires_grad_(True) for v in b0]
        c1 = t(c0).requires_grad_(True)
        sc = t(sc0)
        if bucketed:
            bb = m.bucketed(d, bounds, T)
            R1, R2 = bb.project(W, b, sc)                     # one storage under two autograd outputs (trainops.BandP)
            out = 0.5 * R1.index_select(0, bb.slot) + 0.5 * R2.index_select(0, bb.slot)
        else:
            phi = m(d)
            out = torch.cat([torch.nn.functional.linear(phi[bounds[k]:bounds[k + 1]], W[k] * sc[:, None], b[k] * sc) for k in range(T)])
        L1 = (out * c1).sum()
        leaves = [d] + W + b
        first = torch.autograd.grad(L1, leaves, create_graph=True)
        L2 = (first[0] * t(wd)).sum() + sum((g * g.detach().sign()).sum() for g in first[1:])
        second = torch.autograd.grad(L2, leaves + [c1], allow_unused=True)
        res = [out] + list(first) + list(second)
        return [None if v is None else v.detach().double().cpu() for v in res]

    got, ref = run(True, dev, torch.float32), run(False, torch.device("cpu"), torch.float64)
    for k, (a, b_) in enumerate(zip(got, ref)):
        if b_ is None or float(b_.abs().max()) == 0.0:
            assert a is None or float(a.abs().max()) < 1e-6, k
        else:
            assert a is not None and rel_err(a, b_) < 3e-5, (k, rel_err(a, b_))


@pytest.mark.parametrize("E,N,T,H,has_v", [(4000, 300, 3, 128, True), (900, 77, 2, 64, False), (500, 40, 1, 100, True)])
def test_message_algebra_node_level_matches_autograd_to_second_order(E, N, T, H, has_v):
    """`trainops.MessageAlgebra` (gathers through row indices inside the edge kernels, row sums inside the function:
    node-level inputs and outputs) vs gather -> torch expression -> index_add in float64 autograd, to second order."""
    from hermnet_amd import rmnet, trainops
    dev = _dev()
    gen = torch.Generator().manual_seed(E + N)
    rnd = lambda *s_: torch.randn(*s_, generator=gen)
    tgt = torch.sort(torch.randint(0, N, (E,), generator=gen)).values
    tgt[tgt == 5] = 6                                                    # a row without edges
    src = torch.randint(0, N, (E,), generator=gen)
    rel = torch.sort(torch.randint(0, T, (E,), generator=gen)).values
    xrow = rel * N + src

    def keys(device):
        mk = lambda idx, perm, n: trainops._RowKey(idx.to(device), None if perm is None else perm.to(device),
                                                torch.bincount(idx, minlength=n).to(device), n)
        return trainops.EdgeKeys(mk(tgt, None, N), mk(src, torch.argsort(src, stable=True), N),
                                 mk(xrow, torch.argsort(xrow, stable=True), T * N))

    base = dict(xh=rnd(T * N, 3 * H), vec=rnd(N, 3, H) if has_v else None, R=rnd(E, 3 * H), U=rnd(E, 3),
                wx=rnd(N, H), wv=rnd(N, 3, H))
    wg = dict(xh=rnd(T * N, 3 * H), vec=rnd(N, 3, H), R=rnd(E, 3 * H), U=rnd(E, 3))

    def run(kernels, device, dtype):
        t = {k: (None if v is None else v.to(device=device, dtype=dtype).requires_grad_(True)) for k, v in base.items()}
        if kernels:
            dx, dv = trainops.MessageAlgebra.apply(t["xh"], t["vec"], t["R"], t["U"], keys(device))
        else:
            X = t["xh"][xrow.to(device)]
            V = None if t["vec"] is None else t["vec"][src.to(device)]
            S, M = trainops._edge_message_torch(X, t["R"], V, t["U"])
            dx = torch.zeros(N, H, dtype=dtype, device=device).index_add(0, tgt.to(device), S)
            dv = torch.zeros(N, 3, H, dtype=dtype, device=device).index_add(0, tgt.to(device), M)
        L1 = (dx * t["wx"]).sum() + (dv * t["wv"]).sum()
        names = [k for k in ("xh", "vec", "R", "U") if t[k] is not None]
        first = torch.autograd.grad(L1, [t[k] for k in names], create_graph=True)
        L2 = sum((g * wg[k].to(device=device, dtype=dtype)).sum() for k, g in zip(names, first))
        leaves = names + ["wx", "wv"]
        second = torch.autograd.grad(L2, [t[k] for k in leaves], allow_unused=True)
        out = {"dx": dx, "dv": dv}
        out.update({"g_" + k: g for k, g in zip(names, first)})
        out.update({"dd_" + k: g for k, g in zip(leaves, second)})
        return {k: (None if v is None else v.detach().double().cpu()) for k, v in out.items()}

    got, ref = run(True, dev, torch.float32), run(False, torch.device("cpu"), torch.float64)
    assert set(got) == set(ref)
    for k in ref:
        assert (got[k] is None) == (ref[k] is None), k
        if ref[k] is not None:
            assert rel_err(got[k], ref[k]) < 1e-5, (k, rel_err(got[k], ref[k]))


@pytest.mark.parametrize("K,n_rows,shape", [(5000, 700, (128,)), (5000, 700, (3, 128)), (333, 50, (100,)), (40, 64, (4,)),
                                            (2000, 10, (3, 512))])
def test_segment_sum_kernel_and_its_adjoint_pair(K, n_rows, shape):
    """`hermnet_segment_sum` behind `trainops.SumRows` (rows gathered inside the sum, list order) vs index_add in float64,
    sorted and permuted assignments, empty rows; and `GatherRows` / `SumRows` differentiate into each other."""
    from hermnet_amd import rmnet, trainops
    dev = _dev()
    gen = torch.Generator().manual_seed(K)
    idx = torch.randint(0, n_rows, (K,), generator=gen)
    idx[idx == 3] = 4                                   # an empty row
    x = torch.randn(K, *shape, generator=gen)
    want = torch.zeros(n_rows, *shape, dtype=torch.float64).index_add_(0, idx, x.double())
    for sorted_input in (False, True):
        if sorted_input:
            order = torch.argsort(idx, stable=True)
            idx_, x_, perm = idx[order], x[order], None
        else:
            idx_, x_, perm = idx, x, torch.argsort(idx, stable=True).to(dev)
        key = trainops._RowKey(idx_.to(dev), perm, torch.bincount(idx_, minlength=n_rows).to(dev), n_rows)
        xd = x_.to(dev).requires_grad_(True)
        out = trainops.SumRows.apply(xd, key)
        assert rel_err(out.detach().cpu().double(), want) < 1e-6
        w = torch.randn(n_rows, *shape, generator=gen).to(dev)
        g, = torch.autograd.grad((out * w).sum(), xd, create_graph=True)
        assert torch.equal(g, w.index_select(0, idx_.to(dev)))                       # the adjoint: a gather
        w2 = torch.randn(K, *shape, generator=gen).to(dev)
        back, = torch.autograd.grad((trainops.GatherRows.apply(w.clone().requires_grad_(True), key) * w2).sum(), xd, allow_unused=True)
        assert back is None


@pytest.mark.parametrize("H", [64, 128, 320, 1024])
def test_layernorm_kernels(H):
    """`hermnet_layernorm_fwd/_bwd` (no affine) vs torch.native_layer_norm and its backward."""
    from hermnet_amd import nodeops
    dev = _dev()
    gen = torch.Generator().manual_seed(H)
    rows = 203
    x = torch.randn(rows, H, generator=gen) * 3 + 0.7
    g, add = torch.randn(rows, H, generator=gen), torch.randn(rows, H, generator=gen)
    n, mean, rstd = nodeops.layernorm_fwd(x.to(dev), 1e-5)
    n_r, mean_r, rstd_r = ref_ops.layernorm_fwd(x, 1e-5)
    assert rel_err(n.cpu(), n_r) < 2e-6 and rel_err(mean.cpu(), mean_r) < 2e-6 and rel_err(rstd.cpu(), rstd_r) < 2e-6
    for a in (None, add):
        gx = nodeops.layernorm_bwd(g.to(dev), x.to(dev), mean, rstd, add=None if a is None else a.to(dev))
        assert rel_err(gx.cpu(), ref_ops.layernorm_bwd(g, x, mean_r, rstd_r, add=a)) < 2e-6


def test_energy_head_kernels():
    """`hermnet_energy_head_fwd/_bwd` vs the PyTorch restatement (ScaledSiLU + Linear(H/2, 1))."""
    from hermnet_amd import nodeops
    dev = _dev()
    gen = torch.Generator().manual_seed(3)
    for rows, C in [(257, 64), (31, 32), (100, 256)]:
        h, w, b = torch.randn(rows, C, generator=gen), torch.randn(C, generator=gen), torch.randn(1, generator=gen)
        ge = torch.randn(rows, generator=gen)
        for mask in (None, (torch.arange(rows) % 7 != 0).float()):
            md = None if mask is None else mask.to(dev)
            e = nodeops.energy_head_fwd(h.to(dev), w.to(dev), b.to(dev), md)
            assert rel_err(e.cpu(), ref_ops.energy_head_fwd(h, w, b, mask)) < 2e-6
            gh = nodeops.energy_head_bwd(ge.to(dev), h.to(dev), w.to(dev), md)
            assert rel_err(gh.cpu(), ref_ops.energy_head_bwd(ge, h, w, mask)) < 2e-6
    # the whole read-out in one launch each way (no library GEMM): hermnet.py:113-117,129
    for rows, H, C in [(257, 128, 64), (31, 64, 64), (1000, 64, 128), (100, 256, 64)]:
        assert nodeops.head_fused_supported(H, C)
        x, w0, b0 = torch.randn(rows, H, generator=gen), torch.randn(C, H, generator=gen) * 0.2, torch.randn(C, generator=gen)
        w2, b2, ge = torch.randn(C, generator=gen), torch.randn(1, generator=gen), torch.randn(rows, generator=gen)
        for mask in (None, (torch.arange(rows) % 7 != 0).float()):
            md = None if mask is None else mask.to(dev)
            h_r = x.double() @ w0.double().t() + b0.double()
            e_r = ref_ops.energy_head_fwd(h_r, w2.double(), b2.double(), None if mask is None else mask.double())
            h, e = nodeops.energy_head_fused_fwd(x.to(dev), w0.t().contiguous().to(dev), b0.to(dev), w2.to(dev), b2.to(dev), md)
            assert rel_err(h.cpu().double(), h_r) < 2e-6 and rel_err(e.cpu().double(), e_r) < 3e-6
            gx = nodeops.energy_head_fused_bwd(ge.to(dev), h, w0.to(dev), w2.to(dev), md)
            gx_r = ref_ops.energy_head_bwd(ge.double(), h_r, w2.double(), None if mask is None else mask.double()) @ w0.double()
            assert rel_err(gx.cpu().double(), gx_r) < 3e-6


def test_halo_rows_kernels():
    """`hermnet_halo_rows` (pack / pack-and-clear / unpack) and `hermnet_halo_accumulate` vs the torch index ops of the host path."""
    from hermnet_amd import nodeops
    dev = _dev()
    gen = torch.Generator().manual_seed(9)
    N, H = 50, 128
    x, vec = torch.randn(N, H, generator=gen).to(dev), torch.randn(N, 3, H, generator=gen).to(dev)
    idx = torch.tensor([3, 7, 7, 0, 49, 21, 3], device=dev)                     # repeats: one atom, several neighbours
    uniq = torch.tensor([5, 1, 48, 30], device=dev)
    ref = torch.cat([x[idx], vec[idx].reshape(-1, 3 * H)], 1)
    assert torch.equal(nodeops.halo_rows(0, x, vec, idx), ref)
    x1, v1 = x.clone(), vec.clone()
    buf = nodeops.halo_rows(1, x1, v1, uniq)
    assert torch.equal(buf, torch.cat([x[uniq], vec[uniq].reshape(-1, 3 * H)], 1))
    assert float(x1[uniq].abs().max()) == 0 and float(v1[uniq].abs().max()) == 0
    keep = torch.ones(N, dtype=torch.bool, device=dev)
    keep[uniq] = False
    assert torch.equal(x1[keep], x[keep]) and torch.equal(v1[keep], vec[keep])
    new = torch.randn(4, 4 * H, generator=gen).to(dev)
    x2, v2 = x.clone(), vec.clone()
    nodeops.halo_rows(2, x2, v2, uniq, new)
    assert torch.equal(x2[uniq], new[:, :H]) and torch.equal(v2[uniq], new[:, H:].reshape(-1, 3, H))
    add = torch.randn(7, 4 * H, generator=gen).to(dev)
    with pytest.raises(RuntimeError):            # the float-atomic accumulate mode of ABI <= 6 is gone
        nodeops.halo_rows(3, x.clone(), vec.clone(), idx, add)
    # accumulate at the owner: fixed summation order per owner row, bit-exact
    from hermnet_amd.sharding import ExchangePlan
    plan = ExchangePlan(idx, [3, 4], torch.zeros(0, dtype=torch.long, device=dev), [0, 0])
    x4, v4 = x.clone(), vec.clone()
    nodeops.halo_accumulate(x4, v4, plan, add)
    xe, ve = x.clone().cpu().double(), vec.clone().cpu().double()
    xs, vs = x.clone().cpu(), vec.clone().cpu()
    for k, r in enumerate(idx.cpu().tolist()):                   # sequential fp32 adds in send-list order
        xs[r] += add[k, :H].cpu()
        vs[r] += add[k, H:].cpu().reshape(3, H)
    assert torch.equal(x4.cpu(), xs) and torch.equal(v4.cpu(), vs)
    # ... and through a re-ordering (what HVNet.forward does: atom ids -> relation rows)
    perm = torch.randperm(N, generator=gen).to(dev)
    x5, v5 = torch.empty_like(x), torch.empty_like(vec)
    x5[perm], v5[perm] = x, vec
    nodeops.halo_accumulate(x5, v5, plan.remap(perm), add)
    assert torch.equal(x5[perm].cpu(), xs) and torch.equal(v5[perm].cpu(), vs)


@pytest.mark.parametrize("seed,NA,T,H,R,hub", [(0, 300, 3, 128, 128, 700), (1, 257, 2, 64, 20, 130), (2, 64, 1, 128, 50, 63),
                                                 (3, 500, 3, 64, 128, 1500)])
@pytest.mark.parametrize("bwd_form", ["channel-per-lane", "vw"])
def test_message_scatter_op_on_skewed_random_graphs(seed, NA, T, H, R, hub, bwd_form):
    """The pipelined edge streams of the message kernels on graphs unlike a crystal: a few hub atoms with hundreds of
    in- AND out-edges (segments far longer than the 64-edge index batches), most atoms with a handful, some with none,
    atoms of an element the model does not know, repeated (source, target) pairs at different distances.  Forward and
    backward vs the fp64 restatement."""
    from hermnet_amd.ops import edge_radial_table
    dev = _dev()
    gen = torch.Generator(device="cpu").manual_seed(100 + seed)
    elems = ["Al", "Ni", "Cu"][:T]
    zl = [atomic_numbers[e] for e in elems]
    z = torch.tensor(zl + [14])[torch.randint(0, T + 1, (NA,), generator=gen)]          # Si: not in `elems`
    z[:T] = torch.tensor(zl)                                                              # every element present
    hubs = torch.randint(0, NA, (3,), generator=gen)
    src = [torch.randint(0, NA, (hub,), generator=gen), hubs[torch.randint(0, 3, (hub,), generator=gen)],
           torch.randint(0, NA, (4 * NA,), generator=gen)]
    tgt = [hubs[torch.randint(0, 3, (hub,), generator=gen)], torch.randint(0, NA, (hub,), generator=gen),
           torch.randint(0, NA // 2, (4 * NA,), generator=gen)]                           # the upper half: few in-edges
    ei = torch.stack([torch.cat(src), torch.cat(tgt)])
    ei = ei[:, ei[0] != ei[1]]
    E = ei.size(1)
    graph = RelationalGraph.build(z.to(dev), ei.to(dev), zl, edge_shift=None, batch=torch.zeros(NA, dtype=torch.long, device=dev))
    model = hn.HVNet(elems, rc=5.0, num_layers=1, hidden_channels=H, num_rbf=R).to(dev)
    rbf = model.radial_basis.descriptor()
    N = graph.N
    rnd = lambda *s_: torch.randn(*s_, generator=gen).to(dev)
    # geometry in CSR order: unit vectors and distances spread over (0, rc), a few beyond the cutoff
    D = torch.randn(E, 3, generator=gen)
    dist = (torch.rand(E, generator=gen) * 5.4 + 0.05)
    edge = torch.cat([D / D.norm(dim=1, keepdim=True), dist[:, None]], 1).float().to(dev).contiguous()
    xh, x, vec = rnd(T, N, 3 * H), rnd(N, H), rnd(N, 3, H)
    wt = (rnd(T, R, 3 * H) / math.sqrt(R)).contiguous()
    brbf = (0.1 * rnd(T, 3 * H)).contiguous()
    graph.edge_table = edge_radial_table(graph, rbf, edge) if bwd_form == "channel-per-lane" else None
    xh.requires_grad_(True); x.requires_grad_(True); vec.requires_grad_(True)
    edge_in = edge.detach().clone().requires_grad_(True)
    x1, vec1 = MessageScatter.apply(xh, vec, x, edge_in, wt, brbf, graph, rbf)

    D64 = (edge[:, :3] * edge[:, 3:4]).double().detach().requires_grad_(True)
    dn = D64.norm(dim=-1)
    e64 = torch.cat([D64 / dn[:, None], dn[:, None]], 1)
    xh64, x64, v64 = [t_.detach().double().requires_grad_(True) for t_ in (xh, x, vec)]

    class R64:
        inv_rc, env_kind, env_p, offset = rbf.inv_rc, rbf.env_kind, rbf.env_p, rbf.offset.double()
    x1r, vec1r = ref_ops.message_scatter_ref(xh64, v64, x64, e64, wt.double(), brbf.double(), graph, R64)
    assert rel_err(x1.double(), x1r) < TOL and rel_err(vec1.double(), vec1r) < TOL
    gx1, gv1 = rnd(N, H), rnd(N, 3, H)
    grads = torch.autograd.grad([x1, vec1], [xh, x, edge_in, vec], [gx1, gv1])
    grads_r = torch.autograd.grad([x1r, vec1r], [xh64, x64, D64, v64], [gx1.double(), gv1.double()])
    for nm, a, b in zip(["gxh", "gx", "gD", "gvec"], grads, grads_r):
        a = a[:, :3] if nm == "gD" else a
        assert rel_err(a.double(), b) < 2 * TOL, nm


def test_bias_on_load_equals_bias_in_operand():
    """The stages that add a GEMM's bias on load (include/hermnet_hip.h "Bias convention"): kernel(h, bias)
    must equal kernel(h + expanded bias) for the node kernels and the message kernels (xh_bias)."""
    import ctypes
    from hermnet_amd import nodeops, _lib
    from hermnet_amd.ops import _stream
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    # node kernels: 3 relation blocks of B rows (+ 2 unknown rows), one bias row per block
    T, B, H = 3, 12, 128
    nk, N = T * B, T * B + 2
    expand = lambda b, rows: b.reshape(T, 1, -1).expand(T, B, b.size(-1)).reshape(nk, -1)[:rows]
    h2, b0 = rnd(nk, H), rnd(T, 1, H)
    assert torch.equal(nodeops.ssilu_fwd(h2, bias=b0, rows_per_bias=B), nodeops.ssilu_fwd(h2 + expand(b0, nk)))
    ga2 = rnd(nk, H)
    assert torch.equal(nodeops.ssilu_bwd(ga2, h2, nk, 1, H, H, H, bias=b0, rows_per_bias=B),
                       nodeops.ssilu_bwd(ga2, h2 + expand(b0, nk), nk, 1, H, H, H))
    h, b1 = rnd(N, T * H), rnd(T * H)                     # single bias row over [N, T*H]
    assert torch.equal(nodeops.ssilu_fwd(h, bias=b1), nodeops.ssilu_fwd(h + b1))
    g_tn = rnd(T, N, H)
    assert torch.equal(nodeops.ssilu_bwd(g_tn, h, N, T, H, H, N * H, bias=b1),
                       nodeops.ssilu_bwd(g_tn, h + b1, N, T, H, H, N * H))
    q, qb = rnd(N, 3 * H), rnd(T, 1, 3 * H)
    qfull = q.clone()
    qfull[:nk] += expand(qb, nk)
    vd, vp, x1, vec1 = rnd(N, H), rnd(N, 3, 2 * H), rnd(N, H), rnd(N, 3, H)
    mask = (torch.arange(N) % 5 != 0).float().to(dev)
    for a, b in zip(nodeops.update_out(q, vd, vp, x1, vec1, mask, N, nk, H, qbias=qb, rows_per_bias=B),
                    nodeops.update_out(qfull, vd, vp, x1, vec1, mask, N, nk, H)):
        assert torch.equal(a, b)
    gxo, gvo = rnd(N, H), rnd(N, 3, H)
    outs_a = nodeops.update_out_bwd(gxo, gvo, q, vd, vp, mask, N, nk, H, qbias=qb, rows_per_bias=B)
    outs_b = nodeops.update_out_bwd(gxo, gvo, qfull, vd, vp, mask, N, nk, H)
    for k, (a, b) in enumerate(zip(outs_a, outs_b)):
        if k == 2:
            a, b = a[:nk, :, :H], b[:nk, :, :H]        # the v2 half is written by update_mid_bwd
        elif k in (0, 1):
            a, b = a[:nk], b[:nk]
        assert torch.equal(a, b), k
    # message kernels
    g = Golden("alloy108")
    d, graph = _graph(g, dev)
    model = g.model().to(dev)
    rbf = model.radial_basis.descriptor()
    H, R, T, N = model.hidden_channels, rbf.num_rbf, graph.T, graph.N
    xh, xb, x, vec = rnd(T, N, 3 * H), rnd(T, 3 * H), rnd(N, H), rnd(N, 3, H)
    wt, brbf = (rnd(T, R, 3 * H) / math.sqrt(R)).contiguous(), (0.1 * rnd(T, 3 * H)).contiguous()
    edge = EdgeGeometry.apply(d.pos, d.get("cell"), graph)
    gx1, gv1 = rnd(N, H), rnd(N, 3, H)
    lib, P = _lib.load(), _lib.ptr
    gs, rs = graph.as_struct(), rbf.struct()

    from hermnet_amd.ops import edge_radial_table
    table = edge_radial_table(graph, rbf, edge)
    part = torch.empty(T, N, 3, H, device=dev)

    def run(xh_in, bias, v, tab=None):
        x1, vec1 = torch.empty_like(x), torch.empty(N, 3, H, device=dev)
        assert lib.hermnet_message_scatter_fwd(ctypes.byref(gs), ctypes.byref(rs), H, P(xh_in), P(bias), P(v), P(x), P(wt),
                                               P(brbf), P(edge), P(x1), P(vec1), None, 1, 0, _stream()) == 0
        gxh, gvec, gx = torch.empty_like(xh), torch.empty_like(vec), torch.empty_like(x)
        gedge = torch.zeros(H // 64, graph.E, 4, device=dev)
        assert lib.hermnet_message_scatter_bwd(ctypes.byref(gs), ctypes.byref(rs), H, P(xh_in), P(bias), P(v), P(wt), P(brbf),
                                               P(edge), P(gx1), P(gv1), P(gxh), P(gvec if v is not None else None), P(gx),
                                               P(gedge), 0, P(tab), P(part if tab is not None else None), None, None, 0, _stream()) == 0
        return [x1, vec1, gxh, gx, gedge.sum(0)] + ([gvec] if v is not None else [])

    for v in (vec, None):
        for tab in (None, table):
            for a, b in zip(run(xh, xb, v, tab), run(xh + xb[:, None, :], None, v, tab)):
                assert rel_err(a, b) < 1e-6
        # the two forms of the backward kernel agree with each other (different summation orders: not bit for bit)
        for a, b in zip(run(xh, xb, v, None), run(xh, xb, v, table)):
            assert rel_err(a, b) < 2e-6


@pytest.mark.parametrize("name", ["alloy108", "alloy108_unknown_type", "mol16"])
def test_fused_layer_equals_autograd_composed_layer(name, monkeypatch):
    """The hand-written layer backward vs PyTorch autograd over the same kernels (`switches.fused_layer = False`)."""
    from hermnet_amd import switches
    dev = _dev()
    g = Golden(name)
    model = g.model().to(dev)
    res = []
    for flag in ("1", "0"):
        monkeypatch.setattr(switches, "fused_layer", flag == "1")
        d = g.data().to(dev)
        d.pos.requires_grad_(True)
        e = model(d)
        f = -torch.autograd.grad(e.sum(), d.pos)[0]
        res.append((e.detach(), f))
    assert rel_err(res[0][0], res[1][0]) < 2e-6
    assert rel_err(res[0][1], res[1][1]) < 5e-6


@pytest.mark.parametrize("case", ["eval", "train", "htnet"])
def test_an_evaluation_leaves_only_its_declared_names_on_the_data(case):
    """The 108-atom alloy at width 128 with two layers -- the smallest model that reaches the short last layer, the deferred
    sums and a layer boundary -- in eval(), in train() with create_graph=True and as HTNet: behind the forward and its backward
    the Data holds the four names an evaluation leaves for readers and nothing else of the package's; the rest of what the
    stages hand to each other lives on the `layer.StepState` and goes with it."""
    dev = _dev()
    g = Golden("alloy108")
    torch.manual_seed(3)
    Model = hn.HTNet if case == "htnet" else hn.HVNet
    model = Model(g.elems, rc=5.0, num_layers=2, hidden_channels=128, num_rbf=128)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 7))
    model = model.to(dev)
    d = g.data().to(dev)
    d.pos.requires_grad_(True)
    if case == "train":
        model.train()
        e = model(d)
        f = -torch.autograd.grad(e.sum(), d.pos, create_graph=True)[0]
        (e.sum() + (f ** 2).sum()).backward()
        assert all(p.grad is None or torch.isfinite(p.grad).all() for p in model.parameters())
        assert sum(p.grad is not None for p in model.parameters()) > 0
    else:
        model.eval()
        for p in model.parameters():
            p.requires_grad_(False)
        e = model(d)
        f = -torch.autograd.grad(e.sum(), d.pos)[0]
    assert torch.isfinite(e).all() and torch.isfinite(f).all() and float(f.abs().max()) > 0
    assert {k for k in d.keys() if k.startswith("_hn_")} == {"_hn_step", "_hn_graph", "_hn_edge", "_hn_edge_embed"}
    step = d._hn_step
    assert step.graph is d._hn_graph and step.edge is d._hn_edge and step.edge_embed is d._hn_edge_embed
    assert step.weights is None and step.edge_handles is None and not step.pending and not step.pre_next
    if case == "eval":
        assert d.vec is None                     # (behind the short last layer: tests/test_dead_ends.py)


class _LaunchCounter(object):
    """ops.set_kernel_timer hook that only counts the library launches by name."""

    def __init__(self):
        self.names = []

    def launch(self, name, fn):
        self.names.append(name)
        return fn()


@pytest.mark.parametrize("name,width", [("alloy108", None), ("alloy108_unknown_type", None), ("mol16", None),
                                        ("alloy108", 192), ("alloy108", 256)])
def test_deferred_gradient_sums_equal_the_finishing_launches_bit_for_bit(name, width, monkeypatch):
    """a layer's backward hands (gx, gvec) down as per-relation partial sums and the update backward of
    the layer below forms them in its own launch (hn_pending_grads) -- no message_bwd_finish / layernorm_bwd_parts
    launches, the same bits in energy and forces."""
    from hermnet_amd import ops
    dev = _dev()
    g = Golden(name)
    # (the round-4 forms of both sides: with the layer boundary fused -- round 5's default at width 128 -- the deferred side runs
    # the projection's backward on 16-row tiles, another summation order: test_fused_layer_boundary_changes_no_bit_of_the_model)
    from hermnet_amd import switches
    monkeypatch.setattr(switches, "boundary_mode", 0)
    if width is None:
        model = g.model().to(dev)
    else:
        from hermnet_amd import HVNet
        torch.manual_seed(5)
        kw = dict(g.model_kw)
        kw["hidden_channels"] = width
        model = HVNet(g.elems, **kw).to(dev).eval()
    res = []
    for flag in ("0", "1"):
        monkeypatch.setenv("HERMNET_DEFER_SUMS", flag)
        d = g.data().to(dev)
        d.pos.requires_grad_(True)
        cnt = _LaunchCounter()
        ops.set_kernel_timer(cnt)
        try:
            e = model(d)
            f = -torch.autograd.grad(e.sum(), d.pos)[0]
        finally:
            ops.set_kernel_timer(None)
        torch.cuda.synchronize()
        res.append((e.detach().clone(), f.clone(), cnt.names))
        assert not d._hn_step.pending           # every handed-down gradient was picked up
    assert torch.isfinite(res[1][1]).all()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert len(res[1][2]) == len(res[0][2])     # (the same library calls: the launches they no longer make are inside them)


def test_pending_gradients_in_every_update_backward_form():
    """hn_pending_grads straight through the C ABI for the kernel families the model does not defer to by default (the
    wide kernels, 32-row tiles): gx_out / gvec_out formed inside hermnet_node_update_bwd equal the separate launches'."""
    from hermnet_amd import nodeops
    from hermnet_amd.layer import LayerWeights
    from hermnet_amd.relations import RelationalGraph
    from hermnet_amd.rmnet import PaiNNModule
    dev = _dev()
    for H, n in ((128, 333), (128, 40000), (192, 333), (256, 333), (64, 333)):     # (16-row tiles at 333 rows, 32 at 40k)
        torch.manual_seed(H)
        T = 3
        zs = [13, 28, 29]
        mods = [PaiNNModule(hidden_channels=H, num_rbf=16).to(dev) for _ in range(T)]
        w = LayerWeights(mods).refresh()
        z = torch.tensor(zs + [1], device=dev)[torch.randint(0, T + 1, (n,), device=dev)]      # (some atoms of an unknown element)
        g = RelationalGraph.build(z, torch.stack([torch.randint(0, n, (4 * n,), device=dev),
                                                  torch.randint(0, n, (4 * n,), device=dev)]), zs)
        N = g.N
        r = lambda *s: torch.randn(*s, device=dev)
        gn, gv, x, gx1, gvec1 = r(T, N, H), r(T, N, 3, H), r(N, H), r(N, H), r(N, 3, H)
        mean, rstd = x.mean(1), 1.0 / (x.var(1, unbiased=False) + 1e-5).sqrt()
        vp, h2b, q23, nrm = r(N, 3, 2 * H), r(N, H), r(N, 2 * H), r(N, H).abs() + 0.5
        # the separate launches: LayerNorm backward over the parts + residual, sums of the gvec slices + residual
        ident = torch.zeros(N, 1, device=dev)
        ident[:g.type_rowptr_host[-1]] = 1.0
        gxo = nodeops.layernorm_bwd(gn.sum(0) if False else (gn[0] + gn[1] + gn[2]), x, mean, rstd,
                                    add=gx1 * 0.70710678118654752 * ident)
        gvo = gv[0] + gv[1] + gv[2] + gvec1 * ident[:, :, None]
        want = nodeops.node_update_bwd(gxo, gvo, vp, h2b, q23, nrm, w, g)
        bx, bv = torch.full_like(gxo, float("nan")), torch.full_like(gvo, float("nan"))
        pend = nodeops.PendingGrads(bx, bv, gn, gv, x, mean, rstd, gx1, gvec1, 0)
        got = nodeops.node_update_bwd(bx, bv, vp, h2b, q23, nrm, w, g, pending=pend)
        k = g.type_rowptr_host[-1]
        assert rel_err(bx[:k], gxo[:k]) < 2e-6 and rel_err(bv[:k], gvo[:k]) < 2e-6, H
        assert rel_err(got[0], want[0]) < 5e-6 and rel_err(got[1], want[1]) < 5e-6, H


class _FakeAtoms(object):
    """Duck-typed stand-in for ase.Atoms (ASE is not installed on the MI355X image)."""

    def __init__(self, pos, z, cell):
        from hermnet_amd.elements import chemical_symbols
        self.positions = pos
        self._sym = [chemical_symbols[int(v)] for v in z]
        self.cell = cell
        self.pbc = [cell is not None] * 3

    def get_chemical_symbols(self):
        return self._sym


@pytest.mark.parametrize("name", ["alloy108", "mol16"])
def test_calculator_plugin_energy_forces_virial(name):
    """NNCalculator / model_calc (plugin/ase_interface/calculator.py:30-98 intent) incl. the NPT virial
    (utils.py:138-160) against the oracle differentiated w.r.t. the cell."""
    from hermnet_amd.plugin import NNCalculator
    from hermnet_amd.utils import virial_calc
    from oracle import hermnet_oracle as orc
    dev = _dev()
    g = Golden(name)
    d = g.data()
    if name == "mol16":      # one molecule of the batch, open boundaries
        keep = d.batch == 0
        pos, z, cell = d.pos[keep].numpy(), d.atomic_number[keep].numpy(), None
    else:
        pos, z, cell = d.pos.numpy(), d.atomic_number.numpy(), d.cell[0].numpy()
    calc = NNCalculator(g.model(), None, trn_mean=0.25, device_="cuda:0", ensemble="NPT")
    atoms = _FakeAtoms(pos.astype("float64"), z, cell)
    calc.calculate(atoms, ["energy", "forces", "stress"])
    # oracle on the same graph (the plugin builds it with the build's own neighbour search)
    from hermnet_amd.plugin import build_graph
    dd = build_graph(cell, z, pos, calc.model.rc)
    sd = g.model().state_dict()
    p = dd.pos.clone().requires_grad_(True)
    c = dd.cell.clone().requires_grad_(True) if cell is not None else None
    e = orc.hvnet_energy(sd, g.elems, p, dd.atomic_number, dd.edge_index, dd.batch, dd.get("edge_shift"), c,
                         **g.oracle_kwargs()) + 0.25
    f = -torch.autograd.grad(e.sum(), p, retain_graph=cell is not None)[0]
    w_ev = virial_calc(c, p.detach(), f, e, "lj", pbc=cell is not None).detach()      # W in eV (unit factor 1)
    v = w_ev * 1.6021765e6                                                               # "metal": utils.py:139-140
    vv = torch.tensor([v[0, 0], v[1, 1], v[2, 2], v[0, 1], v[0, 2], v[1, 2]])
    assert abs(calc.results["energy"] - float(e)) < 1e-5 * abs(float(e))
    assert rel_err(torch.from_numpy(calc.results["forces"]), f) < TOL
    assert calc.results["free_energy"] == calc.results["energy"]
    # LAMMPS packing (pressure*volume, [xx,yy,zz,xy,xz,yz]) stays behind model_calc (lmp_calc.py:58-67,232-235)
    _, f_l, v_l = calc.model_calc(build_graph(cell, z, pos, calc.model.rc, device="cuda:0"), "cuda:0", cell is not None, "NPT")
    assert rel_err(torch.from_numpy(f_l), f) < TOL
    assert rel_err(torch.from_numpy(np.asarray(v_l, dtype="float32")), vv) < 5e-5
    # ASE contract for results['stress']: -W / V in eV/A^3, Voigt [xx,yy,zz,yz,xz,xy]; an open system has none
    st = np.asarray(calc.results["stress"], dtype="float64")
    assert st.shape == (6,)
    if cell is None:
        assert not st.any()
    else:
        sig = -w_ev.double().numpy() / abs(np.linalg.det(cell.astype("float64")))
        want = np.array([sig[0, 0], sig[1, 1], sig[2, 2], sig[1, 2], sig[0, 2], sig[0, 1]])
        assert np.abs(st - want).max() < 5e-5 * np.abs(want).max()


def test_ase_stress_equals_strain_derivative_of_the_oracle_energy():
    """`results['stress']` under ASE's contract (the intent of plugin/ase_interface/calculator.py:85-97): sigma_jk =
    (1/V) dE/d(eps_jk) for a symmetric strain, eV/A^3, Voigt [xx,yy,zz,yz,xz,xy].  Checked against central
    differences of the float64 ORACLE energy on a strained TRICLINIC cell (fixed neighbour topology: the same
    (i, j, S) list, coordinates and cell strained together), all six components; NVT ensemble, stress requested
    through `properties` as ASE does."""
    from hermnet_amd.plugin import NNCalculator, build_graph
    from oracle import hermnet_oracle as orc
    _dev()
    g = Golden("alloy108")
    d = g.data()
    cell0 = d.cell[0].numpy().astype("float64")
    shear = np.eye(3) + np.array([[0.0, 0.0, 0.0], [0.06, 0.0, 0.0], [-0.04, 0.05, 0.0]])   # rows: lattice vectors
    # (rounded to float32 values: the calculator uploads float32 coordinates, the oracle gets the same numbers)
    cell = (cell0 @ shear).astype("float32").astype("float64")
    pos = (d.pos.numpy().astype("float64") @ shear).astype("float32").astype("float64")
    z = d.atomic_number.numpy()
    calc = NNCalculator(g.model(), None, trn_mean=0.0, device_="cuda:0", ensemble="NVT")
    calc.calculate(_FakeAtoms(pos, z, cell), ["energy", "stress"])
    st = np.asarray(calc.results["stress"], dtype="float64")
    dd = build_graph(cell, z, pos, calc.model.rc)          # host neighbour list of the sheared cell
    sd = {k: v.double() for k, v in g.model().state_dict().items()}
    vol = abs(np.linalg.det(cell))

    def energy(eps):
        m = torch.from_numpy(np.eye(3) + eps)
        p = torch.from_numpy(pos) @ m
        c = (torch.from_numpy(cell) @ m).reshape(1, 3, 3)
        return float(orc.hvnet_energy(sd, g.elems, p, dd.atomic_number, dd.edge_index, dd.batch,
                                      dd.edge_shift.double(), c, **g.oracle_kwargs()).sum())

    h = 1e-5
    voigt = [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
    fd = np.zeros(6)
    for k, (a, b) in enumerate(voigt):
        eps = np.zeros((3, 3))
        eps[a, b] += 0.5
        eps[b, a] += 0.5
        fd[k] = (energy(h * eps) - energy(-h * eps)) / (2 * h) / vol
    assert np.abs(st - fd).max() < 5e-5 * np.abs(fd).max(), (st, fd)
    assert np.abs(fd).min() > 0                # every component is exercised (sheared cell, jittered atoms)


@pytest.mark.parametrize("name", ["c1_si64", "alloy108", "alloy108_unknown_type", "mol16"])
@pytest.mark.parametrize("uniform", [None, False, True])
def test_native_relation_build_is_bit_exact(name, uniform, monkeypatch):
    """Device-side relation build (csrc/relation_kernels.hip) vs the PyTorch restatement: every
    index array identical (integer work: bit-exact is the bar)."""
    dev = _dev()
    g = Golden(name)
    d = g.data().to(dev)
    zl = [atomic_numbers[e] for e in g.elems]
    shift = d.get("edge_shift") if d.get("cell") is not None else None
    nat = RelationalGraph.build(d.atomic_number, d.edge_index, zl, shift, d.batch, uniform=uniform)
    ref = RelationalGraph._build_torch(d.atomic_number, d.edge_index, zl, shift, d.batch, uniform=uniform)
    assert (nat.N, nat.E, nat.T, nat.num_atoms, nat.uniform, nat.block, nat.num_graphs) == \
           (ref.N, ref.E, ref.T, ref.num_atoms, ref.uniform, ref.block, ref.num_graphs)
    assert nat.type_rowptr_host == ref.type_rowptr_host
    for f in ["node_order", "row_of_node", "z_rows", "type_rowptr", "csr_rowptr", "csr_src", "csr_perm", "csc_rowptr",
              "csc_tgt", "csc_pos", "out_rowptr", "out_edges", "src_id", "tgt_id", "row_real", "row_active", "shift",
              "graph_perm", "graph_lengths"]:
        a, b = getattr(nat, f), getattr(ref, f)
        if f in ("out_rowptr", "out_edges") and a is None:
            continue     # the device build skips the out-adjacency (the position gradient reads the CSC order); see below
        if b is None:
            assert a is None, f
            continue
        n_valid = b.numel()
        if f in ("csc_tgt", "csc_pos"):      # entries past the edges with a known-relation target are undefined
            n_valid = int(ref.csc_rowptr[-1])
        assert torch.equal(a.reshape(-1)[:n_valid].long() if a.dtype != torch.float32 else a.reshape(-1)[:n_valid],
                           b.reshape(-1)[:n_valid].long() if b.dtype != torch.float32 else b.reshape(-1)[:n_valid]), f
    # position gradient: out-edges from the CSC order (device build) == from the out-adjacency (torch build)
    from hermnet_amd import _lib
    from hermnet_amd.ops import _stream
    lib = _lib.load()
    gD = torch.randn(nat.E, 4, generator=torch.Generator().manual_seed(2)).to(dev)
    # edges to unknown-element targets carry no message: their gradient slots are zero in the real step
    known_edge = torch.zeros(nat.E, dtype=torch.bool, device=dev)
    known_edge[:int(ref.csr_rowptr[int(ref.type_rowptr_host[-1])])] = True
    gD = gD * known_edge[:, None]
    ga, gb = torch.empty(nat.N, 3, device=dev), torch.empty(nat.N, 3, device=dev)
    assert lib.hermnet_edge_geometry_bwd_csc(_lib.ptr(gD), _lib.ptr(nat.csr_rowptr), _lib.ptr(nat.csc_rowptr), _lib.ptr(nat.csc_pos),
                                             nat.T, nat.N, _lib.ptr(ga), _stream()) == 0
    assert lib.hermnet_edge_geometry_bwd(_lib.ptr(gD), _lib.ptr(ref.csr_rowptr), None, _lib.ptr(ref.out_rowptr),
                                         _lib.ptr(ref.out_edges), ref.N, _lib.ptr(gb), _stream()) == 0
    assert float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max().clamp(min=1e-30))
    # override of the relation activity (sharded runs)
    nat2 = RelationalGraph.build(d.atomic_number, d.edge_index, zl, shift, d.batch, rel_active=[True] + [False] * (len(zl) - 1),
                                 uniform=uniform)
    ref2 = RelationalGraph._build_torch(d.atomic_number, d.edge_index, zl, shift, d.batch,
                                        rel_active=[True] + [False] * (len(zl) - 1), uniform=uniform)
    assert torch.equal(nat2.row_active, ref2.row_active)


def test_config5_molecule_batch_1024_graphs_vs_oracle():
    """BASELINE.json configs[4]: 1,024 open-boundary molecules (<= 30 atoms) in one batch, HVNet,
    energies per graph and forces vs the CPU oracle (vectorised mode) on the same seeded inputs."""
    from oracle import hermnet_oracle as orc
    dev = _dev()
    data = synth.molecule_batch(num_graphs=1024)
    kw = dict(rc=5.0, num_layers=5, hidden_channels=128, num_rbf=128)      # the depth bench.py times this config at
    model = hn.HVNet(["H", "C", "O"], **kw).eval()
    sd = synth.synth_state_dict(model.state_dict(), 21)
    model.load_state_dict(sd)
    e_ref, f_ref = orc.energy_and_forces(sd, ["H", "C", "O"], data, mode="vectorised", **kw)
    model = model.to(dev)
    d = data.to(dev)
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    assert e.shape == (1024,)
    assert float((e.detach().cpu() - e_ref).abs().max() / e_ref.abs().max()) < TOL
    assert rel_err(f.cpu(), f_ref) < TOL
    # per-graph independence: evaluating one molecule alone gives the same energy
    keep = data.batch == 17
    one = hn.Data(pos=data.pos[keep], atomic_number=data.atomic_number[keep], batch=torch.zeros(int(keep.sum()), dtype=torch.long))
    one.edge_index = hn.neighbor_search(one.pos, 5.0)
    e1 = model(one.to(dev))
    assert abs(float(e1[0]) - float(e[17])) < 1e-5 * max(1.0, abs(float(e[17])))


def test_config4_slab_slice_vs_oracle():
    """A direct oracle link for BASELINE.json configs[3] (whose full 100,000-atom cell is property-checked below): a
    2,400-atom slab-shaped cell of the same lattice, composition statistics, model and WEIGHTS (fcc 10 x 10 x 6, the
    thickness of a rank's slab at 8 GPUs plus its halo), energy and forces vs the vectorised CPU oracle."""
    from oracle import hermnet_oracle as orc
    dev = _dev()
    kw = dict(rc=5.0, num_layers=5, hidden_channels=128, num_rbf=128)
    elems = ["Al", "Ni", "Cu"]
    model = hn.HVNet(elems, **kw).eval()
    sd = synth.synth_state_dict(model.state_dict(), 10)
    model.load_state_dict(sd)
    data = synth.fcc_alloy(reps=(10, 10, 6))
    assert data.pos.size(0) == 2400
    e_ref, f_ref = orc.energy_and_forces(sd, elems, data, mode="vectorised", **kw)
    model = model.to(dev)
    d = data.to(dev)
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    assert float((e.detach().cpu() - e_ref).abs().max() / e_ref.abs().max()) < TOL
    assert rel_err(f.cpu(), f_ref) < TOL


def test_config4_100k_atoms_properties():
    """BASELINE.json configs[3] at full size (100,000 atoms, single GPU here; the sharded variant is
    covered by tests/test_sharding.py): size-independent properties -- momentum conservation,
    extensivity against the 10k cell it replicates statistically, bit reproducibility."""
    dev = _dev()
    kw = dict(rc=5.0, num_layers=5, hidden_channels=128, num_rbf=128)
    model = hn.HVNet(["Al", "Ni", "Cu"], **kw).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
    model = model.to(dev)
    for p in model.parameters():
        p.requires_grad_(False)
    data = synth.fcc_alloy(reps=(10, 10, 250)).to(dev)
    assert data.pos.size(0) == 100000
    data.pos.requires_grad_(True)
    e = model(data)
    f = -torch.autograd.grad(e.sum(), data.pos)[0]
    assert torch.isfinite(e).all() and torch.isfinite(f).all()
    assert float(f.sum(0).abs().max()) < 1e-2 * float(f.abs().max())
    small = synth.fcc_alloy(reps=(10, 10, 25)).to(dev)
    e_small = model(small)
    assert abs(float(e[0]) / 100000 - float(e_small[0]) / 10000) < 0.02 * abs(float(e_small[0]) / 10000)
    data.pos.grad = None
    e2 = model(data)
    f2 = -torch.autograd.grad(e2.sum(), data.pos)[0]
    assert torch.equal(e, e2) and torch.equal(f, f2)


@pytest.mark.parametrize("case", ["cubic", "triclinic", "small_cell", "unwrapped", "open", "alloy10k", "molecule", "dense_stash_overflow"])
def test_device_neighbor_search_bit_exact_vs_host(case):
    """csrc/neighbor_kernels.hip vs the host cell list (itself checked against brute force on CPU):
    identical (i, j, S) lists, identical order -- 'neighbour indices bit-exact' (north_star)."""
    from hermnet_amd.neighbor import neighbor_search
    dev = _dev()
    rs = np.random.RandomState(3)
    cell, rc = None, 4.0
    if case == "cubic":
        cell = np.diag([9.0, 10.0, 11.0]); pos = rs.uniform(0, 1, size=(60, 3)) @ cell
    elif case == "triclinic":
        cell = np.array([[9.0, 0, 0], [2.0, 8.5, 0], [1.0, -1.5, 9.5]]); pos = rs.uniform(0, 1, size=(50, 3)) @ cell
    elif case == "small_cell":
        cell = np.diag([3.0, 3.5, 4.0]); pos = rs.uniform(0, 1, size=(5, 3)) @ cell; rc = 4.9
    elif case == "unwrapped":
        cell = np.diag([8.0, 8.0, 8.0]); rc = 3.5
        pos = rs.uniform(0, 1, size=(40, 3)) @ cell + rs.randint(-2, 3, size=(40, 3)) @ cell
    elif case == "open":
        pos = rs.uniform(-4, 4, size=(80, 3)); rc = 3.0
    elif case == "dense_stash_overflow":      # > 160 pairs per atom: the two-pass form behind the per-atom key stash
        d = synth.fcc_alloy(reps=(3, 3, 3)); pos = d.pos.numpy().astype(np.float64); cell = d.cell[0].numpy().astype(np.float64); rc = 8.0
    elif case == "alloy10k":
        d = synth.fcc_alloy(); pos = d.pos.numpy().astype(np.float64); cell = d.cell[0].numpy().astype(np.float64); rc = 5.0
    else:
        d = synth.molecule_batch(num_graphs=1); pos = d.pos.numpy().astype(np.float64); rc = 5.0
    p = torch.from_numpy(pos).float()
    c = None if cell is None else torch.from_numpy(cell).float()
    for compat in (False, True):
        host = neighbor_search(p, rc, c, reference_compat=compat)
        devr = neighbor_search(p.to(dev), rc, None if c is None else c.to(dev), reference_compat=compat)
        if cell is None:
            assert devr.is_cuda and torch.equal(devr.cpu(), host)
        else:
            assert devr[0].is_cuda and torch.equal(devr[0].cpu(), host[0]) and torch.equal(devr[1].cpu(), host[1])
    # lists of an atom shard: only the edges into flagged targets, straight from the search (both the stash and the
    # two-pass form)
    mask = torch.from_numpy(rs.rand(p.size(0)) < 0.5)
    host = neighbor_search(p, rc, c, target_mask=mask)
    devr = neighbor_search(p.to(dev), rc, None if c is None else c.to(dev), target_mask=mask.to(dev))
    if cell is None:
        assert torch.equal(devr.cpu(), host) and bool(mask[host[1]].all())
    else:
        assert torch.equal(devr[0].cpu(), host[0]) and torch.equal(devr[1].cpu(), host[1]) and bool(mask[host[0][1]].all())


def _oracle_vs_hip(data, elems, kw, seed, tol=TOL, e_floor=0.1):
    from oracle import hermnet_oracle as orc
    dev = _dev()
    model = hn.HVNet(elems, **kw).eval()
    sd = synth.synth_state_dict(model.state_dict(), seed)
    model.load_state_dict(sd)
    okw = dict(rc=kw.get("rc", 5.0), num_layers=kw["num_layers"], hidden_channels=kw["hidden_channels"],
               num_rbf=kw["num_rbf"], intensive=kw.get("intensive", False))
    e_ref, f_ref = orc.energy_and_forces(sd, elems if isinstance(elems, list) else [elems], data, **okw)
    model = model.to(dev)
    d = hn.Data(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in data}).to(dev)
    d.pos.requires_grad_(True)
    e = model(d)
    g = torch.autograd.grad(e.sum(), d.pos, allow_unused=True)[0] if e.requires_grad else None
    f = torch.zeros_like(d.pos) if g is None else -g
    # (energies of a few atoms can cancel to ~1e-2 while the per-atom terms are O(1): absolute floor 1e-6)
    assert float((e.detach().cpu() - e_ref).abs().max()) <= tol * max(float(e_ref.abs().max()), e_floor), (e, e_ref)
    assert float((f.cpu() - f_ref).abs().max()) <= tol * max(float(f_ref.abs().max()), 1e-3)
    return e.detach().cpu(), f.cpu()


@pytest.mark.parametrize("case", ["fcc", "triclinic", "unknown_element"])
def test_padded_neighbour_list_gives_the_exact_lists_results_bit_for_bit(case):
    """SURVEY 8(f) row 1 (data.py:14-24 is rebuilt every step, calculator.py:49): the device list WITHOUT its host read --
    `neighbor_search_padded` fills a capacity with the pairs found and NULL edges (-1, -1) behind them, the relation build
    files those behind every row, and every kernel of the step runs on the padded arrays.  Energy and forces must be
    bit-identical to the exact list's; count and flags arrive on the device; a capacity that is too small is reported."""
    from hermnet_amd.neighbor import neighbor_search_padded, padded_list_ok
    dev = _dev()
    if case == "triclinic":
        rs = np.random.RandomState(4)
        cell = np.array([[11.0, 0.0, 0.0], [2.5, 12.0, 0.0], [-1.5, 3.0, 13.0]])
        pos = rs.rand(260, 3) @ cell
        z = rs.choice([13, 28, 29], size=260)
    else:
        pos, cell, z = synth.fcc_alloy_atoms(reps=(3, 3, 5))
        if case == "unknown_element":
            z = z.copy()
            z[::7] = 79
    pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
    cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
    z_t = torch.from_numpy(z).to(dev)
    kw = dict(rc=5.0, num_layers=3, hidden_channels=128, num_rbf=64)
    model = hn.HVNet(["Al", "Ni", "Cu"], **kw).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 5))
    model = model.to(dev)
    for p_ in model.parameters():
        p_.requires_grad_(False)
    ei, sh = hn.neighbor_search(pos_t, 5.0, cell_t)
    E = int(ei.size(1))
    batch = torch.zeros(len(z), dtype=torch.long, device=dev)

    def run(ei_, sh_, total=None):
        d = hn.Data(pos=pos_t.clone().requires_grad_(True), atomic_number=z_t, batch=batch, cell=cell_t.reshape(1, 3, 3),
                    edge_index=ei_, edge_shift=sh_)
        if total is not None:
            d._hn_edge_count = total
        e = model(d)
        return e.detach(), -torch.autograd.grad(e.sum(), d.pos)[0]

    e0, f0 = run(ei, sh)
    for cap in (E + 777, E):
        eip, shp, total = neighbor_search_padded(pos_t, 5.0, cell_t, cap)
        assert padded_list_ok(total) == (True, E)
        assert torch.equal(eip[:, :E], ei) and torch.equal(shp[:E], sh)
        assert bool((eip[:, E:] == -1).all()) and float(shp[E:].abs().sum()) == 0.0
        os.environ["HERMNET_DEBUG_POISON"] = "1"          # unwritten edge-gradient slots would poison the forces
        try:
            e1, f1 = run(eip, shp, total)
        finally:
            os.environ["HERMNET_DEBUG_POISON"] = "0"
        assert torch.equal(e0, e1) and torch.equal(f0, f1)
    _, _, total = neighbor_search_padded(pos_t, 5.0, cell_t, E - 5)
    ok, found = padded_list_ok(total)
    assert not ok and found == E


def test_a_weight_written_through_dot_data_never_gives_the_old_numbers():
    """the kernel-ready parameter copies are keyed on (identity, version, address) of every parameter; a
    write through `.data` changes none of them.  The device-side guard (`hermnet_param_guard`, one launch per forward)
    must answer the first step after such a write with NaN -- never with the OLD numbers -- and the following step, which
    reads the guard's flag, with the NEW numbers (equal to a model whose caches were invalidated by hand)."""
    import warnings
    dev = _dev()
    g = Golden("alloy108")
    model = g.model().to(dev).eval()
    d0 = g.data().to(dev)

    def run(m):
        d = g.data().to(dev)
        d.pos = d0.pos.detach().clone().requires_grad_(True)
        e = m(d)
        f = -torch.autograd.grad(e.sum(), d.pos)[0]
        return e.detach().clone(), f.clone()

    e_old, f_old = run(model)
    assert rel_err(e_old.cpu(), g.energy) < TOL
    e_again, _ = run(model)
    assert torch.equal(e_old, e_again)                       # an unchanged model passes its checks
    name, p_ = [(n, p) for n, p in model.named_parameters() if n.endswith("update_layer.xvec_proj.2.weight")][1]
    v0 = p_._version
    p_.data.mul_(1.5)
    assert p_._version == v0                                 # (the hazard: nothing the cache key looks at has moved)
    e1, f1 = run(model)
    torch.cuda.synchronize()
    assert bool(torch.isnan(e1).all()) and bool(torch.isnan(f1).any()), "a step on stale copies must not give numbers"
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        e2, f2 = run(model)
    assert any("modified behind the cached" in str(w.message) for w in rec)
    assert bool(torch.isfinite(e2).all()) and not torch.equal(e2, e_old)
    model.invalidate_caches()
    e3, f3 = run(model)
    assert torch.equal(e2, e3) and torch.equal(f2, f3)
    # the same weights loaded into a fresh module agree with the oracle
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    from oracle import hermnet_oracle as orc
    e_ref, f_ref = orc.energy_and_forces(sd, g.elems, g.data(), **g.oracle_kwargs())
    assert rel_err(e2.cpu(), e_ref) < TOL and rel_err(f2.cpu(), f_ref) < TOL
    # load_state_dict / .to() / train()-eval() transitions invalidate by themselves, and a second write is caught again
    p_.data.mul_(1.0 / 1.5)
    model.load_state_dict(model.state_dict())
    e4, _ = run(model)
    assert rel_err(e4.cpu(), g.energy) < TOL


def test_padded_list_with_an_overflowing_stash_holds_no_uninitialised_column():
    """an atom with more pairs than its stash slot (flag bit 1) left the columns offset[i] + stride ..
    offset[i] + count - 1 of the padded list unwritten, and the model -- which an MD loop runs BEFORE the host reads the
    flags -- followed whatever int64 sat there out of bounds.  With the smallest slot (8 keys; fcc at 5 A has 42 pairs per
    atom) every atom overflows: every column must be a real pair of the exact list or a NULL edge, the buffers being
    poisoned first; the step on that list must run (its energy is meaningless, the flags say so), and the repeat on the
    exact list gives the right answer."""
    from hermnet_amd import neighbor as nb
    dev = _dev()
    pos, cell, z = synth.fcc_alloy_atoms(reps=(3, 3, 4))
    pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
    cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
    z_t = torch.from_numpy(z).to(dev)
    ei, sh = hn.neighbor_search(pos_t, 5.0, cell_t)
    E, N = int(ei.size(1)), len(z)
    exact = set(map(tuple, torch.cat([ei.t(), sh.long()], 1).tolist()))
    saved = dict(nb._STASH)
    os.environ["HERMNET_DEBUG_POISON"] = "1"
    try:
        nb._STASH[str(dev)] = 8
        eip, shp, total = nb.neighbor_search_padded(pos_t, 5.0, cell_t, E + 333)
        found, flags = total.tolist()
        assert found == E and (flags & 2)
        null = eip[0] < 0
        assert bool((eip[1][null] == -1).all()) and bool((eip[0][null] == -1).all()) and float(shp[null].abs().sum()) == 0.0
        real = torch.cat([eip.t()[~null], shp[~null].long()], 1).tolist()
        assert 0 < len(real) <= 8 * N and all(tuple(r) in exact for r in real)        # (a NaN shift would not be in the set)
        assert int(eip.max()) < N
        kw = dict(rc=5.0, num_layers=2, hidden_channels=128, num_rbf=64)
        model = hn.HVNet(["Al", "Ni", "Cu"], **kw).eval()
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 5))
        model = model.to(dev)
        d = hn.Data(pos=pos_t.clone().requires_grad_(True), atomic_number=z_t, batch=torch.zeros(N, dtype=torch.long, device=dev),
                    cell=cell_t.reshape(1, 3, 3), edge_index=eip, edge_shift=shp)
        d._hn_edge_count = total
        e = model(d)
        f = torch.autograd.grad(e.sum(), d.pos)[0]
        torch.cuda.synchronize()
        assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(f).all())
        ok, _ = nb.padded_list_ok(total)
        assert not ok and nb._STASH[str(dev)] == 160                     # the repeat gets the largest slot
        eip2, shp2, total2 = nb.neighbor_search_padded(pos_t, 5.0, cell_t, E + 333)
        assert nb.padded_list_ok(total2) == (True, E)
        assert torch.equal(eip2[:, :E], ei) and torch.equal(shp2[:E], sh) and bool((eip2[:, E:] == -1).all())
    finally:
        os.environ["HERMNET_DEBUG_POISON"] = "0"
        nb._STASH.clear()
        nb._STASH.update(saved)


def test_md_step_with_list_rebuild_replays_as_one_graph():
    """`GraphedMDStep`: neighbour search + relation build + forward + force backward captured ONCE, replayed along a random
    walk on which the list changes (different edge counts), with eager steps and unrelated work in between; every replay
    must equal the eager step on the exact list of the same coordinates bit for bit, and the list's edge count arrives
    with the results.  A capacity that becomes too small is reported and repaired by a recapture."""
    from hermnet_amd.graph import GraphedMDStep
    dev = _dev()
    pos, cell, z = synth.fcc_alloy_atoms(reps=(3, 3, 4))
    pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
    cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
    z_t = torch.from_numpy(z).to(dev)
    kw = dict(rc=5.0, num_layers=3, hidden_channels=128, num_rbf=64)
    model = hn.HVNet(["Al", "Ni", "Cu"], **kw).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 8))
    model = model.to(dev)
    for p_ in model.parameters():
        p_.requires_grad_(False)
    batch = torch.zeros(len(z), dtype=torch.long, device=dev)

    def exact(p):
        ei, sh = hn.neighbor_search(p, 5.0, cell_t)
        d = hn.Data(pos=p.clone().requires_grad_(True), atomic_number=z_t, batch=batch, cell=cell_t.reshape(1, 3, 3),
                    edge_index=ei, edge_shift=sh)
        e = model(d)
        return e.detach(), -torch.autograd.grad(e.sum(), d.pos)[0], int(ei.size(1))

    step = GraphedMDStep(model, z_t, cell_t, pos_t)
    gen = torch.Generator().manual_seed(2)
    cur = pos_t.clone()
    counts = set()
    for it in range(12):
        cur = cur + (0.25 * (torch.rand(cur.shape, generator=gen) - 0.5)).to(dev)
        e, f = step(cur)
        e, f = e.clone(), f.clone()
        ok, n = step.check()
        e0, f0, n0 = exact(cur)                                   # eager work between replays (memsets, sorts, ...)
        torch.zeros(1 << 16, device=dev).sum()
        assert ok and n == n0, (it, n, n0)
        assert torch.equal(e, e0) and torch.equal(f, f0), it
        counts.add(n)
    assert len(counts) > 3                                        # the list really changed along the walk
    small = GraphedMDStep(model, z_t, cell_t, pos_t, capacity=1024)
    small(cur)
    ok, n = small.check()
    assert not ok and n == n0
    e, f = small.recapture(cur)
    assert small.check() == (True, n0) and torch.equal(e, e0) and torch.equal(f, f0)


def test_calculator_builds_its_lists_without_a_host_read_after_the_first_call():
    """`NNCalculator.calculate` along a trajectory: the first call searches exactly (and learns a capacity), the following
    ones use padded lists checked behind the step; results equal a fresh calculator's exact evaluation of the same
    coordinates, also when the list outgrows its capacity (that step is repeated exactly)."""
    from hermnet_amd.plugin import NNCalculator
    _dev()
    g = Golden("alloy108")
    d = g.data()
    z, cell = d.atomic_number.numpy(), d.cell[0].numpy().astype("float64")
    rs = np.random.RandomState(1)
    calc = NNCalculator(g.model(), None, trn_mean=0.0, device_="cuda:0")
    ref = NNCalculator(g.model(), None, trn_mean=0.0, device_="cuda:0")
    pos = d.pos.numpy().astype("float64")
    for it in range(4):
        if it == 3:
            calc._edge_capacity = 256                    # far too few columns: the step must notice and redo
        calc.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])
        ref._edge_capacity = None                        # always the exact search
        ref.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])
        assert calc.results["energy"] == ref.results["energy"]
        assert np.array_equal(calc.results["forces"], ref.results["forces"])
        assert (calc._edge_capacity is not None) and (it == 0 or calc._edge_capacity >= 256)
        pos = pos + rs.normal(scale=0.03, size=pos.shape)


def test_calculator_replays_a_captured_step_and_renews_the_capture_when_it_must():
    """`NNCalculator(graph_replay=True)`: the calls of a trajectory replay ONE captured hipGraph (search + relation build +
    forward + force backward); results equal the eager calculator's on the same coordinates (same kernels, same order:
    bit for bit).  The capture is renewed when the weights are reloaded (the derived copies a capture points at are gone)
    and when the list outgrows its columns; a call that needs the stress takes the eager path and leaves the capture
    alone; other species capture again."""
    from hermnet_amd.plugin import NNCalculator
    _dev()
    g = Golden("alloy108")
    d = g.data()
    z, cell = d.atomic_number.numpy(), d.cell[0].numpy().astype("float64")
    rs = np.random.RandomState(2)
    calc = NNCalculator(g.model(), None, trn_mean=0.25, device_="cuda:0", graph_replay=True)
    ref = NNCalculator(g.model(), None, trn_mean=0.25, device_="cuda:0")
    pos = d.pos.numpy().astype("float64")

    def both(pos, z=z, props=("energy", "forces")):
        calc.calculate(_FakeAtoms(pos, z, cell), list(props))
        ref._edge_capacity = None
        ref.calculate(_FakeAtoms(pos, z, cell), list(props))
        assert calc.results["energy"] == ref.results["energy"]
        assert np.array_equal(calc.results["forces"], ref.results["forces"])

    for it in range(4):
        both(pos)
        assert "stress" not in calc.results
        pos = pos + rs.normal(scale=0.03, size=pos.shape)
    assert calc.graph_captures == 1
    both(pos, props=("energy", "forces", "stress"))                 # eager, with the stress
    assert np.allclose(calc.results["stress"], ref.results["stress"]) and calc.graph_captures == 1
    sd = {k: v.clone() for k, v in calc.model.state_dict().items()}
    sd["out_energy.2.bias"] = sd["out_energy.2.bias"] + 1.0         # new weights: every atom's energy + 1
    e_before = calc.results["energy"]
    calc.model.load_state_dict(sd)
    ref.model.load_state_dict(sd)
    both(pos)
    assert calc.graph_captures == 2 and abs(calc.results["energy"] - e_before - len(z)) < 1e-2
    z2 = z.copy()
    z2[:5] = z2[5:10]                                                # other species: another capture
    both(pos, z=z2)
    assert calc.graph_captures == 3
    # a list that outgrows the captured capacity: squeeze the cell's atoms together -> more pairs than columns
    small = NNCalculator(g.model(), None, trn_mean=0.0, device_="cuda:0", graph_replay=True)
    small.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])
    step = small._graphed[1]
    step.recapture(capacity=1024)                                    # far too few columns for this cell
    small.graph_captures = 1
    small.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])
    ref = NNCalculator(g.model(), None, trn_mean=0.0, device_="cuda:0")
    ref.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])
    assert small.graph_captures == 2 and small._graphed[1].capacity > 1024
    assert small.results["energy"] == ref.results["energy"] and np.array_equal(small.results["forces"], ref.results["forces"])


@pytest.mark.parametrize("graph_replay", [False, True])
def test_calculators_never_hand_out_nan_after_a_write_through_dot_data(graph_replay):
    """the stale-cache guard answers a write through `.data` (an EMA swap) with a NaN step.  Eagerly the
    calculator handed that ONE NaN step to ASE; with `graph_replay` the check-and-poison kernel is captured and its flag
    never read, so EVERY replay came back NaN.  Now a non-finite energy on the host drops the caches (and the capture),
    re-evaluates the same call with the current weights, warns once -- and raises if it is still not finite."""
    import warnings
    from hermnet_amd.plugin import NNCalculator
    _dev()
    g = Golden("alloy108")
    d = g.data()
    z, cell = d.atomic_number.numpy(), d.cell[0].numpy().astype("float64")
    pos = d.pos.numpy().astype("float64")
    calc = NNCalculator(g.model(), None, trn_mean=0.0, device_="cuda:0", graph_replay=graph_replay)
    for _ in range(3):                       # (the guard arms on the second forward; a capture on the first call)
        calc.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])
    e_old = calc.results["energy"]
    p_ = [p for n, p in calc.model.named_parameters() if n.endswith("update_layer.xvec_proj.2.weight")][1]
    p_.data.mul_(1.5)                        # nothing a cache key looks at moves
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for it in range(3):
            calc.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])
            assert np.isfinite(calc.results["energy"]) and np.isfinite(calc.results["forces"]).all(), it
            assert calc.results["energy"] != e_old, "the OLD numbers after the weights changed"
    assert any("NaN" in str(w.message) or "modified behind" in str(w.message) for w in rec)
    fresh = NNCalculator(g.model(), None, trn_mean=0.0, device_="cuda:0")
    fresh.model.load_state_dict({k: v.clone() for k, v in calc.model.state_dict().items()})
    fresh.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])
    assert abs(calc.results["energy"] - fresh.results["energy"]) <= 1e-5 * abs(fresh.results["energy"])
    assert np.abs(calc.results["forces"] - fresh.results["forces"]).max() <= 1e-5 * np.abs(fresh.results["forces"]).max()


def test_a_model_with_an_armed_guard_deep_copies_and_pickles():
    """from the second eval() forward on `HVNet.__dict__['_guard']` held a HIP event and
    `copy.deepcopy(model)` (what `torch.optim.swa_utils.AveragedModel` and best-model snapshots do) / `torch.save(model)`
    raised "cannot pickle 'Event' object".  Copies and pickles now carry no guard; the copy arms its own."""
    import copy
    import io
    dev = _dev()
    g = Golden("alloy108")
    model = g.model().to(dev).eval()

    def run(m):
        d = g.data().to(dev)
        d.pos.requires_grad_(True)
        e = m(d)
        return e.detach().clone(), -torch.autograd.grad(e.sum(), d.pos)[0]

    run(model)
    e, f = run(model)
    assert model.__dict__["_guard"]._event is not None          # armed: the situation of the finding
    clone = copy.deepcopy(model)
    assert clone.__dict__.get("_guard") is None
    e_c, f_c = run(clone)
    run(clone)
    assert torch.equal(e, e_c) and torch.equal(f, f_c) and clone.__dict__["_guard"] is not model.__dict__["_guard"]
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    e_l, f_l = run(loaded)
    assert torch.equal(e, e_l) and torch.equal(f, f_l)
    from torch.optim.swa_utils import AveragedModel
    ema = AveragedModel(model)                                   # deep-copies the model
    e_a, _ = run(ema.module)
    assert torch.equal(e, e_a)
    # the copy is guarded on its own: a write through .data to the COPY gives NaN there, the original is untouched
    p_ = [p for n, p in clone.named_parameters() if n.endswith("update_layer.xvec_proj.2.weight")][1]
    p_.data.mul_(1.5)
    e_bad, _ = run(clone)
    assert bool(torch.isnan(e_bad).all()) and torch.equal(run(model)[0], e)


@pytest.mark.parametrize("T,N,H,n", [(3, 500, 128, 77), (1, 64, 64, 64), (3, 300, 128, 0), (2, 257, 192, 5)])
def test_halo_proj_rows_kernels_match_the_restatement(T, N, H, n):
    """hermnet_halo_proj_rows / _accumulate (ABI v12) through the C ABI against tests/ref_ops.py, bit for bit: pack (forward:
    xh [T, N, 3H] | vec; backward: gxh | the per-relation partial sums of gvec, summed in ascending relation order), pack-and-clear,
    unpack, and the owner's ordered accumulation with an atom that several peers return (duplicates in the send list)."""
    from hermnet_amd import nodeops
    from hermnet_amd.sharding import ExchangePlan
    dev = _dev()
    gen = torch.Generator().manual_seed(T * 1000 + N + n)
    W = 3 * H
    xh, vec = torch.randn(T, N, W, generator=gen), torch.randn(N, 3, H, generator=gen)
    gv = torch.randn(T, N, 3, H, generator=gen)
    idx = torch.randperm(N, generator=gen)[:n].contiguous()
    c = lambda t: t.to(dev).clone()
    # pack, forward form (b without a slice axis)
    got = nodeops.halo_proj_rows(0, c(xh), c(vec), idx.to(dev))
    ref = ref_ops.halo_proj_rows(0, xh.clone(), vec.clone(), idx)
    assert got.shape == (n, (T + 1) * W) and torch.equal(got.cpu(), ref)
    # pack and clear, backward form (T slices summed in ascending order while they are packed)
    a_d, b_d, a_r, b_r = c(xh), c(gv), xh.clone(), gv.clone()
    got = nodeops.halo_proj_rows(1, a_d, b_d, idx.to(dev))
    ref = ref_ops.halo_proj_rows(1, a_r, b_r, idx)
    want_last = gv[0].reshape(N, W).index_select(0, idx)
    for t in range(1, T):
        want_last = want_last + gv[t].reshape(N, W).index_select(0, idx)      # the kernel's order: ((s0 + s1) + s2)
    assert torch.equal(got.cpu()[:, :T * W], ref[:, :T * W]) and torch.equal(got.cpu()[:, T * W:], want_last)
    assert torch.allclose(got.cpu(), ref, rtol=0, atol=1e-5)
    assert torch.equal(a_d.cpu(), a_r) and torch.equal(b_d.cpu(), b_r)          # cleared rows, the others untouched
    # unpack
    buf = torch.randn(n, (T + 1) * W, generator=gen)
    a_d, b_d, a_r, b_r = c(xh), c(vec), xh.clone(), vec.clone()
    nodeops.halo_proj_rows(2, a_d, b_d, idx.to(dev), c(buf))
    ref_ops.halo_proj_rows(2, a_r, b_r, idx, buf.clone())
    assert torch.equal(a_d.cpu(), a_r) and torch.equal(b_d.cpu(), b_r)
    # the owner's accumulate: send list with repeats (an atom that is a halo atom of two peers), list order
    if n > 0:
        send = torch.cat([idx, idx[: max(n // 3, 1)]])
        plan = ExchangePlan(send.to(dev), [send.numel()], send.to(dev)[:0], [0])
        back = torch.randn(send.numel(), (T + 1) * W, generator=gen)
        a_d, b_d = c(xh), c(gv)
        nodeops.halo_proj_accumulate(a_d, b_d, plan, c(back))
        a_r, b_r = xh.clone(), gv.clone()
        rows, ptr, pos = [t_.cpu() for t_ in plan.accumulate_lists()]
        for u in range(rows.numel()):                      # ordered sums, exactly as the kernel adds them
            r = int(rows[u])
            for q in pos[int(ptr[u]):int(ptr[u + 1])].tolist():
                a_r[:, r] += back[q, :T * W].view(T, W)
                b_r[0, r] += back[q, T * W:].view(3, H)
        assert torch.equal(a_d.cpu(), a_r) and torch.equal(b_d.cpu(), b_r)


@pytest.mark.parametrize("nc,C,N", [(5, 1024, 384), (3, 64, 96), (7, 256, 192), (2, 32, 32), (4, 1024, 480), (0, 1024, 384), (3, 128, 128),
                                     (2, 192, 256), (300, 1024, 384)])
def test_band_product_kernels_match_fp64(nc, C, N):
    """hermnet_band_product / _grad_a / _grad_b (ABI v13; rbf_proj of the training path on the bucketed basis,
    /root/reference/HermNet/rmnet.py:55) through the C ABI against fp64 products: with and without the bias, with one and with
    two gradient addends; exact fp32 products, so the error is the accumulation's (<= 2e-6 of the operand scale).  Run twice:
    bit-identical (fixed summation order)."""
    from hermnet_amd.trainops import band_product, BandQ, BandS, _band_kernels
    dev = _dev()
    gen = torch.Generator().manual_seed(nc * 7 + C + N)
    r = lambda *s: torch.randn(*s, generator=gen)
    A, B, b, g1, g2 = r(nc, C, 32), r(nc, 32, N), r(nc, N), r(nc, C, N), r(nc, C, N)
    assert _band_kernels(A.to(dev), N)
    d = lambda t: t.double()
    close = lambda got, ref, scale: float((got.cpu().double() - ref).abs().max()) <= 2e-6 * scale if ref.numel() else True
    for bias in (b, None):
        out, out2 = band_product(A.to(dev), B.to(dev), None if bias is None else bias.to(dev))
        ref = torch.bmm(d(A), d(B)) + (0 if bias is None else d(bias)[:, None, :])
        assert out.data_ptr() == out2.data_ptr() and close(out, ref, 32 ** 0.5 * 4)
        assert torch.equal(out, band_product(A.to(dev), B.to(dev), None if bias is None else bias.to(dev))[0])
    for second in (None, g2):
        gs = d(g1) if second is None else d(g1) + d(g2)
        s_dev = None if second is None else second.to(dev)
        gA = BandQ.apply(g1.to(dev), s_dev, B.to(dev))
        assert close(gA, torch.bmm(gs, d(B).transpose(1, 2)), N ** 0.5 * 6)
        gB, gb = BandS.apply(A.to(dev), g1.to(dev), s_dev)
        assert close(gB, torch.bmm(d(A).transpose(1, 2), gs), C ** 0.5 * 6) and close(gb, gs.sum(1), C ** 0.5 * 6)
        assert torch.equal(gA, BandQ.apply(g1.to(dev), s_dev, B.to(dev)))
        gB2, gb2 = BandS.apply(A.to(dev), g1.to(dev), s_dev)
        assert torch.equal(gB, gB2) and torch.equal(gb, gb2)
        # the three from one pass over g1 (+ g2) (hermnet_band_product_grads; staged tiles for widths 128 / 256 / 384)
        from hermnet_amd import _lib
        from hermnet_amd.ops import _stream
        fa, fB, fb = torch.empty_like(gA), torch.empty_like(gB), torch.empty_like(gb)
        Ad, Bd, g1d, P = A.to(dev), B.to(dev), g1.to(dev), _lib.ptr
        for _ in range(2):
            _lib.check(_lib.load().hermnet_band_product_grads(P(Ad), P(Bd), P(g1d), P(s_dev), nc, C, N, P(fa), P(fB), P(fb), _stream()),
                       "hermnet_band_product_grads")
            assert close(fa, torch.bmm(gs, d(B).transpose(1, 2)), N ** 0.5 * 6)
            assert close(fB, torch.bmm(d(A).transpose(1, 2), gs), C ** 0.5 * 6) and close(fb, gs.sum(1), C ** 0.5 * 6)


def test_edge_cases_empty_and_degenerate_graphs():
    """Ragged / empty inputs: no edges at all, a single atom, only atoms of unlisted elements, an
    isolated atom next to a bonded cluster, a listed element without atoms (the reference crashes
    there; the build treats it as a no-op, as does the oracle)."""
    kw = dict(rc=5.0, num_layers=2, hidden_channels=128, num_rbf=128)
    # 1) atoms far apart: E = 0 -> every relation is skipped, rows are zero (hermnet.py:56-57)
    pos = torch.tensor([[0.0, 0, 0], [20.0, 0, 0], [0, 20.0, 0], [0, 0, 20.0]])
    d = hn.Data(pos=pos, atomic_number=torch.tensor([1, 6, 8, 1]), batch=torch.zeros(4, dtype=torch.long),
                edge_index=torch.zeros(2, 0, dtype=torch.long))
    e, f = _oracle_vs_hip(d, ["H", "C", "O"], kw, 31)
    assert float(f.abs().max()) == 0.0
    # 2) a single atom
    d = hn.Data(pos=torch.zeros(1, 3), atomic_number=torch.tensor([6]), batch=torch.zeros(1, dtype=torch.long),
                edge_index=torch.zeros(2, 0, dtype=torch.long))
    _oracle_vs_hip(d, ["C"], kw, 32)
    # 3) only unlisted elements (with edges between them)
    mol = synth.molecule_batch(num_graphs=2, species=(7, 9))
    _oracle_vs_hip(mol, ["H", "C", "O"], kw, 33)
    # 4) isolated atom + cluster, and a listed element ("O") that has no atoms
    mol = synth.molecule_batch(num_graphs=1, species=(1, 6))
    n = mol.pos.size(0)
    pos = torch.cat([mol.pos, torch.tensor([[40.0, 40.0, 40.0]])])
    d = hn.Data(pos=pos, atomic_number=torch.cat([mol.atomic_number, torch.tensor([1])]),
                batch=torch.zeros(n + 1, dtype=torch.long), edge_index=mol.edge_index)
    _oracle_vs_hip(d, ["H", "C", "O"], kw, 34)


@pytest.mark.parametrize("opts", [
    dict(bwd_lanes16=1),                            # the 16-lanes-per-edge backward (vec and layer 0)
    dict(bwd_lanes16=1, bwd_rows=24, fwd_rows=17),  # ... and non-default row chunks in both directions
    dict(bwd_cl_rows=48),                           # channel-per-lane backward on small chunks
    dict(node_chain_wide=1),                        # widths 128 / 256 on the panelled chain kernels (node_chain_wide.hip)
])
def test_alternative_kernel_variants(opts):
    """The non-default forms of the message kernels and the other kernel families (library options, include/hermnet_hip.h:
    HN_OPT_*; set for the block, restored behind it) must give the same energies and forces: four golden cases (H = 128
    and 256) at 1e-5."""
    from hermnet_amd import _lib
    dev = _dev()
    with _lib.options(**opts):
        for name in ["c1_si64", "alloy108", "mol16", "alloy32_h256"]:
            g = Golden(name)
            model = g.model().to(dev)
            d = g.data().to(dev)
            d.pos.requires_grad_(True)
            e = model(d)
            f = -torch.autograd.grad(e.sum(), d.pos)[0]
            ee, fe = rel_err(e.detach().cpu(), g.energy), rel_err(f.cpu(), g.forces)
            assert ee < 1e-5 and fe < 1e-5, (name, opts, ee, fe)
    assert _lib.get_option("bwd_lanes16") == 0


def test_skewed_composition_uses_tight_layout_and_matches_oracle():
    """4/6 Al, 1/6 Ni, 1/6 Cu: padding to equal blocks would cost > 15 %, so the rows are tight and the node GEMMs
    run per relation (biases in the GEMM epilogue instead of on load) -- the other branch of hermnet_amd/layer.py."""
    data = synth.fcc_alloy(reps=(3, 3, 3), species=(13, 13, 13, 13, 28, 29))
    zl = [13, 28, 29]
    g = RelationalGraph.build(data.atomic_number.to(_dev()), data.edge_index.to(_dev()), zl, data.edge_shift.to(_dev()),
                              data.batch.to(_dev()))
    assert not g.uniform
    _oracle_vs_hip(data, ["Al", "Ni", "Cu"], dict(rc=5.0, num_layers=3, hidden_channels=128, num_rbf=64), 77)


@pytest.mark.parametrize("H,R,layers", [(512, 128, 2), (64, 20, 3), (192, 50, 2), (96, 16, 2), (100, 32, 3), (50, 20, 2),
                                        (320, 40, 2), (384, 64, 2), (448, 30, 2), (300, 24, 2), (500, 32, 2),
                                        # beyond the chain kernels' 512: layer.GemmRelationalLayer, 9 and 16 column blocks
                                        (576, 24, 2), (520, 16, 2), (1024, 16, 2)])
def test_other_widths_vs_oracle(H, R, layers):
    """hidden_channels = 512 is the reference default (hermnet.py:86): 8 column blocks; odd num_rbf; and widths that
    are NOT a multiple of 64 (the reference accepts any, hermnet.py:84-88): 96, 100 and 50 run on the same kernels with
    zero-padded channels (layer.LayerWeights.refresh).  576, 520 (padded to 576) and 1024 (the widest: hermnet.MAX_PADDED_WIDTH)
    take library GEMMs joined by the stage kernels, and the read-out's stage form."""
    data = synth.fcc_alloy(reps=(2, 2, 3))
    _oracle_vs_hip(data, ["Al", "Ni", "Cu"], dict(rc=5.0, num_layers=layers, hidden_channels=H, num_rbf=R), 40 + H)


@pytest.mark.parametrize("R", [137, 138, 177, 192, 256, 286, 287])
def test_large_gaussian_basis_vs_oracle(R):
    """The reference accepts any `num_rbf` (hermnet.py:86, rmnet.py:155-158).  Up to 137 the rbf_proj column block fits one
    LDS tile of both message kernels; up to RadialBasis.FUSED_MAX_RBF = 286 the fused kernels run as two launches over
    tap-row windows (backward from 138, forward from 177); beyond it the Gaussian basis takes the materialised route
    (forward AND forces).  HERMNET_DEBUG_POISON: an edge owned by neither window would leave NaN in its gradient slot."""
    from hermnet_amd.rmnet import RadialBasis
    data = synth.fcc_alloy(reps=(2, 2, 3))
    kw = dict(rc=5.0, num_layers=2, hidden_channels=128, num_rbf=R)
    assert hn.HVNet(["Al"], **kw).radial_basis.fused == (R <= RadialBasis.FUSED_MAX_RBF)
    os.environ["HERMNET_DEBUG_POISON"] = "1"
    try:
        _oracle_vs_hip(data, ["Al", "Ni", "Cu"], kw, 300 + R)
    finally:
        del os.environ["HERMNET_DEBUG_POISON"]


@pytest.mark.parametrize("env", [{}, {"option:bwd_lanes16": 1}, {"switch:node_chain": False}])
@pytest.mark.parametrize("case", ["alloy108", "alloy108_h64", "alloy108_unknown_type", "mol16", "skewed", "width100"])
def test_edge_gradient_sink_is_fully_written(case, env, monkeypatch, request):
    """HVNet.forward hands the backward kernels an UNINITIALISED edge-gradient buffer when every edge has a target of a
    known element (hermnet.py: EdgeGradSink(zero=False)): every [layer, H/64, E] slot must then be written by whichever
    backward form runs.  HERMNET_DEBUG_POISON=1 fills the buffer with NaN first: a skipped slot would poison the forces.
    Covers the channel-per-lane and the 16-lanes-per-edge backward, a padded width, rows without edges, and an
    unknown-element case (which must take the zero-filled buffer)."""
    from hermnet_amd import _lib, switches
    monkeypatch.setenv("HERMNET_DEBUG_POISON", "1")
    for k, v in env.items():
        kind, name = k.split(":")
        if kind == "switch":
            monkeypatch.setattr(switches, name, v)
        else:
            old = _lib.set_option(name, v)
            request.addfinalizer(lambda n=name, o=old: _lib.set_option(n, o))
    dev = _dev()
    if case in ("skewed", "width100"):
        if case == "skewed":
            data = synth.fcc_alloy(reps=(2, 2, 3))
            z = data.atomic_number.clone()
            z[3:] = 13                                  # 3 atoms of two elements, the rest Al: tight layout, tiny blocks
            data.atomic_number = z
            kw = dict(rc=5.0, num_layers=2, hidden_channels=128, num_rbf=32)
        else:
            data = synth.molecule_batch(num_graphs=5, seed=3)
            kw = dict(rc=5.0, num_layers=2, hidden_channels=100, num_rbf=32)
        elems = ["Al", "Ni", "Cu"] if case == "skewed" else ["H", "C", "O"]
        # (36 per-atom energies of O(1) cancel to -0.2 here: the energy check gets an absolute floor of 3e-5)
        e, f = _oracle_vs_hip(data, elems, kw, 5, e_floor=3.0)
        assert torch.isfinite(f).all()
        return
    g = Golden(case)
    model = g.model().to(dev)
    d = g.data().to(dev)
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    assert torch.isfinite(f).all()
    assert rel_err(e.detach().cpu(), g.energy) < TOL and rel_err(f.cpu(), g.forces) < TOL


def test_width_not_multiple_of_64_molecule_batch_and_htnet():
    """any `hidden_channels` runs fused -- also for batches (intensive read-out) and HTNet."""
    data = synth.molecule_batch(num_graphs=6, seed=2)
    _oracle_vs_hip(data, ["H", "C", "O"], dict(rc=5.0, num_layers=2, hidden_channels=72, num_rbf=24, intensive=True), 5)
    from oracle import hermnet_oracle as orc
    kw = dict(rc=5.0, num_layers=2, hidden_channels=40, num_rbf=16)
    m = hn.HTNet(["H", "C", "O"], **kw).eval()
    sd = synth.synth_state_dict(m.state_dict(), 3)
    m.load_state_dict(sd)
    for p in m.parameters():
        p.requires_grad_(False)
    e_ref, f_ref = orc.htnet_energy_and_forces(sd, ["H", "C", "O"], data, **kw)
    d = hn.Data(**{k: v.clone() for k, v in data}).to(_dev())
    d.pos.requires_grad_(True)
    e = m.to(_dev())(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    assert rel_err(e.detach().cpu(), e_ref) < TOL and rel_err(f.cpu(), f_ref) < TOL


def test_double_or_half_model_is_refused_on_the_gpu():
    """`model.double()` must not hand fp64 pointers to fp32 kernels."""
    g = Golden("alloy108")
    d = g.data().to(_dev())
    for cast in ("double", "half"):
        with pytest.raises(TypeError, match="float32"):
            getattr(g.model().to(_dev()), cast)()(d)


@pytest.mark.parametrize("name", ["alloy108", "mol16"])
def test_whole_step_graph_replay_100_steps_bit_identical_to_eager(name):
    """relation build + forward + force backward captured once and replayed as one hipGraph.
    100 replays -- with eager steps and other device work in between, and with the coordinates changing -- must equal
    the eager step bit for bit (the single-GPU path has no atomics on floats, so eager itself is reproducible)."""
    from hermnet_amd.graph import GraphedStep
    dev = _dev()
    g = Golden(name)
    model = g.model().to(dev)
    for p in model.parameters():
        p.requires_grad_(False)

    def eager(pos):
        d = g.data().to(dev)
        d.pos = pos.clone().requires_grad_(True)
        e = model(d)
        return e.detach(), -torch.autograd.grad(e.sum(), d.pos)[0]

    data = g.data().to(dev)
    pos0 = data.pos.clone()
    step = GraphedStep(model, data)
    assert step.matches(data)
    gen = torch.Generator().manual_seed(4)
    for k in range(100):
        # small displacements: the neighbour LIST stays as captured (what the graph is valid for)
        pos = pos0 + 1e-3 * torch.randn(pos0.shape, generator=gen).to(dev)
        e, f = step(pos)
        e, f = e.clone(), f.clone()
        if k % 10 == 0:
            e_ref, f_ref = eager(pos)            # an eager step in between (this used to break the next replay)
            assert torch.equal(e, e_ref) and torch.equal(f, f_ref), k
            torch.zeros(1 << 20, device=dev).sum()      # unrelated memsets / reductions between replays
    e, f = step(pos0)
    assert rel_err(e.cpu(), g.energy) < 1e-5 and rel_err(f.cpu(), g.forces) < 1e-5


def test_a_captured_step_keeps_its_read_out_copies_whatever_another_model_does():
    """A capture bakes in the addresses of the model's kernel-ready copies; the read-out's (layer.HeadWeights) belong to the
    model like the layers'.  A second model in the process -- evaluated, invalidated, switched train() / eval(), evaluated
    again -- frees none of them: memory allocated and poisoned behind that cannot be theirs, the replay repeats bit for bit."""
    from hermnet_amd.graph import GraphedStep
    dev = _dev()
    g = Golden("c1_si64")                       # 64 Si atoms, H = 128, two layers
    model_a = g.model().to(dev)
    for p in model_a.parameters():
        p.requires_grad_(False)
    step = GraphedStep(model_a, g.data().to(dev))
    e0, f0 = (t.clone() for t in step())
    assert rel_err(e0.cpu(), g.energy) < 1e-5 and rel_err(f0.cpu(), g.forces) < 1e-5
    head = model_a._head
    assert head.w0f16 is not None and head.builds == 1

    model_b = hn.HVNet(g.elems, **g.model_kw)
    model_b.load_state_dict(synth.synth_state_dict(model_b.state_dict(), g.meta["weight_seed"] + 1))
    model_b = model_b.eval().to(dev)
    for p in model_b.parameters():
        p.requires_grad_(False)

    def eager_b():
        d = g.data().to(dev)
        d.pos.requires_grad_(True)
        e = model_b(d)
        return e.detach(), -torch.autograd.grad(e.sum(), d.pos)[0]

    eb = eager_b()[0]
    model_b.invalidate_caches()
    model_b.train()
    model_b.eval()
    assert torch.equal(eager_b()[0], eb) and not torch.equal(eb, e0)
    poison = [torch.full_like(t, float("nan")) for _ in range(16) for t in (head.w0f16, head.w0tf16)]
    assert len(poison) == 32
    e1, f1 = step()
    assert torch.equal(e1, e0) and torch.equal(f1, f0)
    assert model_a._head is head and head.builds == 1


def test_a_captured_step_keeps_its_atom_set_whatever_else_is_built():
    """A capture bakes in the addresses of the atom set's arrays (relations.AtomSet: row arrays, element list), which the
    relation build kernels READ on every replay.  The step owns its set: twelve other structures evaluated in the process
    push it out of the lookup index and free nothing -- memory allocated behind that cannot be the set's, and the replays
    repeat bit for bit.  (Zeros behind it, not garbage: zero is a valid value of every row array.)"""
    from hermnet_amd import relations
    from hermnet_amd.graph import GraphedMDStep, GraphedStep
    dev = _dev()
    g = Golden("c1_si64")
    model = g.model().to(dev)
    for p in model.parameters():
        p.requires_grad_(False)
    d = g.data().to(dev)
    steps = [GraphedMDStep(model, d.atomic_number, d.cell.reshape(3, 3), d.pos.detach()), GraphedStep(model, g.data().to(dev))]
    first = [tuple(t.clone() for t in s()) for s in steps]
    for e0, f0 in first:
        assert rel_err(e0.cpu(), g.energy) < 1e-5 and rel_err(f0.cpu(), g.forces) < 1e-5
    zl = [atomic_numbers[el] for el in g.elems]
    sets = [relations.AtomSet.of(steps[0].z, steps[0].batch, zl),
            relations.AtomSet.of(steps[1].data.atomic_number, steps[1].data.batch, zl)]
    assert sets[0] is not sets[1]

    def arrays(s):
        assert len(s.rows) == 1 and s.graph_perm is None
        (rows,) = s.rows.values()
        return [s.zl, s.z64] + [getattr(rows, n) for n in relations.RowArrays.__slots__]

    held = [arrays(s) for s in sets]
    ptrs = [[t.data_ptr() for t in a] for a in held]
    assert all(t is not None for a in held for t in a)

    # twelve other structures of 2 to 8 atoms (H, C, O counts: every composition another row layout), open boundaries, fresh
    # tensors each, evaluated eagerly by another model
    gen = torch.Generator().manual_seed(11)
    model_b = hn.HVNet(["H", "C", "O"], rc=5.0, num_layers=2, hidden_channels=128, num_rbf=128).eval()
    model_b.load_state_dict(synth.synth_state_dict(model_b.state_dict(), 31))
    model_b = model_b.to(dev)
    for p in model_b.parameters():
        p.requires_grad_(False)
    counts = [(1, 1, 0), (2, 1, 0), (2, 0, 1), (2, 1, 1), (0, 2, 2), (3, 1, 1), (4, 2, 0), (2, 2, 2), (4, 2, 1), (1, 3, 3),
              (4, 2, 2), (5, 0, 3)]
    assert len(set(counts)) == 12 and all(2 <= sum(c) <= 8 for c in counts)
    corners = 1.6 * torch.tensor([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=torch.float32)
    for c in counts:
        z = torch.tensor([1] * c[0] + [6] * c[1] + [8] * c[2], device=dev)
        n = int(z.numel())
        pos = (corners[:n] + 0.2 * torch.rand(n, 3, generator=gen)).to(dev).requires_grad_(True)
        ei = hn.neighbor_search(pos.detach(), 5.0)
        assert ei.size(1) == n * (n - 1)
        e = model_b(hn.Data(pos=pos, atomic_number=z, edge_index=ei))
        (f,) = torch.autograd.grad(e.sum(), pos)
        assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(f).all())
    assert len(relations._ATOM_SETS) == 8 and not any(s is kept for s in relations._ATOM_SETS for kept in sets)

    # ownership first: the steps hold the sets of their captures, and every array is where it was
    for step, kept, a, p in zip(steps, sets, held, ptrs):
        assert step.atoms is kept
        assert all(x is y for x, y in zip(arrays(kept), a))
        assert [t.data_ptr() for t in arrays(kept)] == p
    # only then: what a freed block would be handed to
    fill = [torch.zeros_like(t) for _ in range(32) for t in held[0]]
    assert len(fill) == 32 * len(held[0]) and {torch.int32, torch.float32} <= {t.dtype for t in fill}
    for step, (e0, f0) in zip(steps, first):
        e, f = step()
        assert torch.equal(e, e0) and torch.equal(f, f0)


def test_a_repeat_build_around_the_same_tensors_does_not_synchronise():
    """An MD-style step makes a fresh `Data` around the same `atomic_number` / `batch` tensors every step: the relation build
    finds their atom set again (`AtomSet.of`) and nothing in the evaluation reads the host."""
    dev = _dev()
    g = Golden("c1_si64")
    model = g.model().to(dev)
    for p in model.parameters():
        p.requires_grad_(False)
    data = g.data().to(dev)

    def fresh():
        return hn.Data(pos=data.pos.clone().requires_grad_(True), atomic_number=data.atomic_number, batch=data.batch,
                       cell=data.cell, edge_index=data.edge_index, edge_shift=data.edge_shift)

    e0 = model(fresh()).detach().clone()
    model(fresh())                                  # (the parameter guard arms on the second forward)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d = fresh()
        e = model(d)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    (f,) = torch.autograd.grad(e.sum(), d.pos)
    assert torch.equal(e.detach(), e0) and rel_err(-f.cpu(), g.forces) < 1e-5


def test_two_calculators_on_one_device_do_not_evict_each_other():
    """Every `NNCalculator` owns its structure tensors (`StructureTensors`): a second calculator with other species, called in
    turns with the first, replaces none of them -- the first one's capture stays the ONE capture and repeats bit for bit."""
    from hermnet_amd.plugin import NNCalculator
    _dev()
    g = Golden("c1_si64")
    d = g.data()
    z, cell, pos = d.atomic_number.numpy(), d.cell[0].numpy().astype("float64"), d.pos.numpy().astype("float64")
    first = NNCalculator(g.model(), None, trn_mean=0.0, device_="cuda:0", graph_replay=True)
    pos2, cell2, z2 = synth.fcc_alloy_atoms(reps=(2, 2, 2))
    model2 = hn.HVNet(["Al", "Ni", "Cu"], rc=5.0, num_layers=2, hidden_channels=128, num_rbf=64).eval()
    model2.load_state_dict(synth.synth_state_dict(model2.state_dict(), 8))
    second = NNCalculator(model2, None, trn_mean=0.0, device_="cuda:0")
    seen = []
    for _ in range(4):
        first.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])
        seen.append((first.results["energy"], first.results["forces"].copy()))
        second.calculate(_FakeAtoms(pos2.astype("float64"), z2, cell2.astype("float64")), ["energy", "forces"])
        seen.append((second.results["energy"], second.results["forces"].copy()))
        assert first.graph_captures == 1
    assert abs(seen[0][0] - float(g.energy[0])) <= 1e-5 * abs(float(g.energy[0]))
    assert first._structure is not second._structure and first._structure.z is not second._structure.z
    for k in range(2, 8):
        assert seen[k][0] == seen[k % 2][0] and np.array_equal(seen[k][1], seen[k % 2][1]), k
    assert np.isfinite(seen[1][0]) and seen[1][1].shape == (len(z2), 3)


def test_nve_energy_conservation_on_a_fixed_neighbour_list():
    """End to end, no oracle: velocity-Verlet on the device with the model's forces (tools/md_nve.py).  With the
    neighbour list held fixed the total energy must stay put while kinetic and potential energy trade ~10 eV -- and the
    residual drift must fall ~4x when the time step is halved (it is the integrator's O(dt^2), not a force error).
    (With the list rebuilt every step the energy is NOT conserved, here or in the reference: rbf_proj's bias sits outside
    the envelope, so an edge crossing the cutoff switches a finite message on or off)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("md_nve", os.path.join(os.path.dirname(__file__), "..", "tools", "md_nve.py"))
    md = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(md)
    _dev()
    drift = {}
    for dt, steps in ((0.5, 80), (0.25, 160)):
        h = md.run(reps=(4, 4, 4), steps=steps, dt=dt, temp=300.0, fixed_list=True)
        et = [p_ + k_ for p_, k_ in h]
        ek = [k_ for _, k_ in h]
        drift[dt] = max(abs(x - et[0]) for x in et)
        assert max(ek) - min(ek) > 1.0                      # energy really moves between the two reservoirs
        assert drift[dt] < 2e-3 * (max(ek) - min(ek)), (dt, drift[dt], max(ek) - min(ek))
    assert drift[0.25] < 0.5 * drift[0.5]

