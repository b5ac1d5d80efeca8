"""CPU tests of the host logic: neighbour list, relation-ordered graph, container, state_dict
layout, and the host pipeline of HVNet with the two fused operators replaced by their plain
PyTorch restatements (tests/ref_ops.py) -- checked against the reference goldens."""
import itertools

import numpy as np
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import synth
from hermnet_amd.elements import atomic_numbers
from hermnet_amd.neighbor import neighbor_list
from hermnet_amd.relations import RelationalGraph
from helpers import Golden, SMALL_CASES, rel_err
import ref_ops


def _brute(pos, cell, rc, nimg=1):
    I, J, S = [], [], []
    for s in itertools.product(range(-nimg, nimg + 1), repeat=3):
        sv = np.array(s) @ cell
        dm = np.linalg.norm(pos[None, :, :] + sv - pos[:, None, :], axis=-1)
        ii, jj = np.nonzero(dm < rc)
        keep = ~((ii == jj) & (s == (0, 0, 0)))
        I.append(ii[keep]); J.append(jj[keep]); S.append(np.broadcast_to(np.array(s), (keep.sum(), 3)))
    I, J, S = np.concatenate(I), np.concatenate(J), np.concatenate(S)
    k = np.lexsort((S[:, 2], S[:, 1], S[:, 0], J, I))
    return I[k], J[k], S[k]


@pytest.mark.parametrize("case", ["cubic", "triclinic", "small_cell", "unwrapped"])
def test_neighbor_list_bit_exact_vs_brute_force(case):
    rs = np.random.RandomState(3)
    if case == "cubic":
        cell = np.diag([9.0, 10.0, 11.0]); n = 60; nimg = 1; rc = 4.0
    elif case == "triclinic":
        cell = np.array([[9.0, 0, 0], [2.0, 8.5, 0], [1.0, -1.5, 9.5]]); n = 50; nimg = 2; rc = 4.0
    elif case == "small_cell":   # cell shorter than rc: self images and several images per pair
        cell = np.diag([3.0, 3.5, 4.0]); n = 5; nimg = 3; rc = 4.9   # (rc=5 would put the (1,0,1)+(−1,0,1) self-images exactly on the cutoff)
    else:
        cell = np.diag([8.0, 8.0, 8.0]); n = 40; nimg = 1; rc = 3.5
    pos = rs.uniform(0, 1, size=(n, 3)) @ cell
    if case == "unwrapped":
        pos = pos + rs.randint(-2, 3, size=(n, 3)) @ cell   # atoms outside the cell
        nimg = 6
    i, j, s = neighbor_list(pos, rc, cell)
    I, J, S = _brute(pos, cell, rc, nimg)
    assert np.array_equal(i, I) and np.array_equal(j, J) and np.array_equal(s, S)
    # identity the reference relies on: |pos[j] - pos[i] + S cell| < rc
    d = np.linalg.norm(pos[j] - pos[i] + s @ cell, axis=1)
    assert d.max() < rc


def test_neighbor_list_open_system_and_empty():
    rs = np.random.RandomState(0)
    pos = rs.uniform(-4, 4, size=(80, 3))
    i, j, s = neighbor_list(pos, 3.0, None)
    dm = np.linalg.norm(pos[None] - pos[:, None], axis=-1)
    ii, jj = np.nonzero((dm < 3.0) & ~np.eye(80, dtype=bool))
    assert np.array_equal(i, ii) and np.array_equal(j, jj) and not s.any()
    i, j, s = neighbor_list(np.zeros((0, 3)), 3.0, None)
    assert len(i) == 0
    ei = hn.neighbor_search(torch.from_numpy(pos).float(), 3.0)
    assert ei.dtype == torch.int64 and ei.shape[0] == 2
    assert np.array_equal(ei[1].numpy(), ii) and np.array_equal(ei[0].numpy(), jj)  # [source; target]


def test_neighbor_search_sign_conventions():
    d = synth.si_diamond()
    dq = synth.si_diamond(reference_compat=True)
    assert torch.equal(d.edge_index, dq.edge_index) and torch.equal(d.edge_shift, -dq.edge_shift)
    # with the build's convention the model-side formula (hermnet.py:135-139) gives true images
    j, i = d.edge_index
    D = d.pos[j] - d.pos[i] + d.edge_shift @ d.cell[0]
    assert float(D.norm(dim=1).max()) < 5.0
    Dq = dq.pos[j] - dq.pos[i] + dq.edge_shift @ dq.cell[0]
    assert float(Dq.norm(dim=1).max()) > 20.0     # the reference's literal pipeline: wrong images
    assert int((dq.edge_shift.abs().sum(1) > 0).sum()) == 822 and d.edge_index.size(1) == 1792


def test_synthetic_config2_shape():
    d = synth.fcc_alloy(reps=(4, 4, 4))
    assert d.pos.shape == (256, 3) and set(d.atomic_number.tolist()) == {13, 28, 29}


def test_data_container_access_forms():
    d = hn.Data(pos=torch.zeros(3, 3), atomic_number=torch.tensor([1, 1, 8]))
    assert d.batch is None and d.get("cell") is None and d["pos"].shape == (3, 3)
    d.edge_index = torch.zeros(2, 0, dtype=torch.long)
    assert d.num_edges == 0 and d.num_nodes == 3 and "edge_index" in d
    assert dict(iter(d)).keys() == {"pos", "atomic_number", "edge_index"}
    import copy
    c = copy.copy(d)
    c.pos = torch.ones(3, 3)
    assert float(d.pos.sum()) == 0.0


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("name", ["alloy108", "alloy108_unknown_type", "mol16"])
def test_relational_graph_structure(name, uniform):
    g = Golden(name)
    d = g.data()
    zl = [atomic_numbers[e] for e in g.elems]
    gr = RelationalGraph.build(d.atomic_number, d.edge_index, zl, d.get("edge_shift"), d.batch, uniform=uniform)
    N, NA, E, T = gr.N, gr.num_atoms, gr.E, gr.T
    z = d.atomic_number
    rp = gr.type_rowptr_host
    assert gr.uniform == uniform and N >= NA and NA == z.numel()
    if uniform:
        assert all(rp[t + 1] - rp[t] == gr.block for t in range(T))
    else:
        assert N == NA
    # every atom has exactly one row; rows of a relation hold its atoms in ascending id, pads are inert
    assert torch.equal(torch.sort(gr.row_of_node).values, torch.nonzero(gr.row_real).flatten())
    assert torch.equal(gr.z_rows[gr.row_of_node], z) and int(gr.row_real.sum()) == NA
    for t in range(T):
        atoms_t = torch.nonzero(z == zl[t]).flatten()
        assert torch.equal(gr.row_of_node[atoms_t], rp[t] + torch.arange(atoms_t.numel()))
    unknown = torch.nonzero(~torch.isin(z, torch.tensor(zl))).flatten()
    assert torch.equal(gr.row_of_node[unknown], rp[T] + torch.arange(unknown.numel()))
    src, tgt = d.edge_index
    # CSR: segment r holds exactly the edges whose target is row r, in ascending edge id
    rowptr = gr.csr_rowptr.long()
    assert rowptr.numel() == N + 1 and int(rowptr[-1]) == E
    tgt_row = torch.repeat_interleave(torch.arange(N), rowptr[1:] - rowptr[:-1])
    assert torch.equal(gr.row_of_node[tgt[gr.csr_perm]], tgt_row)
    assert torch.equal(gr.csr_src.long(), gr.row_of_node[src[gr.csr_perm]])
    for r in range(0, N, 7):
        seg = gr.csr_perm[rowptr[r]:rowptr[r + 1]]
        assert (seg.diff() > 0).all()
    # CSC: segment (t, r) holds the CSR positions of edges from row r to targets of relation t
    cp = gr.csc_rowptr.long()
    assert cp.numel() == T * N + 1
    rel_row = torch.bucketize(torch.arange(N), gr.type_rowptr.long()[1:], right=True)
    n_known = int((rel_row[tgt_row] < T).sum())
    assert int(cp[-1]) == n_known
    pos = gr.csc_pos.long()
    seg_id = torch.repeat_interleave(torch.arange(T * N), cp[1:] - cp[:-1])
    assert torch.equal(seg_id // N, rel_row[tgt_row[pos[:n_known]]])
    assert torch.equal(seg_id % N, gr.csr_src.long()[pos[:n_known]])
    assert torch.equal(gr.csc_tgt.long()[:n_known], tgt_row[pos[:n_known]])
    # out adjacency
    op = gr.out_rowptr.long()
    src_of = torch.repeat_interleave(torch.arange(N), op[1:] - op[:-1])
    assert torch.equal(gr.csr_src.long()[gr.out_edges.long()], src_of)
    # active rows: real atoms of relations that receive at least one edge
    has_edges = torch.tensor([int(((rel_row[tgt_row]) == t).sum()) > 0 for t in range(T)] + [False])
    assert torch.equal(gr.row_active, has_edges[rel_row].float() * gr.row_real)


def _small_relation_case(case):
    """(atomic numbers, 30 random edges, z_list).  "5_1_0+2": three listed elements with 5 / 1 / 0 atoms and 2 atoms of an
    unlisted element (8 atoms); "12": the same with 4 atoms of a second unlisted element (12 atoms); "one": one element."""
    z = {"5_1_0+2": [13] * 5 + [28] + [79] * 2, "12": [13] * 5 + [28] + [79] * 2 + [47] * 4, "one": [14] * 6}[case]
    gen = torch.Generator().manual_seed(12)
    z = torch.tensor(z)[torch.randperm(len(z), generator=gen)]
    return z, torch.randint(0, z.numel(), (2, 30), generator=gen), ([14] if case == "one" else [13, 28, 29])


@pytest.mark.parametrize("case", ["5_1_0+2", "12", "one"])
def test_triadic_source_rows_are_the_uniform_vertex_layout(case):
    """The statement `relations._source_rows` rests on: HTNet's source rows are HVNet's `uniform=True` rows (an element
    without atoms and atoms of unlisted elements included)."""
    z, ei, zl = _small_relation_case(case)
    hv = RelationalGraph._build_torch(z, ei, zl, uniform=True)
    ht = RelationalGraph.build_triadic(z, ei, zl)
    assert ht.num_src == hv.N and ht.block == hv.block
    for a, b in [("node_order", "node_order"), ("row_of_node", "row_of_node"), ("z_rows", "z_rows"), ("src_real", "row_real")]:
        x, y = getattr(ht, a), getattr(hv, b)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), a


@pytest.mark.parametrize("case", ["5_1_0+2", "12"])
def test_edge_orders_do_not_depend_on_the_sort_key_width(case):
    """`relations._order_edges` with int32 and with int64 sort keys (forced; the rule takes int64 from 2^31 keys on): the
    same arrays, which are the graph's."""
    from hermnet_amd import relations
    z, ei, zl = _small_relation_case(case)
    g = RelationalGraph._build_torch(z, ei, zl, uniform=True)
    rel = relations._classify(z, zl)[0]
    args = (g.row_of_node[ei[1]], g.row_of_node[ei[0]], rel[ei[1]], g.N, g.N, len(zl))
    narrow, wide = relations._order_edges(*args, wide=False), relations._order_edges(*args, wide=True)
    mine = (g.csr_perm, g.csr_src, g.csr_rowptr, g.csc_pos, g.csc_tgt, g.csc_rowptr)
    assert len(narrow) == len(wide) == len(mine) == 6
    for a, b, c in zip(narrow, wide, mine):
        assert a.dtype == b.dtype == c.dtype and torch.equal(a, b) and torch.equal(a, c)


def test_state_dict_layout_matches_reference():
    g = Golden("alloy108")
    keys = list(g.model().state_dict().keys())     # Golden.model() verifies the sha256 over keys+values
    assert keys[0] == "embed.weight" and keys[1] == "radial_basis.rbf.offset"
    assert "hermconvs.2.mods.Cu.update_layer.xvec_proj.2.bias" in keys
    assert "hermconvs.0.mods.Al.message_layer.x_layernorm.weight" in keys
    assert keys[-1] == "out_energy.2.bias"
    m = hn.HVNet("C", hidden_channels=64, num_rbf=16, num_layers=1)
    assert m.rc == 5.0 and list(m.hermconvs[0].mods.keys()) == ["C"]
    for spec, key in [({"name": "spherical_bessel"}, "radial_basis.rbf.frequencies"),
                      ({"name": "bernstein"}, "radial_basis.rbf.pregamma")]:
        m = hn.HVNet(["C"], hidden_channels=64, num_rbf=16, num_layers=1, rbf=spec)
        assert key in m.state_dict()


class _FakeFn(object):
    def __init__(self, fn):
        self.apply = fn


# (the reference-default width, hidden 512, is covered by the oracle tests on the CPU and by the HIP path on the GPU: 45 s here)
@pytest.mark.parametrize("name", [c for c in SMALL_CASES if "h512" not in c])
def test_host_pipeline_with_reference_ops_matches_golden(name, monkeypatch):
    """Everything around the two kernels (row ordering, per-relation node algebra, masks,
    read-out) on CPU, with the kernels replaced by tests/ref_ops.py: must reproduce the
    reference's energies and forces."""
    import hermnet_amd.hermnet as hmod
    import hermnet_amd.rmnet as rmod
    g = Golden(name)
    model = g.model()
    from hermnet_amd import switches
    monkeypatch.setattr(switches, "fused_layer", False)      # autograd-composed layer (debug path of the product)
    monkeypatch.setattr(hmod.HVNet, "_require_device", staticmethod(lambda pos: None))
    monkeypatch.setattr(hmod, "EdgeGeometry", _FakeFn(lambda pos, cell, graph: ref_ops.geometry_ref(pos, graph, cell)))
    monkeypatch.setattr(rmod, "MessageScatter", _FakeFn(ref_ops.message_scatter_ref))
    d = g.data()
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    assert rel_err(e.detach(), g.energy) < 2e-6
    assert rel_err(f, g.forces) < 1e-5


@pytest.mark.parametrize("name", ["c1_si64", "alloy108", "alloy108_unknown_type", "mol16_intensive"])
def test_fused_layer_orchestration_matches_golden(name, monkeypatch):
    """The hand-written layer forward/backward (hermnet_amd/layer.py) with every kernel replaced
    by its PyTorch restatement: validates the launch sequence, the folded LayerNorm affine, the
    per-relation GEMM slicing and the manual gradient algebra on CPU against the reference."""
    import hermnet_amd.hermnet as hmod
    import hermnet_amd.layer as lmod
    g = Golden(name)
    model = g.model()
    for p in model.parameters():
        p.requires_grad_(False)
    from hermnet_amd import switches
    monkeypatch.setattr(switches, "fused_layer", True)
    monkeypatch.setattr(hmod.HVNet, "_require_device", staticmethod(lambda pos: None))
    monkeypatch.setattr(hmod, "EdgeGeometry", ref_ops.RefEdgeGeometry)
    ref_ops.install(monkeypatch.setattr)
    # both forms of the backward hand-over between layers: finished gradients, and partial sums the update backward of the
    # layer below finishes (hn_pending_grads; on the GPU the form is picked by `_bwd_sums_deferrable`)
    # ... and the three forms of the layer boundary (round 5): one node launch each way (switches.boundary_mode = 1: the next
    # layer's projection inside this layer's update launch, its backward inside the update backward of the layer below), the
    # same 16-row phases as launches of their own (2), the round-4 form (0)
    calls = {}
    for fn in ("node_update_pre_fwd", "node_pre_fwd16", "node_pre_bwd16", "node_pre_fwd", "node_pre_bwd"):
        def counted(*a, _f=getattr(ref_ops, fn), _n=fn, **k):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(lmod.nodeops, fn, counted)
    L = g.model_kw["num_layers"]
    for deferred in (False, True):
        monkeypatch.setattr(lmod, "_bwd_sums_deferrable", lambda graph, H, v=deferred: v)
        for boundary in ("1", "2", "0"):
            monkeypatch.setattr(switches, "boundary_mode", int(boundary))
            calls.clear()
            d = g.data()
            d.pos.requires_grad_(True)
            e = model(d)
            f = -torch.autograd.grad(e.sum(), d.pos)[0]
            assert not d._hn_step.pending and not d._hn_step.pre_next
            assert rel_err(e.detach(), g.energy) < 2e-6
            assert rel_err(f, g.forces) < 1e-5
            if g.model_kw["hidden_channels"] == 128 and name != "alloy108_unknown_type_":
                want = {"1": dict(node_update_pre_fwd=L - 1, node_pre_fwd=1),
                        "2": dict(node_pre_fwd16=L - 1, node_pre_fwd=1),
                        "0": dict(node_pre_fwd=L)}[boundary]
                for k, v in want.items():
                    assert calls.get(k, 0) == v, (boundary, deferred, calls)
                if deferred and boundary == "1":       # no projection backward launch at all: it runs in the update backward
                    assert calls.get("node_pre_bwd", 0) == 0 and calls.get("node_pre_bwd16", 0) == 0, calls
                if deferred and boundary == "2":
                    assert calls.get("node_pre_bwd16", 0) == L - 1 and calls.get("node_pre_bwd", 0) == 0, calls


def test_lammps_plugin_helpers():
    from hermnet_amd.plugin import lmp_interface as L
    # the reference's own command line (lmp_calc.py:89-127): long names --stats / --radius, -m / -p optional
    a = L.parse_args(["-f", "m.pt", "--stats", "-3.5", "--radius", "5.0", "--periodic", "True",
                      "-t", "Al", "Ni", "Cu", "-e", "NPT"])
    assert a.elems == ["Al", "Ni", "Cu"] and a.radius == 5.0 and a.stats == -3.5 and a.units == "metal"
    assert a.mode == "zmq" and a.ptr == "tmp.couple" and a.device == "cuda" and not a.reference_compat
    b = L.parse_args(["-f", "m.pt", "--mean", "1", "--rc", "4", "-c", "False", "-t", "Si", "--reference-compat"])
    assert b.stats == 1.0 and b.radius == 4.0 and b.periodic == "False" and b.reference_compat
    for missing in (["-s", "0", "-r", "5", "-c", "True", "-t", "Si"],            # no -f
                    ["-f", "m", "-r", "5", "-c", "True", "-t", "Si"],            # no -s
                    ["-f", "m", "-s", "0", "-c", "True", "-t", "Si"],            # no -r
                    ["-f", "m", "-s", "0", "-r", "5", "-t", "Si"]):              # no -c
        with pytest.raises(SystemExit):
            L.parse_args(missing)
    assert list(L.lammps_types_to_numbers([1, 3, 2, 1], a.elems)) == [13, 29, 28, 13]
    assert (L.SETUP, L.STEP, L.FORCES, L.ENERGY, L.VIRIAL) == (1, 2, 1, 2, 3)

    class CS(object):
        def __init__(self):
            self.log = []

        def send(self, *a):
            self.log.append(("send",) + a)

        def pack(self, *a):
            self.log.append(("pack",) + a)

        def pack_double(self, *a):
            self.log.append(("pack_double",) + a)

    cs = CS()
    L.pack_reply(cs, 2, np.arange(6.0), -1.5, np.zeros(6))
    assert cs.log[0] == ("send", 2, 3) and cs.log[1][:4] == ("pack", 1, 4, 6) and cs.log[2] == ("pack_double", 2, -1.5)
    assert cs.log[3][:4] == ("pack", 3, 4, 6)


def test_virial_units():
    from hermnet_amd.utils import virial_calc
    pos = torch.tensor([[0.0, 0, 0], [1.0, 2, 3]])
    f = torch.tensor([[0.5, 0, 0], [-0.5, 0, 0]])
    v = virial_calc(None, pos, f, None, units="metal", pbc=False)
    assert torch.allclose(v[0, 0], torch.tensor(-0.5 * 1.6021765e6)) and torch.allclose(v, v.T)
    with pytest.raises(ValueError):
        virial_calc(None, pos, f, None, units="bogus")


def test_non_fp32_model_or_positions_are_refused(monkeypatch):
    """The kernels read raw pointers as float32: model.double() / .half() or fp64 coordinates must raise
    instead of producing garbage (the reference is fp32-only as well, hermnet.py:146)."""
    import hermnet_amd.hermnet as hmod
    monkeypatch.setattr(hmod.HVNet, "_require_device", staticmethod(lambda pos: None))
    g = Golden("alloy108")
    d = g.data()
    for cast in ("double", "half"):
        with pytest.raises(TypeError, match="float32"):
            getattr(g.model(), cast)()(d)
    d64 = g.data()
    d64.pos = d64.pos.double()
    with pytest.raises(TypeError, match="float32"):
        g.model()(d64)


def test_eval_mode_parameters_are_constants_unless_asked(monkeypatch):
    """eval(): no parameter receives a gradient (not even the embedding: a partial set would mislead);
    `eval_param_grads = True` routes eval() through the differentiable path, which gives all of them."""
    import hermnet_amd.hermnet as hmod
    import hermnet_amd.rmnet as rmod
    monkeypatch.setattr(hmod.HVNet, "_require_device", staticmethod(lambda pos: None))
    monkeypatch.setattr(hmod, "EdgeGeometry", ref_ops.RefEdgeGeometry)
    ref_ops.install(monkeypatch.setattr)
    g = Golden("alloy108")
    model = g.model()                      # eval(), parameters require grad (the nn.Module default)
    d = g.data()
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos, retain_graph=True)[0]
    assert rel_err(f, g.forces) < 1e-5
    grads = torch.autograd.grad(e.sum(), list(model.parameters()), allow_unused=True)
    assert all(gr is None for gr in grads)
    # opt in: same energy, every parameter that takes part gets a gradient
    monkeypatch.setattr(rmod, "message_scatter_generic", rmod.message_scatter_generic)
    model.eval_param_grads = True
    d2 = g.data()
    d2.pos.requires_grad_(True)
    e2 = model(d2)
    assert rel_err(e2.detach(), g.energy) < 2e-6
    grads = torch.autograd.grad(e2.sum(), list(model.parameters()), allow_unused=True)
    assert sum(gr is not None for gr in grads) >= len(grads) - 4     # (unused: e.g. the last layer's update of vec)


@pytest.mark.parametrize("H", [100, 50, 24])
def test_width_not_multiple_of_64_runs_on_zero_padded_channels(H, monkeypatch):
    """hidden_channels the reference accepts but the column-block kernels do not (H % 64 != 0): LayerWeights pads every
    channel axis to the next multiple of 64 and rescales the weights that meet a 1/sqrt(H) factor; with the kernels
    replaced by their PyTorch restatements (which, like the kernels, only see the padded width) the result must equal
    the oracle at the real width."""
    import hermnet_amd.hermnet as hmod
    from hermnet_amd import synth
    from oracle import hermnet_oracle as orc
    monkeypatch.setattr(hmod.HVNet, "_require_device", staticmethod(lambda pos: None))
    monkeypatch.setattr(hmod, "EdgeGeometry", ref_ops.RefEdgeGeometry)
    ref_ops.install(monkeypatch.setattr)
    g = Golden("alloy108")
    kw = dict(rc=5.0, num_layers=2, hidden_channels=H, num_rbf=16)
    model = hn.HVNet(g.elems, **kw).eval()
    sd = synth.synth_state_dict(model.state_dict(), 21)
    model.load_state_dict(sd)
    for p in model.parameters():
        p.requires_grad_(False)
    e_ref, f_ref = orc.energy_and_forces(sd, g.elems, g.data(), **kw)
    d = g.data()
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    assert rel_err(e.detach(), e_ref) < 5e-6 and rel_err(f, f_ref) < 1e-5


def test_message_scatter_on_host_tensors_equals_its_recorded_results_and_keys_are_declared():
    """trainops.message_scatter_generic on host tensors (the torch route, reading the graph's `RowKeys` by name) gives, to the
    last bit, what it gave before the keys were declared objects (tests/golden/message_scatter_host.npz: 12 atoms, three
    elements, one without atoms, H = 8, float64; recorded by tests/golden/gen_message_scatter_host.py), with and without vec.
    `RowKeys` / `EdgeKeys` are read by field name only: no positional index, no stray attribute."""
    import os
    from hermnet_amd import trainops
    ref = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "message_scatter_host.npz"))
    t = {k: torch.from_numpy(ref[k]) for k in ("z", "edge_index", "xh", "vec", "x", "edge", "edge_embed", "w_rbf", "b_rbf")}
    assert t["z"].numel() == 12 and t["x"].dtype == torch.float64 and t["x"].size(1) == 8
    g = RelationalGraph.build(t["z"], t["edge_index"], [13, 28, 29])
    assert g.T == 3 and not bool((t["z"] == 28).any())
    for with_vec in (0, 1):
        x1, vec1 = trainops.message_scatter_generic(t["xh"], t["vec"] if with_vec else None, t["x"], t["edge"], t["edge_embed"],
                                                    list(t["w_rbf"]), list(t["b_rbf"]), g)
        assert np.array_equal(x1.numpy(), ref["x1_vec%d" % with_vec]) and np.array_equal(vec1.numpy(), ref["vec1_vec%d" % with_vec])
        assert float(x1.abs().sum()) > 0 and float(vec1.abs().sum()) > 0
    rk = g._row_keys[1]                                    # (the graph's declared slot: relations.RelationalGraph._DERIVED)
    assert isinstance(rk, trainops.RowKeys) and rk.res is None and rk.known.dtype == torch.float32
    slot, pad = torch.arange(g.rel_edge_total()), torch.zeros(0, dtype=torch.long)
    ek = rk.edge_keys(slot, pad)
    assert isinstance(ek, trainops.EdgeKeys) and ek.tgt is rk.tgt and ek.src is rk.src and ek.xrow is rk.xrow
    assert ek.r_rows is slot and ek.pad is pad and rk.edge_keys().r_rows is None and rk.edge_keys().pad is None
    for keys in (rk, ek):
        assert not hasattr(type(keys), "__getitem__") and not hasattr(type(keys), "__len__") and not hasattr(type(keys), "__iter__")
        with pytest.raises(TypeError):
            keys[0]
        with pytest.raises(AttributeError):
            keys.rows = None


def _layer_weights_and_graph(H, T, counts, seed=0, unknown=3, uniform=None):
    """LayerWeights of T randomly initialised PaiNNModules + a relation-ordered graph with `counts[t]` atoms per element."""
    import hermnet_amd as hn
    from hermnet_amd.layer import LayerWeights
    from hermnet_amd.relations import RelationalGraph
    from hermnet_amd.rmnet import PaiNNModule
    torch.manual_seed(seed)
    mods = [PaiNNModule(hidden_channels=H, num_rbf=16) for _ in range(T)]
    for m in mods:
        for p in m.parameters():
            p.data.normal_(0, 0.3)
    w = LayerWeights(mods).refresh()
    zs = [13, 28, 29, 79][:T]
    z = torch.cat([torch.full((c,), zs[t], dtype=torch.long) for t, c in enumerate(counts)] + [torch.full((unknown,), 1, dtype=torch.long)])
    z = z[torch.randperm(z.numel())]
    n = z.numel()
    src = torch.randint(0, n, (4 * n,))
    tgt = torch.randint(0, n, (4 * n,))
    if T > 1:           # leave the last element without incoming edges: an inactive relation (hermnet.py:56-57)
        keep = z[tgt] != zs[T - 1]
        src, tgt = src[keep], tgt[keep]
    g = RelationalGraph.build(z, torch.stack([src, tgt]), zs, uniform=uniform)
    return w, g


@pytest.mark.parametrize("H,T,counts,uniform", [(64, 3, (20, 31, 9), None), (64, 2, (40, 3), False), (128, 1, (37,), None)])
def test_node_chain_restatements_are_consistent(H, T, counts, uniform):
    """tests/ref_ops.py's restatements of the node chain kernels: the explicit backward formulas (what
    csrc/node_chain.hip implements from the saved vp / h2b / q23) equal autograd of the forward formulas; the
    fragment-ordered weights hold the same values as the plain ones."""
    from hermnet_amd import nodeops
    w, g = _layer_weights_and_graph(H, T, counts, uniform=uniform)
    gen = torch.Generator().manual_seed(1)
    N = g.N
    x1, vec1 = torch.randn(N, H, generator=gen).double(), torch.randn(N, 3, H, generator=gen).double()
    xo, vo, vp, h2b, q23, nrm = ref_ops.node_update_fwd(x1, vec1, w, g)
    act = g.row_active != 0
    assert float(xo[~act].abs().max()) == 0.0 and float(vo[~act].abs().max()) == 0.0 and bool((~act).any())
    gxo, gvo = torch.randn(N, H, generator=gen).double(), torch.randn(N, 3, H, generator=gen).double()
    a = ref_ops.node_update_bwd(gxo, gvo, vp, h2b, q23, nrm, w, g)
    b = ref_ops.node_update_bwd_from_inputs(gxo, gvo, x1, vec1, w, g)
    assert rel_err(a[0], b[0]) < 1e-12 and rel_err(a[1], b[1]) < 1e-12
    # pre chain: backward formulas vs autograd
    x = torch.randn(N, H, generator=gen).double().requires_grad_(True)
    hb, xh, mean, rstd = ref_ops.node_pre_fwd(x, w, T)
    gxh = torch.randn(T, N, 3 * H, generator=gen).double()
    (gx_auto,) = torch.autograd.grad(xh, x, gxh)
    gx = ref_ops.node_pre_bwd(gxh, hb.detach(), x.detach(), mean.detach(), rstd.detach(), w)
    assert rel_err(gx, gx_auto) < 1e-10
    # fragment order (three bf16 planes, smallest first): frag(W)[((cb * K/16 + Q) * 3 + s) * 64 + l][e] = W_(2-s)[32 cb + (l & 31)][16 Q + 8 (l >> 5) + e]
    W = w.wx0_s.float()                                           # [T, H, 2H]
    planes = nodeops._bf16_planes(W)
    assert torch.equal((planes[2].double() + planes[1].double()) + planes[0].double(), W.double())     # the split is exact
    f = nodeops.weight_fragments(W).view(torch.bfloat16).view(T, H // 32, 2 * H // 16, 3, 64, 8)
    for (t, cb, q, s_, l, e) in [(0, 0, 0, 0, 0, 0), (T - 1, H // 32 - 1, 2 * H // 16 - 1, 2, 63, 7), (0, 1, 5, 1, 37, 2)]:
        assert float(f[t, cb, q, s_, l, e]) == float(planes[s_][t, 32 * cb + (l & 31), 16 * q + 8 * (l >> 5) + e])
    assert torch.equal(f.reshape(T, -1).view(torch.float32), w.wx0f)
    f16 = nodeops.weight_fragments16(W).view(torch.bfloat16).view(T, H // 16, 2 * H // 32, 3, 64, 8)
    for (t, b_, q, s_, l, e) in [(0, 0, 0, 0, 0, 0), (T - 1, H // 16 - 1, 2 * H // 32 - 1, 2, 63, 7), (T // 2, 3, 2, 1, 41, 5)]:
        assert float(f16[t, b_, q, s_, l, e]) == float(planes[s_][t, 16 * b_ + (l & 15), 32 * q + 8 * (l >> 4) + e])


def test_tall_bmm_is_a_linear_to_second_order(monkeypatch):
    """trainops.TallBmm / tall_linear (the node-level linears of the training step): y = a w + b with the weight gradient as a
    batched product over row chunks -- gradient and gradient-of-gradient vs finite differences in float64, chunked path on."""
    import hermnet_amd.trainops as tr
    from torch.autograd import gradcheck, gradgradcheck
    monkeypatch.setattr(tr, "_SPLIT_K_ROWS", 8)
    assert tr._split_k_chunk(24) == 8
    torch.manual_seed(0)
    mk = lambda *s: torch.randn(*s, dtype=torch.float64, requires_grad=True)
    a, w, b = mk(2, 24, 3), mk(2, 3, 4), mk(2, 4)
    f = lambda a, w, b: tr.TallBmm.apply(a, w, b)
    assert torch.allclose(f(a, w, b), torch.baddbmm(b[:, None, :], a, w))
    assert gradcheck(f, (a, w, b)) and gradgradcheck(f, (a, w, b))
    assert gradgradcheck(lambda a, w: tr.TallBmm.apply(a, w, None), (mk(1, 23, 3), mk(1, 3, 2)))     # (no divisor: one product)
    x, W, bb = mk(24, 5), mk(3, 5), mk(3)
    assert torch.allclose(tr.tall_linear(x, W, bb), torch.nn.functional.linear(x, W, bb))
    assert gradgradcheck(lambda x, W, bb: tr.tall_linear(x, W, bb), (x, W, bb))


def test_param_guard_stays_out_of_copies_and_pickles():
    """an armed guard (HIP event, pinned flag) made `copy.deepcopy(model)` / `torch.save(model)` raise
    "cannot pickle 'Event' object".  Reproduced on the CPU by attaching an armed guard to a fresh HVNet."""
    import copy
    import io
    import hermnet_amd as hn
    from hermnet_amd.guard import ParamGuard
    model = hn.HVNet(["Si"], num_layers=1, hidden_channels=64, num_rbf=16)
    guard = model.__dict__["_guard"] = ParamGuard(model)
    guard._event = torch.cuda.Event()
    clone = copy.deepcopy(model)
    assert clone.__dict__.get("_guard") is None and model.__dict__["_guard"] is guard
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), clone.state_dict().values()))
    buf = io.BytesIO()
    torch.save(model, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)
    assert loaded.__dict__.get("_guard") is None
    from torch.optim.swa_utils import AveragedModel
    assert AveragedModel(model).module.__dict__.get("_guard") is None


def test_band_product_functions_are_closed_under_differentiation():
    """trainops.BandP / BandQ / BandS (rbf_proj on the bucketed basis, csrc/band_product.hip on the GPU): first and second
    derivatives against plain torch ops in fp64, with both autograd outputs of BandP consumed (their gradients reach the
    backward unsummed)."""
    from hermnet_amd.trainops import band_product
    gen = torch.Generator().manual_seed(0)
    nc, C, N = 3, 32, 64
    r = lambda *s: torch.randn(*s, dtype=torch.double, generator=gen)
    A0, B0, b0, c1, wA = r(nc, C, 32), r(nc, 32, N), r(nc, N), r(nc, C, N), r(nc, C, 32)

    def run(band, bias=True):
        A, B, b, cc = [t.clone().requires_grad_(True) for t in (A0, B0, b0, c1)]
        if band:
            out, out2 = band_product(A, B, b if bias else None)
        else:
            out = out2 = torch.baddbmm(b[:, None, :], A, B) if bias else torch.bmm(A, B)
        leaves = [A, B] + ([b] if bias else [])
        L1 = (out * cc).sum() + 0.1 * (out2 ** 3).sum()
        first = torch.autograd.grad(L1, leaves, create_graph=True)
        L2 = (first[0] * wA).sum() + sum((g ** 2).sum() for g in first[1:]) + (out2 ** 2).sum()
        second = torch.autograd.grad(L2, leaves + [cc])
        return [out.detach()] + [g.detach() for g in first] + list(second)

    for bias in (True, False):
        for x, y in zip(run(True, bias), run(False, bias)):
            assert torch.allclose(x, y, rtol=1e-12, atol=1e-12)


def test_parameter_gradients_are_not_formed_in_a_pass_that_does_not_ask_for_them(monkeypatch):
    """The force pass (autograd.grad(E, pos, create_graph=True), /root/reference/example/dist_train.py:90-92) asks for no
    parameter gradient: the weight-gradient reductions of tall_bmm / band_product sit in graph nodes of their own
    (trainops._TallBmmParams / _BandParams) that the engine prunes there -- and runs in the pass that does ask."""
    import hermnet_amd.trainops as tr
    calls = {"gram": 0, "s": 0}
    gram, s_apply = tr._gram_over_rows, tr.BandS.apply
    monkeypatch.setattr(tr, "_gram_over_rows", lambda a, g: (calls.__setitem__("gram", calls["gram"] + 1), gram(a, g))[1])
    monkeypatch.setattr(tr.BandS, "apply", staticmethod(lambda *a: (calls.__setitem__("s", calls["s"] + 1), s_apply(*a))[1]))
    gen = torch.Generator().manual_seed(1)
    r = lambda *sh: torch.randn(*sh, dtype=torch.double, generator=gen).requires_grad_(True)
    pos, w, b, B, bias = r(2, 32, 32), r(2, 32, 8), r(2, 8), r(2, 32, 64), r(2, 64)
    y = tr.tall_bmm(pos, w, b)
    R1, R2 = tr.band_product(pos, B, bias)
    e = (y ** 2).sum() + (R1 * R2).sum()
    f, = torch.autograd.grad(e, pos, create_graph=True)
    assert calls == {"gram": 0, "s": 0}
    ((f ** 2).sum() + e).backward()
    assert calls["gram"] >= 2 and calls["s"] >= 2          # first-order term and the term through the force pass
    ref_pos = pos.detach().clone().requires_grad_(True)
    params = [t.detach().clone().requires_grad_(True) for t in (w, b, B, bias)]
    y = torch.baddbmm(params[1][:, None, :], ref_pos, params[0])
    R = torch.baddbmm(params[3][:, None, :], ref_pos, params[2])
    e = (y ** 2).sum() + (R * R).sum()
    f, = torch.autograd.grad(e, ref_pos, create_graph=True)
    ((f ** 2).sum() + e).backward()
    for got, ref in zip((pos, w, b, B, bias), [ref_pos] + params):
        assert torch.allclose(got.grad, ref.grad, rtol=1e-10, atol=1e-10)


_STEP_OUTPUTS = {"_hn_step", "_hn_graph", "_hn_edge", "_hn_edge_embed"}


def _reference_ops(monkeypatch, fused_layer=True):
    """The monkeypatched reference ops of `test_fused_layer_orchestration_matches_golden` (fused_layer False: of
    `test_host_pipeline_with_reference_ops_matches_golden`)."""
    import hermnet_amd.hermnet as hmod
    import hermnet_amd.rmnet as rmod
    from hermnet_amd import switches
    monkeypatch.setattr(switches, "fused_layer", fused_layer)
    monkeypatch.setattr(hmod.HVNet, "_require_device", staticmethod(lambda pos: None))
    if not fused_layer:
        monkeypatch.setattr(hmod, "EdgeGeometry", _FakeFn(lambda pos, cell, graph: ref_ops.geometry_ref(pos, graph, cell)))
        monkeypatch.setattr(rmod, "MessageScatter", _FakeFn(ref_ops.message_scatter_ref))
        return
    monkeypatch.setattr(hmod, "EdgeGeometry", ref_ops.RefEdgeGeometry)
    ref_ops.install(monkeypatch.setattr)


def _frozen_model(g):
    model = g.model()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


@pytest.mark.parametrize("fused_layer", [True, False])
def test_an_evaluation_leaves_only_its_declared_names_on_the_data(fused_layer, monkeypatch):
    """What one evaluation hands from stage to stage lives on its `layer.StepState`: behind a forward and its backward the
    caller's Data holds the four names left for readers and nothing else of the package's."""
    _reference_ops(monkeypatch, fused_layer)
    g = Golden("alloy108")
    model = _frozen_model(g)
    d = g.data()
    d.pos.requires_grad_(True)
    e = model(d)
    f = -torch.autograd.grad(e.sum(), d.pos)[0]
    assert rel_err(f, g.forces) < 1e-5
    assert {k for k in d.keys() if k.startswith("_hn_")} == _STEP_OUTPUTS
    step = d._hn_step
    assert step.graph is d._hn_graph and step.edge is d._hn_edge and step.edge_embed is d._hn_edge_embed
    # (nothing of the model or of the autograd graph stays behind on the step either)
    assert step.weights is None and step.edge_handles is None and step.halo is None and step.chain_node is None


def test_step_state_refuses_undeclared_fields():
    from hermnet_amd.layer import StepState
    step = StepState()
    step.layer = 3
    with pytest.raises(AttributeError):
        step.layr = 4
    with pytest.raises(AttributeError):
        step.hallo = None


def test_two_steps_on_one_data_cannot_see_each_others_state(monkeypatch):
    """Two forwards on the SAME Data at the same positions, then the backward of the first energy and of the second: both
    force arrays are the lone evaluation's bit for bit, and both steps end with nothing pending -- with everything the
    layers can hand to each other in flight (gradients as partial sums, the next layer's projection: boundary mode 1).
    (Deterministic algorithms: the scatter-adds of the CPU restatements otherwise add in an order that differs run to run.)"""
    import hermnet_amd.layer as lmod
    from hermnet_amd import switches
    _reference_ops(monkeypatch)
    monkeypatch.setattr(lmod, "_bwd_sums_deferrable", lambda graph, H: True)
    monkeypatch.setattr(switches, "boundary_mode", 1)
    g = Golden("alloy108")
    model = _frozen_model(g)
    deterministic = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        lone = g.data()
        lone.pos.requires_grad_(True)
        e0 = model(lone)
        f0 = -torch.autograd.grad(e0.sum(), lone.pos)[0]
        d = g.data()
        d.pos.requires_grad_(True)
        e1 = model(d)
        step1 = d._hn_step
        e2 = model(d)
        step2 = d._hn_step
        f1 = -torch.autograd.grad(e1.sum(), d.pos)[0]
        f2 = -torch.autograd.grad(e2.sum(), d.pos)[0]
    finally:
        torch.use_deterministic_algorithms(deterministic)
    assert step1 is not step2
    assert torch.equal(e1, e0) and torch.equal(e2, e0)
    assert torch.equal(f1, f0) and torch.equal(f2, f0)
    assert rel_err(f0, g.forces) < 1e-5
    for step in (step1, step2):
        assert not step.pending and not step.pre_next


class _StubPlan(object):
    """What the read-out's sums read of a `sharding.ShardPlan`."""
    world, group = 1, None

    def __init__(self, owned_mask, num_graphs, num_atoms_global):
        self.owned_mask, self.num_graphs, self.num_atoms_global = owned_mask, num_graphs, num_atoms_global

    def graph_order(self, batch):
        return torch.argsort(batch, stable=True), torch.bincount(batch, minlength=self.num_graphs)


@pytest.mark.parametrize("intensive", [False, True])
def test_read_out_sums_in_their_five_forms(intensive):
    """`HVNet._graph_energies` on hand-made per-row energies; the expected value of every form is the expression the read-out
    used before it was cut out of `HVNet.forward`."""
    from types import SimpleNamespace
    from hermnet_amd.hermnet import GraphEnergies
    model = hn.HVNet(["Si"], num_layers=1, hidden_channels=8, num_rbf=4, intensive=intensive)
    gen = torch.Generator().manual_seed(5)
    e_rows = torch.randn(9, generator=gen)
    row_of_node = torch.tensor([0, 2, 3, 5, 6, 8])          # (rows 1, 4, 7: padding)
    batch = torch.tensor([1, 0, 1, 1, 0, 1])
    lengths = torch.bincount(batch, minlength=2)
    one = SimpleNamespace(num_graphs=1, num_atoms=6, row_of_node=row_of_node, graph_perm=None, graph_lengths=None)
    two = SimpleNamespace(num_graphs=2, num_atoms=6, row_of_node=row_of_node, graph_perm=torch.argsort(batch, stable=True),
                          graph_lengths=lengths, _row_graph=None)
    two_train = SimpleNamespace(num_graphs=2, num_atoms=6, row_of_node=row_of_node, graph_perm=None, graph_lengths=lengths)
    own = torch.tensor([1, 1, 0, 1, 0, 1], dtype=torch.bool)
    per_atom = e_rows.index_select(0, row_of_node)
    e_own, ownf = per_atom * own.to(per_atom.dtype), own.to(per_atom.dtype)
    perm = torch.argsort(batch, stable=True)
    seg = lambda v: torch.segment_reduce(v.index_select(0, perm), "sum", lengths=lengths, unsafe=True)
    div = (lambda e, n: e / n) if intensive else (lambda e, n: e)
    zero = torch.zeros(1, dtype=torch.long)
    table = [
        # (case, graph, batch, shard, masked, expected)
        ("shard, one graph, owned rows", one, zero.expand(6), _StubPlan(own, 1, 11), True,
         div(e_rows.sum().reshape(1), max(11, 1))),
        ("single graph", one, zero.expand(6), None, True, div(e_rows.sum().reshape(1), max(one.num_atoms, 1))),
        ("ordered segment sums", two, batch, None, False,
         div(GraphEnergies.apply(e_rows, two, batch), lengths.clamp(min=1).to(e_rows.dtype))),
        ("shard, atom order, one graph", one, zero.expand(6), _StubPlan(own, 1, 11), False,
         div(e_own.sum().reshape(1), ownf.sum().reshape(1).clamp(min=1))),
        ("shard, atom order, two graphs", two_train, batch, _StubPlan(own, 2, 11), False,
         div(seg(e_own), seg(ownf).clamp(min=1))),
        ("train: index_add", two_train, batch, None, False,
         div(torch.zeros(2, dtype=e_rows.dtype).index_add(0, batch, per_atom), lengths.clamp(min=1).to(e_rows.dtype))),
    ]
    for case, graph, b, shard, masked, want in table:
        got = model._graph_energies(e_rows, graph, b, shard, masked)
        assert got.shape == want.shape and torch.equal(got, want), case
    # (the ordered form is the plain scatter of the reference, hermnet.py:130, up to the order of the additions)
    assert torch.allclose(table[2][5], table[5][5], rtol=1e-6, atol=1e-6)
