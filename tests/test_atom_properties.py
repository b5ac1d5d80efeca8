"""Per-atom energies and per-atom virials (hermnet_amd.atomic.atom_properties, the ASE calculator's `energies` /
`stresses`, the C entry point hermnet_edge_geometry_bwd_virial).

Definitions: D_e = pos[src] - pos[tgt] + shift_e @ cell[batch[src]], g_e = dE/dD_e,
W_i = -1/2 sum_{e touching i} D_e (x) g_e (unsymmetrised, [a,b] = D_a g_b); e_i = the read-out term of atom i (intensive:
divided by its graph's atom count).  GPU values are checked against the float64 oracle, against sum rules and symmetry,
and the energy / forces of a call with per-atom outputs against a plain eval() call, bit for bit."""
import numpy as np
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import _lib, switches, synth
from hermnet_amd.plugin import ase_interface as A
from helpers import Golden, rel_err

ORACLE_CASES = ["c1_si64", "c1_si64_refcompat", "alloy108", "alloy108_unknown_type", "alloy108_h512_default", "mol16",
                "mol16_intensive", "alloy32_bessel_expenv", "alloy32_bernstein"]
TOL = 1e-5


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_argument_checks_of_the_per_atom_virial_entry_point_need_no_gpu():
    """hermnet_edge_geometry_bwd_virial refuses malformed calls before a launch; no rows is done."""
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    OK, BAD = 0, 1

    def call(n=4, csc=(p, p, 2), out=(None, None), shift=None, cell=None, gpos=p, vir=p, pos=p, csr=p):
        return lib.hermnet_edge_geometry_bwd_virial(p, csr, csc[0], csc[1], csc[2], out[0], out[1], pos, p, p, shift, cell,
                                                    None, n, gpos, vir, None)

    assert call(n=0) == OK                                             # no rows: done
    assert call(n=0, csc=(None, None, 0), out=(p, p)) == OK
    assert call(n=-1) == BAD and call(csc=(p, p, -1)) == BAD           # negative counts
    assert call(csc=(p, p, 0)) == BAD                                  # CSC form without relations
    assert call(out=(p, p)) == BAD                                     # both out-adjacencies
    assert call(csc=(None, None, 0)) == BAD                            # neither
    assert call(shift=p) == BAD and call(n=0, shift=p) == BAD          # shift without cell
    assert call(gpos=None) == BAD and call(vir=None) == BAD            # a missing output
    assert call(pos=None) == BAD and call(csr=None) == BAD             # missing inputs
    assert call(csc=(None, None, 0), out=(p, None), vir=None) == BAD


def test_ase_calculator_implements_per_atom_properties():
    props = A.NNCalculator.implemented_properties
    assert "energies" in props and "stresses" in props
    assert {"energy", "free_energy", "forces", "stress"} <= set(props)


def test_stresses_from_virials_follow_the_stress_contract():
    """sigma_i = -sym(W_i) / V in Voigt [xx,yy,zz,yz,xz,xy]; summed, they are `stress_from_virial` of the summed W."""
    rs = np.random.RandomState(0)
    w = rs.normal(size=(7, 3, 3))
    s = A.stresses_from_virials(w, 12.5)
    assert s.shape == (7, 6)
    tot = w.sum(0)
    assert np.allclose(s.sum(0), A.stress_from_virial(0.5 * (tot + tot.T), 12.5), rtol=0, atol=1e-12)
    assert np.allclose(s[3], A.stress_from_virial(0.5 * (w[3] + w[3].T), 12.5), rtol=0, atol=1e-12)


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _on(d, dev):
    """A copy of `d` on `dev` (Data.to moves in place)."""
    return hn.Data(**{k: v.to(dev) for k, v in d})


def _plain(model, d):
    """The plain eval() call every caller makes: energy and forces."""
    pos = d.pos.detach().clone().requires_grad_(True)
    d.pos = pos
    e = model(d)
    return e.detach(), -torch.autograd.grad(e.sum(), pos)[0]


def _oracle(g, d, monkeypatch, model=None):
    """float64 oracle on CPU data `d`: (per-atom energies [N], per-atom virials [N,3,3]) by the definitions.  g_e comes from
    autograd on the oracle's own edge vectors (its `edge_geometry`, restated here to keep them)."""
    from oracle import hermnet_oracle as orc
    m = g.model() if model is None else model
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    if model is None:
        kw, elems = g.oracle_kwargs(), g.elems
    else:
        kw = dict(rc=m.rc, intensive=m.intensive, num_layers=m.num_layers, hidden_channels=m.hidden_channels,
                  num_rbf=m.radial_basis.num_radial)
        elems = m.elems
    kept = {}

    def edge_geometry(pos, edge_index, edge_shift=None, cell=None, batch=None):
        j, i = edge_index[0], edge_index[1]
        dvec = pos[j] - pos[i]
        if cell is not None and edge_shift is not None:
            c = cell.reshape(-1, 3, 3)
            dvec = dvec + torch.einsum('ni,nij->nj', edge_shift.to(pos.dtype), c[batch[j]].to(pos.dtype))
        dvec.retain_grad()
        kept["D"] = dvec
        dist = dvec.norm(dim=-1)
        near0 = torch.isclose(dist, torch.zeros((), dtype=dist.dtype), atol=1e-6)
        dist = torch.where(near0, torch.full_like(dist, 1.0e-6), dist)
        return dist, dvec / dist[:, None]

    with monkeypatch.context() as mp:
        mp.setattr(orc, "edge_geometry", edge_geometry)
        pos = d.pos.detach().double().requires_grad_(True)
        cell = None if d.get("cell") is None else d.cell.double()
        e, inter = orc.hvnet_energy(sd, elems, pos, d.atomic_number, d.edge_index, d.batch, d.get("edge_shift"), cell,
                                    return_intermediates=True, **kw)
    x = inter["x"][-1]
    lin = torch.nn.functional.linear
    ea = lin(orc.scaled_silu(lin(x, sd["out_energy.0.weight"], sd["out_energy.0.bias"])),
             sd["out_energy.2.weight"], sd["out_energy.2.bias"]).squeeze(1)
    b = d.batch.long()
    if kw.get("intensive"):
        ea = ea / torch.bincount(b).clamp(min=1).double()[b]
    assert torch.allclose(ea.sum(), e.sum(), rtol=1e-10, atol=1e-12)
    W = torch.zeros(pos.size(0), 3, 3, dtype=torch.float64)
    D = kept["D"]
    if D.numel():
        e.sum().backward()
        outer = -0.5 * D.detach()[:, :, None] * D.grad[:, None, :]
        W.index_add_(0, d.edge_index[0], outer).index_add_(0, d.edge_index[1], outer)
    return ea.detach(), W


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_per_atom_energies_and_virials_match_the_fp64_oracle(name, monkeypatch):
    dev = _dev()
    g = Golden(name)
    d = _on(g.data(), dev)
    out = hn.atom_properties(g.model().to(dev), d)
    e_ref, w_ref = _oracle(g, g.data(), monkeypatch)
    n = d.pos.size(0)
    assert out["energies"].shape == (n,) and out["virials"].shape == (n, 3, 3)
    assert rel_err(out["energies"].cpu().double(), e_ref) <= TOL
    assert rel_err(out["virials"].cpu().double(), w_ref) <= TOL
    # the per-atom energies of every graph sum to its energy
    b = d.batch.long()
    eg = torch.zeros_like(out["energy"]).index_add_(0, b, out["energies"])
    scale = torch.zeros_like(out["energy"]).index_add_(0, b, out["energies"].abs())
    assert bool(((eg - out["energy"]).abs() <= 1e-6 * scale).all())


@pytest.mark.gpu
def test_torch_readout_width_matches_the_fp64_oracle(monkeypatch):
    """A width with (H/2) % 4 != 0 takes the torch read-out (not EnergyHead)."""
    dev = _dev()
    g = Golden("alloy108")
    model = hn.HVNet(g.elems, rc=5.0, num_layers=2, hidden_channels=100, num_rbf=32)
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 3))
    out = hn.atom_properties(model.to(dev).eval(), _on(g.data(), dev))
    e_ref, w_ref = _oracle(g, g.data(), monkeypatch, model=model.cpu())
    assert rel_err(out["energies"].cpu().double(), e_ref) <= TOL
    assert rel_err(out["virials"].cpu().double(), w_ref) <= TOL


def _sym(w):
    return 0.5 * (w + w.transpose(-1, -2))


def _vtol(w):
    """1e-5 of the largest sum of |W_i| over the atoms (the total can be small)."""
    return 1e-5 * float(w.abs().sum(0).max())


@pytest.mark.gpu
def test_sum_rule_against_the_cell_virial_on_periodic_cells():
    """sym(sum_i W_i) is the virial of `virial_calc` (`_evaluate(..., want_virial=True)`): configs[1] cell and alloy108."""
    dev = _dev()
    for g, mk in ((Golden("c2_alloy10k"), lambda: synth.fcc_alloy(device=dev)),
                  (Golden("alloy108"), lambda: _on(Golden("alloy108").data(), dev))):
        model = g.model().to(dev)
        out = hn.atom_properties(model, mk())
        _, _, w = A._evaluate(model, mk(), dev, True, True)
        vir = out["virials"].double()
        assert float((_sym(vir.sum(0)) - w.double()).abs().max()) <= _vtol(vir), g.name


@pytest.mark.gpu
def test_sum_rule_per_molecule_of_an_open_batch():
    """Open systems: sum_{i in g} W_i = sum_{i in g} pos_i (x) F_i per graph (unsymmetrised)."""
    dev = _dev()
    g = Golden("mol16")
    d = _on(g.data(), dev)
    out = hn.atom_properties(g.model().to(dev), d)
    b = d.batch.long()
    ng = int(b.max()) + 1
    pf = d.pos.double()[:, :, None] * out["forces"].double()[:, None, :]
    want = torch.zeros(ng, 3, 3, dtype=torch.float64, device=dev).index_add_(0, b, pf)
    got = torch.zeros(ng, 3, 3, dtype=torch.float64, device=dev).index_add_(0, b, out["virials"].double())
    assert float((got - want).abs().max()) <= _vtol(out["virials"].double())


def _two_cells():
    """Two periodic Si cells of different shape and size in one batch."""
    a = synth.si_diamond(reps=(2, 2, 2), a=5.43, seed=1)
    b = synth.si_diamond(reps=(2, 2, 3), a=5.50, seed=2)
    na = a.pos.size(0)
    return hn.Data(pos=torch.cat([a.pos, b.pos]), atomic_number=torch.cat([a.atomic_number, b.atomic_number]),
                   edge_index=torch.cat([a.edge_index, b.edge_index + na], 1),
                   edge_shift=torch.cat([a.edge_shift, b.edge_shift]), cell=torch.cat([a.cell, b.cell]),
                   batch=torch.cat([a.batch, b.batch + 1]))


@pytest.mark.gpu
def test_sum_rule_per_graph_of_a_batch_of_different_cells():
    """Per graph: sum_{i in g} W_i = sum_{i in g} pos_i (x) F_i - cell_g^T dE/dcell_g, the cell gradient taken here."""
    dev = _dev()
    model = Golden("c1_si64").model().to(dev)
    d = _on(_two_cells(), dev)
    out = hn.atom_properties(model, d)
    pos = d.pos.detach().clone().requires_grad_(True)
    cell = d.cell.detach().clone().requires_grad_(True)
    e = model(hn.Data(pos=pos, atomic_number=d.atomic_number, edge_index=d.edge_index, edge_shift=d.edge_shift, cell=cell,
                      batch=d.batch))
    gp, gc = torch.autograd.grad(e.sum(), (pos, cell))
    b = d.batch.long()
    pf = pos.detach().double()[:, :, None] * (-gp).double()[:, None, :]
    want = torch.zeros(2, 3, 3, dtype=torch.float64, device=dev).index_add_(0, b, pf)
    want = want - cell.detach().double().transpose(1, 2) @ gc.double()
    got = torch.zeros(2, 3, 3, dtype=torch.float64, device=dev).index_add_(0, b, out["virials"].double())
    assert float((got - want).abs().max()) <= _vtol(out["virials"].double())
    assert torch.equal(out["energy"], e.detach())
    eg = torch.zeros(2, dtype=out["energies"].dtype, device=dev).index_add_(0, b, out["energies"])
    assert float((eg - out["energy"]).abs().max()) <= 1e-6 * float(out["energies"].abs().sum())


@pytest.mark.gpu
def test_every_atom_of_a_perfect_diamond_crystal_gets_the_same_share():
    """No oracle needed: in a perfect crystal every atom is equivalent, so W_i = W / N and e_i = E / N."""
    dev = _dev()
    d = _on(synth.si_diamond(reps=(2, 2, 2), sigma=0.0), dev)
    out = hn.atom_properties(Golden("c1_si64").model().to(dev), d)
    n = d.pos.size(0)
    W = out["virials"].double()
    assert rel_err(W, (W.sum(0) / n).expand_as(W)) <= 1e-5
    e = out["energies"].double()
    assert rel_err(e, (out["energy"].double() / n).expand_as(e)) <= 1e-5


def _padded(g, dev):
    from hermnet_amd.neighbor import neighbor_search_padded
    d = _on(g.data(), dev)
    ei, sh, total = neighbor_search_padded(d.pos, 5.0, d.cell[0], d.edge_index.size(1) + 777)
    return hn.Data(pos=d.pos, atomic_number=d.atomic_number, batch=d.batch, cell=d.cell, edge_index=ei, edge_shift=sh,
                   _hn_edge_count=total)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["csc", "host_relations", "padded", "bessel", "unfused_layer"])
def test_energy_and_forces_are_unchanged_by_the_request(route, monkeypatch):
    """With per-atom outputs on, energy and forces are bit for bit those of a plain eval() call, on every route; the
    per-atom values agree with the default route's."""
    dev = _dev()
    g = Golden("alloy32_bessel_expenv" if route == "bessel" else "alloy108")
    model = g.model().to(dev)
    ref = hn.atom_properties(model, _on(g.data(), dev))
    if route == "host_relations":          # (out-adjacency graphs: the kernel's out-segment form)
        monkeypatch.setattr(switches, "native_relations", False)
    if route == "unfused_layer":           # (the torch read-out)
        monkeypatch.setattr(switches, "fused_layer", False)
    mk = (lambda: _padded(g, dev)) if route == "padded" else (lambda: _on(g.data(), dev))
    e0, f0 = _plain(model, mk())
    out = hn.atom_properties(model, mk())
    assert torch.equal(out["energy"], e0) and torch.equal(out["forces"], f0)
    assert rel_err(out["energies"], ref["energies"]) <= TOL
    assert rel_err(out["virials"], ref["virials"]) <= TOL


@pytest.mark.gpu
def test_no_nan_under_debug_poison_and_bit_reproducible_on_the_10k_cell(monkeypatch):
    dev = _dev()
    monkeypatch.setenv("HERMNET_DEBUG_POISON", "1")
    model = Golden("c2_alloy10k").model().to(dev)
    d = synth.fcc_alloy(device=dev)
    a = hn.atom_properties(model, d)
    b = hn.atom_properties(model, d)
    for k in ("energy", "forces", "energies", "virials"):
        assert bool(torch.isfinite(a[k]).all()), k
        assert torch.equal(a[k], b[k]), k
    e0, f0 = _plain(model, synth.fcc_alloy(device=dev))
    assert torch.equal(a["energy"], e0) and torch.equal(a["forces"], f0)


@pytest.mark.gpu
def test_edge_less_graph_and_single_atom(monkeypatch):
    """No edge: every virial is zero and the energies are the read-out terms."""
    dev = _dev()
    g = Golden("mol16")
    model = g.model().to(dev)
    none = torch.zeros(2, 0, dtype=torch.long)
    cases = [hn.Data(pos=torch.tensor([[0.0, 0.0, 0.0], [20.0, 0.0, 0.0], [0.0, 20.0, 0.0]]),
                     atomic_number=torch.tensor([1, 6, 8]), edge_index=none, batch=torch.zeros(3, dtype=torch.long)),
             hn.Data(pos=torch.tensor([[1.0, 2.0, 3.0]]), atomic_number=torch.tensor([6]), edge_index=none,
                     batch=torch.zeros(1, dtype=torch.long))]
    for d in cases:
        out = hn.atom_properties(model, _on(d, dev))
        assert out["virials"].shape == (d.pos.size(0), 3, 3) and not bool(out["virials"].any())
        e_ref, _ = _oracle(g, d, monkeypatch)
        assert rel_err(out["energies"].cpu().double(), e_ref) <= TOL


@pytest.mark.gpu
def test_refusals():
    from hermnet_amd.sharding import partition
    dev = _dev()
    g = Golden("alloy108")
    model = g.model().to(dev)
    local, _plan = partition(g.data(), 0, 1)                 # a world-1 plan
    with pytest.raises(NotImplementedError):
        hn.atom_properties(model, local.to(dev))
    ht = hn.HTNet(["Si"], rc=5.0, num_layers=1, hidden_channels=64, num_rbf=32).eval().to(dev)
    with pytest.raises(NotImplementedError):
        hn.atom_properties(ht, _on(Golden("c1_si64").data(), dev))
    with pytest.raises(RuntimeError):                        # CPU tensors: there is no CPU path
        hn.atom_properties(model, g.data())


class _FakeAtoms(object):
    """Duck-typed stand-in for ase.Atoms (ASE is not installed on the MI355X image)."""

    def __init__(self, pos, z, cell):
        self.positions = pos
        self.numbers = np.asarray(z)
        self.cell = cell
        self.pbc = [cell is not None] * 3


@pytest.mark.gpu
def test_ase_energies_and_stresses():
    dev = str(_dev())
    g = Golden("alloy108")
    d = g.data()
    z = d.atomic_number.numpy()
    atoms = _FakeAtoms(d.pos.numpy().astype("float64"), z, d.cell[0].numpy().astype("float64"))
    calc = A.NNCalculator(g.model(), None, trn_mean=0.25, device_=dev)
    calc.calculate(atoms, ["energy", "forces", "stress", "energies", "stresses"])
    r = dict(calc.results)
    assert r["energies"].shape == (len(z),) and r["stresses"].shape == (len(z), 6)
    assert abs(r["energies"].sum() - r["energy"]) <= 1e-6 * np.abs(r["energies"]).sum()
    assert np.abs(r["stresses"].sum(0) - r["stress"]).max() <= 1e-5 * np.abs(r["stresses"]).sum(0).max()
    plain = A.NNCalculator(g.model(), None, trn_mean=0.25, device_=dev)
    plain.calculate(atoms, ["energy", "forces"])
    assert plain.results["energy"] == r["energy"] and np.array_equal(plain.results["forces"], r["forces"])
    # a replaying calculator asked for a per-atom property runs eagerly and gives the same values
    rep = A.NNCalculator(g.model(), None, trn_mean=0.25, device_=dev, graph_replay=True)
    rep.calculate(atoms, ["energy", "forces", "energies"])
    assert rep.graph_captures == 0 and "stresses" not in rep.results
    assert np.array_equal(rep.results["energies"], r["energies"]) and rep.results["energy"] == r["energy"]
    # the next call without per-atom properties leaves none behind
    calc.calculate(atoms, ["energy", "forces"])
    assert "energies" not in calc.results and "stresses" not in calc.results
    rep.calculate(atoms, ["energy", "forces"])
    assert "energies" not in rep.results and "stresses" not in rep.results
    # an open molecule: zero stresses
    m = Golden("mol16")
    md = m.data()
    keep = md.batch == 0
    mol = _FakeAtoms(md.pos[keep].numpy().astype("float64"), md.atomic_number[keep].numpy(), None)
    mc = A.NNCalculator(m.model(), None, trn_mean=0.1, device_=dev)
    mc.calculate(mol, ["energy", "forces", "energies", "stresses"])
    assert mc.results["stresses"].shape == (int(keep.sum()), 6) and not mc.results["stresses"].any()
    assert abs(mc.results["energies"].sum() - mc.results["energy"]) <= 1e-6 * np.abs(mc.results["energies"]).sum()
