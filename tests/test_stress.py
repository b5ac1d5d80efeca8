"""Stress from the ONE force backward (hermnet_amd.stress.energy_forces_stress, the C entry points hermnet_graph_virial and
hermnet_neighbor_count_devcell), in the captured steps (graph.GraphedStep / GraphedMDStep with `stress` / `variable_cell`)
and in the ASE calculator (`replay_stress`).

Definitions ("Stress"): W_b = sum_{i in b} W_i = -sum_{e in b} D_e (x) dE/dD_e (unsymmetrised, energy
units), stress_b = -sym(W_b) / |det cell_b|.  Bounds are the project's own: 5e-5 of the largest component for stresses and
virials (tests/test_gpu_parity.py, the ASE stress tests), bit-equality for energies and forces against a plain call and for
every replay against the eager evaluation of the same coordinates."""
import numpy as np
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import _lib, synth
from hermnet_amd.plugin import ase_interface as A
from helpers import Golden

ORACLE_CASES = ["c1_si64", "c1_si64_refcompat", "alloy108", "alloy108_unknown_type", "alloy108_h512_default", "mol16",
                "mol16_intensive", "alloy32_bessel_expenv", "alloy32_bernstein"]      # tests/test_atom_properties.py
BOUND = 5e-5
VOIGT = [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]


class _FakeAtoms(object):
    """Duck-typed stand-in for ase.Atoms (ASE is not installed on the MI355X image)."""

    def __init__(self, pos, z, cell):
        self.positions = pos
        self.numbers = np.asarray(z)
        self.cell = cell
        self.pbc = [cell is not None] * 3


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_argument_checks_of_the_graph_virial_entry_point_need_no_gpu():
    """hermnet_graph_virial refuses malformed calls before a launch; no graphs / no atoms is done."""
    lib = _lib.load()
    buf = np.zeros(256, dtype=np.float32)
    p = buf.ctypes.data
    OK, BAD = 0, 1
    need = lib.hermnet_graph_virial_workspace(1000)
    assert need >= 4 * 9 * 4 and lib.hermnet_graph_virial_workspace(0) > 0

    def call(n=1000, b=3, vir=p, rows=p, perm=p, batch=p, work=p, wbytes=None, out=p):
        return lib.hermnet_graph_virial(vir, rows, perm, batch, n, b, work, need if wbytes is None else wbytes, out, None)

    assert call(b=0) == OK and call(n=0) == OK and call(n=0, b=0) == OK          # nothing to sum: done
    assert call(n=0, vir=None, rows=None, perm=None, batch=None, work=None, wbytes=0) == OK
    assert call(n=-1) == BAD and call(b=-1) == BAD                                 # negative counts
    assert call(out=None) == BAD and call(n=0, out=None) == BAD                    # a missing output
    assert call(vir=None) == BAD and call(rows=None) == BAD and call(work=None) == BAD
    assert call(batch=None) == BAD                                                 # several graphs need the batch vector
    assert call(wbytes=need - 1) == BAD                                            # workspace too small


def test_argument_checks_of_the_device_cell_search_need_no_gpu():
    lib = _lib.load()
    buf = np.zeros(256, dtype=np.float32)
    p = buf.ctypes.data
    ws = lib.hermnet_neighbor_workspace(8)

    def call(n=8, pos=p, cell=p, rc=5.0, work=p, wbytes=ws, total=p):
        return lib.hermnet_neighbor_count_devcell(pos, n, cell, rc, work, wbytes, None, total, None)

    assert call(n=0) == 1 and call(n=-1) == 1 and call(rc=0.0) == 1 and call(rc=-1.0) == 1
    assert call(pos=None) == 1 and call(cell=None) == 1 and call(work=None) == 1 and call(total=None) == 1
    assert call(wbytes=64) == 1                                                    # a workspace without a stash slot


def test_stress_of_a_hand_made_virial():
    """stress = -sym(W) / V with V = |det cell|; graphs without a cell: zeros."""
    from hermnet_amd.stress import stress_of_virial
    w = torch.tensor([[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 10.0]],
                      [[0.5, -1.0, 0.0], [3.0, 0.25, 2.0], [-2.0, 0.0, 1.5]]], dtype=torch.float64)
    cell = torch.tensor([[[2.0, 0.0, 0.0], [0.5, 3.0, 0.0], [0.0, 0.25, 4.0]],
                         [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 2.0]]], dtype=torch.float64)      # det 24, det -2
    s = stress_of_virial(w, cell)
    for b, vol in ((0, 24.0), (1, 2.0)):
        want = -0.5 * (w[b] + w[b].T) / vol
        assert torch.allclose(s[b], want, rtol=0, atol=1e-14)
    assert torch.equal(s, s.transpose(1, 2))
    assert not bool(stress_of_virial(w, None).any())
    assert not bool(stress_of_virial(w, torch.zeros(2, 3, 3, dtype=torch.float64)).any())
    # the calculator's Voigt packing of the same tensor
    v = A.stress_from_virial(0.5 * (w[0] + w[0].T).numpy(), 24.0)
    assert np.allclose(v, [s[0][a, b] for a, b in VOIGT], rtol=0, atol=1e-14)


def test_energy_forces_stress_refusals_need_no_gpu():
    from hermnet_amd.sharding import partition
    g = Golden("alloy108")
    model = g.model()
    with pytest.raises(RuntimeError, match="MI355X only"):               # CPU tensors: there is no CPU path
        hn.energy_forces_stress(model, g.data())
    ht = hn.HTNet(["Si"], rc=5.0, num_layers=1, hidden_channels=64, num_rbf=32).eval()
    with pytest.raises(NotImplementedError):
        hn.energy_forces_stress(ht, Golden("c1_si64").data())
    with pytest.raises(NotImplementedError):
        hn.energy_forces_stress(g.model().train(), g.data())
    local, _plan = partition(g.data(), 0, 1)
    with pytest.raises(NotImplementedError):
        hn.energy_forces_stress(model, local)
    assert hn.energy_forces_stress is hn.stress.energy_forces_stress


def test_replay_stress_on_a_cpu_device_leaves_the_eager_path_in_charge(monkeypatch):
    g = Golden("alloy108")
    d = g.data()
    calc = A.NNCalculator(g.model(), None, trn_mean=0.0, device_="cpu", graph_replay=True, replay_stress=True)
    assert calc.replay_stress and A.NNCalculator(g.model(), None, 0.0, device_="cpu").replay_stress is False
    seen = []

    def eager(model, data, device, pbc, want, trn_mean=0.0, atom_props=None):
        seen.append(want)
        n = data.pos.size(0)
        return torch.zeros(1), torch.zeros(n, 3), torch.eye(3)

    monkeypatch.setattr(A, "_evaluate_finite", eager)
    monkeypatch.setattr(A.NNCalculator, "_replayed", lambda *a, **k: pytest.fail("no replay on a CPU device"))
    atoms = _FakeAtoms(d.pos.numpy().astype("float64"), d.atomic_number.numpy(), d.cell[0].numpy().astype("float64"))
    calc.calculate(atoms, ["energy", "forces", "stress"])
    assert seen == [True] and calc.graph_captures == 0 and calc.results["stress"].shape == (6,)
    calc.calculate(atoms, ["energy", "forces"])
    assert seen == [True, False] and "stress" not in calc.results


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _on(d, dev):
    """A copy of `d` on `dev` (Data.to moves in place)."""
    return hn.Data(**{k: v.to(dev) for k, v in d})


def _plain(model, d):
    pos = d.pos.detach().clone().requires_grad_(True)
    d.pos = pos
    e = model(d)
    return e.detach(), -torch.autograd.grad(e.sum(), pos)[0]


def _sym(w):
    return 0.5 * (w + w.transpose(-1, -2))


def _sheared(pos, cell, shear):
    """(pos, cell) strained by `shear` (rows of cell = lattice vectors), rounded to float32 values."""
    return ((pos.astype("float64") @ shear).astype("float32").astype("float64"),
            (cell.astype("float64") @ shear).astype("float32").astype("float64"))


def _periodic_batch(parts):
    """One Data from [(pos, cell, z)] float64 arrays: host neighbour lists, one graph each."""
    ds, off = [], 0
    out = dict(pos=[], atomic_number=[], edge_index=[], edge_shift=[], cell=[], batch=[])
    for b, (pos, cell, z) in enumerate(parts):
        d = synth.periodic_data(pos, cell, z, 5.0)
        out["pos"].append(d.pos)
        out["atomic_number"].append(d.atomic_number)
        out["edge_index"].append(d.edge_index + off)
        out["edge_shift"].append(d.edge_shift)
        out["cell"].append(d.cell)
        out["batch"].append(d.batch + b)
        off += d.pos.size(0)
        ds.append(d)
    return hn.Data(pos=torch.cat(out["pos"]), atomic_number=torch.cat(out["atomic_number"]),
                   edge_index=torch.cat(out["edge_index"], 1), edge_shift=torch.cat(out["edge_shift"]),
                   cell=torch.cat(out["cell"]), batch=torch.cat(out["batch"])), ds


def _three_cells():
    """Three jittered Si cells of different shape, size and shear."""
    shears = [np.eye(3) + np.array([[0.0, 0.0, 0.0], [0.06, 0.0, 0.0], [-0.04, 0.05, 0.0]]),
              np.eye(3) + np.array([[0.02, 0.03, 0.0], [0.0, -0.01, 0.04], [0.05, 0.0, 0.0]]),
              np.eye(3) + np.array([[-0.02, 0.0, 0.05], [0.04, 0.03, 0.0], [0.0, -0.03, 0.01]])]
    parts = []
    for k, (reps, a) in enumerate((((2, 2, 2), 5.43), ((2, 2, 3), 5.50), ((2, 3, 2), 5.38))):
        pos, cell = synth._lattice(synth._DIAMOND, a, reps)
        pos = pos + np.random.RandomState(10 + k).normal(scale=0.05, size=pos.shape)
        pos, cell = _sheared(pos, cell, shears[k])
        parts.append((pos, cell, np.full(len(pos), 14, dtype=np.int64)))
    return parts


def _fd_stress(g, d, model_sd=None):
    """[B,6] Voigt stresses by central differences of the float64 oracle energy under symmetric strain (fixed (i, j, S)
    list, coordinates and cells strained together: tests/test_gpu_parity.py's method), per graph."""
    from oracle import hermnet_oracle as orc
    sd = {k: v.double() for k, v in g.model().state_dict().items()}
    pos, cell = d.pos.double(), d.cell.double()
    vol = torch.linalg.det(cell).abs().numpy()

    def energy(eps):
        m = torch.from_numpy(np.eye(3) + eps)
        return orc.hvnet_energy(sd, g.elems, pos @ m, d.atomic_number, d.edge_index, d.batch, d.edge_shift.double(),
                                cell @ m, **g.oracle_kwargs()).detach().numpy()

    h = 1e-5
    fd = np.zeros((cell.size(0), 6))
    for k, (a, b) in enumerate(VOIGT):
        eps = np.zeros((3, 3))
        eps[a, b] += 0.5
        eps[b, a] += 0.5
        fd[:, k] = (energy(h * eps) - energy(-h * eps)) / (2 * h) / vol
    return fd


def _voigt(s):
    s = s.detach().cpu().double().numpy()
    return np.stack([s[:, a, b] for a, b in VOIGT], axis=1)


@pytest.mark.gpu
def test_stress_equals_the_strain_derivative_of_the_oracle_energy_on_the_sheared_alloy_cell():
    dev = _dev()
    g = Golden("alloy108")
    d0 = g.data()
    shear = np.eye(3) + np.array([[0.0, 0.0, 0.0], [0.06, 0.0, 0.0], [-0.04, 0.05, 0.0]])
    pos, cell = _sheared(d0.pos.numpy(), d0.cell[0].numpy(), shear)
    d = synth.periodic_data(pos, cell, d0.atomic_number.numpy(), 5.0)
    out = hn.energy_forces_stress(g.model().to(dev), _on(d, dev))
    assert out["virial"].shape == (1, 3, 3) and out["stress"].shape == (1, 3, 3)
    st, fd = _voigt(out["stress"]), _fd_stress(g, d)
    print("alloy108 sheared: stress", st, "fd", fd, "err/max", np.abs(st - fd).max() / np.abs(fd).max())
    assert np.abs(fd).min() > 0
    assert np.abs(st - fd).max() < BOUND * np.abs(fd).max(), (st, fd)


@pytest.mark.gpu
def test_stress_of_every_graph_of_a_batch_of_three_cells_equals_the_strain_derivative():
    dev = _dev()
    g = Golden("c1_si64")
    d, _ = _periodic_batch(_three_cells())
    out = hn.energy_forces_stress(g.model().to(dev), _on(d, dev))
    assert out["virial"].shape == (3, 3, 3)
    st, fd = _voigt(out["stress"]), _fd_stress(g, d)
    assert np.abs(fd).min() > 0                       # every component of every graph is exercised
    for b in range(3):
        print("graph", b, "err/max", np.abs(st[b] - fd[b]).max() / np.abs(fd[b]).max())
        assert np.abs(st[b] - fd[b]).max() < BOUND * np.abs(fd[b]).max(), (b, st[b], fd[b])


@pytest.mark.gpu
def test_virial_is_the_sum_of_the_per_atom_virials_and_its_symmetric_part_the_two_backward_virial():
    dev = _dev()
    batch3, _ = _periodic_batch(_three_cells())
    cases = [(Golden("c2_alloy10k"), lambda: synth.fcc_alloy(device=dev), True),
             (Golden("alloy108"), lambda: _on(Golden("alloy108").data(), dev), True),
             (Golden("c1_si64"), lambda: _on(batch3, dev), False),
             (Golden("mol16"), lambda: _on(Golden("mol16").data(), dev), False)]
    for g, mk, single in cases:
        model = g.model().to(dev)
        out = hn.energy_forces_stress(model, mk())
        d = mk()
        props = hn.atom_properties(model, d)
        nb = out["virial"].size(0)
        want = torch.zeros(nb, 3, 3, dtype=torch.float64).index_add_(0, d.batch.long().cpu(), props["virials"].double().cpu())
        got = out["virial"].double().cpu()
        assert float((got - want).abs().max()) <= BOUND * float(want.abs().max()), g.name
        if single:      # the parent's path: autograd.grad(E, pos) and virial_calc's autograd.grad(E, cell)
            _, _, w = A._evaluate(model, mk(), dev, True, True)
            w = w.double().cpu()
            assert float((_sym(got[0]) - w).abs().max()) <= BOUND * float(w.abs().max()), g.name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_energy_and_forces_are_those_of_a_plain_call(name):
    dev = _dev()
    g = Golden(name)
    model = g.model().to(dev)
    e0, f0 = _plain(model, _on(g.data(), dev))
    out = hn.energy_forces_stress(model, _on(g.data(), dev))
    assert torch.equal(out["energy"], e0) and torch.equal(out["forces"], f0)
    nb = e0.numel()
    assert out["virial"].shape == (nb, 3, 3) and out["stress"].shape == (nb, 3, 3)
    assert bool(torch.isfinite(out["virial"]).all()) and bool(torch.isfinite(out["stress"]).all())
    if g.data().get("cell") is None:
        assert not bool(out["stress"].any())
    off = hn.energy_forces_stress(model, _on(g.data(), dev), trn_mean=0.5)
    assert torch.equal(off["energy"], e0 + 0.5) and torch.equal(off["virial"], out["virial"])


@pytest.mark.gpu
def test_mixed_open_and_periodic_batch():
    """A batch with a cell for every graph where only some edges carry a shift (an "open" graph in a big box): energy and
    forces as a plain call, the open graph's virial is sum_i pos_i (x) F_i."""
    dev = _dev()
    g = Golden("c1_si64")
    a = synth.si_diamond(reps=(2, 2, 2), seed=3)
    pos_b = synth._lattice(synth._DIAMOND, 5.43, (1, 1, 2))[0] + np.random.RandomState(5).normal(scale=0.05, size=(16, 3))
    i, j, _ = synth.neighbor_list(pos_b, 5.0, None)
    nb_, na = len(pos_b), a.pos.size(0)
    d = hn.Data(pos=torch.cat([a.pos, torch.from_numpy(pos_b.astype(np.float32))]),
                atomic_number=torch.cat([a.atomic_number, torch.full((nb_,), 14, dtype=torch.long)]),
                edge_index=torch.cat([a.edge_index, torch.from_numpy(np.vstack([j, i])).long() + na], 1),
                edge_shift=torch.cat([a.edge_shift, torch.zeros(len(i), 3)]),
                cell=torch.cat([a.cell, 100.0 * torch.eye(3).reshape(1, 3, 3)]),
                batch=torch.cat([a.batch, torch.ones(nb_, dtype=torch.long)]))
    model = g.model().to(dev)
    e0, f0 = _plain(model, _on(d, dev))
    out = hn.energy_forces_stress(model, _on(d, dev))
    assert torch.equal(out["energy"], e0) and torch.equal(out["forces"], f0)
    pf = (d.pos[na:].double()[:, :, None] * out["forces"][na:].double().cpu()[:, None, :]).sum(0)
    assert float((out["virial"][1].double().cpu() - pf).abs().max()) <= BOUND * float(pf.abs().max())


@pytest.mark.gpu
def test_bit_reproducible_also_under_debug_poison_and_batch_rows_equal_the_graphs_alone(monkeypatch):
    dev = _dev()
    g = Golden("c1_si64")
    model = g.model().to(dev)
    batch3, singles = _periodic_batch(_three_cells())
    alloy = Golden("c2_alloy10k").model().to(dev)
    for poison in ("0", "1"):
        monkeypatch.setenv("HERMNET_DEBUG_POISON", poison)
        for m, mk in ((model, lambda: _on(batch3, dev)), (alloy, lambda: synth.fcc_alloy(reps=(6, 6, 6), device=dev))):
            a, b = hn.energy_forces_stress(m, mk()), hn.energy_forces_stress(m, mk())
            for k in ("energy", "forces", "virial", "stress"):
                assert bool(torch.isfinite(a[k]).all()), k
                assert torch.equal(a[k], b[k]), (poison, k)
    monkeypatch.setenv("HERMNET_DEBUG_POISON", "0")
    # every graph alone: the same rows within the bound (the chunks of the ordered sum are aligned to the batch's atom
    # positions, so a graph's summation order depends on where it starts in the batch: not bitwise)
    both = hn.energy_forces_stress(model, _on(batch3, dev))
    for b, d in enumerate(singles):
        alone = hn.energy_forces_stress(model, _on(d, dev))
        scale = float(alone["virial"].abs().max())
        assert float((both["virial"][b] - alone["virial"][0]).abs().max()) <= BOUND * scale, b


def _walk_model(dev):
    kw = dict(rc=5.0, num_layers=3, hidden_channels=128, num_rbf=64)
    model = hn.HVNet(["Al", "Ni", "Cu"], **kw).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 8))
    model = model.to(dev)
    for p_ in model.parameters():
        p_.requires_grad_(False)
    return model


def _exact(model, p, cell_t, z_t, batch):
    """Eager `energy_forces_stress` on the exact list of (p, cell_t) -> (energy, forces, virial, edges)."""
    ei, sh = hn.neighbor_search(p, 5.0, cell_t)
    d = hn.Data(pos=p.clone(), atomic_number=z_t, batch=batch, cell=cell_t.reshape(1, 3, 3), edge_index=ei, edge_shift=sh)
    out = hn.energy_forces_stress(model, d)
    return out["energy"], out["forces"], out["virial"], int(ei.size(1))


@pytest.mark.gpu
def test_md_step_and_fixed_list_step_with_stress_replay_as_one_graph():
    """The random walk of test_md_step_with_list_rebuild_replays_as_one_graph with `stress=True`: every replay's (energy,
    forces, virial) equals the eager `energy_forces_stress` on the exact list of the same coordinates bit for bit, `fetch()`
    returns the same numbers, and energy / forces equal the plain captured step's.  `GraphedStep(stress=True)` holds ONE list
    by construction (the exact list of the walk's first coordinates): its replays along the walk are compared with the eager
    evaluation of the walk's coordinates on that list."""
    from hermnet_amd.graph import GraphedMDStep, GraphedStep
    dev = _dev()
    pos, cell, z = synth.fcc_alloy_atoms(reps=(3, 3, 4))
    pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
    cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
    z_t = torch.from_numpy(z).to(dev)
    model = _walk_model(dev)
    batch = torch.zeros(len(z), dtype=torch.long, device=dev)
    step = GraphedMDStep(model, z_t, cell_t, pos_t, stress=True)
    plain = GraphedMDStep(model, z_t, cell_t, pos_t)
    assert len(plain.fetch()) == 4 and len(plain()) == 2                  # stress=False: what they return today
    gen = torch.Generator().manual_seed(2)
    cur = pos_t.clone()
    fixed = fixed_d = None
    counts = set()
    for it in range(12):
        cur = cur + (0.25 * (torch.rand(cur.shape, generator=gen) - 0.5)).to(dev)
        e, f, w = [t.clone() for t in step(cur)]
        he, hf, ok, n, hw = step.fetch()
        ep, fp = [t.clone() for t in plain(cur)]
        e0, f0, w0, n0 = _exact(model, cur, cell_t, z_t, batch)          # eager work between replays
        torch.zeros(1 << 16, device=dev).sum()
        assert ok and n == n0, (it, n, n0)
        assert torch.equal(e, e0) and torch.equal(f, f0) and torch.equal(w, w0), it
        assert torch.equal(ep, e0) and torch.equal(fp, f0), it
        assert np.array_equal(he, e0.cpu().numpy()) and np.array_equal(hf, f0.cpu().numpy())
        assert hw.shape == (1, 3, 3) and np.array_equal(hw, w0.cpu().numpy())
        counts.add(n)
        if fixed is None:
            ei, sh = hn.neighbor_search(cur, 5.0, cell_t)
            fixed_d = hn.Data(pos=cur.clone(), atomic_number=z_t, batch=batch, cell=cell_t.reshape(1, 3, 3), edge_index=ei,
                              edge_shift=sh)
            fixed = GraphedStep(model, hn.Data(**{k: v for k, v in fixed_d}), stress=True)
        eg, fg, wg = [t.clone() for t in fixed(cur)]
        fixed_d.pos = cur.clone()
        ref = hn.energy_forces_stress(model, fixed_d)
        assert torch.equal(eg, ref["energy"]) and torch.equal(fg, ref["forces"]) and torch.equal(wg, ref["virial"]), it
        if it == 0:
            assert torch.equal(wg, w0)
    assert len(counts) > 3


def _bins(cell, rc=5.0):
    """floor(h / rc) per axis, h = plane spacings of the cell (rows = lattice vectors): the search's bin grid."""
    inv = np.linalg.inv(np.asarray(cell, dtype=np.float64))
    h = 1.0 / np.sqrt((inv ** 2).sum(0))
    return tuple(int(max(1, min(1024, np.floor(x / rc)))) for x in h), h


def _strain_walk(steps=14):
    """(strain matrices) with diagonal and shear components of a few percent; zz runs from -2 % to +6 %."""
    rs = np.random.RandomState(7)
    out = []
    for k in range(steps):
        eps = rs.uniform(-0.03, 0.03, size=(3, 3))
        eps = 0.5 * (eps + eps.T)
        eps[2, 2] = -0.02 + 0.08 * k / (steps - 1)
        out.append(np.eye(3) + eps)
    return out


@pytest.mark.gpu
def test_variable_cell_md_step_replays_one_capture_while_positions_and_cell_are_strained():
    from hermnet_amd.graph import GraphedMDStep
    from hermnet_amd.neighbor import neighbor_search_padded
    dev = _dev()
    pos, cell, z = synth.fcc_alloy_atoms(reps=(3, 3, 4))
    z_t = torch.from_numpy(z).to(dev)
    model = _walk_model(dev)
    batch = torch.zeros(len(z), dtype=torch.long, device=dev)
    pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
    cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
    n_first = int(hn.neighbor_search(pos_t, 5.0, cell_t)[0].size(1))
    step = GraphedMDStep(model, z_t, cell_t, pos_t, capacity=int(1.4 * n_first), stress=True, variable_cell=True)
    with pytest.raises(RuntimeError):
        GraphedMDStep(model, z_t, cell_t, pos_t, capacity=int(1.4 * n_first))(pos_t, cell_t)     # a baked-in cell
    captured = step.graph
    gen = np.random.RandomState(3)
    grids, counts = set(), set()
    for it, m in enumerate(_strain_walk()):
        p64 = (pos + gen.uniform(-0.1, 0.1, size=pos.shape)) @ m
        c32 = (cell @ m).astype(np.float32)
        grid, h = _bins(c32)
        assert np.abs(h / 5.0 - np.round(h / 5.0)).min() > 1e-6          # (no spacing on a bin boundary: the grid is decided)
        grids.add(grid)
        cur = torch.from_numpy(p64.astype(np.float32)).to(dev)
        cur_cell = torch.from_numpy(c32).to(dev)
        e, f, w = [t.clone() for t in step(cur, cur_cell)]
        he, hf, ok, n, hw = step.fetch()
        e0, f0, w0, n0 = _exact(model, cur, cur_cell, z_t, batch)
        torch.zeros(1 << 16, device=dev).sum()
        assert ok and n == n0, (it, n, n0)
        assert torch.equal(e, e0) and torch.equal(f, f0) and torch.equal(w, w0), it
        assert np.array_equal(hw, w0.cpu().numpy())
        # the list itself: bit for bit the host-cell search's
        a = neighbor_search_padded(cur, 5.0, cur_cell, step.capacity, device_cell=True)
        b = neighbor_search_padded(cur, 5.0, cur_cell, step.capacity)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), it
        ei, sh = hn.neighbor_search(cur, 5.0, cur_cell)
        assert torch.equal(a[0][:, :n0], ei) and torch.equal(a[1][:n0], sh)
        counts.add(n)
    assert len(grids) > 1, grids                                        # the bin grid changed along the walk
    assert len(counts) > 3 and step.graph is captured                   # ONE capture for the whole walk


@pytest.mark.gpu
def test_degenerate_cell_raises_the_flag_and_the_capture_survives():
    from hermnet_amd import neighbor as nb
    from hermnet_amd.graph import GraphedMDStep
    dev = _dev()
    pos, cell, z = synth.fcc_alloy_atoms(reps=(3, 3, 4))
    z_t = torch.from_numpy(z).to(dev)
    model = _walk_model(dev)
    batch = torch.zeros(len(z), dtype=torch.long, device=dev)
    pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
    cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
    step = GraphedMDStep(model, z_t, cell_t, pos_t, stress=True, variable_cell=True)
    captured, stash = step.graph, dict(nb._STASH)
    squeezed = cell_t * 0.05                                             # plane spacings ~0.6 A: reach = ceil(5 / 0.54) > 8
    assert int(np.ceil(5.0 / _bins(squeezed.cpu().numpy())[1].min())) > 8
    step(pos_t * 0.05, squeezed)
    out = step.fetch()
    assert out[2] is False and (step.last_flags & 8)
    assert step.check()[0] is False
    for singular in (torch.zeros(3, 3, device=dev), torch.ones(3, 3, device=dev)):
        step(pos_t, singular)
        assert step.fetch()[2] is False and (step.last_flags & 8)
    assert dict(nb._STASH) == stash and step.graph is captured
    e, f, w = [t.clone() for t in step(pos_t, cell_t)]                   # a sane cell: the same capture, correct again
    he, hf, ok, n, hw = step.fetch()
    e0, f0, w0, n0 = _exact(model, pos_t, cell_t, z_t, batch)
    assert ok and n == n0 and step.last_flags == 0
    assert torch.equal(e, e0) and torch.equal(f, f0) and torch.equal(w, w0)


@pytest.mark.gpu
def test_calculator_replays_the_stress_along_a_trajectory_of_changing_cells():
    dev = str(_dev())
    g = Golden("alloy108")
    d = g.data()
    z, cell0, pos0 = d.atomic_number.numpy(), d.cell[0].numpy().astype("float64"), d.pos.numpy().astype("float64")
    calc = A.NNCalculator(g.model(), None, trn_mean=0.25, device_=dev, graph_replay=True, replay_stress=True)
    ref = A.NNCalculator(g.model(), None, trn_mean=0.25, device_=dev)
    rs = np.random.RandomState(4)
    for it, m in enumerate(_strain_walk(5)):
        pos = (pos0 + rs.normal(scale=0.03, size=pos0.shape)) @ m
        cell = cell0 @ m
        calc.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces", "stress"])
        ref._edge_capacity = None
        ref.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces", "stress"])
        assert calc.results["energy"] == ref.results["energy"]
        assert np.array_equal(calc.results["forces"], ref.results["forces"])
        st, want = calc.results["stress"], ref.results["stress"]
        print("step", it, "stress err/max", np.abs(st - want).max() / np.abs(want).max())
        assert st.shape == (6,) and np.abs(st - want).max() <= BOUND * np.abs(want).max(), (it, st, want)
    assert calc.graph_captures == 1                                      # a cell change alone never recaptures
    calc.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])       # without the stress: the key is dropped
    assert "stress" not in calc.results and calc.graph_captures == 1
    assert np.array_equal(calc.results["forces"], ref.results["forces"])
    npt = A.NNCalculator(g.model(), None, trn_mean=0.25, device_=dev, ensemble="NPT", graph_replay=True, replay_stress=True)
    npt.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])        # NPT: the stress comes with every call
    assert npt.graph_captures == 1 and np.abs(npt.results["stress"] - want).max() <= BOUND * np.abs(want).max()
    # a degenerate cell: the capture is dropped and the eager path answers (here: with its own refusal of that cell)
    with pytest.raises(RuntimeError):
        calc.calculate(_FakeAtoms(pos * 0.05, z, cell * 0.05), ["energy", "forces", "stress"])
    assert calc._graphed is None
    # the default (replay_stress=False): a call that needs the stress takes the eager path and leaves the capture alone
    plain = A.NNCalculator(g.model(), None, trn_mean=0.25, device_=dev, graph_replay=True)
    plain.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces"])
    plain.calculate(_FakeAtoms(pos, z, cell), ["energy", "forces", "stress"])
    assert plain.graph_captures == 1 and not plain._graphed[1].stress and not plain._graphed[1].variable_cell
    assert np.abs(plain.results["stress"] - want).max() <= BOUND * np.abs(want).max()
