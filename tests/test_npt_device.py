"""GPU: `hermnet_amd.md.DeviceNPT` -- the Berendsen barostat inside the replayed hipGraph -- against the host-driven NPT loop
it replaces (tests/npt_reference.NumpyNPT around a plain `GraphedMDStep(stress=True, variable_cell=True)` /
`GraphedBatchMDStep(stress=True)` that is fed the float32 roundings of coordinates and cell), bit for bit; the device kernels
against the library's host twins; compressibility 0 against `DeviceMD`; halt under compression and resume; replicas at
different pressures in one capture; the ASE hand-off.

The model and the systems are tests/test_md_device.py's (3 layers, width 128; the 144-atom cell; the batch of 32, 48 and 144
atoms): the smallest shapes with a graph below a wave, unequal ranges and boxes under twice the cutoff."""
import numpy as np
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import _lib
from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep
from hermnet_amd.md import GPA, HALT_CAPACITY, DeviceNPT
from md_reference import AMU, advance_np, bits
from npt_reference import HostNPT, NumpyNPT
import test_md_device as mdt
import test_npt_host as nph

pytestmark = pytest.mark.gpu

DT = mdt.DT
_CACHE = {}


def _system(name):
    return mdt._single() if name == "single" else mdt._batched()


def _data(s):
    """The start configuration on the exact list."""
    z, cell, batch = mdt._tensors(s)
    p = torch.from_numpy(s["pos"].astype(np.float32)).to(mdt._dev())
    if batch is None:
        ei, sh = hn.neighbor_search(p, 5.0, cell)
        return hn.Data(pos=p, atomic_number=z, cell=cell.reshape(1, 3, 3), edge_index=ei, edge_shift=sh)
    B = int(s["batch"][-1]) + 1
    ei, sh = hn.neighbor_search(p, 5.0, cell, batch=batch, num_graphs=B)
    return hn.Data(pos=p, atomic_number=z, batch=batch, cell=cell, edge_index=ei, edge_shift=sh)


def _start_pressure(name):
    """(P_start [B], edges of the start list) from `energy_forces_stress` on the start configuration plus the ideal-gas term
    of the start velocities: the reference, never the code under test."""
    if ("p", name) not in _CACHE:
        s = _system(name)
        d = _data(s)
        stress = hn.energy_forces_stress(mdt._shared_model(), d)["stress"].double().cpu().numpy()
        b = np.zeros(len(s["z"]), dtype=np.int64) if s["batch"] is None else s["batch"]
        B = int(b[-1]) + 1
        vol = np.abs(np.linalg.det(s["cell"].astype(np.float32).astype(np.float64).reshape(B, 3, 3)))
        kin = np.bincount(b, weights=s["m"] * AMU * (s["v"] ** 2).sum(axis=1), minlength=B)
        _CACHE[("p", name)] = (-np.trace(stress, axis1=1, axis2=2) / 3.0 + kin / (3.0 * vol), int(d.edge_index.size(1)))
    return _CACHE[("p", name)]


OFFSET = 0.05                   # eV/A^3 (8 GPa) between target and start pressure: see `_target`


def _target(name):
    """The target pressures [B] of the trajectory tests: OFFSET below each graph's start pressure, so the cells expand (the
    list shrinks: no capacity halt).  OFFSET is about three times the ideal-gas pressure n kB T = 0.018 eV/A^3 of these cells
    at 2500 K -- the scale on which the pressure of such a small hot cell fluctuates --, so P0 - P stays within a small factor
    of its start value and the strain per step (2e-3 at the start) stays below the default max_strain of 1e-2."""
    return _start_pressure(name)[0] - OFFSET


def _compressibility(name, strain=2e-3):
    """taup = dt, so c = compressibility / 3: chosen so that c |P0 - P_start| = `strain` for every graph."""
    return 3.0 * strain / np.abs(_target(name) - _start_pressure(name)[0])


def _npt(s, **kw):
    z, _, batch = mdt._tensors(s)
    if batch is not None:
        kw.update(batch=batch, num_graphs=int(s["batch"][-1]) + 1)
    kw.setdefault("velocities", s["v"])
    return DeviceNPT(mdt._shared_model(), z, s["cell"], s["pos"], s["m"], DT, taup=DT, **kw)      # (the cell in float64)


class _LoopNPT(NumpyNPT):
    """NumpyNPT with the Gaussians of the DEVICE's generator (hermnet_md_noise: the device's log / cos / sqrt differ from the
    host's in the last bits, tests/test_md_device.py), so that a Langevin trajectory can be compared bit for bit."""

    def advance(self):
        xi = None
        if self.c1_atom is not None:
            g = torch.zeros(len(self.x), 3, dtype=torch.float64, device=mdt._dev())
            _lib.check(_lib.load().hermnet_md_noise(self.seed, self.step, len(self.x), None, _lib.ptr(g),
                                                    torch.cuda.current_stream().cuda_stream), "noise")
            xi = g.cpu().numpy()
        advance_np(self.x, self.v, self.image, self.f, self.kick, self.dt, self.c1_atom, self.sigma, xi, self.cell, self.inv)
        return self.x.astype(np.float32)


def _host_driven(s, steps, **baro):
    """The host-driven NPT loop: numpy float64 integrator and barostat, each step's forces and virial from a plain graphed
    step on float32(x) in float32(cell), fetched in one packed copy.  A list of per-step records."""
    dev = mdt._dev()
    z, cell, batch = mdt._tensors(s)
    B = 1 if batch is None else int(s["batch"][-1]) + 1
    p0 = torch.from_numpy(s["pos"].astype(np.float32)).to(dev)
    if batch is None:
        step = GraphedMDStep(mdt._shared_model(), z, cell, p0, stress=True, variable_cell=True)
    else:
        step = GraphedBatchMDStep(mdt._shared_model(), z, cell, p0, batch, B, stress=True)

    def evaluate(p32, cell32):
        shape = (3, 3) if batch is None else (B, 3, 3)
        step(torch.from_numpy(p32).to(dev), torch.from_numpy(cell32.reshape(shape)).to(dev))
        e, f, ok, n, w = step.fetch()
        assert ok
        return e.copy(), f.copy(), n, w.copy()

    ref = _LoopNPT(s["pos"], s["v"], s["m"], DT, s["cell"], taup=DT, batch=s["batch"], num_graphs=B, **baro)
    _, ref.f, _, _ = evaluate(ref.x.astype(np.float32), ref.cell32)
    hist = []
    for _ in range(steps):
        e, f, n, w = evaluate(ref.advance(), ref.cell32)
        ref.finish(f, w, energy=e, edges=n)
        hist.append(dict(x=ref.x.copy(), v=ref.v.copy(), image=ref.image.copy(), f=f, cell=ref.cell64.copy(), n=n,
                         log=ref.log[-1].copy()))
    return ref, hist


def _equals(snap, rec):
    return (np.array_equal(bits(snap.positions), bits(rec["x"])) and np.array_equal(bits(snap.velocities), bits(rec["v"]))
            and np.array_equal(snap.images, rec["image"]) and np.array_equal(snap.forces, rec["f"])
            and np.array_equal(bits(snap.cell.reshape(-1, 9)), bits(rec["cell"])))


@pytest.mark.parametrize("friction", [None, 0.01], ids=["verlet", "langevin"])
@pytest.mark.parametrize("coupling", ["isotropic", "full"])
@pytest.mark.parametrize("name", ["single", "batch"])
def test_npt_trajectory_equals_the_host_driven_loop_bit_for_bit(name, coupling, friction):
    """`DeviceNPT.run(20)` against the host-driven loop: x, v, images, cell and forces bit-equal after 20 steps; every logged
    E_pot, pressure and volume that step's, bit for bit; the volume moved by more than 1 %, the list took more than three
    sizes and the clamp never acted."""
    s = _system(name)
    B = 1 if name == "single" else 3
    baro = dict(pressure=_target(name), compressibility=_compressibility(name), coupling=coupling)
    if friction is not None:
        baro.update(friction=friction, temperature=600.0 if B == 1 else [300.0, 600.0, 900.0], seed=(5 << 32) + 3)
    ref, hist = _host_driven(s, 20, **baro)
    md = _npt(s, **baro)
    md.run(20)
    snap = md.fetch()
    assert (snap.step, snap.halted, snap.halt_code, snap.halt_step) == (20, False, 0, None)
    assert snap.log.shape == (20, B, 5)
    for row, rec in zip(snap.log, hist):
        for col in (0, 3, 4):                                        # E_pot, pressure, volume: bit for bit
            assert np.array_equal(bits(row[:, col]), bits(rec["log"][:, col])), col
        assert np.all(row[:, 2] == rec["n"])
        assert np.array_equal(bits(row[:, 1]), bits(rec["log"][:, 1]))       # E_kin: the canonical sums on both sides
    assert _equals(snap, hist[-1])
    assert np.allclose(snap.volume, np.abs(np.linalg.det(snap.cell)), rtol=1e-12, atol=0)
    v_first, v_last = snap.log[0, :, 4], snap.volume
    assert np.all(np.abs(v_last / v_first - 1.0) > 1e-2), v_last / v_first            # the cell really moved
    assert len(set(rec["n"] for rec in hist)) > 3                                     # ... and so did the list
    assert not snap.clamped.any() and not ref.clamped.any()                           # the clamp never engaged
    assert md.fetch().log.shape[0] == 0


def _on_device(host, dev):
    names = ["x", "v", "x0", "v0", "image", "image0", "f_prev", "kick", "c1", "sigma", "batch", "cell", "inv", "pos32", "state",
             "graph_ptr", "half_mass", "ke_atom", "log", "cell64", "mu", "clamped", "p0", "c"]
    return {k: None if getattr(host, k) is None else torch.from_numpy(getattr(host, k).copy()).to(dev) for k in names}


@pytest.mark.parametrize("coupling", ["isotropic", "axes", "full"])
def test_device_kernels_equal_the_host_twin(coupling):
    """Two steps of hermnet_md_advance + hermnet_md_finish_npt on the synthetic inputs of tests/test_npt_host.py, uploaded,
    against the host twins: everything bit-equal (the second step wraps with the inverse the first one made)."""
    dev, lib, P = mdt._dev(), _lib.load(), _lib.ptr
    s = nph.synthetic()
    n = s["n"]
    host = nph.make(HostNPT, s, coupling, log_steps=4)
    rs = np.random.RandomState(31)
    host.f_prev[:] = rs.normal(size=(n, 3)).astype(np.float32)
    host.state[0] = 6
    d = _on_device(host, dev)
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(2):
        f, w, e = nph.evaluation(rs, n)
        total = np.array([4321 + k, 0], dtype=np.int64)
        f_d, w_d, e_d, t_d = (torch.from_numpy(a).to(dev) for a in (f, w, e, total))
        _lib.check(lib.hermnet_md_advance(n, 4, host.flags, host.dt, host.seed, P(d["x"]), P(d["v"]), P(d["x0"]), P(d["v0"]),
                                          P(d["image"]), P(d["image0"]), P(d["f_prev"]), P(d["kick"]), P(d["c1"]), P(d["sigma"]),
                                          P(d["batch"]), P(d["cell"]), P(d["inv"]), P(d["pos32"]), P(d["state"]), stream),
                   "advance")
        _lib.check(lib.hermnet_md_finish_npt(
            n, 4, P(d["graph_ptr"]), P(d["batch"]), P(f_d), P(e_d), P(w_d), P(t_d), 5000, host.coupling, host.mask,
            host.max_strain, P(d["p0"]), P(d["c"]), P(d["x"]), P(d["v"]), P(d["x0"]), P(d["v0"]), P(d["image"]), P(d["image0"]),
            P(d["f_prev"]), P(d["kick"]), P(d["half_mass"]), P(d["pos32"]), P(d["ke_atom"]), P(d["cell64"]), P(d["cell"]),
            P(d["inv"]), P(d["mu"]), P(d["clamped"]), P(d["log"]), 4, P(d["state"]), stream), "finish")
        torch.cuda.synchronize()
        host.advance()
        host.finish(f, w, energy=e, total=total, capacity=5000)
        got = {key: d[key].cpu().numpy() for key in ("x", "v", "image", "f_prev", "state", "log", "cell64", "cell", "inv", "mu",
                                                     "clamped", "pos32")}
        assert got["state"].tolist() == host.state.tolist() == [7 + k, 0, 0, 0]
        assert np.array_equal(got["image"], host.image) and np.array_equal(got["f_prev"], host.f_prev)
        assert np.array_equal(bits(got["x"]), bits(host.x)) and np.array_equal(bits(got["v"]), bits(host.v))
        assert np.array_equal(got["pos32"], host.pos32) and np.array_equal(got["cell"], host.cell)
        assert np.array_equal(bits(got["cell64"]), bits(host.cell64)) and np.array_equal(bits(got["inv"]), bits(host.inv))
        assert np.array_equal(bits(got["mu"]), bits(host.mu)) and np.array_equal(got["clamped"], host.clamped)
        assert np.array_equal(bits(got["log"]), bits(host.log))
    assert np.abs(host.image).max() >= 1 and not host.clamped.any()
    assert np.all(host.log[[0, 1]] == -7.0) and np.all(host.log[[2, 3]][:, :, 2] >= 4321)


@pytest.mark.parametrize("name", ["single", "batch"])
def test_zero_compressibility_matches_device_md(name):
    """compressibility 0: ten steps and their forces bit-equal to `DeviceMD` on the same system -- the virial kernels in the
    capture do not perturb energy or forces, and mu = I moves nothing."""
    s = _system(name)
    md = mdt._device_md(s)
    npt = _npt(s, pressure=0.01, compressibility=0.0, coupling="full")
    md.run(10)
    npt.run(10)
    a, b = md.fetch(), npt.fetch()
    assert (a.step, b.step, a.halted, b.halted) == (10, 10, False, False)
    assert np.array_equal(bits(a.positions), bits(b.positions)) and np.array_equal(bits(a.velocities), bits(b.velocities))
    assert np.array_equal(a.images, b.images) and np.array_equal(a.forces, b.forces)
    assert np.array_equal(bits(a.log[:, :, 0]), bits(b.log[:, :, 0])) and np.array_equal(a.log[:, :, 2], b.log[:, :, 2])
    assert np.array_equal(b.cell.astype(np.float32), s["cell"].astype(np.float32).reshape(-1, 3, 3)) and not b.clamped.any()


def test_halt_under_compression_and_resume():
    """A capacity equal to the first list's count and a pressure far above the start's: the cell shrinks, the list outgrows
    its columns, the run halts with the capacity bit in the state (cell included) of the last committed step; resume()
    recaptures and the run ends bit-equal to an uninterrupted one with a generous capacity."""
    s = dict(_system("single"))
    s["v"] = 0.2 * s["v"]                                # cool: the list grows because the cell shrinks
    p_start, first = _start_pressure("single")
    baro = dict(pressure=float(p_start[0]) + 1.0, compressibility=3.0 * 5e-3, coupling="isotropic")     # c (P0 - P) = 5e-3
    free = _npt(s, capacity=4 * first, **baro)
    md = _npt(s, capacity=first, **baro)
    assert md.capacity == first
    md.run(20)
    snap = md.fetch()
    k = snap.step
    assert snap.halted and 1 <= k < 20 and snap.halt_step == k and (snap.halt_code & HALT_CAPACITY)
    assert snap.log.shape[0] == k
    free.run(k)
    want = free.fetch()
    assert not want.halted and want.step == k

    def same(a, b):
        return (np.array_equal(bits(a.positions), bits(b.positions)) and np.array_equal(bits(a.velocities), bits(b.velocities))
                and np.array_equal(a.images, b.images) and np.array_equal(a.forces, b.forces)
                and np.array_equal(bits(a.cell), bits(b.cell)) and np.array_equal(bits(a.mu), bits(b.mu)))

    assert same(snap, want) and np.array_equal(bits(snap.log), bits(want.log))
    assert np.all(snap.volume < 0.99 * snap.log[0, :, 4])                            # it was compression that did it
    md.resume()
    assert md.capacity > first
    md.run(20 - k)
    free.run(20 - k)
    end, want = md.fetch(), free.fetch()
    assert (end.step, end.halted, want.step, want.halted) == (20, False, 20, False)
    assert same(end, want) and np.array_equal(bits(end.log), bits(want.log))


def test_replicas_at_different_pressures_in_one_capture():
    """Three copies of one cell at three target pressures in one capture: each equals its own single-structure run, bit for
    bit over ten steps."""
    from hermnet_amd import synth
    pos, cell, z = synth.fcc_alloy_atoms(reps=(2, 2, 3), seed=1)
    n = len(z)
    m = np.array([mdt.MASS[int(a)] for a in z])
    v = mdt._velocities(m, mdt.HOT, 6)
    dev, model = mdt._dev(), mdt._shared_model()
    pressures = [-2.0 * GPA, 0.0, 5.0 * GPA]
    baro = dict(compressibility=0.5, taup=20.0 * DT, coupling="full")
    z_t = torch.from_numpy(np.tile(z, 3)).to(dev)
    batch = torch.from_numpy(np.repeat(np.arange(3), n)).to(dev)
    both = DeviceNPT(model, z_t, np.stack([cell] * 3).astype(np.float32), np.tile(pos, (3, 1)), np.tile(m, 3), DT,
                     velocities=np.tile(v, (3, 1)), pressure=pressures, batch=batch, num_graphs=3, **baro)
    both.run(10)
    got = both.fetch()
    assert got.step == 10 and not got.halted and got.log.shape == (10, 3, 5)
    cells = set()
    for g, p in enumerate(pressures):
        one = DeviceNPT(model, z_t[:n], cell.astype(np.float32), pos, m, DT, velocities=v, pressure=p, **baro)
        one.run(10)
        alone = one.fetch()
        sl = slice(g * n, (g + 1) * n)
        assert np.array_equal(bits(got.positions[sl]), bits(alone.positions)), g
        assert np.array_equal(bits(got.velocities[sl]), bits(alone.velocities)) and np.array_equal(got.images[sl], alone.images)
        assert np.array_equal(got.forces[sl], alone.forces) and np.array_equal(bits(got.cell[g]), bits(alone.cell[0]))
        # E_kin, pressure, volume.  (Not E_pot: the model's float32 energy read-out sums a graph's atoms in an order that
        # depends on where the graph lies in the batch; nothing of the trajectory is made from it.)
        assert np.array_equal(bits(got.log[:, g, [1, 3, 4]]), bits(alone.log[:, 0, [1, 3, 4]]))
        cells.add(bits(alone.cell).tobytes())
    assert len(cells) == 3


class _FakeAtoms(mdt._FakeAtoms):
    def set_cell(self, cell, scale_atoms=False):
        assert not scale_atoms
        self.cell = np.array(cell)


def test_ase_hand_off_round_trips_the_cell_and_open_batches_are_refused():
    s = _system("single")
    cell = s["cell"].astype(np.float64) * (1.0 + 1e-9)                                # not representable in float32
    atoms = _FakeAtoms(s["pos"], s["z"], cell, s["m"], s["v"] * hn.md.ASE_TIME_FS)
    md = DeviceNPT.from_atoms(atoms, mdt._shared_model(), DT, pressure=0.0, compressibility=_compressibility("single")[0],
                              taup=DT)
    snap = md.fetch()
    assert np.array_equal(bits(snap.cell[0]), bits(cell)) and snap.step == 0 and snap.volume.shape == (1,)
    out = _FakeAtoms(np.zeros_like(s["pos"]), s["z"], np.zeros((3, 3)), s["m"], None)
    md.to_atoms(out, snap)
    assert np.array_equal(bits(out.cell), bits(cell)) and np.array_equal(out.positions, s["pos"])
    md.run(2)
    two = md.to_atoms(out)
    assert two.step == 2 and np.array_equal(bits(out.cell), bits(two.cell[0])) and not np.array_equal(out.cell, cell)
    assert np.array_equal(out.positions, two.positions)
    b = _system("batch")
    z, _, batch = mdt._tensors(b)
    with pytest.raises(RuntimeError, match="periodic"):
        DeviceNPT(mdt._shared_model(), z, None, b["pos"], b["m"], DT, compressibility=1.0, batch=batch, num_graphs=3)
