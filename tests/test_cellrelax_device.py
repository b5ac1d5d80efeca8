"""GPU: `hermnet_amd.relax.DeviceCellRelax` -- FIRE on atoms and cell inside the replayed hipGraph -- against the host-driven
loop it replaces (tests/cellrelax_reference.NumpyCellRelax around a plain `GraphedMDStep(stress=True, variable_cell=True)` /
`GraphedBatchMDStep(stress=True)` that is fed the float32 roundings of coordinates and cell), bit for bit; the device kernels
against the library's host twins; per-graph convergence; halt under a shrinking cell and resume; a mask of zeros against
`DeviceRelax`; the ASE hand-off.

The model and the systems are tests/test_relax_device.py's (3 layers, width 128; the 144-atom cell; the batch of 32, 48 and
144 atoms), every cell strained by about 2 % (atoms with it) so that the cell's forces are not negligible."""
import numpy as np
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import _lib
from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep
from hermnet_amd.md import HALT_CAPACITY
from hermnet_amd.relax import DeviceCellRelax, DeviceRelax
from cellrelax_reference import HostCellRelax, NumpyCellRelax, bits
from npt_reference import det3
import test_relax_device as rdt

pytestmark = pytest.mark.gpu

STEPS = 20
STRAIN = np.array([[0.02, 0.006, 0.0], [0.0, -0.018, 0.004], [0.005, 0.0, 0.021]])
_CACHE = {}


def _system(name):
    """test_relax_device's system, its cells deformed by I + STRAIN (graph g of the batch: by I + (1 - 0.3 g) STRAIN)."""
    if name not in _CACHE:
        s = dict(rdt._system(name))
        B = s["B"]
        cell = np.asarray(s["cell"], dtype=np.float64).reshape(B, 3, 3).copy()
        pos = np.asarray(s["pos"], dtype=np.float64).copy()
        b = np.zeros(len(pos), dtype=np.int64) if s["batch"] is None else s["batch"]
        for g in range(B):
            d = np.eye(3) + (1.0 - 0.3 * g) * STRAIN
            cell[g], pos[b == g] = cell[g] @ d, pos[b == g] @ d
        s["cell"], s["pos"] = (cell[0] if s["batch"] is None else cell), pos
        _CACHE[name] = s
    return _CACHE[name]


def _device(s, cls=DeviceCellRelax, cell=None, **kw):
    z, _, batch = rdt._tensors(s)
    if batch is not None:
        kw.update(batch=batch, num_graphs=s["B"])
    return cls(rdt._shared_model(), z, s["cell"] if cell is None else cell, s["pos"], **kw)      # (the cell in float64)


def _reference(name, fmax, steps=STEPS, **options):
    """The host-driven cell relaxation DeviceCellRelax replaces, computed once per (system, fmax, options): NumpyCellRelax,
    each evaluation's forces and virial from a plain graphed step on float32(x) in float32(C), fetched in one packed copy.
    (system, the NumpyCellRelax at the end, a list of per-evaluation records)."""
    key = (name, float(np.max(fmax)), steps, tuple(sorted(options.items())))
    if key in _CACHE:
        return _CACHE[key]
    s = _system(name)
    dev, B = rdt._dev(), s["B"]
    z, _, batch = rdt._tensors(s)
    cell32 = torch.from_numpy(np.asarray(s["cell"]).astype(np.float32)).to(dev)
    p0 = torch.from_numpy(s["pos"].astype(np.float32)).to(dev)
    if batch is None:
        step = GraphedMDStep(rdt._shared_model(), z, cell32, p0, stress=True, variable_cell=True)
    else:
        step = GraphedBatchMDStep(rdt._shared_model(), z, cell32, p0, batch, B, stress=True)
    ref = NumpyCellRelax(s["pos"], s["cell"], batch=s["batch"], num_graphs=B, fmax=fmax, **options)
    hist = []
    for _ in range(steps):
        p32, c32 = ref.advance()
        step(torch.from_numpy(p32).to(dev), torch.from_numpy(c32.reshape((3, 3) if batch is None else (B, 3, 3))).to(dev))
        e, f, ok, n, w = step.fetch()
        assert ok
        before = ref.step
        ref.finish(f, w, energy=e, total=(n, 0))
        hist.append(dict(x=ref.x.copy(), v=ref.v.copy(), image=ref.image.copy(), f=ref.f.copy(), e=ref.energy.copy(), n=n,
                         cell=ref.cell64.copy(), deform=ref.deform.copy(), rows_v=ref.rows_v.copy(), stress=ref.obs[:, 2:].copy(),
                         w=w.copy(), dt=ref.dt.copy(), a=ref.a.copy(), scale=ref.scale.copy(), nsteps=ref.nsteps.copy(),
                         fnorm=ref.fnorm.copy(), converged=ref.converged.copy(), conv_step=ref.conv_step.copy(), step=ref.step,
                         done=ref.done, counted=ref.step > before))
    _CACHE[key] = (s, ref, hist)
    return _CACHE[key]


def _equals(snap, rec):
    B = len(rec["dt"])
    assert np.array_equal(bits(snap.positions), bits(rec["x"])) and np.array_equal(bits(snap.velocities), bits(rec["v"]))
    assert np.array_equal(snap.images, rec["image"]) and np.array_equal(snap.forces, rec["f"])
    assert np.array_equal(bits(snap.cell.reshape(B, 9)), bits(rec["cell"]))
    assert np.array_equal(bits(snap.deform_grad.reshape(B, 9)), bits(rec["deform"]))
    assert np.array_equal(bits(snap.cell_velocity.reshape(B, 9)), bits(rec["rows_v"]))
    assert np.array_equal(bits(snap.stress.reshape(B, 9)), bits(rec["stress"]))
    assert np.array_equal(bits(snap.volume), bits(np.abs([det3(c) for c in rec["cell"]])))
    for name in ("dt", "a", "scale"):
        assert np.array_equal(bits(getattr(snap, name)), bits(rec[name])), name
    assert np.array_equal(bits(snap.fmax), bits(rec["fnorm"])) and np.array_equal(snap.nsteps, rec["nsteps"])
    assert np.array_equal(bits(snap.energy), bits(rec["e"]))
    assert np.array_equal(snap.converged, rec["converged"] != 0) and np.array_equal(snap.converged_step, rec["conv_step"])
    assert snap.step == rec["step"] and snap.done == bool(rec["done"])
    return True


def _log_equals(log, ref_log, hist):
    assert log.shape[0] == len(ref_log)
    for row, want in zip(log, ref_log):
        assert np.array_equal(bits(row), bits(want))
    for row, rec in zip(log, hist):
        assert np.all(row[:, 3] == rec["n"])


def _state_bits(snap):
    return (bits(snap.positions).tobytes(), bits(snap.velocities).tobytes(), snap.images.tobytes(), snap.forces.tobytes(),
            bits(snap.cell).tobytes(), bits(snap.deform_grad).tobytes(), bits(snap.cell_velocity).tobytes(),
            bits(snap.stress).tobytes(), bits(snap.dt).tobytes(), bits(snap.a).tobytes(), bits(snap.scale).tobytes(),
            bits(snap.fmax).tobytes(), bits(snap.energy).tobytes(), snap.nsteps.tobytes(), snap.converged.tobytes(),
            snap.converged_step.tobytes(), snap.step, snap.done)


def test_device_kernels_equal_the_host_twins():
    """One advance + finish with the same inputs through hermnet_cellrelax_advance / _finish and their host twins, on random
    f, v, rows, rows' velocities, virial and per-graph state (a graph that had converged before, a downhill one past Nmin, an
    uphill one, an unclamped one, an empty fresh one, one that converges now), one fixed atom, a mask, constant volume and
    pressures: everything bit-equal -- the per-graph scalars, cell32 and the inverse of F included."""
    dev, lib, P = rdt._dev(), _lib.load(), _lib.ptr
    sizes = [1, 255, 257, 600, 0, 40]
    n, B = sum(sizes), len(sizes)
    rs = np.random.RandomState(3)
    tri = np.array([[19.3, 0.4, -0.7], [2.1, 21.2, 0.3], [-1.6, 3.3, 24.9]])
    cell = np.stack([tri * s for s in (1.0, 1.1, 0.9, 1.2, 1.0, 1.05)])
    batch = np.repeat(np.arange(B), sizes)
    x = np.einsum("nk,nkj->nj", rs.uniform(-2.5, 3.5, (n, 3)), cell[batch])          # some atoms cells away: wrap and image
    fixed = np.zeros(n, dtype=bool)
    fixed[300] = True
    fmax = np.array([0.05, 0.05, 0.05, 0.05, 0.05, 10.0])
    host = HostCellRelax(x, cell, batch=batch, num_graphs=B, fixed=fixed, fmax=fmax, log_steps=4, constant_volume=True,
                         mask=[[1.0, 0.5, 1.0], [1.0, 1.0, 0.0], [1.0, 1.0, 2.0]], scalar_pressure=rs.uniform(-0.01, 0.03, B),
                         cell_factor=[1.0, 255.0, 100.0, 600.0, 2.0, 40.0])
    ptr = host.graph_ptr
    host.rows[1:] = host.cf[1:, None] * (np.eye(3).reshape(9) + rs.normal(scale=0.02, size=(B - 1, 9)))
    host.rows_v[1:] = rs.normal(scale=0.3, size=(B - 1, 9))
    host.v[:] = rs.normal(scale=0.3, size=(n, 3))
    host.v[fixed] = 0.0
    f_new = rs.normal(size=(n, 3)).astype(np.float32)
    w_new = rs.normal(scale=20.0, size=(B, 9)).astype(np.float32)
    w_new[5] *= 0.01                                                                             # graph 5: a small cell force
    host.v[ptr[2]:ptr[3]] = -np.abs(host.v[ptr[2]:ptr[3]]) * np.sign(f_new[ptr[2]:ptr[3]])       # graph 2: uphill
    host.v[ptr[1]:ptr[2]] = np.abs(host.v[ptr[1]:ptr[2]]) * np.sign(f_new[ptr[1]:ptr[2]])        # graph 1: downhill
    host.v[ptr[3]:ptr[4]] = 0.001 * f_new[ptr[3]:ptr[4]]                                        # graph 3: downhill, small
    f_new[ptr[3]:ptr[4]] *= 0.03                                                                 # ... and not clamped
    w_new[3] *= 0.03
    host.rows_v[3] *= 1e-4
    host.gf[:, 0] = [0.1, 0.37, 0.8, 0.21, 0.1, 0.1]
    host.gf[:, 1] = [0.1, 0.083, 0.1 * 0.99 ** 3, 0.1, 0.1, 0.1]
    host.gf[:, 2] = [0.0, 0.013, 0.004, 0.21, 0.0, 0.05]
    host.gi[:, 0] = [0, 9, 4, 2, 0, 3]
    host.gi[:, 1] = [0, 0, 0, 0, 1, 0]
    host.gi[0, 2:] = [1, 2]                                                          # graph 0 converged at evaluation 2
    host.v[ptr[0]:ptr[1]] = 0.0
    host.gf_new[:], host.gi_new[:] = host.gf, host.gi
    host.state[0] = 6                                                                # (log slot 2)
    energy = rs.normal(size=B).astype(np.float32)
    total = np.array([4321, 0], dtype=np.int64)
    names = ["q", "q0", "x", "x0", "v", "image", "image0", "f_prev", "batch", "cell0", "inv0", "cf", "p", "rows", "rows0", "rows_v",
             "deform", "deform_inv", "det_f", "cell64", "cell32", "obs", "pos32", "state", "gf", "gi", "gf_new", "gi_new", "log",
             "graph_ptr", "fmax", "fixed"]
    d = {k: torch.from_numpy(getattr(host, k).copy()).to(dev) for k in names}
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.hermnet_cellrelax_advance(n, B, host.flags, P(d["q"]), P(d["q0"]), P(d["x"]), P(d["x0"]), P(d["v"]), P(d["image"]),
                                             P(d["image0"]), P(d["fixed"]), P(d["batch"]), P(d["cell0"]), P(d["inv0"]), P(d["cf"]),
                                             P(d["rows"]), P(d["rows0"]), P(d["rows_v"]), P(d["deform"]), P(d["deform_inv"]),
                                             P(d["det_f"]), P(d["cell64"]), P(d["cell32"]), P(d["pos32"]), P(d["state"]),
                                             P(d["gf"]), P(d["gi"]), stream), "advance")
    before = {k: getattr(host, k).copy() for k in ("x", "cell32", "rows")}
    host.advance()
    for k in ("q", "q0", "x", "x0", "rows", "rows0", "deform", "deform_inv", "det_f", "cell64"):
        assert np.array_equal(bits(d[k].cpu().numpy()), bits(getattr(host, k))), k
    for k in ("image", "image0", "pos32", "cell32"):
        assert np.array_equal(d[k].cpu().numpy(), getattr(host, k)), k
    assert np.abs(host.image).max() >= 2 and not np.array_equal(host.cell32[1:], before["cell32"][1:])
    assert np.array_equal(bits(host.q[300]), bits(x[300])) and not np.array_equal(host.x[300], x[300])   # held: rides the cell
    assert np.array_equal(host.cell32[0], before["cell32"][0]) and np.array_equal(bits(host.x[0]), bits(before["x"][0]))
    f_d, e_d, w_d, t_d = (torch.from_numpy(a).to(dev) for a in (f_new, energy, w_new, total))
    _lib.check(lib.hermnet_cellrelax_finish(n, B, host.cell_flags, P(d["graph_ptr"]), P(f_d), P(e_d), P(w_d), P(t_d), 5000, host.dt,
                                            host.dtmax, host.maxstep, float(fmax[0]), P(d["fmax"]), P(d["p"]), host.mask.ctypes.data,
                                            P(d["cell0"]), P(d["inv0"]), P(d["cf"]), P(d["q"]), P(d["q0"]), P(d["x"]), P(d["x0"]),
                                            P(d["v"]), P(d["image"]), P(d["image0"]), P(d["f_prev"]), P(d["fixed"]), P(d["pos32"]),
                                            P(d["rows"]), P(d["rows0"]), P(d["rows_v"]), P(d["deform"]), P(d["deform_inv"]),
                                            P(d["det_f"]), P(d["cell64"]), P(d["cell32"]), P(d["obs"]), P(d["gf"]), P(d["gi"]),
                                            P(d["gf_new"]), P(d["gi_new"]), P(d["log"]), 4, P(d["state"]), stream), "finish")
    torch.cuda.synchronize()
    host.finish(f_new, w_new, energy=energy, total=total, capacity=5000)
    got = {k: d[k].cpu().numpy() for k in names}
    assert got["state"].tolist() == host.state.tolist() == [7, 0, 0, 0]
    for k in ("q", "x", "v", "gf", "log", "rows", "rows_v", "obs", "deform", "deform_inv", "cell64"):
        assert np.array_equal(bits(got[k]), bits(getattr(host, k))), k
    for k in ("image", "f_prev", "gi", "pos32", "cell32"):
        assert np.array_equal(got[k], getattr(host, k)), k
    # the inputs did reach every branch: frozen, growth + clamp, uphill reset, unclamped, fresh, converged on fmax
    gf, gi = host.gf, host.gi
    assert gi[0].tolist() == [0, 0, 1, 2] and not host.obs[0].any()
    assert gi[1, 0] == 10 and gf[1, 0] == min(0.37 * 1.1, 1.0) and gf[1, 2] < gf[1, 0]          # grown, then clamped
    assert gi[2, 0] == 0 and gf[2, 0] == 0.4 and gf[2, 1] == 0.1
    assert gi[3, 0] == 3 and gf[3, 2] == gf[3, 0] == 0.21                                        # no clamp
    assert gi[4].tolist() == [0, 0, 0, -1] and gf[4, 0] == 0.1                                   # the empty graph: fresh, its cell moves
    assert gi[5, 2:].tolist() == [1, 6] and not host.v[ptr[5]:ptr[6]].any() and not host.rows_v[5].any()
    assert np.all(got["log"][[0, 1, 3]] == -7.0) and np.all(got["log"][2][:, 3] == 4321)
    assert not host.v[300].any()


@pytest.mark.parametrize("name", ["single", "batch"])
def test_trajectory_equals_the_host_driven_loop_bit_for_bit(name):
    """20 replays against NumpyCellRelax around a plain graphed step: positions, cell, F, velocities of atoms and cell rows,
    images, forces, stress, the per-graph state, every log row; the volume moved and the largest generalised force fell."""
    s, ref, hist = _reference(name, 1e-6)
    rx = _device(s, fmax=1e-6)
    rx.run(STEPS)
    snap = rx.fetch()
    assert (snap.step, snap.halted, snap.halt_code, snap.halt_step, snap.done) == (STEPS, False, 0, None, False)
    assert _equals(snap, hist[-1])
    _log_equals(snap.log, ref.log, hist)
    assert snap.log.shape == (STEPS, s["B"], 6)
    for g in range(s["B"]):
        assert snap.log[-1, g, 1] < snap.log[0, g, 1]                  # FIRE did something
        assert abs(snap.log[-1, g, 4] / snap.log[0, g, 4] - 1.0) > 1e-4   # ... to the cell too
    assert rx.fetch().log.shape[0] == 0


def test_per_graph_convergence_on_the_device():
    """A threshold that every graph reaches by evaluation 15 (taken from a free reference run, as in test_relax_device: the
    smallest largest-generalised-force each graph shows there -- cell rows included, so neither `hydrostatic_strain` nor a
    smaller strain is needed), at different evaluations: converged_step, done and the final step equal the reference's, the
    frozen graphs keep positions and cell, replays after `done` change and log nothing, `run_until` stops there, and an eager
    `energy_forces_stress` at the fetched float32 positions and cells reproduces every graph's accepted forces and stress bit
    for bit."""
    s, _, free = _reference("batch", 1e-6)
    assert not free[-1]["converged"].any()
    fnorm = np.array([rec["fnorm"] for rec in free])
    T = fnorm[1:16].min(axis=0).max() * (1.0 + 1e-6)
    s, ref, hist = _reference("batch", T)
    conv = ref.conv_step
    assert ref.done and np.all(conv >= 0) and conv.max() <= 15
    assert len(set(conv.tolist())) > 1, "all graphs converge at the same evaluation: change the strains"
    last, first = int(conv.max()), int(conv.min())
    rx = _device(s, fmax=T)
    ptr = np.searchsorted(s["batch"], np.arange(s["B"] + 1))
    rx.run(first + 1)
    early = rx.fetch()
    assert _equals(early, hist[first]) and not early.done and early.converged.sum() >= 1
    rx.run(STEPS - first - 1)
    snap = rx.fetch()
    assert _equals(snap, hist[-1])
    assert snap.done and snap.step == last + 1 and np.array_equal(snap.converged_step, conv)
    assert early.log.shape[0] + snap.log.shape[0] == last + 1          # no rows behind `done`
    _log_equals(np.concatenate([early.log, snap.log]), ref.log, hist)
    for g in np.flatnonzero(early.converged):                          # frozen since then, the cell too
        a, b = ptr[g], ptr[g + 1]
        assert np.array_equal(bits(snap.positions[a:b]), bits(early.positions[a:b]))
        assert np.array_equal(bits(snap.cell[g]), bits(early.cell[g]))
        assert np.array_equal(bits(snap.cell[g].reshape(9)), bits(hist[conv[g]]["cell"][g]))
    cell32_end = rx.step.cell.cpu().numpy().copy()
    rx.run(5)
    again = rx.fetch()
    assert _state_bits(again) == _state_bits(snap) and again.log.shape[0] == 0
    assert np.array_equal(rx.step.cell.cpu().numpy(), cell32_end)
    assert np.array_equal(cell32_end.reshape(-1, 9), snap.cell.reshape(-1, 9).astype(np.float32))
    rx2 = _device(s, fmax=T)
    end = rx2.run_until(100, chunk=8)
    assert end.done and _state_bits(end) == _state_bits(snap)
    # the eager evaluation of the relaxed batch
    dev = rdt._dev()
    z, _, batch = rdt._tensors(s)
    p = torch.from_numpy(snap.positions.astype(np.float32)).to(dev)
    c = torch.from_numpy(cell32_end.reshape(-1, 3, 3)).to(dev)
    ei, sh = hn.neighbor_search(p, 5.0, c, batch=batch, num_graphs=s["B"])
    data = hn.Data(pos=p, atomic_number=z, batch=batch, cell=c, edge_index=ei, edge_shift=sh)
    out = hn.energy_forces_stress(rdt._shared_model(), data)
    assert np.array_equal(out["forces"].cpu().numpy(), snap.forces)
    w = out["virial"].cpu().numpy().astype(np.float64).reshape(-1, 3, 3)
    for g in range(s["B"]):
        assert np.array_equal(bits(-(0.5 * (w[g] + w[g].T)) / snap.volume[g]), bits(snap.stress[g])), g


def test_halt_on_list_overflow_under_a_shrinking_cell_and_resume():
    """Under an external pressure the cell shrinks and the list grows: with a capacity that the list outgrows at evaluation k
    the run halts there with the capacity bit, in the state of the last completed evaluation -- the cell taken back with the
    atoms --, with exactly k log rows; resume() recaptures with more columns and the run ends bit-equal to the uninterrupted
    reference."""
    start = _reference("single", 1e-6)[1].log[0][0, 5]              # tr W / 3V of the start configuration
    p = float(start) + 0.08                                          # 0.08 eV/A^3 (13 GPa) above it: the cell shrinks
    s, ref, hist = _reference("single", 1e-6, scalar_pressure=p)
    counts = [rec["n"] for rec in hist]
    assert hist[-1]["cell"][0, 0] < hist[0]["cell"][0, 0]
    at = [k for k in range(2, STEPS) if counts[k] > max(counts[:k])]
    assert at, "the edge count never exceeded its running maximum: no overflow to test"
    k = at[0]
    capacity = max(counts[:k])
    rx = _device(s, fmax=1e-6, capacity=capacity, scalar_pressure=p)
    assert rx.capacity == capacity
    rx.run(STEPS)
    snap = rx.fetch()
    assert snap.halted and snap.step == k and snap.halt_step == k and (snap.halt_code & HALT_CAPACITY)
    assert _equals(snap, hist[k - 1])
    _log_equals(snap.log, ref.log[:k], hist[:k])
    assert np.array_equal(rx.step.cell.cpu().numpy().reshape(1, 9), hist[k - 1]["cell"].astype(np.float32))
    assert np.array_equal(rx.step.pos.detach().cpu().numpy(), hist[k - 1]["x"].astype(np.float32))
    rx.run(3)                                            # halted: replays change nothing
    again = rx.fetch()
    assert _state_bits(again) == _state_bits(snap) and again.log.shape[0] == 0 and again.halted
    rx.resume()
    assert rx.capacity > capacity
    rx.run(STEPS - k)
    end = rx.fetch()
    assert (end.step, end.halted) == (STEPS, False)
    assert _equals(end, hist[-1])
    _log_equals(end.log, ref.log[k:], hist[k:])


@pytest.mark.parametrize("name", ["single", "batch"])
def test_a_mask_of_zeros_is_device_relax(name):
    """With every entry of the mask zero the cell never moves (F = I exactly): positions, velocities, images, forces and the
    FIRE state equal `DeviceRelax`'s bit for bit over 20 replays (the cells given are float32 values, so both wrap with the
    same lattice vectors)."""
    s = _system(name)
    cell32 = np.asarray(s["cell"]).astype(np.float32)
    rx = _device(s, cell=cell32.astype(np.float64), fmax=1e-6, mask=np.zeros((3, 3)))
    plain = _device(s, cls=DeviceRelax, cell=torch.from_numpy(cell32).to(rdt._dev()), fmax=1e-6)
    rx.run(STEPS)
    plain.run(STEPS)
    a, b = rx.fetch(), plain.fetch()
    assert a.step == b.step == STEPS and not a.halted and not b.halted
    assert np.array_equal(bits(a.positions), bits(b.positions)) and np.array_equal(bits(a.velocities), bits(b.velocities))
    assert np.array_equal(a.images, b.images) and np.array_equal(a.forces, b.forces)
    for k in ("dt", "a", "scale", "fmax", "energy"):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert np.array_equal(a.nsteps, b.nsteps) and np.array_equal(bits(a.log[:, :, :4]), bits(b.log))
    assert np.array_equal(a.deform_grad, np.tile(np.eye(3), (s["B"], 1, 1))) and not a.cell_velocity.any()
    assert np.array_equal(bits(a.cell), bits(cell32.astype(np.float64).reshape(-1, 3, 3)))


class _FakeAtoms(rdt._FakeAtoms):
    def set_cell(self, cell, scale_atoms=False):
        assert not scale_atoms
        self.cell = np.array(cell)
        self.cell_set_before_positions = self.positions.copy()


def test_ase_hand_off():
    """from_atoms takes one duck-typed structure or a list, the cell in float64; to_atoms writes each member's cell (first,
    without moving atoms) and positions; the cell round-trips bit for bit; open structures are refused with a message."""
    s, _, hist = _reference("batch", 1e-6)
    ptr = np.searchsorted(s["batch"], np.arange(4))
    odd = s["cell"] * (1.0 + 2.0 ** -40)                               # not float32 values: float64 must survive
    atoms = [_FakeAtoms(s["pos"][a:b], s["z"][a:b], odd[g]) for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:]))]
    rx = DeviceCellRelax.from_atoms(atoms, rdt._shared_model(), fmax=1e-6)
    assert rx.num_graphs == 3 and rx.n == len(s["z"])
    start = rx.to_atoms(atoms)
    assert start.step == 0 and np.array_equal(bits(start.cell), bits(odd))
    for g, m in enumerate(atoms):
        assert np.array_equal(bits(m.cell), bits(odd[g]))
    rx.run(3)
    snap = rx.to_atoms(atoms)
    assert snap.step == 3
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        assert np.array_equal(atoms[g].positions, snap.positions[a:b]) and np.array_equal(atoms[g].cell, snap.cell[g])
        assert not np.array_equal(atoms[g].cell, odd[g])
        assert np.array_equal(atoms[g].cell_set_before_positions, s["pos"][a:b])       # the cell went in first
    with pytest.raises(ValueError, match="do not match"):
        rx.to_atoms(atoms[:2], snap)
    exact = [_FakeAtoms(s["pos"][a:b], s["z"][a:b], s["cell"][g]) for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:]))]
    same = DeviceCellRelax.from_atoms(exact, rdt._shared_model(), fmax=1e-6)
    same.run(3)
    assert _equals(same.fetch(), hist[2])
    opened = atoms[:2] + [_FakeAtoms(s["pos"][:4], s["z"][:4], s["cell"][0], pbc=False)]
    with pytest.raises(RuntimeError, match="no cell to relax"):
        DeviceCellRelax.from_atoms(opened, rdt._shared_model())
    with pytest.raises(RuntimeError, match="no cell to relax"):
        DeviceCellRelax(rdt._shared_model(), torch.from_numpy(s["z"]).to(rdt._dev()), None, s["pos"],
                        batch=torch.from_numpy(s["batch"]).to(rdt._dev()), num_graphs=3)
    one = DeviceCellRelax.from_atoms(exact[2], rdt._shared_model(), fmax=1e-6)
    assert one.num_graphs == 1 and one.batch is None and one.n == 144
    one.run(2)
    lone = _FakeAtoms(s["pos"][ptr[2]:], s["z"][ptr[2]:], s["cell"][2])
    got = one.to_atoms(lone)
    assert np.array_equal(lone.cell, got.cell[0]) and np.array_equal(lone.positions, got.positions)


def _many_on_the_device(host):
    """Device copies of a HostCellRelax's arrays and (advance, finish) closures over hermnet_cellrelax_advance / _finish."""
    dev, lib, P = rdt._dev(), _lib.load(), _lib.ptr
    names = ["q", "q0", "x", "x0", "v", "image", "image0", "f_prev", "batch", "cell0", "inv0", "cf", "p", "rows", "rows0", "rows_v",
             "deform", "deform_inv", "det_f", "cell64", "cell32", "obs", "pos32", "state", "gf", "gi", "gf_new", "gi_new", "log",
             "graph_ptr", "fmax"]
    d = {k: torch.from_numpy(getattr(host, k).copy()).to(dev) for k in names}
    stream = torch.cuda.current_stream().cuda_stream
    n, B = host.n, host.B

    def advance():
        _lib.check(lib.hermnet_cellrelax_advance(n, B, host.flags, P(d["q"]), P(d["q0"]), P(d["x"]), P(d["x0"]), P(d["v"]),
                                                 P(d["image"]), P(d["image0"]), None, P(d["batch"]), P(d["cell0"]), P(d["inv0"]),
                                                 P(d["cf"]), P(d["rows"]), P(d["rows0"]), P(d["rows_v"]), P(d["deform"]),
                                                 P(d["deform_inv"]), P(d["det_f"]), P(d["cell64"]), P(d["cell32"]), P(d["pos32"]),
                                                 P(d["state"]), P(d["gf"]), P(d["gi"]), stream), "advance")

    def finish(f, w, e, tot):
        f_d, e_d, w_d, t_d = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (f, e, w.reshape(B, 9), tot))
        _lib.check(lib.hermnet_cellrelax_finish(n, B, host.cell_flags, P(d["graph_ptr"]), P(f_d), P(e_d), P(w_d), P(t_d), 5000,
                                                host.dt, host.dtmax, host.maxstep, float(host.fmax[0]), P(d["fmax"]), P(d["p"]),
                                                host.mask.ctypes.data, P(d["cell0"]), P(d["inv0"]), P(d["cf"]), P(d["q"]),
                                                P(d["q0"]), P(d["x"]), P(d["x0"]), P(d["v"]), P(d["image"]), P(d["image0"]),
                                                P(d["f_prev"]), None, P(d["pos32"]), P(d["rows"]), P(d["rows0"]), P(d["rows_v"]),
                                                P(d["deform"]), P(d["deform_inv"]), P(d["det_f"]), P(d["cell64"]), P(d["cell32"]),
                                                P(d["obs"]), P(d["gf"]), P(d["gi"]), P(d["gf_new"]), P(d["gi_new"]), P(d["log"]),
                                                host.log_steps, P(d["state"]), stream), "finish")
        torch.cuda.synchronize()

    return d, advance, finish


_MANY_F64 = ("q", "q0", "x", "x0", "v", "rows", "rows0", "rows_v", "deform", "deform_inv", "det_f", "cell64", "obs", "gf",
             "gf_new", "log")
_MANY_EXACT = ("image", "image0", "f_prev", "gi", "gi_new", "pos32", "cell32", "state")


def _many_equal(d, host):
    for key in _MANY_F64:
        assert np.array_equal(bits(d[key].cpu().numpy()), bits(getattr(host, key))), key
    for key in _MANY_EXACT:
        assert np.array_equal(d[key].cpu().numpy(), getattr(host, key)), key


def test_more_graphs_than_lanes():
    """tests/test_cellrelax_host.py's B = 257 (graph 256 moving beside 256 converged graphs, graph 3 empty), kernel-direct: two
    advance + finish through hermnet_cellrelax_advance / _finish against their host twins, bit for bit -- graph 256 (the second
    block of the advance's lane-per-graph kernel) is moved, committed and counted in `all` (done stays 0), and done is 1 once
    the second evaluation puts it under fmax."""
    import test_cellrelax_host as cht
    host, _, first, second = cht.many_graphs()
    d, advance, finish = _many_on_the_device(host)
    start = {k: getattr(host, k).copy() for k in ("x", "cell32")}
    for k, (f, w) in enumerate((first, second)):
        e, tot = np.zeros(host.B, dtype=np.float32), np.array([11 + k, 0], dtype=np.int64)
        advance()
        finish(f, w, e, tot)
        host.advance()
        host.finish(f, w, energy=e, total=tot, capacity=5000)
        _many_equal(d, host)
        assert host.state.tolist() == [k + 1, 0, 0, k]
        assert host.gi[256, 1:].tolist() == [[0, 0, -1], [0, 1, 1]][k] and (host.gf[256, 2] > 0.0) == (k == 0)
    x, cell32 = d["x"].cpu().numpy(), d["cell32"].cpu().numpy()
    assert np.array_equal(bits(x[:-2]), bits(start["x"][:-2])) and not np.array_equal(x[-2:], start["x"][-2:])
    assert np.array_equal(cell32[:256], start["cell32"][:256]) and not np.array_equal(cell32[256], start["cell32"][256])
    assert np.all(host.log[2:] == -7.0)


def test_more_graphs_than_lanes_void_on_the_last_virial():
    """The virial of graph 256 alone is NaN (an input the kernels answer with a halt code): code 256, graph 256's atoms and
    cell back to the start of the step, graphs 0..255 untouched, no log row -- every array bit-equal to the host twins'."""
    import test_cellrelax_host as cht
    host, _, (f, w), _ = cht.many_graphs()
    d, advance, finish = _many_on_the_device(host)
    names = ("q", "x", "image", "pos32", "rows", "deform", "cell64", "cell32", "gf", "gi", "log")
    keep = {k: getattr(host, k).copy() for k in names}
    w = w.copy()
    w[256, 1, 2] = np.nan
    e, tot = np.zeros(host.B, dtype=np.float32), np.array([11, 0], dtype=np.int64)
    advance()
    moved = d["cell32"].cpu().numpy()
    assert not np.array_equal(moved[256], keep["cell32"][256]) and np.array_equal(moved[:256], keep["cell32"][:256])
    finish(f, w, e, tot)
    host.advance()
    host.finish(f, w, energy=e, total=tot, capacity=5000)
    _many_equal(d, host)
    assert d["state"].cpu().numpy().tolist() == [0, 256, 0, 0]
    for key, want in keep.items():
        assert np.array_equal(d[key].cpu().numpy().view(np.uint8), want.view(np.uint8)), key
