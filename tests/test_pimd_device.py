"""GPU: `hermnet_amd.pimd.DevicePIMD` -- ring-polymer path-integral MD inside the replayed hipGraph.  The kernels against the
library's host twins; an RPMD trajectory against the host-driven loop it replaces, bit for bit after every step; one bead
against `DeviceMD`; determinism, halt and resume; the estimators; the refusals, the ASE hand-off and the launch list."""
import warnings
from collections import Counter

import numpy as np
import pytest
import torch

from hermnet_amd import _lib, synth
from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.md import ASE_TIME_FS, HALT_CAPACITY, HALT_NONFINITE, DeviceMD
from hermnet_amd.pimd import DevicePIMD
from md_reference import AMU, KB, bits, host_noise
from pimd_reference import HostPIMD
from resident_helpers import _FakeAtoms, _model, _shared_model

pytestmark = pytest.mark.gpu

MASS = {13: 26.9815, 28: 58.6934, 29: 63.546}
TRICLINIC = np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]])
CASES = [(1, 5), (2, 3), (3, 1), (4, 257), (6, 63), (32, 9), (128, 2)]
DT, T, TAU0, SEED, BEADS = 1.0, 600.0, 50.0, (5 << 32) + 77, 4      # 4 beads at 2400 K: the neighbour list changes
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


# ---- 1. the kernels against the host twins ----------------------------------------------------------------------------------------
NAMES = ["x", "v", "x0", "v0", "image", "image0", "f_prev", "kick", "cmat", "cs", "sw", "ws", "c1", "sigma", "cell", "inv", "pos32",
         "centroid", "state", "graph_ptr", "half_mass", "ke_atom", "spring_c", "log"]


def _host_ring(P, n_rep, thermostat):
    """A synthetic ring in a triclinic cell: an atom of infinite mass where there are two or more, atom 0's centroid about to
    cross the face s_0 = 1 with beads on both sides of it, step 6 (log slot 2)."""
    rs = np.random.RandomState(100 * P + n_rep)
    cell = TRICLINIC.astype(np.float32).astype(np.float64)
    base = rs.uniform(0.05, 0.95, (n_rep, 3)) @ cell
    base[0] = np.array([0.9995, 0.4, 0.6]) @ cell
    x = base[None] + rs.normal(scale=0.05, size=(P, n_rep, 3))
    x[:, 0] -= x[:, 0].mean(axis=0) - base[0]              # (atom 0's centroid exactly there, whatever P)
    v = rs.normal(scale=0.02, size=(P, n_rep, 3))
    v[:, 0] = [0.05, 0.0, 0.0]
    m_rep = rs.uniform(1.0, 40.0, n_rep)
    if n_rep > 1:
        m_rep[1], v[:, 1] = np.inf, 0.0
    host = HostPIMD(P, x.reshape(-1, 3), v.reshape(-1, 3), np.tile(m_rep, P), 0.5, 300.0, tau0=40.0, thermostat=thermostat,
                    seed=SEED, log_steps=4, cell=TRICLINIC)
    host.f_prev[:] = rs.normal(scale=0.1, size=(P * n_rep, 3)).astype(np.float32)
    host.state[0] = 6
    return host, rs


def _both(P, n_rep, thermostat, what="step"):
    """One hermnet_pimd_advance + hermnet_pimd_finish and their host twins on the same state, forces and energies.  `what`:
    "step", "void" (more pairs than capacity) or "prime".  (host, the device's arrays behind the advance, behind the finish)."""
    dev, lib, p = _dev(), _lib.load(), _lib.ptr
    host, rs = _host_ring(P, n_rep, thermostat)
    n = P * n_rep
    if what == "prime":
        host.state[3] = 1
    f_new, energy = rs.normal(size=(n, 3)).astype(np.float32), rs.normal(size=P).astype(np.float32)
    total = np.array([5001 if what == "void" else 4321, 0], dtype=np.int64)
    d = {k: torch.from_numpy(np.ascontiguousarray(getattr(host, k)).copy()).to(dev) for k in NAMES}
    stream = torch.cuda.current_stream().cuda_stream
    f_d, e_d, t_d = (torch.from_numpy(a).to(dev) for a in (f_new, energy, total))
    _lib.check(lib.hermnet_pimd_advance(n, P, host.flags, host.seed, host.inv_beads, p(d["x"]), p(d["v"]), p(d["x0"]), p(d["v0"]),
                                        p(d["image"]), p(d["image0"]), p(d["f_prev"]), p(d["kick"]), p(d["cmat"]), p(d["cs"]),
                                        p(d["sw"]), p(d["ws"]), p(d["c1"]), p(d["sigma"]), p(d["cell"]), p(d["inv"]), p(d["pos32"]),
                                        p(d["centroid"]), p(d["state"]), stream), "advance")
    torch.cuda.synchronize()
    mid = {k: d[k].cpu().numpy() for k in NAMES}
    _lib.check(lib.hermnet_pimd_finish(n, P, p(d["graph_ptr"]), p(f_d), p(e_d), p(t_d), 5000, p(d["x"]), p(d["v"]), p(d["x0"]),
                                       p(d["v0"]), p(d["image"]), p(d["image0"]), p(d["f_prev"]), p(d["kick"]), p(d["half_mass"]),
                                       p(d["pos32"]), p(d["ke_atom"]), p(d["spring_c"]), p(d["centroid"]), p(d["log"]), 4,
                                       p(d["state"]), stream), "finish")
    torch.cuda.synchronize()
    end = {k: d[k].cpu().numpy() for k in NAMES}
    host.advance()
    host_mid = host.snapshot()
    host.finish(f_new, energy, total=total, capacity=5000)
    return host, host_mid, mid, end


def _close(a, b, exact):
    if exact:
        return np.array_equal(bits(a), bits(b))
    return np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("thermostat", [False, True], ids=["rpmd", "pile"])
@pytest.mark.parametrize("P,n_rep", CASES)
def test_device_kernels_equal_the_host_twins(P, n_rep, thermostat):
    """Thermostat off: every array bit for bit, behind the advance and behind the finish.  Thermostat on: x, v, the centroid
    and the sums carry this step's Gaussians (the device's float64 log / cos / sqrt differ from the host's in the last
    digits, as in test_md_device.py) and agree within 1e-12 of the state's scale; everything else stays bit-equal.  The state
    has an atom of infinite mass and a centroid that crosses a face with beads on both sides."""
    host, host_mid, mid, end = _both(P, n_rep, thermostat)
    exact = not thermostat
    for k in ("x0", "v0"):
        assert np.array_equal(bits(mid[k]), bits(getattr(host_mid, k))), k
    assert np.array_equal(mid["image0"], host_mid.image0) and np.array_equal(mid["image"], host_mid.image)
    for k in ("x", "v", "centroid"):
        assert _close(mid[k], getattr(host_mid, k), exact), k
    if exact:
        assert np.array_equal(mid["pos32"], host_mid.pos32)
    img = mid["image"].reshape(P, n_rep, 3)
    assert np.all(img == img[0]) and np.all(img[:, 0] == [1, 0, 0])                 # atom 0 crossed, every bead with it
    assert end["state"].tolist() == host.state.tolist() == [7, 0, 0, 0]
    assert np.array_equal(end["image"], host.image) and np.array_equal(end["f_prev"], host.f_prev)
    assert _close(end["x"], host.x, exact) and _close(end["v"], host.v, exact)
    want, have = host.log[2], end["log"][2]
    assert np.array_equal(bits(have[:, [0, 2]]), bits(want[:, [0, 2]])) and np.all(have[:, 2] == 4321)
    if exact:
        assert np.array_equal(bits(have), bits(want))
    else:
        # what 1e-12 of the scale in x and v does to the sums: E_kin (quadratic in v) 1e-11 relative, as test_md_device.py
        # asks; a difference of two coordinates is off by 2e-12 |x|max at most, so spring_j by sum_a spring_c 2 |d| 3 that
        # much and vir_j by sum_a 3 |f|max that much
        dx = 2e-12 * np.abs(host.x).max()
        X = host.x.reshape(P, n_rep, 3)
        d_max = np.abs(X - np.roll(X, -1, axis=0)).max()
        assert np.all(np.abs(have[:, 1] - want[:, 1]) <= 1e-11 * np.abs(want[:, 1]).max())
        assert np.all(np.abs(have[:, 3] - want[:, 3]) <= host.spring_c.sum() * 6.0 * d_max * dx + 1e-15 * np.abs(want[:, 3]).max())
        assert np.all(np.abs(have[:, 4] - want[:, 4]) <= n_rep * 3.0 * np.abs(host.f_prev).max() * dx)
    assert np.all(end["log"][[0, 1, 3]] == -7.0)
    if n_rep > 1:                                                                    # the atom of infinite mass stayed
        assert np.array_equal(end["x"].reshape(P, n_rep, 3)[:, 1], end["x0"].reshape(P, n_rep, 3)[:, 1])
        assert not end["v"].reshape(P, n_rep, 3)[:, 1].any()


@pytest.mark.parametrize("what", ["void", "prime"])
def test_device_void_step_and_prime_equal_the_host_twins(what):
    """More pairs than capacity: x, v and image of every bead are back where the step began, no row, the halt recorded.  A
    prime: nothing moves, f_prev takes the forces, the mode is cleared.  Bit for bit the host twins', thermostat on."""
    P, n_rep = 6, 63
    host, host_mid, mid, end = _both(P, n_rep, True, what)
    start = _host_ring(P, n_rep, True)[0]
    for k in ("x", "v"):
        assert np.array_equal(bits(end[k]), bits(getattr(start, k))) and np.array_equal(bits(end[k]), bits(getattr(host, k))), k
    assert not end["image"].any() and not host.image.any()
    assert np.array_equal(end["pos32"], start.x.astype(np.float32)) and np.array_equal(end["pos32"], host.pos32)
    assert np.all(end["log"] == -7.0) and np.all(host.log == -7.0)
    assert end["state"].tolist() == host.state.tolist() == ([6, 4, 6, 0] if what == "void" else [6, 0, 0, 0])
    if what == "void":
        assert not np.array_equal(mid["x"], start.x)                                # the advance had moved the beads
        assert np.array_equal(end["f_prev"], start.f_prev)
    else:
        assert np.array_equal(bits(mid["x"]), bits(start.x)) and np.array_equal(mid["pos32"], start.x.astype(np.float32))
        assert np.array_equal(end["f_prev"], host.f_prev) and not np.array_equal(end["f_prev"], start.f_prev)


def test_device_noise_words_are_the_hosts():
    dev, lib, p = _dev(), _lib.load(), _lib.ptr
    n = 6 * 63
    words_d = torch.zeros(n, 8, dtype=torch.int32, device=dev)
    _lib.check(lib.hermnet_md_noise(SEED, 6, n, p(words_d), None, torch.cuda.current_stream().cuda_stream), "noise")
    assert np.array_equal(words_d.cpu().numpy().view(np.uint32), host_noise(SEED, 6, n)[0])


# ---- the driver on 4 beads x 32 atoms ---------------------------------------------------------------------------------------------
def _system(beads=BEADS):
    """`beads` copies of one 32-atom alloy cell, spread by 0.02 A around their atom, Maxwell-Boltzmann velocities at P T."""
    key = ("system", beads)
    if key not in _CACHE:
        pos, cell, z = synth.fcc_alloy_atoms(reps=(2, 2, 2))
        rs = np.random.RandomState(3)
        m = np.tile(np.array([MASS[int(v)] for v in z]), beads)
        x = np.tile(pos, (beads, 1)) + rs.normal(scale=0.02, size=(beads * len(z), 3))
        v = rs.normal(size=(len(m), 3)) * np.sqrt(KB * beads * T / (m * AMU))[:, None]
        _CACHE[key] = dict(pos=x, z=np.tile(z, beads), cell=np.tile(cell, (beads, 1, 1)), m=m, v=v,
                           batch=np.repeat(np.arange(beads), len(z)), n_rep=len(z), one_cell=cell)
    return _CACHE[key]


def _args(s):
    dev = _dev()
    return (torch.from_numpy(s["z"]).to(dev), torch.from_numpy(s["cell"].astype(np.float32)).to(dev), s["pos"], s["m"], DT)


def _pimd(system=None, model=None, **kw):
    s = system if system is not None else _system()
    args = dict(tau0=TAU0, seed=SEED, velocities=s["v"], batch=torch.from_numpy(s["batch"]).to(_dev()),
                num_graphs=int(s["batch"][-1]) + 1)
    args.update(kw)
    return DevicePIMD(model if model is not None else _shared_model(), *_args(s), T, **args)


def _state_bits(snap):
    return (bits(snap.positions).tobytes(), bits(snap.velocities).tobytes(), snap.images.tobytes(), snap.forces.tobytes(),
            snap.step)


def test_rpmd_trajectory_equals_the_host_driven_loop_bit_for_bit():
    """20 RPMD steps of 4 beads x 32 atoms against GraphedBatchMDStep + hermnet_host_pimd_advance / _finish: x, v, image and
    forces bit-equal after EVERY step, the log rows too; beads of an atom hold equal images throughout."""
    s, dev = _system(), _dev()
    z, cell, pos, m, dt = _args(s)
    batch = torch.from_numpy(s["batch"]).to(dev)
    step = GraphedBatchMDStep(_shared_model(), z, cell, torch.from_numpy(pos.astype(np.float32)).to(dev), batch, BEADS)

    def forces(p32):
        e, f = step(torch.from_numpy(p32).to(dev))
        e, f = e.cpu().numpy().copy(), f.cpu().numpy().copy()
        ok, n = step.check()
        assert ok
        return e, f, n

    host = HostPIMD(BEADS, pos, s["v"], m, dt, T, thermostat=False, log_steps=32, cell=s["one_cell"])
    _, host.f_prev[:], _ = forces(host.pos32)
    pimd = _pimd(thermostat=False)
    counts = set()
    for k in range(20):
        e, f, n = forces(host.advance().copy())
        host.finish(f, e, total=(n, 0))
        counts.add(n)
        pimd.run(1)
        snap = pimd.fetch()
        assert (snap.step, snap.halted) == (k + 1, False)
        assert np.array_equal(bits(snap.positions), bits(host.x)) and np.array_equal(bits(snap.velocities), bits(host.v)), k
        assert np.array_equal(snap.images, host.image) and np.array_equal(snap.forces, host.f_prev), k
        assert snap.log.shape == (1, BEADS, 5) and np.array_equal(bits(snap.log[0]), bits(host.log[k])), k
        img = snap.images.reshape(BEADS, -1, 3)
        assert np.all(img == img[0])
    assert len(counts) > 3                                            # the list really changed along the run


@pytest.mark.parametrize("thermostat", [False, True], ids=["nve", "langevin"])
def test_one_bead_equals_device_md_bit_for_bit(thermostat):
    """`DevicePIMD` on a single structure (`batch=None`: P = 1) against `DeviceMD` over 20 steps -- NVE with the thermostat
    off, Langevin with friction = 1 / tau0 and the same seed: positions, velocities, images, forces and the log's columns
    0-2 bit-equal; the spring column is 0."""
    pos, cell, z = synth.fcc_alloy_atoms(reps=(3, 3, 4))
    m = np.array([MASS[int(v)] for v in z])
    v = np.random.RandomState(1).normal(size=(len(m), 3)) * np.sqrt(KB * 2500.0 / (m * AMU))[:, None]
    dev = _dev()
    z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
    ring = DevicePIMD(_shared_model(), z_t, cell_t, pos, m, DT, T, tau0=TAU0, thermostat=thermostat, seed=SEED, velocities=v)
    kw = dict(temperature=T, friction=1.0 / TAU0) if thermostat else {}
    md = DeviceMD(_shared_model(), z_t, cell_t, pos, m, DT, seed=SEED, velocities=v, **kw)
    assert ring.beads == 1 and ring.num_graphs == 1
    ring.run(20)
    md.run(20)
    a, b = ring.fetch(), md.fetch()
    assert (a.step, a.halted, b.step, b.halted) == (20, False, 20, False)
    assert _state_bits(a) == _state_bits(b)
    assert a.log.shape == (20, 1, 5) and np.array_equal(bits(a.log[:, :, :3]), bits(b.log)) and not a.log[:, :, 3].any()
    assert len(set(a.log[:, 0, 2])) > 1 and np.abs(a.images).max() >= 0


def test_thermostatted_run_is_a_function_of_the_seed_alone():
    """The same seed twice: bit-equal state and log; run(7) + fetch() + run(13) equals run(20); another seed differs."""
    def go(seed, pieces, fetch_between=False):
        pimd = _pimd(seed=seed)
        logs = []
        for k in pieces:
            pimd.run(k)
            if fetch_between:
                logs.append(pimd.fetch().log)
        snap = pimd.fetch()
        logs.append(snap.log)
        return _state_bits(snap), np.concatenate(logs)

    a, log_a = go(11, [20])
    _CACHE["pile"] = (a, log_a)
    for pieces, between in (([20], False), ([7, 13], True)):
        b, log_b = go(11, pieces, between)
        assert a == b and np.array_equal(bits(log_a), bits(log_b)), (pieces, between)
    assert log_a.shape == (20, BEADS, 5) and np.all(np.isfinite(log_a))
    c, log_c = go(12, [20])
    assert a[:2] != c[:2] and not np.array_equal(log_a[:, :, 1], log_c[:, :, 1])


def test_halt_on_list_overflow_and_resume():
    """A capacity that the list outgrows at step k (found from an uninterrupted run's edge column): the thermostatted run
    halts there with the capacity bit and exactly k rows, in the state of the last completed step; resume() recaptures with
    more columns and the run ends bit-equal to the uninterrupted one (the noise is a function of seed, step and index)."""
    base = _pimd()
    _, n0 = base.step.check()
    base.run(30)
    end = base.fetch()
    log = end.log
    assert end.step == 30 and not end.halted
    counts = log[:, 0, 2].astype(int).tolist()
    at = [k for k in range(2, 30) if counts[k] > max([int(n0)] + counts[:k])]
    assert at, "the edge count never exceeded its running maximum: no overflow to test"
    k = at[0]
    capacity = max([int(n0)] + counts[:k])
    pimd = _pimd(capacity=capacity)
    assert pimd.capacity == capacity
    pimd.run(30)
    snap = pimd.fetch()
    assert snap.halted and snap.step == k and snap.halt_step == k and (snap.halt_code & HALT_CAPACITY)
    assert not (snap.halt_code & HALT_NONFINITE)
    assert snap.log.shape[0] == k and np.array_equal(bits(snap.log), bits(log[:k]))
    pimd.run(3)                                          # halted: replays change nothing
    again = pimd.fetch()
    assert _state_bits(again) == _state_bits(snap) and again.log.shape[0] == 0 and again.halted
    pimd.resume()
    assert pimd.capacity > capacity
    pimd.run(30 - k)
    last = pimd.fetch()
    assert (last.step, last.halted) == (30, False)
    assert _state_bits(last) == _state_bits(end) and np.array_equal(bits(last.log), bits(log[k:]))


def test_halt_on_a_non_finite_energy_and_resume():
    """A weight written through `.data` between two runs: the run halts with the non-finite bit in the state of the last good
    step; fetch drops the caches (with a warning), resume() recaptures and the run continues; no NaN reaches the log."""
    model = _model(seed=9)
    pimd = _pimd(model=model)
    pimd.run(5)
    good = pimd.fetch()
    assert good.step == 5 and not good.halted
    p_ = [p for n, p in model.named_parameters() if n.endswith("update_layer.xvec_proj.2.weight")][1]
    p_.data.mul_(1.5)
    pimd.run(5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        snap = pimd.fetch()
    assert any("resume()" in str(w.message) for w in rec)
    assert snap.halted and snap.halt_code == HALT_NONFINITE and snap.step == snap.halt_step == 5 and snap.log.shape[0] == 0
    assert _state_bits(snap) == _state_bits(good)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pimd.resume()
    pimd.run(5)
    end = pimd.fetch()
    assert (end.step, end.halted) == (10, False) and end.log.shape == (5, BEADS, 5) and np.all(np.isfinite(end.log))
    assert np.all(np.isfinite(end.positions)) and np.all(np.isfinite(end.velocities))


def test_estimators_equal_the_sums_recomputed_from_the_fetched_state():
    """The last logged step's `potential`, `kinetic_primitive`, `kinetic_virial` and `ring_energy` against the same sums made
    on the host from the fetched positions, velocities and forces (float64, math.fsum), within 1e-12 relative; one atom of
    infinite mass is left out of N and of every sum."""
    import math
    s = dict(_system())
    n_rep = s["n_rep"]
    m = s["m"].copy()
    m[5::n_rep] = np.inf
    s["m"] = m
    pimd = _pimd(system=s)
    pimd.run(6)
    snap = pimd.fetch()
    est = pimd.estimators(snap)
    assert snap.step == 6 and est.potential.shape == (6,) and est.centroid.shape == (n_rep, 3)
    X, V, F = (a.reshape(BEADS, n_rep, 3).astype(np.float64) for a in (snap.positions, snap.velocities, snap.forces))
    free = np.isfinite(m[:n_rep])
    mass = m[:n_rep] * AMU
    c = est.centroid
    omega_p = BEADS * KB * T / 0.6582119569
    spring = math.fsum((0.5 * mass[free, None] * omega_p ** 2 * (X[j] - X[(j + 1) % BEADS])[free] ** 2).sum() for j in range(BEADS))
    vir = math.fsum((((X[j] - c) * F[j])[free]).sum() for j in range(BEADS))
    kin = math.fsum((0.5 * mass[free, None] * V[j][free] ** 2).sum() for j in range(BEADS))
    pot = math.fsum(snap.log[-1, :, 0])
    n_free = int(free.sum())
    assert n_free == n_rep - 1 and not V[:, 5].any()
    want = dict(potential=pot / BEADS, kinetic_primitive=1.5 * n_free * BEADS * KB * T - spring / BEADS,
                kinetic_virial=1.5 * n_free * KB * T - vir / (2 * BEADS), ring_energy=kin + spring + pot)
    for name, value in want.items():
        got = getattr(est, name)[-1]
        print("%s: %.15g (log) %.15g (recomputed)" % (name, got, value))
        assert abs(got - value) <= 1e-12 * abs(value), name
    assert spring > 0.0 and abs(vir) > 0.0


# ---- refusals, hand-off, launches -------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    s = _system()
    z, cell, pos, m, dt = _args(s)
    batch = torch.from_numpy(s["batch"]).to(_dev())
    model, n_rep = _shared_model(), s["n_rep"]

    def make(z=z, cell=cell, pos=pos, m=m, temperature=T, batch=batch, num_graphs=BEADS, **kw):
        return DevicePIMD(model, z, cell, pos, m, dt, temperature, batch=batch, num_graphs=num_graphs, **kw)

    with pytest.raises(ValueError, match="atom count"):
        make(z=z[:-1], pos=pos[:-1], m=m[:-1], batch=batch[:-1])
    z2 = z.clone()
    z2[n_rep + 1] = 13 if int(z2[n_rep + 1]) != 13 else 28
    with pytest.raises(ValueError, match="atomic numbers"):
        make(z=z2)
    m2 = m.copy()
    m2[2 * n_rep] *= 1.5
    with pytest.raises(ValueError, match="masses"):
        make(m=m2)
    cell2 = cell.clone()
    cell2[3, 0, 0] += 0.25
    with pytest.raises(ValueError, match="in cell"):
        make(cell=cell2)
    with pytest.raises(ValueError, match="at most 128"):
        make(batch=torch.arange(129, device=_dev()), num_graphs=129, z=z[:1].repeat(129), pos=np.tile(pos[:1], (129, 1)),
             m=np.tile(m[:1], 129), cell=cell[:1].repeat(129, 1, 1))
    for bad in (0.0, -300.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="temperature must be positive and finite"):
            make(temperature=bad)
        with pytest.raises(ValueError, match="tau0 must be positive and finite"):
            make(tau0=bad)
        with pytest.raises(ValueError, match="pile_lambda must be positive and finite"):
            make(pile_lambda=bad)
    with pytest.raises(ValueError, match="tau0=.*pile_lambda="):
        make(friction=0.01)
    with pytest.raises(ValueError, match="one number"):
        make(temperature=[300.0, 310.0, 320.0, 330.0])


def test_ase_hand_off():
    """`from_atoms` replicates one structure into `beads` graphs, or takes the list of the P beads; `to_atoms` writes the
    beads back, `centroid_atoms` the centroid; `maxwell_boltzmann()` draws at P T."""
    s, n_rep = _system(), _system()["n_rep"]
    parts = [slice(j * n_rep, (j + 1) * n_rep) for j in range(BEADS)]
    one = _FakeAtoms(s["pos"][parts[0]], s["z"][parts[0]], s["one_cell"], s["m"][parts[0]], None)
    pimd = DevicePIMD.from_atoms(one, _shared_model(), DT, T, beads=BEADS, tau0=TAU0, seed=SEED)
    start = pimd.fetch()
    assert pimd.beads == BEADS and pimd.n_rep == n_rep and start.step == 0 and np.abs(start.forces).max() > 0
    assert np.array_equal(start.positions, np.tile(s["pos"][parts[0]], (BEADS, 1))) and not start.velocities.any()
    pimd.maxwell_boltzmann(seed=4)
    v = pimd.fetch().velocities
    t_mb = (s["m"][:, None] * AMU * v ** 2).sum() / (3 * len(v)) / KB
    assert abs(t_mb / (BEADS * T) - 1) < 5.0 * np.sqrt(2.0 / (3 * len(v))), t_mb
    images = [_FakeAtoms(s["pos"][p], s["z"][p], s["one_cell"], s["m"][p], s["v"][p] * ASE_TIME_FS) for p in parts]
    pimd = DevicePIMD.from_atoms(images, _shared_model(), DT, T, tau0=TAU0, seed=SEED)
    start = pimd.fetch()
    assert np.array_equal(start.positions, s["pos"]) and np.allclose(start.velocities, s["v"], rtol=1e-15, atol=0)
    out = [_FakeAtoms(np.zeros((n_rep, 3)), s["z"][p], s["one_cell"], s["m"][p], None) for p in parts]
    assert pimd.to_atoms(out, start) is start
    for j, p in enumerate(parts):
        assert np.array_equal(out[j].positions, s["pos"][p])
        assert np.allclose(out[j].get_velocities(), s["v"][p] * ASE_TIME_FS, rtol=1e-15, atol=0)
    pimd.centroid_atoms(out[0], start)
    assert np.allclose(out[0].positions, s["pos"].reshape(BEADS, n_rep, 3).mean(axis=0), rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="list of 4"):
        pimd.to_atoms(out[:3], start)
    with pytest.raises(ValueError, match="list of the P beads"):
        DevicePIMD.from_atoms(images, _shared_model(), DT, T, beads=3)


def test_a_replay_has_the_launches_of_a_device_md_replay_and_no_copies():
    """The device activity of two replays of `DevicePIMD` and of `DeviceMD` (Langevin) on the same batch: the same number of
    kernels -- one advance kernel for one, three finish kernels for three -- and no memcpy or memset."""
    from torch.profiler import ProfilerActivity, profile
    s = _system()
    md = DeviceMD(_shared_model(), *_args(s), temperature=BEADS * T, friction=1.0 / TAU0, seed=SEED, velocities=s["v"],
                  batch=torch.from_numpy(s["batch"]).to(_dev()), num_graphs=BEADS)
    pimd = _pimd()

    def events(driver):
        driver.run(2)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            driver.run(2)
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    plain, ours = events(md), events(pimd)
    assert sum(ours.values()) > 0, "the profiler recorded no device activity for graph launches"
    assert sum(ours.values()) == sum(plain.values()), (ours - plain, plain - ours)
    assert not [k for k in ours if "memcpy" in k.lower() or "memset" in k.lower()]
    named = lambda c, word: sum(v for k, v in c.items() if word in k)
    assert named(ours, "pimd_advance_kernel") == named(plain, "md_advance_kernel") == 2
    # the ends of the finish are DeviceMD's own kernels (csrc/md_finish.h); the advance and the log row are the ring's
    for shared in ("md_finish_atoms_kernel", "md_commit_kernel"):
        assert named(ours, shared) == named(plain, shared) == 2
    assert named(ours, "pimd_log_kernel") == named(plain, "md_log_kernel") == 2
    assert named(ours, "pimd_") == 4 and named(ours, "md_") == named(plain, "md_") == 8      # ("md_" counts "pimd_" too)
