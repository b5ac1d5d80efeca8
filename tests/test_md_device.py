"""GPU: `hermnet_amd.md.DeviceMD` -- the integrator inside the replayed hipGraph -- against the host-driven loop it replaces
(numpy float64 velocity Verlet around a plain `GraphedMDStep` / `GraphedBatchMDStep`), bit for bit; the device kernels
against the library's host twins; Langevin determinism; the halt-and-resume protocol; the ASE hand-off.

Why bit for bit can be asked: replayed forces equal the exact-list forces bit for bit (test_gpu_parity.py:
test_md_step_with_list_rebuild_replays_as_one_graph), and the integrator's arithmetic is contraction-free IEEE float64 that
numpy's elementwise operations reproduce (tests/md_reference.py, checked on the host twins in tests/test_md_host.py)."""
import warnings

import numpy as np
import pytest
import torch

from hermnet_amd import _lib, synth
from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep
from hermnet_amd.md import ASE_TIME_FS, HALT_CAPACITY, HALT_NONFINITE, DeviceMD
from md_reference import AMU, KB, HostMD, NumpyMD, bits, host_noise
from resident_helpers import _FakeAtoms, _model, _shared_model

pytestmark = pytest.mark.gpu

MASS = {13: 26.9815, 28: 58.6934, 29: 63.546}
DT, HOT = 1.0, 2500.0          # fs, K: hot enough that the neighbour list changes every few steps
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _velocities(m, temp, seed):
    return np.random.RandomState(seed).normal(size=(len(m), 3)) * np.sqrt(KB * temp / (m * AMU))[:, None]


def _single():
    """144 atoms: two full waves plus 16 lanes."""
    pos, cell, z = synth.fcc_alloy_atoms(reps=(3, 3, 4))
    m = np.array([MASS[int(v)] for v in z])
    return dict(pos=pos, cell=cell, z=z, m=m, v=_velocities(m, HOT, 1), batch=None)


def _batched():
    """32, 48 and 144 atoms: one graph below a wave, unequal ranges, boxes under twice the cutoff."""
    parts = [synth.fcc_alloy_atoms(reps=r, seed=s) for s, r in enumerate([(2, 2, 2), (2, 2, 3), (3, 3, 4)])]
    pos, z = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
    cell = np.stack([p[1] for p in parts])
    batch = np.repeat(np.arange(3), [len(p[0]) for p in parts])
    m = np.array([MASS[int(v)] for v in z])
    return dict(pos=pos, cell=cell, z=z, m=m, v=_velocities(m, HOT, 2), batch=batch)


def _tensors(s):
    dev = _dev()
    z = torch.from_numpy(s["z"]).to(dev)
    cell = torch.from_numpy(s["cell"].astype(np.float32)).to(dev)
    batch = None if s["batch"] is None else torch.from_numpy(s["batch"]).to(dev)
    return z, cell, batch


def _device_md(s, **kw):
    z, cell, batch = _tensors(s)
    if batch is not None:
        kw.update(batch=batch, num_graphs=int(s["batch"][-1]) + 1)
    return DeviceMD(_shared_model(), z, cell, s["pos"], s["m"], DT, velocities=s["v"], **kw)


def _reference(name, steps):
    """The host-driven loop DeviceMD replaces, `steps` steps of it, computed once per system: numpy float64 velocity Verlet,
    each step's forces from a plain graphed step on float32(x).  A list of per-step records."""
    key = (name, steps)
    if key in _CACHE:
        return _CACHE[key]
    s = _single() if name == "single" else _batched()
    dev = _dev()
    z, cell, batch = _tensors(s)
    p0 = torch.from_numpy(s["pos"].astype(np.float32)).to(dev)
    if batch is None:
        step = GraphedMDStep(_shared_model(), z, cell, p0)
    else:
        step = GraphedBatchMDStep(_shared_model(), z, cell, p0, batch, 3)

    def forces(p32):
        e, f = step(torch.from_numpy(p32).to(dev))
        e, f = e.cpu().numpy().copy(), f.cpu().numpy().copy()
        ok, n = step.check()
        assert ok
        return e, f, n

    ref = NumpyMD(s["pos"], s["v"], s["m"], DT, cell=s["cell"], batch=s["batch"])
    _, ref.f, s["n0"] = forces(ref.x.astype(np.float32))           # (n0: the list of the start coordinates)
    ptr = np.searchsorted(ref.batch, np.arange(int(ref.batch[-1]) + 2))
    hist = []
    for _ in range(steps):
        e, f, n = forces(ref.advance())
        ref.finish(f)
        ke = np.array([ref.ke[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])])
        hist.append(dict(x=ref.x.copy(), v=ref.v.copy(), image=ref.image.copy(), f=f, e=e, n=n, ke=ke))
    _CACHE[key] = (s, hist)
    return s, hist


def _equals(snap, rec):
    return (np.array_equal(bits(snap.positions), bits(rec["x"])) and np.array_equal(bits(snap.velocities), bits(rec["v"]))
            and np.array_equal(snap.images, rec["image"]) and np.array_equal(snap.forces, rec["f"]))


def _log_equals(log, hist, n_atoms):
    assert log.shape[0] == len(hist)
    for row, rec in zip(log, hist):
        assert np.array_equal(bits(row[:, 0]), bits(rec["e"].astype(np.float64)))       # E_pot: that step's energy, bit for bit
        assert np.all(row[:, 2] == rec["n"])
        assert np.all(np.abs(row[:, 1] - rec["ke"]) <= n_atoms * 2.0 ** -52 * np.abs(rec["ke"]))


@pytest.mark.parametrize("name", ["single", "batch"])
def test_nve_trajectory_equals_the_host_driven_loop_bit_for_bit(name):
    """`DeviceMD.run(20)` against the host-driven loop: x, v, image and forces bit-equal after 20 steps, every logged E_pot
    that step's energy bit for bit, the logged edge counts `check()`'s -- on a run hot enough that the list changes."""
    s, hist = _reference(name, 30 if name == "single" else 20)
    hist = hist[:20]
    md = _device_md(s)
    md.run(20)
    snap = md.fetch()
    assert (snap.step, snap.halted, snap.halt_code, snap.halt_step) == (20, False, 0, None)
    assert len(set(rec["n"] for rec in hist)) > 3                    # the list really changed along the run
    _log_equals(snap.log, hist, len(s["z"]))
    assert _equals(snap, hist[-1])
    assert np.abs(snap.images).max() >= 0 and snap.log.shape == (20, 1 if name == "single" else 3, 3)
    # nothing pending: the next fetch carries no rows; run() refuses to overwrite rows that were not fetched
    assert md.fetch().log.shape[0] == 0
    small = _device_md(s, log_steps=8) if name == "single" else None
    if small is not None:
        small.run(8)
        with pytest.raises(RuntimeError, match="not fetched"):
            small.run(1)
        assert _equals(small.fetch(), hist[7])
        small.run(8)                                                  # the ring wraps
        got = small.fetch()
        assert _equals(got, hist[15])
        _log_equals(got.log, hist[8:16], len(s["z"]))


def _on_device(host, dev):
    """The arrays of a HostMD as device tensors."""
    names = ["x", "v", "x0", "v0", "image", "image0", "f_prev", "kick", "c1", "sigma", "batch", "cell", "inv", "pos32", "state",
             "graph_ptr", "half_mass", "ke_atom", "log"]
    return {k: None if getattr(host, k) is None else torch.from_numpy(getattr(host, k).copy()).to(dev) for k in names}


@pytest.mark.parametrize("friction", [None, 0.02], ids=["nve", "langevin"])
def test_device_kernels_equal_the_host_twins(friction):
    """One advance + finish with the same inputs through hermnet_md_advance / _finish and their host twins: NVE bit-equal;
    Langevin within 1e-12 (a few ulp of the device's float64 log / cos / sqrt in the Gaussians) of the state's scale.  Raw
    Philox words: bit-equal."""
    dev, lib, P = _dev(), _lib.load(), _lib.ptr
    n = 257 + 144
    rs = np.random.RandomState(3)
    cell = np.stack([np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]]), np.diag([8.0, 9.0, 10.0])])
    batch = np.repeat([0, 1], [257, 144])
    x = np.einsum("nk,nkj->nj", rs.uniform(-2.5, 3.5, (n, 3)), cell[batch])          # some atoms cells away: wrap and image
    m = rs.uniform(10.0, 60.0, n)
    m[100] = np.inf
    host = HostMD(x, rs.normal(scale=0.02, size=(n, 3)), m, 0.5, cell=cell, batch=batch, friction=friction,
                  temperature=None if friction is None else [300.0, 900.0], seed=(7 << 32) + 5, log_steps=4)
    host.f_prev[:] = rs.normal(size=(n, 3)).astype(np.float32)
    host.state[0] = 6                                                                # (log slot 2, noise of step 6)
    f_new = rs.normal(size=(n, 3)).astype(np.float32)
    energy, total = np.array([-3.5, 2.25], dtype=np.float32), np.array([4321, 0], dtype=np.int64)
    d = _on_device(host, dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.hermnet_md_advance(n, 2, host.flags, host.dt, host.seed, P(d["x"]), P(d["v"]), P(d["x0"]), P(d["v0"]),
                                      P(d["image"]), P(d["image0"]), P(d["f_prev"]), P(d["kick"]), P(d["c1"]), P(d["sigma"]),
                                      P(d["batch"]), P(d["cell"]), P(d["inv"]), P(d["pos32"]), P(d["state"]), stream), "advance")
    host.advance()
    mid = {k: d[k].cpu().numpy() for k in ("x", "v", "image", "pos32", "x0", "v0")}
    f_d, e_d, t_d = (torch.from_numpy(a).to(dev) for a in (f_new, energy, total))
    _lib.check(lib.hermnet_md_finish(n, 2, P(d["graph_ptr"]), P(f_d), P(e_d), P(t_d), 5000, P(d["x"]), P(d["v"]), P(d["x0"]),
                                     P(d["v0"]), P(d["image"]), P(d["image0"]), P(d["f_prev"]), P(d["kick"]), P(d["half_mass"]),
                                     P(d["pos32"]), P(d["ke_atom"]), P(d["log"]), 4, P(d["state"]), stream), "finish")
    torch.cuda.synchronize()
    x_mid_host = host.x.copy()
    host.finish(f_new, energy=energy, total=total, capacity=5000)
    got = {k: d[k].cpu().numpy() for k in ("x", "v", "image", "f_prev", "state", "log")}
    assert got["state"].tolist() == host.state.tolist() == [7, 0, 0, 0]
    assert np.array_equal(got["image"], host.image) and np.array_equal(got["f_prev"], host.f_prev)
    assert np.abs(host.image).max() >= 2
    assert np.array_equal(mid["x0"], host.x0) and np.array_equal(mid["v0"], host.v0)
    if friction is None:
        assert np.array_equal(bits(mid["x"]), bits(x_mid_host)) and np.array_equal(mid["pos32"], host.pos32)
        assert np.array_equal(bits(got["x"]), bits(host.x)) and np.array_equal(bits(got["v"]), bits(host.v))
    else:
        assert np.abs(got["x"] - host.x).max() <= 1e-12 * np.abs(host.x).max()
        assert np.abs(got["v"] - host.v).max() <= 1e-12 * np.abs(host.v).max()
    want, have = host.log[2], got["log"][2]
    assert np.array_equal(have[:, 0], want[:, 0]) and np.array_equal(have[:, 2], want[:, 2]) and np.all(have[:, 2] == 4321)
    assert np.all(np.abs(have[:, 1] - want[:, 1]) <= (n * 2.0 ** -52 + (0 if friction is None else 1e-11)) * np.abs(want[:, 1]))
    assert np.all(got["log"][[0, 1, 3]] == -7.0)
    # the noise itself
    words_d = torch.zeros(n, 8, dtype=torch.int32, device=dev)
    gauss_d = torch.zeros(n, 3, dtype=torch.float64, device=dev)
    _lib.check(lib.hermnet_md_noise(host.seed, 6, n, P(words_d), P(gauss_d), stream), "noise")
    words_h, gauss_h = host_noise(host.seed, 6, n)
    assert np.array_equal(words_d.cpu().numpy().view(np.uint32), words_h)
    assert np.abs(gauss_d.cpu().numpy() - gauss_h).max() <= 1e-12


def _state_bits(snap):
    return (bits(snap.positions).tobytes(), bits(snap.velocities).tobytes(), snap.images.tobytes(), snap.forces.tobytes(),
            snap.step)


def test_langevin_run_is_a_function_of_the_seed_alone():
    """The same seed twice: bit-equal state and log; run(7); run(13) equals run(20), with or without a fetch in between;
    another seed differs; replicas of a batch take their own temperatures' noise."""
    s = _single()
    kw = dict(friction=0.01, temperature=600.0)

    def go(seed, pieces, fetch_between=False):
        md = _device_md(s, seed=seed, **kw)
        logs = []
        for k in pieces:
            md.run(k)
            if fetch_between:
                logs.append(md.fetch().log)
        snap = md.fetch()
        logs.append(snap.log)
        return _state_bits(snap), np.concatenate(logs)

    a, log_a = go(11, [20])
    for pieces, between in (([20], False), ([7, 13], False), ([7, 13], True)):
        b, log_b = go(11, pieces, between)
        assert a == b and np.array_equal(bits(log_a), bits(log_b)), (pieces, between)
    assert log_a.shape == (20, 1, 3) and np.all(np.isfinite(log_a))
    c, log_c = go(12, [20])
    assert a[:2] != c[:2] and not np.array_equal(log_a[:, :, :2], log_c[:, :, :2])


def test_halt_on_list_overflow_and_resume():
    """A capacity that the list outgrows at step s: the run halts there with the capacity bit, in the state of the last
    completed step, with exactly s log rows; resume() recaptures with more columns and the run ends bit-equal to the
    uninterrupted reference.  (The overflowing replays are ordinary padded searches that report a flag.)"""
    s, hist = _reference("single", 30)
    counts = [rec["n"] for rec in hist]                 # counts[k]: the list of step k (0-based), built inside replay k
    first = s["n0"]             # the construction evaluates the start coordinates as well: their list must fit too
    at = [k for k in range(2, 30) if counts[k] > max([first] + counts[:k])]
    assert at, "the edge count never exceeded its running maximum: no overflow to test"
    k = at[0]
    capacity = max([first] + counts[:k])
    md = _device_md(s, capacity=capacity)
    assert md.capacity == capacity
    md.run(30)
    snap = md.fetch()
    assert snap.halted and snap.step == k and snap.halt_step == k and (snap.halt_code & HALT_CAPACITY)
    assert not (snap.halt_code & HALT_NONFINITE)
    assert _equals(snap, hist[k - 1])
    _log_equals(snap.log, hist[:k], len(s["z"]))
    md.run(3)                                            # halted: replays change nothing
    again = md.fetch()
    assert _state_bits(again) == _state_bits(snap) and again.log.shape[0] == 0 and again.halted
    md.resume()
    assert md.capacity > capacity
    md.run(30 - k)
    end = md.fetch()
    assert (end.step, end.halted) == (30, False)
    assert _equals(end, hist[29])
    _log_equals(end.log, hist[k:], len(s["z"]))


def test_halt_on_a_non_finite_energy_and_resume():
    """A weight written through `.data` between two runs: the stale-weight guard poisons the step, the run halts with the
    non-finite bit in the state of the last good step; after the caches are dropped (fetch does it, with a warning) resume()
    recaptures and the run continues; no NaN ever reaches the log."""
    s = _single()
    model = _model(seed=9)
    z, cell, _ = _tensors(s)
    md = DeviceMD(model, z, cell, s["pos"], s["m"], DT, velocities=s["v"])
    md.run(5)
    good = md.fetch()
    assert good.step == 5 and not good.halted
    p_ = [p for n, p in model.named_parameters() if n.endswith("update_layer.xvec_proj.2.weight")][1]
    p_.data.mul_(1.5)
    md.run(5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        snap = md.fetch()
    assert any("resume()" in str(w.message) for w in rec)
    assert snap.halted and snap.halt_code == HALT_NONFINITE and snap.step == snap.halt_step == 5 and snap.log.shape[0] == 0
    assert _state_bits(snap) == _state_bits(good)
    assert md.stale()
    with pytest.raises(RuntimeError, match="resume"):
        md.run(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        md.resume()
    md.run(5)
    end = md.fetch()
    assert (end.step, end.halted) == (10, False) and end.log.shape == (5, 1, 3) and np.all(np.isfinite(end.log))
    assert np.all(np.isfinite(end.positions)) and np.all(np.isfinite(end.velocities))
    assert not np.array_equal(end.log[0, :, 0], good.log[4, :, 0])                  # the new weights' energies


def test_ase_hand_off_and_momentum():
    """from_atoms / to_atoms round trip (ASE's time unit is sqrt(103.642696562) = 10.18051 fs), fixed atoms through an
    infinite mass, Maxwell-Boltzmann velocities and zero_momentum: sum m v <= N 2^-52 sum |m v|."""
    import math
    s = _single()
    n = len(s["z"])
    assert abs(ASE_TIME_FS - 10.18051) < 1e-5
    atoms = _FakeAtoms(s["pos"], s["z"], s["cell"], s["m"], s["v"] * ASE_TIME_FS)
    md = DeviceMD.from_atoms(atoms, _shared_model(), DT)
    snap = md.fetch()
    assert np.array_equal(snap.positions, s["pos"]) and snap.step == 0 and not snap.halted
    assert np.allclose(snap.velocities, s["v"], rtol=1e-15, atol=0)
    assert np.all(np.isfinite(snap.forces)) and np.abs(snap.forces).max() > 0                # primed at construction
    out = _FakeAtoms(np.zeros_like(s["pos"]), s["z"], s["cell"], s["m"], None)
    md.to_atoms(out, snap)
    assert np.array_equal(out.positions, s["pos"]) and np.allclose(out.get_velocities(), atoms.get_velocities(), rtol=1e-15, atol=0)
    # one step through the hand-off equals the reference's first step
    _, hist = _reference("single", 30)
    md.run(1)
    one = md.to_atoms(out)          # (v / 10.18051 * 10.18051 may differ from v in the last bit: close, not bit-equal)
    assert one.step == 1 and np.allclose(out.positions, hist[0]["x"], rtol=0, atol=1e-9)
    assert np.allclose(one.velocities, hist[0]["v"], rtol=0, atol=1e-9 * np.abs(hist[0]["v"]).max())
    # momentum
    m = s["m"].copy()
    m[5] = np.inf
    z, cell, _ = _tensors(s)
    md = DeviceMD(_shared_model(), z, cell, s["pos"], m, DT, velocities=s["v"])
    md.maxwell_boltzmann(300.0, seed=4)
    before = md.fetch().velocities
    t_mb = (m[np.isfinite(m), None] * AMU * before[np.isfinite(m)] ** 2).sum() / (3 * (n - 1)) / KB
    assert not before[5].any() and abs(t_mb / 300.0 - 1) < 5.0 * np.sqrt(2.0 / (3 * (n - 1))), t_mb
    md.zero_momentum()
    v = md.fetch().velocities
    free = np.isfinite(m)
    mv = m[free, None] * v[free]
    for k in range(3):
        assert abs(math.fsum(mv[:, k])) <= n * 2.0 ** -52 * math.fsum(np.abs(mv[:, k]))
    assert abs(math.fsum((m[free, None] * before[free])[:, 0])) > 1e3 * n * 2.0 ** -52 * math.fsum(np.abs(mv[:, 0]))
    assert not v[5].any()
    md.run(2)
    moved = md.fetch()
    assert np.array_equal(moved.positions[5], s["pos"][5]) and not moved.velocities[5].any() and moved.step == 2
