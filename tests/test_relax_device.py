"""GPU: `hermnet_amd.relax.DeviceRelax` -- FIRE inside the replayed hipGraph -- against the host-driven loop it replaces (the
numpy float64 transcription of tests/relax_reference.py around a plain `GraphedMDStep` / `GraphedBatchMDStep`), bit for
bit; the device kernels against the library's host twins, the per-graph scalars that involve `/` and sqrt included;
per-graph convergence; the halt-and-resume protocol; the ASE hand-off.

Why bit for bit can be asked: replayed forces equal the plain step's forces bit for bit (test_md_device.py relies on the
same), and the optimiser's arithmetic is contraction-free IEEE float64 in one documented order (tests/test_relax_host.py
checks the transcription on the host twins)."""
import warnings

import numpy as np
import pytest
import torch

from hermnet_amd import _lib, synth
from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep
from hermnet_amd.md import HALT_CAPACITY, HALT_NONFINITE
from hermnet_amd.relax import DeviceRelax
from relax_reference import HostRelax, NumpyRelax, bits
from resident_helpers import _model, _shared_model

pytestmark = pytest.mark.gpu

RATTLE = (0.02, 0.08, 0.15)      # A, per graph of the batch; the single cell takes the last
STEPS = 30
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _single():
    """144 atoms: two full waves plus 16 lanes."""
    pos, cell, z = synth.fcc_alloy_atoms(reps=(3, 3, 4), sigma=RATTLE[2])
    return dict(pos=pos, cell=cell, z=z, batch=None, B=1)


def _batched():
    """32, 48 and 144 atoms: one graph below a wave, unequal ranges, every graph rattled by its own amplitude."""
    parts = [synth.fcc_alloy_atoms(reps=r, seed=s, sigma=RATTLE[s]) for s, r in enumerate([(2, 2, 2), (2, 2, 3), (3, 3, 4)])]
    pos, z = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
    cell = np.stack([p[1] for p in parts])
    batch = np.repeat(np.arange(3), [len(p[0]) for p in parts])
    return dict(pos=pos, cell=cell, z=z, batch=batch, B=3)


def _system(name):
    return _single() if name == "single" else _batched()


def _tensors(s):
    dev = _dev()
    z = torch.from_numpy(s["z"]).to(dev)
    cell = torch.from_numpy(s["cell"].astype(np.float32)).to(dev)
    batch = None if s["batch"] is None else torch.from_numpy(s["batch"]).to(dev)
    return z, cell, batch


def _device_relax(s, model=None, **kw):
    z, cell, batch = _tensors(s)
    if batch is not None:
        kw.update(batch=batch, num_graphs=s["B"])
    return DeviceRelax(model if model is not None else _shared_model(), z, cell, s["pos"], **kw)


def _reference(name, fmax, steps=STEPS):
    """The host-driven loop DeviceRelax replaces, computed once per (system, fmax): NumpyRelax, each evaluation's forces from
    a plain graphed step on float32(x).  (system, the NumpyRelax at the end, a list of per-evaluation records)."""
    key = (name, float(np.max(fmax)), steps)
    if key in _CACHE:
        return _CACHE[key]
    s = _system(name)
    dev = _dev()
    z, cell, batch = _tensors(s)
    p0 = torch.from_numpy(s["pos"].astype(np.float32)).to(dev)
    if batch is None:
        step = GraphedMDStep(_shared_model(), z, cell, p0)
    else:
        step = GraphedBatchMDStep(_shared_model(), z, cell, p0, batch, s["B"])
    ref = NumpyRelax(s["pos"], cell=s["cell"], batch=s["batch"], num_graphs=s["B"], fmax=fmax)
    hist = []
    for _ in range(steps):
        e, f = step(torch.from_numpy(ref.advance()).to(dev))
        e, f = e.cpu().numpy().copy(), f.cpu().numpy().copy()
        ok, n = step.check()
        assert ok
        before = ref.step
        ref.finish(f, energy=e, total=(n, 0))
        hist.append(dict(x=ref.x.copy(), v=ref.v.copy(), image=ref.image.copy(), f=ref.f.copy(), e=e, n=n, dt=ref.dt.copy(),
                         a=ref.a.copy(), scale=ref.scale.copy(), nsteps=ref.nsteps.copy(), fnorm=ref.fnorm.copy(),
                         converged=ref.converged.copy(), conv_step=ref.conv_step.copy(), step=ref.step, done=ref.done,
                         counted=ref.step > before))
    _CACHE[key] = (s, ref, hist)
    return _CACHE[key]


def _equals(snap, rec):
    assert np.array_equal(bits(snap.positions), bits(rec["x"])) and np.array_equal(bits(snap.velocities), bits(rec["v"]))
    assert np.array_equal(snap.images, rec["image"]) and np.array_equal(snap.forces, rec["f"])
    for name in ("dt", "a", "scale"):
        assert np.array_equal(bits(getattr(snap, name)), bits(rec[name])), name
    assert np.array_equal(bits(snap.fmax), bits(rec["fnorm"])) and np.array_equal(snap.nsteps, rec["nsteps"])
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
            bits(snap.dt).tobytes(), bits(snap.a).tobytes(), bits(snap.scale).tobytes(), snap.nsteps.tobytes(),
            snap.converged.tobytes(), snap.converged_step.tobytes(), snap.step, snap.done)


def test_device_kernels_equal_the_host_twins():
    """One advance + finish with the same inputs through hermnet_relax_advance / _finish and their host twins, on random f,
    v and per-graph state (a fresh graph, a downhill one past Nmin, an uphill one, a clamped one, an empty one, one that
    converges), one fixed atom: everything bit-equal -- the per-graph scalars that come out of `/` and sqrt included."""
    dev, lib, P = _dev(), _lib.load(), _lib.ptr
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
    host = HostRelax(x, cell=cell, batch=batch, num_graphs=B, fixed=fixed, fmax=fmax, log_steps=4)
    host.v[:] = rs.normal(scale=0.3, size=(n, 3))
    host.v[fixed] = 0.0
    f_new = rs.normal(size=(n, 3)).astype(np.float32)
    ptr = host.graph_ptr
    host.v[ptr[2]:ptr[3]] = -np.abs(host.v[ptr[2]:ptr[3]]) * np.sign(f_new[ptr[2]:ptr[3]])       # graph 2: uphill
    host.v[ptr[1]:ptr[2]] = np.abs(host.v[ptr[1]:ptr[2]]) * np.sign(f_new[ptr[1]:ptr[2]])        # graph 1: downhill
    host.v[ptr[3]:ptr[4]] = 0.001 * f_new[ptr[3]:ptr[4]]                                        # graph 3: downhill, small
    f_new[ptr[3]:ptr[4]] *= 0.03                                                                 # ... and not clamped
    host.gf[:, 0] = [0.1, 0.37, 0.8, 0.21, 0.1, 0.1]
    host.gf[:, 1] = [0.1, 0.083, 0.1 * 0.99 ** 3, 0.1, 0.1, 0.1]
    host.gf[:, 2] = [0.0, 0.013, 0.004, 0.21, 0.0, 0.05]
    host.gi[:, 0] = [0, 9, 4, 2, 0, 3]
    host.gi[:, 1] = [1, 0, 0, 0, 1, 0]
    host.state[0] = 6                                                                # (log slot 2)
    energy = rs.normal(size=B).astype(np.float32)
    total = np.array([4321, 0], dtype=np.int64)
    names = ["x", "x0", "v", "image", "image0", "f_prev", "batch", "cell", "inv", "pos32", "state", "gf", "gi", "gf_new",
             "gi_new", "log", "graph_ptr", "fmax", "fixed"]
    d = {k: torch.from_numpy(getattr(host, k).copy()).to(dev) for k in names}
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.hermnet_relax_advance(n, B, host.flags, P(d["x"]), P(d["x0"]), P(d["v"]), P(d["image"]), P(d["image0"]),
                                         P(d["fixed"]), P(d["batch"]), P(d["cell"]), P(d["inv"]), P(d["pos32"]), P(d["state"]),
                                         P(d["gf"]), P(d["gi"]), stream), "advance")
    host.advance()
    mid = {k: d[k].cpu().numpy() for k in ("x", "x0", "image", "image0", "pos32")}
    assert np.array_equal(bits(mid["x"]), bits(host.x)) and np.array_equal(bits(mid["x0"]), bits(host.x0))
    assert np.array_equal(mid["image"], host.image) and np.array_equal(mid["image0"], host.image0)
    assert np.array_equal(mid["pos32"], host.pos32) and np.abs(host.image).max() >= 2
    assert np.array_equal(bits(host.x[300]), bits(x[300]))                            # the fixed atom is not even wrapped
    f_d, e_d, t_d = (torch.from_numpy(a).to(dev) for a in (f_new, energy, total))
    _lib.check(lib.hermnet_relax_finish(n, B, P(d["graph_ptr"]), P(f_d), P(e_d), P(t_d), 5000, host.dt, host.dtmax, host.maxstep,
                                        float(fmax[0]), P(d["fmax"]), P(d["x"]), P(d["v"]), P(d["x0"]), P(d["image"]),
                                        P(d["image0"]), P(d["f_prev"]), P(d["fixed"]), P(d["pos32"]), P(d["gf"]), P(d["gi"]),
                                        P(d["gf_new"]), P(d["gi_new"]), P(d["log"]), 4, P(d["state"]), stream), "finish")
    torch.cuda.synchronize()
    host.finish(f_new, energy=energy, total=total, capacity=5000)
    got = {k: d[k].cpu().numpy() for k in ("x", "v", "image", "f_prev", "state", "log", "gf", "gi", "pos32")}
    assert got["state"].tolist() == host.state.tolist() == [7, 0, 0, 0]
    for k in ("x", "v", "gf", "log"):
        assert np.array_equal(bits(got[k]), bits(getattr(host, k))), k
    for k in ("image", "f_prev", "gi", "pos32"):
        assert np.array_equal(got[k], getattr(host, k)), k
    # the inputs did reach every branch: fresh, growth, uphill reset, unclamped, empty -> converged, converged on fmax
    gf, gi = host.gf, host.gi
    assert gi[0].tolist() == [0, 0, 0, -1] and gf[0, 0] == 0.1
    assert gi[1, 0] == 10 and gf[1, 0] == min(0.37 * 1.1, 1.0) and gf[1, 2] < gf[1, 0]          # grown, then clamped
    assert gi[2, 0] == 0 and gf[2, 0] == 0.4 and gf[2, 1] == 0.1
    assert gi[3, 0] == 3 and gf[3, 2] == gf[3, 0] == 0.21                                        # no clamp
    assert gi[4].tolist() == [0, 1, 1, 6] and gi[5, 2:].tolist() == [1, 6] and not host.v[ptr[5]:ptr[6]].any()
    assert np.all(got["log"][[0, 1, 3]] == -7.0) and np.all(got["log"][2][:, 3] == 4321)
    assert not host.v[300].any()


@pytest.mark.parametrize("name", ["single", "batch"])
def test_trajectory_equals_the_host_driven_loop_bit_for_bit(name):
    """30 replays against NumpyRelax around a plain graphed step: positions, velocities, images, forces, the per-graph
    state, every log row (E_pot that evaluation's energy bit for bit, max |f|, dt, the edge count `check()` saw)."""
    s, ref, hist = _reference(name, 1e-6)
    rx = _device_relax(s, fmax=1e-6)
    rx.run(STEPS)
    snap = rx.fetch()
    assert (snap.step, snap.halted, snap.halt_code, snap.halt_step, snap.done) == (STEPS, False, 0, None, False)
    assert _equals(snap, hist[-1])
    _log_equals(snap.log, ref.log, hist)
    assert snap.log.shape == (STEPS, s["B"], 4)
    for g in range(s["B"]):                                           # FIRE did something: the largest force fell
        assert snap.log[-1, g, 1] < snap.log[0, g, 1]
    assert np.array_equal(bits(snap.energy), bits(hist[-1]["e"].astype(np.float64)))
    assert rx.fetch().log.shape[0] == 0                               # nothing pending: the next fetch carries no rows


def test_per_graph_convergence_on_the_device():
    """A threshold that every graph reaches by evaluation 25, at different evaluations: converged_step, done and the final
    step equal the reference's, the frozen graphs' positions stay, replays after `done` change and log nothing."""
    s, _, free = _reference("batch", 1e-6)          # (a threshold out of reach: the entry points refuse fmax = 0)
    assert not free[-1]["converged"].any()
    fnorm =np.array([rec["fnorm"] for rec in free])                  # [30, B]: max |f_i| per evaluation (nothing converges)
    T = fnorm[1:26].min(axis=0).max() * (1.0 + 1e-6)
    s, ref, hist = _reference("batch", T)
    conv = ref.conv_step
    assert ref.done and np.all(conv >= 0) and conv.max() <= 25
    assert len(set(conv.tolist())) > 1, "all graphs converge at the same evaluation: change the rattle amplitudes"
    last = int(conv.max())
    rx = _device_relax(s, fmax=T)
    ptr = np.searchsorted(s["batch"], np.arange(s["B"] + 1))
    first = int(conv.min())
    rx.run(first + 1)
    early = rx.fetch()
    assert _equals(early, hist[first]) and not early.done and early.converged.sum() >= 1
    rx.run(STEPS - first - 1)
    snap = rx.fetch()
    assert _equals(snap, hist[-1])
    assert snap.done and snap.step == last + 1 and np.array_equal(snap.converged_step, conv)
    assert early.log.shape[0] + snap.log.shape[0] == last + 1          # no rows behind `done`
    _log_equals(np.concatenate([early.log, snap.log]), ref.log, hist)
    for g in np.flatnonzero(early.converged):                          # frozen since then
        a, b = ptr[g], ptr[g + 1]
        assert np.array_equal(bits(snap.positions[a:b]), bits(early.positions[a:b]))
        assert np.array_equal(bits(snap.positions[a:b]), bits(hist[conv[g]]["x"][a:b]))
    rx.run(5)
    again = rx.fetch()
    assert _state_bits(again) == _state_bits(snap) and again.log.shape[0] == 0
    # run_until stops there by itself
    rx2 = _device_relax(s, fmax=T)
    end = rx2.run_until(100, chunk=8)
    assert end.done and _state_bits(end) == _state_bits(snap)


def test_halt_on_list_overflow_and_resume():
    """A capacity that the list outgrows at evaluation k: the run halts there with the capacity bit, in the state of the
    last completed evaluation, with exactly k log rows; resume() recaptures with more columns and the run ends bit-equal to
    the uninterrupted reference.  (The overflowing replays are ordinary padded searches that report a flag.)"""
    s, ref, hist = _reference("single", 1e-6)
    counts = [rec["n"] for rec in hist]                 # counts[k]: the list of evaluation k; counts[0]: the start's
    at = [k for k in range(2, STEPS) if counts[k] > max(counts[:k])]
    assert at, "the edge count never exceeded its running maximum: no overflow to test"
    k = at[0]
    capacity = max(counts[:k])
    rx = _device_relax(s, fmax=1e-6, capacity=capacity)
    assert rx.capacity == capacity
    rx.run(STEPS)
    snap = rx.fetch()
    assert snap.halted and snap.step == k and snap.halt_step == k and (snap.halt_code & HALT_CAPACITY)
    assert not (snap.halt_code & HALT_NONFINITE)
    assert _equals(snap, hist[k - 1])
    _log_equals(snap.log, ref.log[:k], hist[:k])
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


def test_halt_on_a_non_finite_energy_and_resume():
    """A weight written through `.data` between two runs: the run halts with the non-finite bit in the state of the last
    good evaluation; after the caches are dropped (fetch does it, with a warning) resume() recaptures and the run goes on;
    no NaN ever reaches the state or the log."""
    s = _single()
    model = _model(seed=9)
    rx = _device_relax(s, model=model, fmax=1e-6)
    rx.run(5)
    good = rx.fetch()
    assert good.step == 5 and not good.halted
    p_ = [p for n, p in model.named_parameters() if n.endswith("update_layer.xvec_proj.2.weight")][1]
    p_.data.mul_(1.5)
    rx.run(5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        snap = rx.fetch()
    assert any("resume()" in str(w.message) for w in rec)
    assert snap.halted and snap.halt_code == HALT_NONFINITE and snap.step == snap.halt_step == 5 and snap.log.shape[0] == 0
    assert _state_bits(snap) == _state_bits(good)
    assert rx.stale()
    with pytest.raises(RuntimeError, match="resume"):
        rx.run(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rx.resume()
    rx.run(5)
    end = rx.fetch()
    assert (end.step, end.halted) == (10, False) and end.log.shape == (5, 1, 4) and np.all(np.isfinite(end.log))
    assert np.all(np.isfinite(end.positions)) and np.all(np.isfinite(end.velocities))
    assert not np.array_equal(end.log[0, :, 0], good.log[4, :, 0])                  # the new weights' energies


def test_a_run_in_pieces_equals_the_run_and_unfetched_rows_are_kept():
    """run(7); run(13) equals run(20), with or without a fetch() in between; `run` refuses to overwrite log rows that were
    not fetched, and the ring wraps once they were."""
    s, ref, hist = _reference("batch", 1e-6)

    def go(pieces, fetch_between=False, **kw):
        rx = _device_relax(s, fmax=1e-6, **kw)
        logs = []
        for k in pieces:
            rx.run(k)
            if fetch_between:
                logs.append(rx.fetch().log)
        snap = rx.fetch()
        logs.append(snap.log)
        return snap, np.concatenate(logs)

    whole, log_w = go([20])
    assert _equals(whole, hist[19])
    for pieces, between in (([7, 13], False), ([7, 13], True)):
        snap, log = go(pieces, between)
        assert _state_bits(snap) == _state_bits(whole) and np.array_equal(bits(log), bits(log_w)), (pieces, between)
    small = _device_relax(s, fmax=1e-6, log_steps=8)
    small.run(8)
    with pytest.raises(RuntimeError, match="not fetched"):
        small.run(1)
    assert _equals(small.fetch(), hist[7])
    small.run(8)                                                      # the ring wraps
    got = small.fetch()
    assert _equals(got, hist[15])
    _log_equals(got.log, ref.log[8:16], hist[8:16])


class _FakeAtoms(object):
    """What `from_atoms` / `to_atoms` touch of an ase.Atoms."""

    def __init__(self, positions, numbers, cell, pbc=True):
        self.positions, self.numbers, self.cell, self.pbc = positions.copy(), numbers, cell, np.array([pbc] * 3)


def test_ase_hand_off():
    """from_atoms on a list of three duck-typed structures is the batch; to_atoms writes each member's positions back; a
    list that mixes periodic and open members is refused."""
    s, _, hist = _reference("batch", 1e-6)
    ptr = np.searchsorted(s["batch"], np.arange(4))
    atoms = [_FakeAtoms(s["pos"][a:b], s["z"][a:b], s["cell"][g]) for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:]))]
    rx = DeviceRelax.from_atoms(atoms, _shared_model(), fmax=1e-6)
    assert rx.num_graphs == 3 and rx.n == len(s["z"])
    start = rx.fetch()
    assert np.array_equal(start.positions, s["pos"]) and start.step == 0 and not start.halted and not start.done
    rx.run(3)
    snap = rx.to_atoms(atoms)
    assert _equals(snap, hist[2])
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        assert np.array_equal(atoms[g].positions, hist[2]["x"][a:b])
    with pytest.raises(ValueError, match="do not match"):
        rx.to_atoms(atoms[:2], snap)
    mixed = atoms[:2] + [_FakeAtoms(s["pos"][:4], s["z"][:4], s["cell"][0], pbc=False)]
    with pytest.raises(RuntimeError, match="all periodic"):
        DeviceRelax.from_atoms(mixed, _shared_model())
    one = DeviceRelax.from_atoms(atoms[2], _shared_model(), fmax=1e-6)
    assert one.num_graphs == 1 and one.batch is None and one.n == 144


def test_more_graphs_than_lanes():
    """tests/test_relax_host.py's B = 257 (graph 256 moving beside 256 converged graphs, graph 3 empty), kernel-direct: two
    advance + finish through hermnet_relax_advance / _finish against their host twins, bit for bit -- graph 256 is moved,
    committed and counted in `all` (done stays 0), and done is 1 once the second evaluation puts it under fmax."""
    import test_relax_host as rht
    dev, lib, P = _dev(), _lib.load(), _lib.ptr
    host, _, f1, f2 = rht.many_graphs()
    n, B = host.n, host.B
    names = ["x", "x0", "v", "image", "image0", "f_prev", "batch", "pos32", "state", "gf", "gi", "gf_new", "gi_new", "log",
             "graph_ptr", "fmax"]
    d = {k: torch.from_numpy(getattr(host, k).copy()).to(dev) for k in names}
    stream = torch.cuda.current_stream().cuda_stream
    start = host.x.copy()
    for k, f in enumerate((f1, f2)):
        e, tot = np.zeros(B, dtype=np.float32), np.array([11 + k, 0], dtype=np.int64)
        f_d, e_d, t_d = (torch.from_numpy(a).to(dev) for a in (f, e, tot))
        _lib.check(lib.hermnet_relax_advance(n, B, host.flags, P(d["x"]), P(d["x0"]), P(d["v"]), P(d["image"]), P(d["image0"]),
                                             None, P(d["batch"]), None, None, P(d["pos32"]), P(d["state"]), P(d["gf"]), P(d["gi"]),
                                             stream), "advance")
        _lib.check(lib.hermnet_relax_finish(n, B, P(d["graph_ptr"]), P(f_d), P(e_d), P(t_d), 5000, host.dt, host.dtmax,
                                            host.maxstep, float(host.fmax[0]), P(d["fmax"]), P(d["x"]), P(d["v"]), P(d["x0"]),
                                            P(d["image"]), P(d["image0"]), P(d["f_prev"]), None, P(d["pos32"]), P(d["gf"]),
                                            P(d["gi"]), P(d["gf_new"]), P(d["gi_new"]), P(d["log"]), host.log_steps,
                                            P(d["state"]), stream), "finish")
        torch.cuda.synchronize()
        host.advance()
        host.finish(f, energy=e, total=tot, capacity=5000)
        got = {k: d[k].cpu().numpy() for k in names}
        assert got["state"].tolist() == host.state.tolist() == [k + 1, 0, 0, k]
        for key in ("x", "x0", "v", "gf", "gf_new", "log"):
            assert np.array_equal(bits(got[key]), bits(getattr(host, key))), key
        for key in ("image", "image0", "f_prev", "gi", "gi_new", "pos32"):
            assert np.array_equal(got[key], getattr(host, key)), key
        assert got["gi"][256, 1:].tolist() == [[0, 0, -1], [0, 1, 1]][k] and (got["gf"][256, 2] > 0.0) == (k == 0)
    assert np.array_equal(bits(got["x"][:-2]), bits(start[:-2])) and np.abs(got["x"][-2:] - start[-2:]).min() > 1e-4
    assert np.all(got["log"][2:] == -7.0) and np.all(got["log"][:2, :, 3] == [[11], [12]])
