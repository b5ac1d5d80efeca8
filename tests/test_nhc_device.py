"""GPU: `hermnet_amd.nhc.DeviceNHC` -- Nose-Hoover chain NVT inside the replayed hipGraph.  The kernels against the library's
host twins on synthetic state; a run against the host-driven loop it replaces after every step; `tau=inf` against `DeviceMD`
NVE with observers; velocities written between two runs; halt on a list overflow and resume; the launch list; the ASE
hand-off."""
from collections import Counter

import numpy as np
import pytest
import torch

from hermnet_amd import _lib, synth
from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.md import ASE_TIME_FS, HALT_CAPACITY, HALT_NONFINITE, DeviceMD
from hermnet_amd.nhc import DeviceNHC, conserved
from hermnet_amd.observe import MSD, Frames
from md_reference import AMU, KB, bits
from nhc_reference import HostNHC
import resident_helpers as rh
from resident_helpers import _flat, _put
import test_md_device as mdt

pytestmark = pytest.mark.gpu

DT = 1.0
T_START = 1500.0                                          # K: the Maxwell-Boltzmann velocities every driver here starts from
T_NHC = np.array([300.0, 600.0, 900.0, 1500.0])           # K, per graph
TAU = np.array([20.0, 40.0, 60.0, 100.0])                 # fs, per graph: short, so that 20 steps move the chains
DOF = 3.0 * 32 - 3.0
PARKED = 1 << 20
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


# ---- 1. the kernels against the host twins ----------------------------------------------------------------------------------------
NAMES = ["x", "v", "x0", "v0", "image", "image0", "f_prev", "kick", "batch", "cell", "inv", "pos32", "state", "graph_ptr",
         "half_mass", "ke_atom", "log", "delta", "kt", "dof_kt", "q", "inv_q", "xi", "v_xi", "xi0", "v_xi0", "scale"]
COUNTS = [1, 32, 257, 256, 5]


def _replay_on_both(host, d, f_new, energy, total, capacity=5000):
    """One hermnet_nhc_advance + hermnet_nhc_finish and their host twins on the same state and evaluation."""
    lib, P, stream = _lib.load(), _lib.ptr, torch.cuda.current_stream().cuda_stream
    n, B = host.n, host.B
    chains = (host.chain, host.order, host.substeps) + tuple(P(d[k]) for k in ("delta", "kt", "dof_kt", "q", "inv_q", "xi", "v_xi",
                                                                                "xi0", "v_xi0", "scale"))
    atoms = [P(d[k]) for k in ("x", "v", "x0", "v0", "image", "image0", "f_prev", "kick")]
    _lib.check(lib.hermnet_nhc_advance(n, B, host.flags, host.dt, *atoms, P(d["batch"]), P(d["cell"]), P(d["inv"]), P(d["pos32"]),
                                       P(d["state"]), P(d["graph_ptr"]), P(d["half_mass"]), *chains, stream), "advance")
    f_d, e_d, t_d = _put(f_new), _put(energy), _put(np.array(total, dtype=np.int64))
    _lib.check(lib.hermnet_nhc_finish(n, B, P(d["graph_ptr"]), P(d["batch"]), P(f_d), P(e_d), P(t_d), capacity, *atoms,
                                      P(d["half_mass"]), P(d["pos32"]), P(d["ke_atom"]), *chains, P(d["log"]), host.log_steps,
                                      P(d["state"]), stream), "finish")
    torch.cuda.synchronize()
    host.advance()
    host.finish(f_new, energy, total=total, capacity=capacity)


def _equal_everywhere(host, d, what):
    for k in NAMES:
        got, want = d[k].cpu().numpy(), getattr(host, k)
        same = np.array_equal(bits(got), bits(want)) if want.dtype == np.float64 else np.array_equal(got, want)
        assert same, (what, k)


@pytest.mark.parametrize("chain,order,substeps", [(1, 1, 1), (3, 3, 2), (8, 5, 1)])
def test_device_kernels_equal_the_host_twins(chain, order, substeps):
    """Graphs of 1, 32, 257, 256 and 5 atoms (one workgroup's tile, one atom more, below a wave) in triclinic cells, an atom of
    infinite mass in the third, per-graph temperatures and time constants, the last thermostat off, on synthetic state with
    chains in motion: two steps, a void step (NaN energy: atoms and chains return), a prime and a parked replay.  Every array
    of the state, backups and scratch included, is bit-equal after each of the five replays."""
    B, n = len(COUNTS), sum(COUNTS)
    rs = np.random.RandomState(10 * chain + order)
    cell = np.tile(np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]]), (B, 1, 1))
    batch = np.repeat(np.arange(B), COUNTS)
    m = rs.uniform(10.0, 60.0, n)
    m[40] = np.inf
    x = np.einsum("nk,nkj->nj", rs.uniform(-1.5, 2.5, (n, 3)), cell[batch])
    temperature = np.linspace(300.0, 900.0, B)
    host = HostNHC(x, rs.normal(scale=0.004, size=(n, 3)), m, 0.5, temperature, [15.0, 30.0, 45.0, 60.0, np.inf],
                   [3.0, 93.0, 768.0, 765.0, 12.0], chain=chain, order=order, substeps=substeps, cell=cell, batch=batch,
                   log_steps=4, num_graphs=B)
    host.v[40] = 0.0
    host.f_prev[:] = rs.normal(size=(n, 3)).astype(np.float32)
    host.image[:] = rs.randint(-2, 3, (n, 3))
    host.state[0] = 6
    host.xi[:4], host.v_xi[:4] = rs.normal(scale=0.5, size=(4, chain)), rs.normal(scale=0.02, size=(4, chain))
    d = {k: _put(getattr(host, k)) for k in NAMES}
    for k in (0, 1):
        _replay_on_both(host, d, rs.normal(size=(n, 3)).astype(np.float32), rs.normal(size=B).astype(np.float32), (4321 + k, 0))
        _equal_everywhere(host, d, (chain, "step", k))
        assert (host.scale[:4] != 1.0).all() and (host.scale[4] == 1.0).all() and not host.xi[4].any()
    assert host.state.tolist() == [8, 0, 0, 0] and np.abs(host.image).max() >= 2 and not host.v[40].any()
    assert np.all(host.log[7 % 4, :, 2] == 4322) and np.all(host.log[[0, 1]] == -7.0)
    before = {k: getattr(host, k).copy() for k in ("x", "v", "image", "pos32", "f_prev", "xi", "v_xi", "log")}
    bad = rs.normal(size=B).astype(np.float32)
    bad[B - 1] = np.nan
    _replay_on_both(host, d, rs.normal(size=(n, 3)).astype(np.float32), bad, (4323, 0))
    _equal_everywhere(host, d, (chain, "void"))
    assert host.state.tolist() == [8, 256, 8, 0]
    assert all(getattr(host, k).tobytes() == v.tobytes() for k, v in before.items())
    host.state[:] = (8, 0, 0, 1)
    d["state"].copy_(_put(host.state))
    _replay_on_both(host, d, rs.normal(size=(n, 3)).astype(np.float32), rs.normal(size=B).astype(np.float32), (4324, 0))
    _equal_everywhere(host, d, (chain, "prime"))
    assert host.state.tolist() == [8, 0, 0, 0] and host.xi.tobytes() == before["xi"].tobytes()
    assert host.v.tobytes() == before["v"].tobytes() and host.f_prev.tobytes() != before["f_prev"].tobytes()
    host.state[:] = (8, PARKED, 0, 0)
    d["state"].copy_(_put(host.state))
    parked = {k: getattr(host, k).copy() for k in NAMES}
    _replay_on_both(host, d, rs.normal(size=(n, 3)).astype(np.float32), rs.normal(size=B).astype(np.float32), (4325, 0))
    _equal_everywhere(host, d, (chain, "parked"))
    assert all(getattr(host, k).tobytes() == v.tobytes() for k, v in parked.items())


# ---- the driver on 4 x 32 atoms ---------------------------------------------------------------------------------------------------
def _system():
    """Four DIFFERENT 32-atom alloy cells (their own jitter and species), Maxwell-Boltzmann velocities at T_START."""
    if "system" not in _CACHE:
        parts = [synth.fcc_alloy_atoms(reps=(2, 2, 2), seed=10 + g) for g in range(4)]
        pos, z = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
        m = np.array([rh.MASS[int(v)] for v in z])
        v = np.random.RandomState(3).normal(size=(len(m), 3)) * np.sqrt(KB * T_START / (m * AMU))[:, None]
        _CACHE["system"] = dict(pos=pos, z=z, cell=np.stack([p[1] for p in parts]), m=m, v=v, batch=np.repeat(np.arange(4), 32))
    return _CACHE["system"]


def _args(s):
    return (_put(s["z"]), _put(s["cell"].astype(np.float32)), s["pos"], s["m"], DT)


def _nhc(temperature=T_NHC, tau=TAU, model=None, **kw):
    s = _system()
    args = dict(velocities=s["v"], batch=_put(s["batch"]), num_graphs=4)
    args.update(kw)
    return DeviceNHC(model or rh._shared_model(), *_args(s), temperature=temperature, tau=tau, **args)


def _host(s, x, v, temperature=T_NHC, tau=TAU, **kw):
    return HostNHC(x, v, s["m"], DT, temperature, tau, DOF, cell=s["cell"], batch=s["batch"], log_steps=64, num_graphs=4, **kw)


def _state_bits(snap):
    return (bits(snap.positions).tobytes(), bits(snap.velocities).tobytes(), snap.images.tobytes(), snap.forces.tobytes(),
            snap.step, bits(snap.xi).tobytes(), bits(snap.v_xi).tobytes())


def _evaluator():
    s, dev = _system(), _dev()
    z, cell, pos, _, _ = _args(s)
    step = GraphedBatchMDStep(rh._shared_model(), z, cell, torch.from_numpy(pos.astype(np.float32)).to(dev), _put(s["batch"]), 4)

    def forces(p32):
        e, f = step(torch.from_numpy(np.ascontiguousarray(p32)).to(dev))
        e, f = e.cpu().numpy().copy(), f.cpu().numpy().copy()
        ok, n = step.check()
        assert ok
        return e, f, n
    return forces


def test_run_equals_the_host_driven_loop_after_every_step():
    """4 x 32 atoms at four temperatures and time constants, M = 3, order 3, 20 steps against GraphedBatchMDStep + fetch() + the
    host twins: positions, images, velocities, forces, xi, v_xi, both factors and the log row are bit-equal after EVERY
    step; `temperature_now` and `conserved` are what their definitions say; the chains moved."""
    s = _system()
    forces = _evaluator()
    host = _host(s, s["pos"], s["v"])
    host.state[3] = 1
    e, f, n = forces(host.advance().copy())
    host.finish(f, e, total=(n, 0))
    md = _nhc()
    assert md.dof.tolist() == [DOF] * 4
    first = md.fetch()
    assert first.step == 0 and np.array_equal(first.forces, host.f_prev) and not first.xi.any() and first.log.shape == (0, 4, 4)
    for k in range(20):
        e, f, n = forces(host.advance().copy())
        host.finish(f, e, total=(n, 0))
        md.run(1)
        snap = md.fetch()
        assert (snap.step, snap.halted) == (k + 1, False)
        assert np.array_equal(bits(snap.positions), bits(host.x)) and np.array_equal(bits(snap.velocities), bits(host.v)), k
        assert np.array_equal(snap.images, host.image) and np.array_equal(snap.forces, host.f_prev), k
        assert np.array_equal(bits(snap.xi), bits(host.xi)) and np.array_equal(bits(snap.v_xi), bits(host.v_xi)), k
        assert np.array_equal(bits(snap.nhc_scale), bits(host.scale)), k
        assert snap.log.shape == (1, 4, 4) and np.array_equal(bits(snap.log[0]), bits(host.log[k % 64])), k
    assert (snap.nhc_scale != 1.0).all() and (snap.v_xi != 0.0).all() and snap.xi.shape == (4, 3)
    ke = 0.5 * s["m"] * AMU * (snap.velocities ** 2).sum(axis=1)
    t_now = 2.0 * np.array([ke[32 * g:32 * (g + 1)].sum() for g in range(4)]) / (DOF * KB)
    assert np.allclose(snap.temperature_now, t_now, rtol=1e-13, atol=0.0)
    assert np.allclose(snap.log[0, :, 1], 0.5 * DOF * KB * t_now, rtol=1e-12, atol=0.0)
    assert np.array_equal(conserved(snap), (snap.log[..., 0] + snap.log[..., 1]) + snap.log[..., 3])


def _observers():
    return [Frames(stride=3, frames=16, velocities=True, images=True), MSD(stride=1, rows=32)]


def test_tau_inf_equals_device_md_nve_bit_for_bit_with_observers():
    """`DeviceNHC(tau=inf)` against `DeviceMD(friction=None)` on the same batch: positions, velocities, images, forces, the
    log's columns 0 to 2 and everything Frames and MSD recorded are bit-equal after 20 steps; xi = v_xi = E_nhc = 0 and both
    factors are exactly 1."""
    s = _system()
    ours = _nhc(tau=np.inf, observers=_observers())
    plain = DeviceMD(rh._shared_model(), *_args(s), velocities=s["v"], batch=_put(s["batch"]), num_graphs=4, observers=_observers())
    ours.run(20)
    plain.run(20)
    a, b = ours.fetch(), plain.fetch()
    assert (a.step, a.halted, b.step, b.halted) == (20, False, 20, False)
    assert _state_bits(a)[:5] == (bits(b.positions).tobytes(), bits(b.velocities).tobytes(), b.images.tobytes(), b.forces.tobytes(), 20)
    assert a.log.shape == (20, 4, 4) and np.array_equal(bits(a.log[:, :, :3]), bits(b.log)) and not a.log[:, :, 3].any()
    assert not a.xi.any() and not a.v_xi.any() and (a.nhc_scale == 1.0).all()
    assert len(a.observers) == 2 and len(a.observers[0].steps) == 7 and a.observers[1].steps.tolist() == list(range(21))
    for p, q in zip(a.observers, b.observers):
        assert _flat(p) == _flat(q)


def test_velocities_written_between_two_runs_steer_the_next_opening_factor():
    """After 3 steps `maxwell_boltzmann` (then `set_velocities` with twice those) rewrites v; the next step's opening factor,
    chains and velocities are the host twin's from the fetched state with the NEW velocities, bit for bit -- and not what
    the old velocities would have given: the opening half step takes E_kin from v, not from a number the last finish left."""
    s = _system()
    forces = _evaluator()
    md = _nhc()
    md.run(3)
    old = md.fetch()
    for write in ("maxwell_boltzmann", "set_velocities"):
        if write == "maxwell_boltzmann":
            md.maxwell_boltzmann([200.0, 400.0, 2000.0, 3000.0], seed=5)
        else:
            md.set_velocities(2.0 * old.velocities)
        start = md.fetch()
        assert not np.array_equal(start.velocities, old.velocities) and np.array_equal(bits(start.xi), bits(old.xi))
        opening = []
        for v in (start.velocities, old.velocities):
            host = _host(s, start.positions, v)
            host.image[:], host.f_prev[:], host.state[0] = start.images, start.forces, start.step
            host.xi[:], host.v_xi[:] = start.xi, start.v_xi
            e, f, n = forces(host.advance().copy())
            host.finish(f, e, total=(n, 0))
            opening.append(host.scale[:, 0].copy())
            if v is start.velocities:
                want = host
        md.run(1)
        old = md.fetch()
        assert np.array_equal(bits(old.nhc_scale), bits(want.scale)) and (opening[0] != opening[1]).all()
        assert np.array_equal(bits(old.velocities), bits(want.v)) and np.array_equal(bits(old.positions), bits(want.x))
        assert np.array_equal(bits(old.xi), bits(want.xi)) and np.array_equal(bits(old.v_xi), bits(want.v_xi))
        assert np.array_equal(bits(old.log[0]), bits(want.log[start.step % 64]))


def test_halt_on_list_overflow_and_resume_continue_to_the_same_bits():
    """An uninterrupted 30-step run at 2500 K shows the edge count of every step.  With a capacity that the list outgrows at
    step k a second driver halts there with the capacity bit in the state of step k -- chains included --, halted replays
    change nothing, resume() recaptures with more columns and the run ends bit-equal to the uninterrupted one, xi and v_xi
    and the log included.  (The overflowing replays are ordinary padded searches that report a flag.)"""
    s = _system()
    v = np.random.RandomState(8).normal(size=(len(s["m"]), 3)) * np.sqrt(KB * mdt.HOT / (s["m"] * AMU))[:, None]
    whole = _nhc(temperature=mdt.HOT, tau=50.0, velocities=v)
    snaps = []
    for _ in range(30):
        whole.run(1)
        snaps.append(whole.fetch())
    counts = [int(p.log[0, 0, 2]) for p in snaps]          # counts[k]: the list of step k (0-based), built inside replay k
    first = _evaluator()(s["pos"].astype(np.float32))[2]  # the construction evaluates the start coordinates as well
    at = [k for k in range(2, 30) if counts[k] > max([first] + counts[:k])]
    assert at, "the edge count never exceeded its running maximum: no overflow to test"
    k = at[0]
    capacity = max([first] + counts[:k])
    md = _nhc(temperature=mdt.HOT, tau=50.0, velocities=v, capacity=capacity)
    assert md.capacity == capacity
    md.run(30)
    snap = md.fetch()
    assert snap.halted and snap.step == k and snap.halt_step == k and (snap.halt_code & HALT_CAPACITY)
    assert not (snap.halt_code & HALT_NONFINITE)
    assert _state_bits(snap) == _state_bits(snaps[k - 1]) and snap.xi.any() and snap.log.shape[0] == k
    assert np.array_equal(bits(snap.log), bits(np.concatenate([p.log for p in snaps[:k]])))
    md.run(3)                                            # halted: replays change nothing
    again = md.fetch()
    assert _state_bits(again) == _state_bits(snap) and again.log.shape[0] == 0 and again.halted
    md.resume()
    assert md.capacity > capacity
    md.run(30 - k)
    end = md.fetch()
    assert (end.step, end.halted) == (30, False) and _state_bits(end) == _state_bits(snaps[29])
    assert np.array_equal(bits(end.log), bits(np.concatenate([p.log for p in snaps[k:]])))
    assert np.array_equal(bits(end.nhc_scale), bits(snaps[29].nhc_scale))


def test_a_replay_has_six_integrator_launches_for_device_mds_four_and_no_copies():
    """The device activity of two replays of `DeviceNHC` and of `DeviceMD` (NVE) on the same batch, from the captures' own
    lists: the six kernels of the step are there once per replay, `md_advance_kernel` and `md_log_kernel` are gone, everything
    else is DeviceMD's, and there is no memcpy or memset."""
    from torch.profiler import ProfilerActivity, profile
    s = _system()
    plain = DeviceMD(rh._shared_model(), *_args(s), velocities=s["v"], batch=_put(s["batch"]), num_graphs=4)
    ours = _nhc()

    def events(driver):
        driver.run(2)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            driver.run(2)
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    a, b = events(ours), events(plain)
    assert sum(a.values()) > 0, "the profiler recorded no device activity for graph launches"
    assert not [k for k in a if "memcpy" in k.lower() or "memset" in k.lower()]
    named = lambda c, word: sum(v for k, v in c.items() if word in k)
    for kernel in ("nhc_open_kernel", "nhc_advance_kernel", "md_finish_atoms_kernel", "nhc_close_kernel", "nhc_scale_kernel",
                   "md_commit_kernel"):
        assert named(a, kernel) == 2, (kernel, a)
    for kernel in ("md_advance_kernel", "md_log_kernel"):
        assert named(a, kernel) == 0 and named(b, kernel) == 2, (kernel, a, b)
    assert named(b, "nhc_") == 0 and sum(a.values()) == sum(b.values()) + 4, (a - b, b - a)
    ours_only = Counter({k: v for k, v in a.items() if "nhc_" in k})
    theirs_only = Counter({k: v for k, v in b.items() if "md_advance_kernel" in k or "md_log_kernel" in k})
    assert a - ours_only == b - theirs_only


def test_ase_hand_off_round_trip():
    """`from_atoms` on a duck-typed periodic structure (ASE's velocity unit converted), two steps, `to_atoms`: positions and
    velocities of the snapshot arrive in the structure; the default dof is 3 n - 3."""
    s = _system()
    p = slice(0, 32)
    atoms = rh._FakeAtoms(s["pos"][p], s["z"][p], s["cell"][0], s["m"][p], s["v"][p] * ASE_TIME_FS)
    md = DeviceNHC.from_atoms(atoms, rh._shared_model(), DT, temperature=600.0, tau=30.0, chain=2)
    start = md.fetch()
    assert md.num_graphs == 1 and md.dof.tolist() == [93.0] and start.xi.shape == (1, 2)
    assert np.array_equal(start.positions, s["pos"][p]) and np.allclose(start.velocities, s["v"][p], rtol=1e-15, atol=0)
    md.run(2)
    out = rh._FakeAtoms(np.zeros((32, 3)), s["z"][p], s["cell"][0], s["m"][p], None)
    snap = md.to_atoms(out)
    assert snap.step == 2 and not snap.halted and snap.v_xi.all() and snap.log.shape == (2, 1, 4)
    assert np.array_equal(out.positions, snap.positions) and np.array_equal(out.get_velocities(), snap.velocities * ASE_TIME_FS)
    assert abs(snap.temperature_now[0] / T_START - 1.0) < 0.5
