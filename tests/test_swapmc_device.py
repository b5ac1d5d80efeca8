"""GPU: `hermnet_amd.swapmc.DeviceSwapMD` -- species-swap Monte Carlo inside the replayed hipGraph.  The kernels against the
library's host twins on synthetic state; a run against the host-driven loop it replaces after every replay; every decision of
a run recomputed on the host from `swap_log`; `swaps=0` against `DeviceMD`; the observers; halt on a void trial and resume."""
import warnings

import numpy as np
import pytest
import torch

from hermnet_amd import _lib, synth
from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.md import HALT_NONFINITE, DeviceMD
from hermnet_amd.observe import MSD, RDF, Frames
from hermnet_amd.swapmc import DeviceSwapMD
from md_reference import AMU, KB, advance_np, bits
from observe_reference import NumpyRDF, state_words
from swapmc_reference import HostSwapMC, decide, pick_pair, tables, trial_uniform
import resident_helpers as rh
from resident_helpers import _flat, _put

pytestmark = pytest.mark.gpu

DT, FRICTION, SEED, MARGIN = 1.0, 0.02, (6 << 32) + 41, 1e-9
T_MD = 1500.0
# K, per graph: a decade of kB T_mc (0.013 to 0.13 eV), so that whatever one swap changes in this model's E_pot of a
# 32-atom cell, some graph rejects uphill trials and some graph accepts them.  Seen on an MI355X in the 60-replay run
# below: |d| from 0.0016 to 0.23 eV, 77 accepted and 43 rejected trials, none within the margin of its threshold.
T_MC = np.array([150.0, 400.0, 800.0, 1500.0])
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


# ---- 1. the kernels against the host twins ----------------------------------------------------------------------------------------
NAMES = ["x", "v", "x0", "v0", "image", "image0", "f_prev", "kick", "batch", "cell", "inv", "pos32", "state", "graph_ptr",
         "half_mass", "ke_atom", "log", "mc", "cand", "cand_ptr", "beta", "e_ref", "pair", "dval", "outcome", "attempts",
         "accepts", "swap_log"]
# (graphs, atoms per graph, what each graph's trial is to be: "down" d < 0, "draw" accepted by the draw, "reject", None: the
# graph has one species and is not tried)
KERNEL_CASES = [(5, 257, ("down", None, "reject", "draw", "reject")), (3, 63, ("reject", "draw", None)), (2, 2, ("down", None)),
                (2, 2, ("reject", None))]


def _replay_on_both(host, d, f_new, energy, total, capacity=5000):
    """One hermnet_swapmc_advance + hermnet_swapmc_finish and their host twins on the same state and evaluation."""
    lib, P, stream = _lib.load(), _lib.ptr, torch.cuda.current_stream().cuda_stream
    n, B = host.n, host.B
    tables_d = (P(d["cand"]), P(d["cand_ptr"]), host.S, host.num_cand)
    atoms = [P(d[k]) for k in ("x", "v", "x0", "v0", "image", "image0", "f_prev", "kick")]
    _lib.check(lib.hermnet_swapmc_advance(n, B, host.flags, host.dt, host.seed, *atoms, None, None, P(d["batch"]), P(d["cell"]),
                                          P(d["inv"]), P(d["pos32"]), P(d["state"]), P(d["mc"]), P(d["graph_ptr"]), *tables_d,
                                          stream), "advance")
    f_d, e_d, t_d = _put(f_new), _put(energy), _put(np.array(total, dtype=np.int64))
    _lib.check(lib.hermnet_swapmc_finish(n, B, P(d["graph_ptr"]), P(d["batch"]), P(f_d), P(e_d), P(t_d), capacity, host.interval,
                                         host.swaps, host.seed, *atoms, P(d["half_mass"]), P(d["pos32"]), P(d["ke_atom"]),
                                         P(d["beta"]), P(d["e_ref"]), P(d["mc"]), *tables_d, P(d["pair"]), P(d["dval"]),
                                         P(d["outcome"]), P(d["attempts"]), P(d["accepts"]), P(d["swap_log"]), host.swap_rows,
                                         P(d["log"]), host.log_steps, P(d["state"]), stream), "finish")
    torch.cuda.synchronize()
    host.advance()
    host.finish(f_new, energy, total=total, capacity=capacity)


def _equal_everywhere(host, d, what):
    for k in NAMES:
        got, want = d[k].cpu().numpy(), getattr(host, k)
        same = np.array_equal(bits(got), bits(want)) if want.dtype == np.float64 else np.array_equal(got, want)
        assert same, (what, k)


@pytest.mark.parametrize("case", range(len(KERNEL_CASES)))
def test_device_kernels_equal_the_host_twins(case):
    """(5, 257), (3, 63) and (2, 2) graphs x atoms, NVE, on synthetic state from t = 5, left = 2 at step 6 with
    swap_interval = 7: a trial with an accepted, a rejected and a not-tried graph in ONE launch (the energies are made so;
    each decision is further than 1e-9 from its threshold on the host values), a second trial, the MD step behind them (it
    makes step 7: left = swaps again), a void trial (NaN energy) and a prime.  Every array of the state, scratch included, is
    bit-equal after each of the five replays."""
    B, n_g, kinds = KERNEL_CASES[case]
    n = B * n_g
    rs = np.random.RandomState(100 * B + n_g + case)
    cell = np.tile(np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]]), (B, 1, 1))
    batch = np.repeat(np.arange(B), n_g)
    z = rs.choice([13, 28, 29], size=n)
    for g, kind in enumerate(kinds):
        z[batch == g] = 28 if kind is None else z[batch == g]
        if kind is not None:
            z[g * n_g:g * n_g + 2] = [13, 29]             # (two species at the least)
    m = rs.uniform(10.0, 60.0, n)
    if n_g > 100:
        m[100] = np.inf
    x = np.einsum("nk,nkj->nj", rs.uniform(-1.5, 2.5, (n, 3)), cell[batch])
    host = HostSwapMC(x, rs.normal(scale=0.02, size=(n, 3)), z, m, 0.5, 7, 2, np.linspace(300.0, 900.0, B), cell=cell, batch=batch,
                      seed=SEED, log_steps=4, swap_rows=4, num_graphs=B)
    host.v[~np.isfinite(m)] = 0.0
    host.f_prev[:] = rs.normal(size=(n, 3)).astype(np.float32)
    host.image[:] = rs.randint(-2, 3, (n, 3))
    host.state[0], host.mc[:], host.e_ref[:] = 6, (5, 2), rs.normal(size=B)
    host.attempts[:], host.accepts[:] = 10 + np.arange(B), 3 + np.arange(B)
    d = {k: _put(getattr(host, k)) for k in NAMES}
    want = {"down": 2, "draw": 2, "reject": 1, None: 0}
    for t in (5, 6):
        energy = np.zeros(B, dtype=np.float32)
        for g, kind in enumerate(kinds):
            log_u = np.log(trial_uniform(SEED, t, g))
            delta = {"down": 1.0, "draw": 0.5 * log_u, "reject": 2.0 * log_u - 1.0, None: 0.0}[kind]
            energy[g] = np.float32(host.e_ref[g] - delta / host.beta[g])
            if kind is not None:
                _, delta, log_u, yes = decide(SEED, t, g, host.beta[g], energy[g], host.e_ref[g])
                assert abs(log_u - delta) > MARGIN and yes == (kind != "reject") and (delta >= 0.0) == (kind == "down")
        _replay_on_both(host, d, rs.normal(size=(n, 3)).astype(np.float32), energy, (4321, 0))
        _equal_everywhere(host, d, (case, t))
        assert host.swap_log[t % 4, :, 3].tolist() == [want[k] for k in kinds] and host.mc.tolist() == [t + 1, 6 - t]
    assert host.state.tolist() == [6, 0, 0, 0]
    _replay_on_both(host, d, rs.normal(size=(n, 3)).astype(np.float32), rs.normal(size=B).astype(np.float32), (4322, 0))
    _equal_everywhere(host, d, (case, "md"))
    assert host.state.tolist() == [7, 0, 0, 0] and host.mc.tolist() == [7, 2] and np.abs(host.image).max() >= 2
    assert np.all(host.log[6 % 4, :, 2] == 4322) and np.all(host.log[[0, 1, 3]] == -7.0)
    before = {k: getattr(host, k).copy() for k in ("x", "image", "pos32", "f_prev", "e_ref", "swap_log", "attempts")}
    bad = rs.normal(size=B).astype(np.float32)
    bad[B - 1] = np.nan
    _replay_on_both(host, d, rs.normal(size=(n, 3)).astype(np.float32), bad, (4323, 0))
    _equal_everywhere(host, d, (case, "void"))
    assert host.state.tolist() == [7, 256, 7, 0] and host.mc.tolist() == [7, 2]
    assert all(getattr(host, k).tobytes() == v.tobytes() for k, v in before.items())
    host.state[:] = (7, 0, 0, 1)
    d["state"].copy_(_put(host.state))
    _replay_on_both(host, d, rs.normal(size=(n, 3)).astype(np.float32), rs.normal(size=B).astype(np.float32), (4324, 0))
    _equal_everywhere(host, d, (case, "prime"))
    assert host.state.tolist() == [7, 0, 0, 0] and host.mc.tolist() == [7, 2]


# ---- the driver on 4 x 32 atoms ---------------------------------------------------------------------------------------------------
def _system():
    """Four DIFFERENT 32-atom alloy cells (their own jitter and species), Maxwell-Boltzmann velocities at T_MD."""
    if "system" not in _CACHE:
        parts = [synth.fcc_alloy_atoms(reps=(2, 2, 2), seed=10 + g) for g in range(4)]
        pos, z = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
        m = np.array([rh.MASS[int(v)] for v in z])
        v = np.random.RandomState(3).normal(size=(len(m), 3)) * np.sqrt(KB * T_MD / (m * AMU))[:, None]
        _CACHE["system"] = dict(pos=pos, z=z, cell=np.stack([p[1] for p in parts]), m=m, v=v, batch=np.repeat(np.arange(4), 32))
    return _CACHE["system"]


def _args(s):
    return (_put(s["z"]), _put(s["cell"].astype(np.float32)), s["pos"], s["m"], DT)


def _swapmd(interval=2, swaps=2, friction=None, model=None, cls=DeviceSwapMD, **kw):
    s = _system()
    args = dict(seed=SEED, velocities=s["v"], batch=_put(s["batch"]), num_graphs=4)
    if friction is not None:
        args.update(friction=friction, temperature=T_MD)
    args.update(kw)
    if cls is DeviceMD:
        return DeviceMD(model or rh._shared_model(), *_args(s), **args)
    return DeviceSwapMD(model or rh._shared_model(), *_args(s), interval, swaps, mc_temperature=T_MC, **args)


def _state_bits(snap):
    return (bits(snap.positions).tobytes(), bits(snap.velocities).tobytes(), snap.images.tobytes(), snap.forces.tobytes(),
            snap.step, snap.swap_trials, snap.swaps_left, snap.swap_attempts.tobytes(), snap.swap_accepts.tobytes(),
            bits(snap.energy_ref).tobytes())


def _evaluator(model=None):
    s, dev = _system(), _dev()
    z, cell, pos, _, _ = _args(s)
    step = GraphedBatchMDStep(model or rh._shared_model(), z, cell, torch.from_numpy(pos.astype(np.float32)).to(dev),
                              _put(s["batch"]), 4)

    def forces(p32):
        e, f = step(torch.from_numpy(np.ascontiguousarray(p32)).to(dev))
        e, f = e.cpu().numpy().copy(), f.cpu().numpy().copy()
        ok, n = step.check()
        assert ok
        return e, f, n
    return forces


@pytest.mark.parametrize("friction", [None, FRICTION], ids=["nve", "langevin"])
def test_run_equals_the_host_driven_loop_after_every_replay(friction):
    """4 x 32 atoms, swap_interval = 2, swaps = 2, 24 replays against GraphedBatchMDStep + fetch() + the host twins: positions,
    images, velocities, forces, energy_ref, the words, the counters, the MD log row and the swap_log row are bit-equal after
    EVERY replay.  NVE: every advance is hermnet_host_swapmc_advance.  Langevin: the device's Gaussians differ from the
    host's in the last digits (its float64 log / cos / sqrt; tests/test_md_device.py), so an MD step's advance is md_step.h's
    numpy transcription fed with the Gaussians of the device's own hermnet_md_noise; trials and the prime stay the twin's."""
    s = _system()
    forces = _evaluator()
    host = HostSwapMC(s["pos"], s["v"], s["z"], s["m"], DT, 2, 2, T_MC, cell=s["cell"], batch=s["batch"], friction=friction,
                      temperature=None if friction is None else T_MD, seed=SEED, log_steps=64, swap_rows=64, num_graphs=4)
    cell_atom = host.cell.astype(np.float64).reshape(-1, 3, 3)[host.batch]
    inv_atom = host.inv.reshape(-1, 3, 3)[host.batch]

    def advance():
        if friction is None or host.kind() != "md":
            return host.advance().copy()
        gauss = torch.zeros(host.n, 3, dtype=torch.float64, device=_dev())
        _lib.call("hermnet_md_noise", SEED, int(host.state[0]), host.n, None, _lib.ptr(gauss), torch.cuda.current_stream().cuda_stream)
        host.x0[:], host.v0[:], host.image0[:] = host.x, host.v, host.image
        advance_np(host.x, host.v, host.image, host.f_prev, host.kick, host.dt, host.c1[host.batch], host.sigma,
                   gauss.cpu().numpy(), cell_atom, inv_atom)
        host.pos32[:] = host.x.astype(np.float32)
        return host.pos32.copy()

    host.state[3] = 1
    e, f, n = forces(advance())
    host.finish(f, e, total=(n, 0))
    md = _swapmd(friction=friction)
    first = md.fetch()
    assert first.step == 0 and np.array_equal(first.forces, host.f_prev) and np.array_equal(bits(first.energy_ref), bits(host.e_ref))
    outcomes = []
    for k in range(24):
        kind, step, t = host.kind(), int(host.state[0]), int(host.mc[0])
        assert kind == ("md" if k % 4 < 2 else "trial")
        e, f, n = forces(advance())
        host.finish(f, e, total=(n, 0))
        md.run(1)
        snap = md.fetch()
        assert (snap.step, snap.halted, snap.swap_trials, snap.swaps_left) == (int(host.state[0]), False, int(host.mc[0]), int(host.mc[1])), k
        assert np.array_equal(bits(snap.positions), bits(host.x)) and np.array_equal(bits(snap.velocities), bits(host.v)), k
        assert np.array_equal(snap.images, host.image) and np.array_equal(snap.forces, host.f_prev), k
        assert np.array_equal(bits(snap.energy_ref), bits(host.e_ref)), k
        assert np.array_equal(snap.swap_attempts, host.attempts) and np.array_equal(snap.swap_accepts, host.accepts), k
        if kind == "md":
            assert snap.log.shape == (1, 4, 3) and snap.swap_log.shape == (0, 4, 4), k
            assert np.array_equal(bits(snap.log[0]), bits(host.log[step % 64])), k
        else:
            assert snap.log.shape == (0, 4, 3) and snap.swap_log.shape == (1, 4, 4), k
            assert np.array_equal(bits(snap.swap_log[0]), bits(host.swap_log[t % 64])), k
            outcomes += snap.swap_log[0, :, 3].tolist()
    assert snap.step == 12 and snap.swap_trials == 12 and set(outcomes) == {1.0, 2.0}


def _long_run():
    """The uninterrupted 60-replay NVE run the tests below refer to, once: (the driver, its snapshot, the 30 swap_log rows)."""
    if "long" not in _CACHE:
        md = _swapmd()
        assert md.replays_for(30) == 58 and md.replays_for(1) == 1 and md.replays_for(0) == 0
        md.run(60)
        with pytest.raises(RuntimeError, match="fetch"):
            md.replays_for(1)
        snap = md.fetch()
        assert md.replays_for(2) == 2 and md.replays_for(3) == 5
        _CACHE["long"] = (md, snap, snap.swap_log)
    return _CACHE["long"]


def test_every_decision_of_a_run_is_the_hosts_from_the_swap_log():
    """60 replays = 30 time steps and 30 trial replays of 4 graphs.  Every row's pair is the host's pick from (seed, t, g) and
    the candidate tables, its atoms are of two species and of graph g; every outcome is the host's decision from the row's d,
    beta and the host's Philox (a decision within 1e-9 of its threshold is left out).  Afterwards `energy_ref` and `forces`
    equal, bit for bit, a fresh GraphedBatchMDStep evaluation of the fetched positions -- whichever trial each graph last
    accepted.  Seen on an MI355X with T_MC above: 77 accepted, 43 rejected, none within the margin (asserted: both occur;
    the counts are printed)."""
    s = _system()
    md, snap, log = _long_run()
    assert (snap.step, snap.halted, snap.swap_trials, snap.swaps_left) == (30, False, 30, 0) and log.shape == (30, 4, 4)
    cand, ptr, S = tables(s["z"], s["m"], s["batch"], 4)
    assert np.array_equal(md.cand.cpu().numpy(), cand) and np.array_equal(md.cand_ptr.cpu().numpy(), ptr) and md.num_species == S
    beta = 1.0 / (KB * T_MC)
    assert np.array_equal(bits(md.beta.cpu().numpy()), bits(beta))
    accepted = rejected = omitted = 0
    sizes = []
    for t in range(30):
        for g in range(4):
            i, j, d, o = log[t, g]
            assert (int(i), int(j)) == pick_pair(SEED, t, g, cand, ptr[g]) and o in (1.0, 2.0)
            assert s["z"][int(i)] != s["z"][int(j)] and s["batch"][int(i)] == s["batch"][int(j)] == g
            delta = -beta[g] * d
            log_u = np.log(trial_uniform(SEED, t, g))
            sizes.append(abs(d))
            if abs(log_u - delta) <= MARGIN:
                omitted += 1
                continue
            assert (o == 2.0) == bool(delta >= 0.0 or log_u < delta), (t, g, d, delta, log_u)
            accepted += o == 2.0
            rejected += o == 1.0
    print("DeviceSwapMD 4 x 32, T_mc %s, 30 trial replays: %d accepted, %d rejected, %d within the margin; |d| from %.3g to %.3g eV"
          % (T_MC.tolist(), accepted, rejected, omitted, min(sizes), max(sizes)))
    assert omitted <= 1 and accepted >= 1 and rejected >= 1
    assert np.array_equal(snap.swap_attempts, [30] * 4) and snap.swap_accepts.sum() >= accepted
    assert np.array_equal(snap.swap_accepts, (log[:, :, 3] == 2.0).sum(axis=0))
    e, f, _ = _evaluator()(snap.positions.astype(np.float32))
    assert np.array_equal(bits(snap.energy_ref), bits(e.astype(np.float64))) and np.array_equal(snap.forces, f)
    assert snap.log.shape == (30, 4, 3) and np.all(np.isfinite(snap.log))


def _observers(rows=32):
    return [Frames(stride=3, frames=16, velocities=True, images=True), RDF(r_max=3.5, bins=35, stride=2), MSD(stride=1, rows=rows)]


def test_no_swaps_equals_device_md_bit_for_bit_with_observers():
    """`DeviceSwapMD(swaps=0)` against `DeviceMD` on the same batch and seed: positions, velocities, images, forces, the log
    and everything Frames, RDF and MSD recorded are bit-equal after 20 Langevin steps; nothing was tried."""
    ours = _swapmd(swaps=0, friction=FRICTION, observers=_observers())
    plain = _swapmd(cls=DeviceMD, friction=FRICTION, observers=_observers())
    ours.run(20)
    plain.run(20)
    a, b = ours.fetch(), plain.fetch()
    assert (a.step, a.halted, b.step, b.halted) == (20, False, 20, False)
    assert _state_bits(a)[:5] == (bits(b.positions).tobytes(), bits(b.velocities).tobytes(), b.images.tobytes(), b.forces.tobytes(), 20)
    assert np.array_equal(bits(a.log), bits(b.log)) and a.log.shape == (20, 4, 3)
    assert (a.swap_trials, a.swaps_left) == (0, 0) and not a.swap_attempts.any() and a.swap_log.shape == (0, 4, 4)
    assert np.array_equal(bits(a.energy_ref), bits(a.log[-1, :, 0]))
    assert len(a.observers) == 3 and len(a.observers[0].steps) == 7 and a.observers[1].counts.sum() > 0
    for p, q in zip(a.observers, b.observers):
        assert _flat(p) == _flat(q)


def test_observers_sample_behind_committed_md_steps_only():
    """swaps = 2, 40 replays = 20 time steps: the sample steps of Frames, RDF and MSD are those of the unswapped driver's 20
    steps; the RDF counts equal numpy's over the configurations a second, unobserved driver shows behind each committed MD
    step (and at the start); the trajectory is the unobserved driver's."""
    s = _system()
    ours = _swapmd(observers=_observers(rows=64))          # (run's room check counts every replay as a sample)
    ours.run(40)
    a = ours.fetch()
    plain = _swapmd(cls=DeviceMD, observers=_observers())
    plain.run(20)
    b = plain.fetch()
    assert a.step == b.step == 20 and a.swap_trials == 20 and a.swap_accepts.sum() > 0
    f, r, m = a.observers
    assert f.steps.tolist() == b.observers[0].steps.tolist() == list(range(0, 21, 3))
    assert m.steps.tolist() == b.observers[2].steps.tolist() == list(range(21))
    assert np.array_equal(r.samples, b.observers[1].samples) and r.samples.tolist() == [11] * 4 and not r.skipped.any()
    walker = _swapmd()
    ptr = np.searchsorted(s["batch"], np.arange(5))
    c32 = s["cell"].astype(np.float32)
    ref = NumpyRDF(s["z"], ptr, 3.5, 35, 2)
    snap = walker.fetch()
    ref.offer(state_words(0), snap.positions, c32, np.linalg.inv(c32.astype(np.float64)))
    for _ in range(40):
        step = snap.step
        walker.run(1)
        snap = walker.fetch()
        if snap.step != step:
            ref.offer(state_words(snap.step), snap.positions, c32, np.linalg.inv(c32.astype(np.float64)))
    assert _state_bits(snap) == _state_bits(a)
    assert np.array_equal(r.counts, ref.counts) and r.counts.sum() > 0 and np.array_equal(r.samples, ref.samples)


def test_halt_on_a_void_trial_and_resume_continue_to_the_same_bits():
    """run(7) and fetch() stand in the middle of a block (t = 3, one trial left).  A weight written through `.data` makes
    the stale-weight guard answer NaN: the next replay, a trial, is void -- the halt is recorded, the words, the counters,
    positions and forces are the fetched ones bit for bit, nothing is logged.  With the weight restored, resume()
    recaptures, its prime leaves (t, left) alone, the same trial is drawn, and the run ends bit-equal to an uninterrupted
    one -- swap_log rows included.  (The handled non-finite halt of test_md_device.py; nothing faults.)"""
    model = rh._model(seed=9)
    whole = _swapmd(model=model)
    whole.run(11)
    mid = whole.fetch()
    whole.run(13)
    end = whole.fetch()
    assert (mid.step, mid.swap_trials, mid.swaps_left) == (6, 5, 1) and (end.step, end.swap_trials, end.swaps_left) == (12, 12, 0)
    md = _swapmd(model=model)
    md.run(7)
    good = md.fetch()
    assert (good.step, good.swap_trials, good.swaps_left) == (4, 3, 1)
    p_ = [p for n, p in model.named_parameters() if n.endswith("update_layer.xvec_proj.2.weight")][1]
    saved = p_.data.clone()
    p_.data.mul_(1.5)
    md.run(5)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        snap = md.fetch()
    assert any("resume()" in str(w.message) for w in rec)
    assert snap.halted and snap.halt_code == HALT_NONFINITE and snap.halt_step == 4
    assert _state_bits(snap) == _state_bits(good) and snap.swap_log.shape[0] == 0 and snap.log.shape[0] == 0
    p_.data.copy_(saved)
    assert md.stale()
    with pytest.raises(RuntimeError, match="resume"):
        md.run(1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        md.resume()
    md.run(4)
    again = md.fetch()
    assert _state_bits(again) == _state_bits(mid) and again.swap_log.shape[0] == 2
    assert np.array_equal(bits(again.swap_log), bits(mid.swap_log[3:5]))
    md.run(13)
    last = md.fetch()
    assert (last.step, last.halted) == (end.step, False) and _state_bits(last) == _state_bits(end)
    assert np.array_equal(bits(last.swap_log), bits(end.swap_log)) and np.array_equal(bits(last.log), bits(end.log))
    assert last.swap_log.shape == (7, 4, 4) and last.log.shape == (6, 4, 3)


def test_ase_hand_off_for_one_structure_and_for_a_list():
    """`from_atoms` on a list builds the batch through `stack_atoms` (ASE's velocity unit converted); after 6 replays (two
    steps, two trials, two steps: a new block is due) `to_atoms` writes the graphs back in order; one structure goes through
    `DeviceMD`'s hand-off."""
    from hermnet_amd.md import ASE_TIME_FS
    s = _system()
    parts = [slice(32 * g, 32 * (g + 1)) for g in range(4)]
    atoms = [rh._FakeAtoms(s["pos"][p], s["z"][p], s["cell"][g], s["m"][p], s["v"][p] * ASE_TIME_FS) for g, p in enumerate(parts)]
    md = DeviceSwapMD.from_atoms(atoms, rh._shared_model(), DT, 2, 2, mc_temperature=T_MC, seed=SEED)
    start = md.fetch()
    assert np.array_equal(start.positions, s["pos"]) and np.allclose(start.velocities, s["v"], rtol=1e-15, atol=0)
    md.run(6)
    end = md.to_atoms(atoms)
    assert (end.step, end.swap_trials, end.swaps_left) == (4, 2, 2) and end.swap_attempts.tolist() == [2] * 4
    for g, p in enumerate(parts):
        assert np.array_equal(atoms[g].positions, end.positions[p])
        assert np.array_equal(atoms[g].get_velocities(), end.velocities[p] * ASE_TIME_FS)
    with pytest.raises(ValueError, match="list of 4"):
        md.to_atoms(atoms[:3], snapshot=end)
    one = DeviceSwapMD.from_atoms(atoms[0], rh._shared_model(), DT, 1, 1, mc_temperature=300.0, seed=SEED)
    one.run(2)
    out = rh._FakeAtoms(np.zeros((32, 3)), s["z"][parts[0]], s["cell"][0], s["m"][parts[0]], None)
    snap = one.to_atoms(out)
    assert (snap.step, snap.swap_trials, one.num_graphs) == (1, 1, 1) and np.array_equal(out.positions, snap.positions)
    assert snap.swap_log.shape == (1, 1, 4) and snap.swap_log[0, 0, 3] in (1.0, 2.0)
