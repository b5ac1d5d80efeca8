"""GPU: `hermnet_amd.remd.DeviceREMD` -- temperature replica exchange inside the replayed hipGraph.  The kernels against the
library's host twin; a ladder that never exchanges against `DeviceMD` bit for bit; every decision of a run recomputed on the
host from the log; what an accepted swap does to the velocities; determinism, halt and resume; the refusals."""
import types

import numpy as np
import pytest
import torch

from hermnet_amd import _lib, synth
from hermnet_amd.md import HALT_CAPACITY, DeviceMD
from hermnet_amd.remd import DeviceREMD
from md_reference import AMU, KB, bits
from remd_reference import HostREMD, attempt_of, decide, ladder, pair_uniform
from resident_helpers import _FakeAtoms, _shared_model

pytestmark = pytest.mark.gpu

MASS = {13: 26.9815, 28: 58.6934, 29: 63.546}
DT, FRICTION, SEED, MARGIN = 1.0, 0.02, (5 << 32) + 77, 1e-9
# K.  A ratio of 1.1 between rungs (2000, 2200, 2420, 2662 K) gave 29 accepted pairs and 1 rejected one in the 40-step run
# below: this model's E_pot differs by some 0.2 eV between replicas, against 1 / (beta_r - beta_(r+1)) = 1.9 eV there.  With
# a ratio of 4/3 the same run has 26 accepted and 4 rejected (MI355X), nearest |log u - delta| = 0.06.
LADDER = np.array([1200.0, 1600.0, 2100.0, 2800.0])
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


# ---- 1. the kernels against the host twin -----------------------------------------------------------------------------------------
def _on_device(host, dev):
    names = ["x", "v", "x0", "v0", "image", "image0", "f_prev", "kick", "c1", "sigma", "batch", "cell", "inv", "pos32", "state",
             "graph_ptr", "half_mass", "ke_atom", "log", "beta", "up", "down", "sigma_table", "rung", "replica_at", "rung_new",
             "vscale", "outcome", "attempts", "accepts"]
    return {k: None if getattr(host, k) is None else torch.from_numpy(getattr(host, k).copy()).to(dev) for k in names}


# (replicas, atoms per replica, step, the way each pair of the step's attempt is to go, in ascending r)
KERNEL_CASES = [(5, 257, 6, ("up", "reject")), (5, 257, 7, ("draw", "up")), (3, 63, 9, ("draw",)), (2, 1, 4, ("reject",))]


def _one_step_on_both(R, n_rep, step, kinds):
    """One hermnet_md_advance + hermnet_remd_finish (interval 1: attempt `step` falls on step `step`) and their host twins
    on the same synthetic state, forces and energies; the energies are made so that the pairs go as `kinds` says.  Returns
    (host, the device's arrays, the host's decisions)."""
    dev, lib, P = _dev(), _lib.load(), _lib.ptr
    n = R * n_rep
    rs = np.random.RandomState(R * 1000 + n_rep + step)
    temps = np.linspace(300.0, 500.0, R)
    cell = np.tile(np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]]), (R, 1, 1))
    batch = np.repeat(np.arange(R), n_rep)
    x = np.einsum("nk,nkj->nj", rs.uniform(-1.5, 2.5, (n, 3)), cell[batch])
    m_rep = rs.uniform(10.0, 60.0, n_rep)
    if n_rep > 100:
        m_rep[100] = np.inf
    host = HostREMD(x, rs.normal(scale=0.02, size=(n, 3)), np.tile(m_rep, R), 0.5, temps, FRICTION, 1, seed=SEED, log_steps=4,
                    cell=cell)
    host.v[~np.isfinite(np.tile(m_rep, R))] = 0.0
    host.f_prev[:] = rs.normal(size=(n, 3)).astype(np.float32)
    host.state[0] = step
    # an assignment that is not the identity, with its sigma and counters that are not zero
    host.rung[:] = rs.permutation(R)
    host.replica_at[host.rung] = np.arange(R)
    host.sigma[:] = host.sigma_table[host.rung].reshape(-1)
    host.attempts[:], host.accepts[:] = 10 + np.arange(R - 1), 3 + np.arange(R - 1)
    # energies: pair r's delta is +1 ("up"), log(u) / 2 ("draw": negative, above log u) or 2 log(u) - 1 ("reject")
    pairs = [r for r in range(R - 1) if r % 2 == step % 2]
    assert len(pairs) == len(kinds)
    energy = rs.normal(size=R).astype(np.float32)
    for r, kind in zip(pairs, kinds):
        log_u = np.log(pair_uniform(SEED, step, r))
        delta = {"up": 1.0, "draw": 0.5 * log_u, "reject": 2.0 * log_u - 1.0}[kind]
        ga, gb = host.replica_at[r], host.replica_at[r + 1]
        energy[ga] = np.float32(energy[gb] + delta / (host.beta[r] - host.beta[r + 1]))
    decisions = decide(SEED, step, 1, host.beta, energy, host.replica_at)
    for (r, _, _, delta, log_u, yes), kind in zip(decisions, kinds):
        assert abs(log_u - delta) > MARGIN
        assert (kind == "up") == (delta >= 0.0) and yes == (kind != "reject"), (r, kind, delta, log_u)
    f_new, total = rs.normal(size=(n, 3)).astype(np.float32), np.array([4321, 0], dtype=np.int64)
    d = _on_device(host, dev)
    stream = torch.cuda.current_stream().cuda_stream
    f_d, e_d, t_d = (torch.from_numpy(a).to(dev) for a in (f_new, energy, total))
    _lib.check(lib.hermnet_md_advance(n, R, host.flags, host.dt, host.seed, P(d["x"]), P(d["v"]), P(d["x0"]), P(d["v0"]),
                                      P(d["image"]), P(d["image0"]), P(d["f_prev"]), P(d["kick"]), P(d["c1"]), P(d["sigma"]),
                                      P(d["batch"]), P(d["cell"]), P(d["inv"]), P(d["pos32"]), P(d["state"]), stream), "advance")
    _lib.check(lib.hermnet_remd_finish(n, R, P(d["graph_ptr"]), P(f_d), P(e_d), P(t_d), 5000, 1, host.seed, P(d["x"]), P(d["v"]),
                                       P(d["x0"]), P(d["v0"]), P(d["image"]), P(d["image0"]), P(d["f_prev"]), P(d["kick"]),
                                       P(d["half_mass"]), P(d["pos32"]), P(d["ke_atom"]), P(d["beta"]), P(d["up"]), P(d["down"]),
                                       P(d["sigma_table"]), P(d["sigma"]), P(d["rung"]), P(d["replica_at"]), P(d["rung_new"]),
                                       P(d["vscale"]), P(d["outcome"]), P(d["attempts"]), P(d["accepts"]), P(d["log"]), 4,
                                       P(d["state"]), stream), "finish")
    torch.cuda.synchronize()
    host.advance()
    host.finish(f_new, energy, total=total, capacity=5000)
    return host, {k: None if t is None else t.cpu().numpy() for k, t in d.items()}, decisions


def test_device_kernels_equal_the_host_twin():
    """5 x 257 (two attempts of either parity), 3 x 63 and 2 x 1 atoms, from an assignment that is not the identity: rung,
    replica_at, counters, sigma, state, f_prev, image and the log's columns 0 and 2-4 are bit-equal; x, v and E_kin carry this
    step's Gaussians (the device's float64 log / cos / sqrt differ from the host's in the last digits, as in
    test_md_device.py) and agree within 1e-12 of the state's scale.  A pair accepted through delta >= 0, one through the
    draw and a rejected one are all among the decisions, each further than 1e-9 from its threshold on the host values."""
    seen = set()
    for R, n_rep, step, kinds in KERNEL_CASES:
        host, got, decisions = _one_step_on_both(R, n_rep, step, kinds)
        what = (R, n_rep, step)
        seen.update(kinds)
        assert got["state"].tolist() == host.state.tolist() == [step + 1, 0, 0, 0], what
        for k in ("rung", "replica_at", "attempts", "accepts", "outcome", "rung_new", "image", "f_prev"):
            assert np.array_equal(got[k], getattr(host, k)), (what, k)
        assert np.array_equal(bits(got["sigma"]), bits(host.sigma)) and np.array_equal(bits(got["vscale"]), bits(host.vscale)), what
        assert np.array_equal(bits(got["sigma"].reshape(R, -1)), bits(host.sigma_table[host.rung])), what
        assert sum(d[5] for d in decisions) == (host.outcome == 2).sum() and len(decisions) == (host.outcome != 0).sum()
        assert np.abs(got["x"] - host.x).max() <= 1e-12 * np.abs(host.x).max(), what
        assert np.abs(got["v"] - host.v).max() <= 1e-12 * np.abs(host.v).max(), what
        slot = step % 4
        want, have = host.log[slot], got["log"][slot]
        assert np.array_equal(bits(have[:, [0, 2, 3, 4]]), bits(want[:, [0, 2, 3, 4]])) and np.all(have[:, 2] == 4321), what
        assert np.all(np.abs(have[:, 1] - want[:, 1]) <= 1e-12 * np.abs(want[:, 1]).max()), what
        assert np.array_equal(have[:, 4], host.rung) and np.all(got["log"][[s for s in range(4) if s != slot]] == -7.0), what
    assert seen == {"up", "draw", "reject"}


# ---- the driver on 4 x 32 atoms ---------------------------------------------------------------------------------------------------
def _system():
    """Four replicas of one 32-atom alloy cell (one seed for all), Maxwell-Boltzmann velocities at the ladder's temperatures."""
    if "system" not in _CACHE:
        pos, cell, z = synth.fcc_alloy_atoms(reps=(2, 2, 2))
        R = len(LADDER)
        m = np.tile(np.array([MASS[int(v)] for v in z]), R)
        t_atom = np.repeat(LADDER, len(z))
        v = np.random.RandomState(3).normal(size=(len(m), 3)) * np.sqrt(KB * t_atom / (m * AMU))[:, None]
        _CACHE["system"] = dict(pos=np.tile(pos, (R, 1)), z=np.tile(z, R), cell=np.tile(cell, (R, 1, 1)), m=m, v=v,
                                batch=np.repeat(np.arange(R), len(z)), n_rep=len(z))
    return _CACHE["system"]


def _args(s):
    dev = _dev()
    return (torch.from_numpy(s["z"]).to(dev), torch.from_numpy(s["cell"].astype(np.float32)).to(dev), s["pos"], s["m"], DT)


def _hot_system():
    """`_system()` after 200 steps of the ladder without exchange: the replicas have left their common start, so their
    energies differ by what the ladder's temperatures make them differ (from one start they stay within a fraction of
    1 / (beta_r - beta_(r+1)) of each other for tens of steps, and every pair is accepted)."""
    if "hot" not in _CACHE:
        md = _remd(10 ** 6, system=_system())
        md.run(200)
        snap = md.fetch()
        assert snap.step == 200 and not snap.halted
        _CACHE["hot"] = dict(_system(), pos=snap.positions, v=snap.velocities)
    return _CACHE["hot"]


def _remd(interval, system=None, **kw):
    s = system if system is not None else _hot_system()
    return DeviceREMD(_shared_model(), *_args(s), LADDER, FRICTION, interval, batch=torch.from_numpy(s["batch"]).to(_dev()),
                      num_graphs=len(LADDER), seed=SEED, velocities=s["v"], **kw)


def _state_bits(snap):
    return (bits(snap.positions).tobytes(), bits(snap.velocities).tobytes(), snap.images.tobytes(), snap.forces.tobytes(),
            snap.step, snap.rung.tobytes(), snap.replica_at.tobytes(), snap.attempts.tobytes(), snap.accepts.tobytes())


def _base_run():
    """The uninterrupted run the other tests refer to, once: interval 2, run(20), fetch, run(20), fetch.  (the list's size at
    the start, the snapshot at 20, the snapshot at 40, the 40 log rows)."""
    if "base" not in _CACHE:
        remd = _remd(2)
        _, n0 = remd.step.check()
        remd.run(20)
        mid = remd.fetch()
        remd.run(20)
        end = remd.fetch()
        _CACHE["base"] = (int(n0), mid, end, np.concatenate([mid.log, end.log]))
    return _CACHE["base"]


def _recount(log, upto):
    """(attempts, accepts) [R-1] of the rows before `upto`, from the rung columns alone."""
    R = log.shape[1]
    attempts, accepts = np.zeros(R - 1, dtype=np.int64), np.zeros(R - 1, dtype=np.int64)
    for step in range(upto):
        a = attempt_of(step, 2)
        before, after = log[step, :, 3].astype(int), log[step, :, 4].astype(int)
        for r in range(R - 1):
            if a >= 0 and r % 2 == a % 2:
                attempts[r] += 1
                accepts[r] += after[list(before).index(r)] == r + 1
    return attempts, accepts


def test_no_exchange_equals_device_md_bit_for_bit():
    """`DeviceREMD(exchange_interval=10**6).run(10)` against `DeviceMD(friction=, temperature=ladder, batch=).run(10)` with
    the same seed: positions, velocities, images, forces and the log's columns 0-2 are bit-equal; the rung columns say
    identity and nothing was attempted."""
    s = _system()
    remd = _remd(10 ** 6, system=s)
    md = DeviceMD(_shared_model(), *_args(s), temperature=LADDER, friction=FRICTION, seed=SEED, velocities=s["v"],
                  batch=torch.from_numpy(s["batch"]).to(_dev()), num_graphs=len(LADDER))
    assert np.array_equal(bits(remd.sigma.cpu().numpy()), bits(md.sigma.cpu().numpy()))
    assert np.array_equal(bits(remd.sigma_table.cpu().numpy().reshape(-1)), bits(md.sigma.cpu().numpy()))
    remd.run(10)
    md.run(10)
    a, b = remd.fetch(), md.fetch()
    assert (a.step, a.halted, b.step, b.halted) == (10, False, 10, False)
    assert _state_bits(a)[:5] == (bits(b.positions).tobytes(), bits(b.velocities).tobytes(), b.images.tobytes(),
                                  b.forces.tobytes(), 10)
    assert a.log.shape == (10, 4, 5) and b.log.shape == (10, 4, 3) and np.array_equal(bits(a.log[:, :, :3]), bits(b.log))
    assert np.all(a.log[:, :, 3] == np.arange(4)) and np.all(a.log[:, :, 4] == np.arange(4))
    assert not a.attempts.any() and not a.accepts.any() and np.array_equal(a.temperature, LADDER)
    assert np.abs(a.velocities).max() > 0 and len(set(a.log[:, 0, 2])) > 1


def test_every_decision_of_a_run_is_the_hosts_from_the_log():
    """4 x 32 atoms at 1200, 1600, 2100 and 2800 K (why: at `LADDER`), interval 2, 40 steps = 20 attempts, 30 pairs.  Every attempt's pairs are decided again on the host -- from that row's logged E_pot and rung column and the host's
    Philox -- and the row's column 4 must say the same; a pair within 1e-9 of its threshold is left out (at most one in the
    run), and each attempt is checked from the logged state before it.  Rows are permutations and chain; the counters equal
    the recount; temperature = ladder[rung].  Seen on an MI355X with this ladder and seed: 26 accepted, 4 rejected, none
    within the margin (the test asserts at least one accepted and one rejected pair, and prints the counts)."""
    _, mid, end, log = _base_run()
    R = len(LADDER)
    beta = ladder(LADDER, np.ones(1), DT, FRICTION)[0]
    assert log.shape == (40, R, 5) and end.step == 40 and not end.halted
    accepted = rejected = omitted = 0
    held = np.arange(R)
    for step in range(40):
        before, after = log[step, :, 3].astype(int), log[step, :, 4].astype(int)
        assert np.array_equal(before, held), step                     # the rows chain: what a step held, the last one left
        assert sorted(before) == list(range(R)) and sorted(after) == list(range(R)), step
        replica_at = np.argsort(before)
        want = before.copy()
        for r, ga, gb, delta, log_u, yes in decide(SEED, step, 2, beta, log[step, :, 0].astype(np.float32), replica_at):
            if abs(log_u - delta) <= MARGIN:
                omitted += 1
                yes = after[ga] == r + 1
            if yes:
                want[ga], want[gb] = r + 1, r
            accepted += yes
            rejected += not yes
        assert np.array_equal(after, want), (step, before, after, want)
        held = after
    print("DeviceREMD 4 x 32, ladder %s, 40 steps, interval 2: %d accepted, %d rejected, %d within the margin"
          % (LADDER.tolist(), accepted, rejected, omitted))
    assert omitted <= 1 and accepted + rejected == 30 and accepted >= 1 and rejected >= 1
    for snap, rows in ((mid, 20), (end, 40)):
        attempts, accepts = _recount(log, rows)
        assert np.array_equal(snap.attempts, attempts) and np.array_equal(snap.accepts, accepts)
        assert np.array_equal(snap.rung, log[rows - 1, :, 4].astype(int)) and np.array_equal(snap.replica_at[snap.rung], np.arange(R))
        assert np.array_equal(snap.temperature, LADDER[snap.rung])
    assert end.attempts.tolist() == [10, 10, 10] and end.accepts.sum() == accepted


def test_an_accepted_swap_rescales_the_velocities_of_the_pair_alone():
    """The run against a twin with exchange_interval = 10**6 and the same seed, both stopped behind the step of the first
    accepted swap (found in the log): positions bit-equal; the velocities of a replica that went from rung r up are the
    twin's times up[r], of one that came down to r times down[r], bit for bit; everyone else's equal the twin's."""
    log = _base_run()[3]
    swapped = [s for s in range(40) if not np.array_equal(log[s, :, 3], log[s, :, 4])]
    assert swapped
    first, n_rep = swapped[0], _system()["n_rep"]
    a, b = _remd(2), _remd(10 ** 6)
    a.run(first + 1)
    b.run(first + 1)
    sa, sb = a.fetch(), b.fetch()
    assert sa.step == sb.step == first + 1 and not sb.attempts.any()
    assert np.array_equal(bits(sa.positions), bits(sb.positions)) and np.array_equal(sa.images, sb.images)
    assert np.array_equal(sa.forces, sb.forces) and np.array_equal(bits(sa.log[:, :, :3]), bits(sb.log[:, :, :3]))
    _, up, down, _ = ladder(LADDER, np.ones(1), DT, FRICTION)
    before, after = log[first, :, 3].astype(int), log[first, :, 4].astype(int)
    assert np.array_equal(sa.rung, after) and np.array_equal(sb.rung, np.arange(4)) and np.array_equal(before, np.arange(4))
    moved = 0
    for g in range(4):
        mine = slice(g * n_rep, (g + 1) * n_rep)
        want = sb.velocities[mine]
        if after[g] == before[g] + 1:
            want, moved = want * up[before[g]], moved + 1
        elif after[g] == before[g] - 1:
            want, moved = want * down[after[g]], moved + 1
        else:
            assert after[g] == before[g]
        assert np.array_equal(bits(sa.velocities[mine]), bits(want)), g
    assert moved >= 2 and moved % 2 == 0
    sigma = a.sigma.cpu().numpy().reshape(4, n_rep)
    assert np.array_equal(bits(sigma), bits(a.sigma_table.cpu().numpy()[after]))


def test_a_run_is_a_function_of_the_seed_alone_however_it_is_split():
    """run(7); run(13) equals run(20) -- positions, velocities, images, forces, rung, replica_at, counters and the log -- with
    or without a fetch() in between."""
    _, mid, _, log = _base_run()
    for fetch_between in (False, True):
        remd = _remd(2)
        logs = []
        remd.run(7)
        if fetch_between:
            logs.append(remd.fetch().log)
        remd.run(13)
        snap = remd.fetch()
        logs.append(snap.log)
        assert _state_bits(snap) == _state_bits(mid), fetch_between
        assert np.array_equal(bits(np.concatenate(logs)), bits(log[:20])), fetch_between


def test_halt_on_list_overflow_and_resume():
    """A capacity that the list outgrows at step k (found from the uninterrupted run's edge column): the run halts there with
    the capacity bit and exactly k log rows; rung, replica_at and the counters are those of the last completed step;
    resume() recaptures with more columns and the run ends bit-equal to the uninterrupted one."""
    n0, _, end, log = _base_run()
    counts = log[:, 0, 2].astype(int).tolist()
    at = [k for k in range(2, 40) if counts[k] > max([n0] + counts[:k])]
    assert at, "the edge count never exceeded its running maximum: no overflow to test"
    k = at[0]
    capacity = max([n0] + counts[:k])
    remd = _remd(2, capacity=capacity)
    assert remd.capacity == capacity
    remd.run(40)
    snap = remd.fetch()
    assert snap.halted and snap.step == k and snap.halt_step == k and (snap.halt_code & HALT_CAPACITY)
    assert snap.log.shape[0] == k and np.array_equal(bits(snap.log), bits(log[:k]))
    attempts, accepts = _recount(log, k)
    assert np.array_equal(snap.rung, log[k - 1, :, 4].astype(int)) and np.array_equal(snap.replica_at[snap.rung], np.arange(4))
    assert np.array_equal(snap.attempts, attempts) and np.array_equal(snap.accepts, accepts)
    remd.run(3)                                          # halted: replays change nothing
    again = remd.fetch()
    assert _state_bits(again) == _state_bits(snap) and again.log.shape[0] == 0 and again.halted
    remd.resume()
    assert remd.capacity > capacity
    remd.run(40 - k)
    last = remd.fetch()
    assert (last.step, last.halted) == (40, False)
    assert _state_bits(last) == _state_bits(end) and np.array_equal(bits(last.log), bits(log[k:]))


def test_ase_hand_off_in_batch_and_in_ladder_order():
    """`from_atoms` on the list of replicas builds the batch (ASE's velocity unit converted); `to_atoms` writes the replicas
    back in batch order, or with `by_rung` in ladder order: entry k is the replica at temperatures[k]."""
    from hermnet_amd.md import ASE_TIME_FS
    s, n_rep = _hot_system(), _system()["n_rep"]
    parts = [slice(g * n_rep, (g + 1) * n_rep) for g in range(4)]
    atoms = [_FakeAtoms(s["pos"][p], s["z"][p], s["cell"][g], s["m"][p], s["v"][p] * ASE_TIME_FS) for g, p in enumerate(parts)]
    remd = DeviceREMD.from_atoms(atoms, _shared_model(), DT, LADDER, FRICTION, 2, seed=SEED)
    start = remd.fetch()
    assert np.array_equal(start.positions, s["pos"]) and np.allclose(start.velocities, s["v"], rtol=1e-15, atol=0)
    assert np.array_equal(start.rung, np.arange(4)) and start.step == 0 and np.abs(start.forces).max() > 0
    # a snapshot whose assignment is not the identity (to_atoms reads positions, velocities and replica_at of it)
    end = types.SimpleNamespace(positions=start.positions + 1.0, velocities=start.velocities * 2.0, replica_at=np.array([2, 0, 3, 1]))
    for by_rung in (False, True):
        assert remd.to_atoms(atoms, by_rung=by_rung, snapshot=end) is end
        for k in range(4):
            g = int(end.replica_at[k]) if by_rung else k
            assert np.array_equal(atoms[k].positions, end.positions[parts[g]])
            assert np.array_equal(atoms[k].get_velocities(), end.velocities[parts[g]] * ASE_TIME_FS)
    with pytest.raises(ValueError, match="list of 4"):
        remd.to_atoms(atoms[:3], snapshot=end)


def test_refusals_name_their_reason():
    s = _system()
    z, cell, pos, m, dt = _args(s)
    batch = torch.from_numpy(s["batch"]).to(_dev())
    model = _shared_model()

    def make(z=z, cell=cell, pos=pos, m=m, temperatures=LADDER, friction=FRICTION, interval=2, batch=batch, num_graphs=4):
        return DeviceREMD(model, z, cell, pos, m, dt, temperatures, friction, interval, batch=batch, num_graphs=num_graphs)

    n_rep = s["n_rep"]
    with pytest.raises(ValueError, match="thermostat"):
        make(friction=None)
    with pytest.raises(ValueError, match="2 replicas"):
        make(batch=None)
    with pytest.raises(ValueError, match="2 replicas"):
        make(z=z[:n_rep], pos=pos[:n_rep], m=m[:n_rep], cell=cell[:1], batch=batch[:n_rep], num_graphs=1, temperatures=LADDER[:1])
    with pytest.raises(ValueError, match="3 temperatures for 4 replicas"):
        make(temperatures=LADDER[:3])
    for bad in (0.0, -300.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="positive and finite"):
            make(temperatures=[300.0, bad, 400.0, 500.0])
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="exchange_interval"):
            make(interval=bad)
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
