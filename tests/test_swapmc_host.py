"""CPU: species-swap Monte Carlo between MD steps (hermnet_amd/csrc/swapmc_step.h) through the library's host twins
hermnet_host_swapmc_advance / _finish -- against the numpy transcription bit for bit, the pair picking against its stated
distribution, the sampled ensemble against an exact enumeration, the two temperature limits, a void trial, the refusals."""
import itertools
import math

import numpy as np
import pytest

from hermnet_amd import _lib
from hermnet_amd.swapmc import DeviceSwapMD, candidate_tables
from md_reference import KB, _p, bits
from swapmc_reference import HostSwapMC, NumpySwapMC, decide, pick_pair, tables

MARGIN = 1e-9          # |log u - delta| above this: a last-bit difference between two log implementations cannot flip a decision
FIELDS = ("x", "v", "image", "f_prev", "pos32", "e_ref", "mc", "attempts", "accepts", "swap_log", "log", "state")
AMPLITUDE = {13: 0.05, 28: -0.08, 29: 0.11}            # eV: the synthetic potential's per-species amplitude


def _same(a, b, what):
    for k in FIELDS:
        p, q = getattr(a, k), getattr(b, k)
        if p.dtype == np.float64:
            assert np.array_equal(bits(p), bits(q)), (what, k)
        else:
            assert np.array_equal(p, q), (what, k)


def _potential(z, batch, B):
    """A synthetic float32 potential that knows which species sits where: E_g = sum_i a(z_i) (sin x_i + sin y_i + sin z_i)
    over graph g in float32, f_i = -a(z_i) cos(.)."""
    a = np.array([AMPLITUDE[int(v)] for v in z], dtype=np.float32)

    def evaluate(pos32):
        per_atom = a * np.sin(pos32).sum(axis=1, dtype=np.float32)
        e = np.array([per_atom[batch == g].sum(dtype=np.float32) for g in range(B)], dtype=np.float32)
        return (-a[:, None] * np.cos(pos32)).astype(np.float32), e
    return evaluate


def _unequal_batch():
    """40 / 33 / 64 atoms, three species, an atom of infinite mass in graph 0, graph 1 of a single species."""
    rs = np.random.RandomState(5)
    counts = [40, 33, 64]
    batch = np.repeat(np.arange(3), counts)
    z = rs.choice([13, 28, 29], size=sum(counts))
    z[batch == 1] = 28
    m = np.array([{13: 26.98, 28: 58.69, 29: 63.55}[int(v)] for v in z])
    m[7] = np.inf
    cell = np.stack([np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]]), np.diag([8.0, 9.0, 10.0]),
                     np.diag([12.0, 11.0, 10.5])])
    x = np.einsum("nk,nkj->nj", rs.uniform(-0.5, 1.5, (len(z), 3)), cell[batch])
    v = rs.normal(scale=0.02, size=(len(z), 3))
    v[7] = 0.0
    return dict(x=x, v=v, z=z, m=m, batch=batch, cell=cell)


@pytest.mark.parametrize("friction", [None, 0.02], ids=["nve", "langevin"])
def test_host_twin_equals_the_numpy_transcription_bit_for_bit(friction):
    """200 replays from the prime on, swap_interval = 3, swaps = 2, energies and forces from the synthetic potential at the
    float32 coordinates each advance hands out: state, mc, x, image, v, f_prev, pos32, e_ref, the counters and both rings are
    bit-equal after every replay.  The decisions hold accepted and rejected trials, each 1e-9 from its threshold; the graph
    of one species is never tried; the atom of infinite mass is never picked."""
    s = _unequal_batch()
    kw = dict(cell=s["cell"], batch=s["batch"], friction=friction, temperature=None if friction is None else [600.0, 700.0, 800.0],
              seed=(3 << 32) + 11, log_steps=16, swap_rows=8, num_graphs=3)
    host, ref = (cls(s["x"], s["v"], s["z"], s["m"], 0.5, 3, 2, [700.0, 800.0, 900.0], **kw) for cls in (HostSwapMC, NumpySwapMC))
    evaluate = _potential(s["z"], s["batch"], 3)
    for p in (host, ref):
        p.state[3] = 1
    kinds = []
    for replay in range(200):
        kinds.append(ref.kind())
        assert host.kind() == kinds[-1]
        pos_h, pos_r = host.advance(), ref.advance()
        assert np.array_equal(pos_h, pos_r), replay
        f, e = evaluate(pos_r)
        host.finish(f, e, total=(100 + replay, 0))
        ref.finish(f, e, total=(100 + replay, 0))
        _same(host.snapshot(), ref.snapshot(), replay)
    assert kinds[:7] == ["prime", "md", "md", "md", "trial", "trial", "md"]
    assert host.state.tolist() == [120, 0, 0, 0] and host.mc.tolist() == [79, 1]
    assert all(abs(d[6] - d[5]) > MARGIN for d in ref.decisions)
    yes = sum(d[7] for d in ref.decisions)
    assert yes >= 10 and len(ref.decisions) - yes >= 10, (yes, len(ref.decisions))
    assert host.attempts.tolist() == [79, 0, 79] and host.accepts.sum() == yes and host.accepts[1] == 0
    assert all(d[1] != 1 and 7 not in d[2:4] and s["z"][d[2]] != s["z"][d[3]] and s["batch"][d[2]] == s["batch"][d[3]] == d[1]
               for d in ref.decisions)
    last = host.swap_log[(79 - 1) % 8]
    assert last[1].tolist() == [-1.0, -1.0, 0.0, 0.0] and last[0, 3] in (1.0, 2.0)
    assert not host.v[7].any()


def test_candidate_tables_of_the_driver_equal_the_reference():
    s = _unequal_batch()
    cand, ptr, S = tables(s["z"], s["m"], s["batch"], 3)
    got = candidate_tables(s["z"], np.isfinite(s["m"]), s["batch"], 3)
    assert S == got[2] == 3 and np.array_equal(cand, got[0]) and np.array_equal(ptr, got[1])
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[1].shape == (3, 4)
    assert 7 not in cand and len(cand) == len(s["z"]) - 1
    assert ptr[1].tolist() == [39, 39, 72, 72]           # graph 1: nickel alone


def _small_graph():
    """11 atoms: 5 + 3 + 2 candidates and one atom of infinite mass, with distinct coordinates."""
    z = np.array([13] * 5 + [28] * 3 + [29] * 3)
    m = np.array([26.98] * 5 + [58.69] * 3 + [63.55] * 3)
    m[9] = np.inf
    x = np.arange(33, dtype=np.float64).reshape(11, 3)
    return z, m, x


def test_pair_picking_follows_its_stated_distribution():
    """20,000 trials of one graph through the host twin's advance (the pair read off the exchanged coordinates): the pick is
    `pick_pair`'s, never two atoms of one species, never the fixed atom, and every unordered pair's frequency is within 5
    binomial sigma of p = (1 / m) (1 / (m - m_si) + 1 / (m - m_sj))."""
    z, m, x = _small_graph()
    seed, trials = (11 << 32) + 4, 20000
    host = HostSwapMC(x, np.zeros((11, 3)), z, m, 1.0, 1, 1, 300.0, seed=seed)
    counts = {}
    for t in range(trials):
        host.x[:], host.mc[:] = x, (t, 1)
        host.advance()
        moved = np.nonzero((host.x != x).any(axis=1))[0]
        assert len(moved) == 2
        i, j = (int(a) for a in moved)
        assert np.array_equal(host.x[i], x[j]) and np.array_equal(host.x[j], x[i])
        assert np.array_equal(host.pos32[[i, j]], x[[j, i]].astype(np.float32))
        assert {i, j} == set(pick_pair(seed, t, 0, host.cand, host.cand_ptr[0])), t
        counts[(i, j)] = counts.get((i, j), 0) + 1
    free = [a for a in range(11) if a != 9]
    size = {13: 5, 28: 3, 29: 2}
    want = {(i, j) for i, j in itertools.combinations(free, 2) if z[i] != z[j]}
    assert set(counts) == want and len(want) == 5 * 3 + 5 * 2 + 3 * 2
    for (i, j), c in sorted(counts.items()):
        p = (1.0 / 10) * (1.0 / (10 - size[z[i]]) + 1.0 / (10 - size[z[j]]))
        assert abs(c - trials * p) <= 5.0 * math.sqrt(trials * p * (1.0 - p)), (i, j, c, trials * p)


def _ring_energy(pos32, species, J):
    """J x (unlike nearest-neighbour bonds) of the 8-site ring; site = the atom's x coordinate."""
    arrangement = np.empty(8, dtype=np.int64)
    arrangement[np.rint(pos32[:, 0]).astype(np.int64)] = species
    return np.float32(J * np.count_nonzero(arrangement != np.roll(arrangement, 1)))


def test_swaps_sample_the_exact_ensemble_of_a_ring():
    """An 8-site ring of 4 A and 4 B atoms with E = J (unlike nearest-neighbour bonds), J = kB T, zero forces and zero
    velocities (the MD steps between the blocks move nothing).  The 70 arrangements are enumerated here: <E> = 2.8660 J.
    20,000 trials per seed through the host twins, the first 1,000 dropped: each of the 4 seeds' means is within 5 blocked
    standard errors (19 blocks of 1,000).  A plain numpy Metropolis of this set-up gave 0.6 to 1.3 standard errors and an
    acceptance of 0.41."""
    T = 1000.0
    J = KB * T
    levels = [sum((k in occ) != ((k + 1) % 8 in occ) for k in range(8)) for occ in map(set, itertools.combinations(range(8), 4))]
    assert len(levels) == 70
    weights = np.exp(-np.array(levels, dtype=np.float64))
    exact = float((np.array(levels) * weights).sum() / weights.sum())
    assert abs(exact - 2.8660) < 5e-5
    species = np.array([0, 0, 0, 0, 1, 1, 1, 1])
    x = np.zeros((8, 3))
    x[:, 0] = [0, 2, 4, 6, 1, 3, 5, 7]
    zero = np.zeros((8, 3), dtype=np.float32)
    for seed in range(4):
        host = HostSwapMC(x, np.zeros((8, 3)), species + 28, np.full(8, 50.0), 1.0, 1, 1000, T, seed=(seed << 32) + 17,
                          swap_rows=4)
        host.state[3] = 1
        samples = []
        while host.mc[0] < 20000:
            trial = host.kind() == "trial"
            e = np.array([_ring_energy(host.advance(), species, J)])
            host.finish(zero, e)
            if trial:
                samples.append(host.e_ref[0] / J)
        assert len(samples) == 20000 and host.state[0] == 20 and host.attempts[0] == 20000
        assert np.array_equal(np.sort(host.x[:, 0]), np.arange(8.0)) and not host.v.any()
        blocks = np.array(samples[1000:]).reshape(19, 1000).mean(axis=1)
        mean, err = blocks.mean(), blocks.std(ddof=1) / math.sqrt(19)
        acceptance = host.accepts[0] / 20000.0
        print("ring, seed %d: <E>/J = %.4f +- %.4f (exact %.4f), acceptance %.3f" % (seed, mean, err, exact, acceptance))
        assert abs(mean - exact) <= 5.0 * err, (seed, mean, err, exact)
        assert 0.3 < acceptance < 0.5


def _after_some_cycles(mc_temperature, seed=(2 << 32) + 9):
    s = _unequal_batch()
    host = HostSwapMC(s["x"], s["v"], s["z"], s["m"], 0.5, 2, 3, mc_temperature, cell=s["cell"], batch=s["batch"], seed=seed,
                      swap_rows=64, num_graphs=3)
    host.state[3] = 1
    return s, host, _potential(s["z"], s["batch"], 3)


@pytest.mark.parametrize("limit", ["cold", "hot"])
def test_the_two_temperature_limits_and_what_a_rejection_leaves(limit):
    """mc_temperature = 1e-6 K accepts exactly the trials with d <= 0, 1e12 K accepts every trial made; a trial in which
    every graph is rejected or not tried leaves x, image, v, f_prev, pos32 and e_ref bit-identical."""
    s, host, evaluate = _after_some_cycles(1e-6 if limit == "cold" else 1e12)
    seen = {0: 0, 1: 0, 2: 0}
    untouched = 0
    for replay in range(61):
        trial, t = host.kind() == "trial", int(host.mc[0])
        before = host.snapshot()
        f, e = evaluate(host.advance())
        host.finish(f, e)
        if not trial:
            continue
        row = host.swap_log[t % 64]
        for g in range(3):
            i, j, d, o = row[g]
            seen[int(o)] += 1
            assert (g == 1) == (o == 0)
            if o != 0:
                assert bits(np.float64(d)) == bits(np.float64(e[g]) - before.e_ref[g])
                assert o == (2 if (d <= 0.0 or limit == "hot") else 1)
        if not (row[:, 3] == 2).any():
            untouched += 1
            after = host.snapshot()
            for k in ("x", "v", "image", "f_prev", "pos32", "e_ref"):
                assert getattr(after, k).tobytes() == getattr(before, k).tobytes(), k
        for g in np.nonzero(row[:, 3] == 2)[0]:
            mine = s["batch"] == g
            assert np.array_equal(host.f_prev[mine], f[mine]) and host.e_ref[g] == np.float64(e[g])
        for g in np.nonzero(row[:, 3] != 2)[0]:
            mine = s["batch"] == g
            assert np.array_equal(host.f_prev[mine], before.f_prev[mine]) and host.e_ref[g] == before.e_ref[g]
            assert host.x[mine].tobytes() == before.x[mine].tobytes() and np.array_equal(host.image[mine], before.image[mine])
    assert host.mc[0] == 36 and seen[0] == 36
    if limit == "hot":
        assert seen[2] == 72 and seen[1] == 0
    else:
        assert seen[1] >= 10 and seen[2] >= 10 and untouched >= 3, (seen, untouched)


def test_a_trial_fed_a_nan_energy_is_void_and_is_repeated_after_the_prime():
    """The pair is back where it was bit for bit, the halt is recorded with the non-finite bit, t and left are unchanged,
    nothing is logged or counted; halted replays change nothing; after the prime the same pair is drawn and the trial
    commits as it would have."""
    s, host, evaluate = _after_some_cycles(800.0)
    twin = _after_some_cycles(800.0)[1]
    for p in (host, twin):
        for replay in range(8):                           # prime, 2 MD steps, 3 trials, 2 MD steps: a block is due
            f, e = evaluate(p.advance())
            p.finish(f, e)
        assert p.kind() == "trial" and p.mc.tolist() == [3, 3] and p.state.tolist() == [4, 0, 0, 0]
    before = host.snapshot()
    moved = host.advance().copy()
    pairs = [pick_pair(host.seed, 3, g, host.cand, host.cand_ptr[g]) for g in range(3)]
    assert pairs[1] is None and all(not np.array_equal(moved[k], before.pos32[k]) for p in (pairs[0], pairs[2]) for k in p)
    f, e = evaluate(moved)
    bad = e.copy()
    bad[2] = np.nan
    host.finish(f, bad)
    after = host.snapshot()
    assert after.state.tolist() == [4, 256, 4, 0] and after.mc.tolist() == [3, 3]
    for k in ("x", "v", "image", "f_prev", "pos32", "e_ref", "attempts", "accepts", "swap_log", "log"):
        assert getattr(after, k).tobytes() == getattr(before, k).tobytes(), k
    host.finish(f, e)                                     # halted: nothing
    assert np.array_equal(host.advance(), before.pos32) and host.snapshot().state.tolist() == [4, 256, 4, 0]
    # resume: the halt cleared, the prime, then the same trial
    host.state[1:3] = 0
    host.state[3] = 1
    f0, e0 = evaluate(host.advance())
    host.finish(f0, e0)
    assert host.kind() == "trial" and host.mc.tolist() == [3, 3]
    assert host.f_prev.tobytes() == before.f_prev.tobytes() and host.e_ref.tobytes() == before.e_ref.tobytes()
    for p in (host, twin):
        f, e = evaluate(p.advance())
        p.finish(f, e)
    assert np.array_equal(host.swap_log[3, [0, 2], :2], np.array([pairs[0], pairs[2]], dtype=np.float64))
    _same(host.snapshot(), twin.snapshot(), "resumed")
    d = decide(host.seed, 3, 0, host.beta[0], e[0], before.e_ref[0])
    assert host.swap_log[3, 0, 2] == d[0] and host.swap_log[3, 0, 3] == (2.0 if d[3] else 1.0)


def test_refusals_name_their_reason_without_a_gpu():
    z, m, x = _small_graph()
    make = lambda **kw: DeviceSwapMD(None, z, np.eye(3) * 20.0, x, m, 1.0, **dict(dict(swap_interval=2, swaps=1, temperature=300.0), **kw))
    with pytest.raises(ValueError, match="need a temperature"):
        make(temperature=None)
    for bad in (0.0, -5.0, np.inf, np.nan, [300.0, 0.0]):
        with pytest.raises(ValueError, match="positive and finite"):
            make(mc_temperature=bad)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="swap_interval"):
            make(swap_interval=bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="swaps must be"):
            make(swaps=bad)
    with pytest.raises(ValueError, match="swap_rows"):
        make(swap_rows=0)


def test_malformed_calls_are_refused_by_the_argument_checks():
    """HN_ERR_BAD_ARG from the host twins for what the header lists, the tables' checks included; the device entry points
    refuse what they can read -- before anything is launched, so with no GPU."""
    z, m, x = _small_graph()
    bad_arg = _lib.HN_ERR_BAD_ARG

    def fresh():
        host = HostSwapMC(x, np.zeros((11, 3)), z, m, 1.0, 2, 1, 300.0, seed=5)
        host.mc[:] = (0, 1)
        return host

    zero_f = np.zeros((11, 3), dtype=np.float32)
    host = fresh()
    host.advance()
    host.finish(zero_f)
    assert host.mc.tolist() == [1, 0]
    for name, value in (("interval", 0), ("swaps", -1), ("swap_rows", 0), ("S", 0)):
        host = fresh()
        setattr(host, name, value)
        host.finish(zero_f, expect=bad_arg)
        if name == "S":
            host.advance(expect=bad_arg)
    for name in ("beta", "e_ref", "mc", "pair", "dval", "outcome", "attempts", "accepts", "swap_log", "cand_ptr", "cand"):
        host = fresh()
        setattr(host, name, None)
        host.finish(zero_f, expect=bad_arg)
    for breakage in ("descending range", "beyond cand", "foreign atom", "unsorted", "negative word"):
        host = fresh()
        if breakage == "descending range":
            host.cand_ptr[0, 1], host.cand_ptr[0, 2] = 8, 5
        elif breakage == "beyond cand":
            host.cand_ptr[0, 3] = 11
        elif breakage == "foreign atom":
            host.cand[4] = 11
        elif breakage == "unsorted":
            host.cand[[0, 1]] = host.cand[[1, 0]]
        else:
            host.mc[1] = -1
        before = host.snapshot()
        host.advance(expect=bad_arg)
        host.finish(zero_f, expect=bad_arg)
        assert host.snapshot().x.tobytes() == before.x.tobytes() and host.snapshot().state.tolist() == [0, 0, 0, 0]
    # the device entry points: refused before a launch
    lib, h = _lib.load(), fresh()
    rc = lib.hermnet_swapmc_advance(11, 1, 0, 1.0, 5, _p(h.x), _p(h.v), _p(h.x0), _p(h.v0), _p(h.image), _p(h.image0), _p(h.f_prev),
                                    _p(h.kick), None, None, None, None, None, _p(h.pos32), _p(h.state), None, _p(h.graph_ptr),
                                    _p(h.cand), _p(h.cand_ptr), 3, 10, None)
    assert rc == bad_arg
    e, tot = np.zeros(1, dtype=np.float32), np.zeros(2, dtype=np.int64)
    rc = lib.hermnet_swapmc_finish(11, 1, _p(h.graph_ptr), None, _p(zero_f), _p(e), _p(tot), 100, 0, 1, 5, *h._finish_atoms(),
                                   _p(h.beta), _p(h.e_ref), _p(h.mc), _p(h.cand), _p(h.cand_ptr), 3, 10, _p(h.pair), _p(h.dval),
                                   _p(h.outcome), _p(h.attempts), _p(h.accepts), _p(h.swap_log), 64, _p(h.log), 64, _p(h.state), None)
    assert rc == bad_arg
