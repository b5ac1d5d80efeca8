"""CPU: the replica-exchange finish (hermnet_amd/csrc/remd_step.h) through the library's host twin
hermnet_host_remd_finish -- against its numpy transcription bit for bit, its uniform against a pure-Python Philox, and its
physics on a harmonic well (mean energy per rung, acceptance per pair, mixing)."""
import math

import numpy as np
import pytest

from md_reference import KB, bits, philox4x32_10
from remd_reference import HostREMD, NumpyREMD, pair_uniform, pair_words

MARGIN = 1e-9          # |log u - delta| above this: a last-bit difference between two log implementations cannot flip a decision
FIELDS = ("x", "v", "image", "f_prev", "pos32", "sigma", "rung", "replica_at", "attempts", "accepts", "log", "state")


def _same(a, b, what):
    for k in FIELDS:
        p, q = getattr(a, k), getattr(b, k)
        if p.dtype == np.float64:
            assert np.array_equal(bits(p), bits(q)), (what, k)
        else:
            assert np.array_equal(p, q), (what, k)


def _pair(R, n_rep, interval, seed, temperatures, inf_atom=None, cell=None, rs_seed=0):
    """A host twin and the numpy reference of one ladder in one start state; and the generator of its forces and energies."""
    rs = np.random.RandomState(rs_seed)
    n = R * n_rep
    m_rep = rs.uniform(10.0, 60.0, n_rep)
    if inf_atom is not None:
        m_rep[inf_atom] = np.inf
    m = np.tile(m_rep, R)
    x, v = rs.uniform(-3.0, 3.0, (n, 3)), rs.normal(scale=0.02, size=(n, 3))
    v[~np.isfinite(m)] = 0.0
    kw = dict(seed=seed, log_steps=8, cell=cell)
    pair = [cls(x, v, m, 0.5, temperatures, 0.02, interval, **kw) for cls in (HostREMD, NumpyREMD)]
    f0 = rs.normal(size=(n, 3)).astype(np.float32)
    for p in pair:
        p.f_prev[:] = f0
    return pair[0], pair[1], rs


def _kinds(decisions):
    """How often each way a decision can go occurred: (delta >= 0, accepted by the draw, rejected); the margin is asserted."""
    up = draw = no = 0
    for _, _, _, _, delta, log_u, yes in decisions:
        assert abs(log_u - delta) > MARGIN
        up += delta >= 0.0
        draw += delta < 0.0 and yes
        no += not yes
    return up, draw, no


LADDER5 = [300.0, 330.0, 363.0, 400.0, 440.0]
CASES = {
    # R, atoms per replica, interval, steps, the noise's seed (chosen on the CPU so that all three ways occur), infinite mass
    "R2": dict(R=2, n_rep=5, interval=1, steps=12, seed=(4 << 32) + 5, inf_atom=None),
    "R3": dict(R=3, n_rep=1, interval=1, steps=12, seed=1, inf_atom=None),
    "R5": dict(R=5, n_rep=7, interval=2, steps=12, seed=(1 << 32) + 2, inf_atom=None),
    "R5-fixed-atom": dict(R=5, n_rep=300, interval=2, steps=12, seed=1, inf_atom=4),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_the_numpy_transcription_bit_for_bit(name):
    """Every step of a short run, attempts and the steps between them: x, v, image, f_prev, pos32, sigma, rung, replica_at,
    the counters, the log ring and state are bit-equal.  R = 2: odd attempts have no pair.  R = 3: the pair alternates and one
    replica sits out.  R = 5: six consecutive attempts, with steps in between that attempt nothing.  The decisions compared
    contain one accepted through delta >= 0, one accepted through the draw and one rejected, each 1e-9 from its threshold."""
    c = CASES[name]
    R = c["R"]
    cell = None
    if name == "R5":
        cell = np.tile(np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]]), (R, 1, 1))
    host, ref, rs = _pair(R, c["n_rep"], c["interval"], c["seed"], LADDER5[:R], c["inf_atom"], cell)
    n = R * c["n_rep"]
    rungs = []
    for step in range(c["steps"]):
        f = rs.normal(size=(n, 3)).astype(np.float32)
        e = rs.normal(scale=0.4, size=R).astype(np.float32)
        assert np.array_equal(host.advance(), ref.advance())
        host.finish(f, e, total=(100 + step, 0))
        ref.finish(f, e, total=(100 + step, 0))
        _same(host.snapshot(), ref.snapshot(), step)
        assert sorted(host.rung) == list(range(R)) and np.array_equal(host.replica_at[host.rung], np.arange(R))
        rungs.append(host.rung.copy())
    assert host.state.tolist() == [c["steps"], 0, 0, 0]
    up, draw, no = _kinds(ref.decisions)
    assert up >= 1 and draw >= 1 and no >= 1, (up, draw, no)
    attempts = c["steps"] // c["interval"]
    tried = np.array([sum(1 for a in range(attempts) if a % 2 == r % 2) for r in range(R - 1)])
    assert np.array_equal(host.attempts, tried) and host.accepts.sum() == up + draw and len(ref.decisions) == tried.sum()
    if name == "R2":
        assert [d[0] for d in ref.decisions] == list(range(0, 12, 2))          # odd attempts: no pair
    if name == "R3":
        assert [d[1] for d in ref.decisions] == [0, 1] * 6                      # the pair alternates
    if c["interval"] == 2:
        assert all(np.array_equal(rungs[s], rungs[s - 1]) for s in range(2, c["steps"], 2))   # even steps attempt nothing
    if c["inf_atom"] is not None:
        held = np.arange(R) * c["n_rep"] + c["inf_atom"]
        assert not host.v[held].any() and not host.sigma[held].any()
    assert np.array_equal(bits(host.sigma.reshape(R, -1)), bits(host.sigma_table[host.rung]))


@pytest.mark.parametrize("what", ["capacity", "nonfinite", "prime", "halted"])
def test_a_step_that_is_not_committed_attempts_nothing(what):
    """On a step index at which an attempt falls, after exchanges have already happened: a void step (capacity bit; an energy
    that is not finite), a prime and a set halt code leave rung, replica_at, sigma, v and the counters as they were -- in
    the host twin and in the transcription alike."""
    host, ref, rs = _pair(5, 7, 1, (9 << 32) + 2, LADDER5)
    n = 35
    for step in range(4):
        f, e = rs.normal(size=(n, 3)).astype(np.float32), rs.normal(scale=0.4, size=5).astype(np.float32)
        for p in (host, ref):
            p.advance()
            p.finish(f, e)
    assert host.accepts.sum() >= 2 and not np.array_equal(host.rung, np.arange(5))
    if what == "prime":
        host.state[3] = ref.state[3] = 1
    if what == "halted":
        host.state[1] = ref.state[1] = 2
        host.state[2] = ref.state[2] = 3
    before = host.snapshot()
    f, e = rs.normal(size=(n, 3)).astype(np.float32), rs.normal(scale=0.4, size=5).astype(np.float32)
    total, capacity = (500, 0), 1000
    if what == "capacity":
        total = (1001, 0)
    if what == "nonfinite":
        e[3] = np.nan
    for p in (host, ref):
        p.advance()
        p.finish(f, e, total=total, capacity=capacity)
    after = host.snapshot()
    _same(after, ref.snapshot(), what)
    for k in ("rung", "replica_at", "attempts", "accepts", "log", "x", "image"):
        assert np.array_equal(getattr(before, k), getattr(after, k)), k
    assert np.array_equal(bits(before.sigma), bits(after.sigma)) and np.array_equal(bits(before.v), bits(after.v))
    want = {"capacity": [4, 4, 4, 0], "nonfinite": [4, 256, 4, 0], "prime": [4, 0, 0, 0], "halted": [4, 2, 3, 0]}[what]
    assert after.state.tolist() == want
    assert np.array_equal(after.f_prev, f if what == "prime" else before.f_prev)


def _decision_of_the_twin(seed, step, r, delta):
    """Pair r's decision at `step` by the host twin when its delta is exactly `delta`: beta = (delta, 0) on the pair and
    energies (1, 0), so (beta_r - beta_(r+1)) (E_a - E_b) is delta with no rounding.  R = r + 2 rungs, interval 1."""
    R = r + 2
    if step % 2 != r % 2:          # attempt a = step with interval 1: the pair's parity must be the attempt's
        raise ValueError("pair %d is not tried at step %d" % (r, step))
    host = HostREMD(np.zeros((R, 3)), np.zeros((R, 3)), np.full(R, 20.0), 1.0, np.linspace(300.0, 400.0, R), 0.05, 1, seed=seed)
    host.state[0] = step
    host.beta[:] = 0.0
    host.beta[r] = delta
    e = np.zeros(R, dtype=np.float32)
    e[r] = 1.0
    host.finish(np.zeros((R, 3), dtype=np.float32), e)
    assert host.attempts[r] == 1
    return bool(host.accepts[r])


def test_the_uniform_is_philox_stream_2_of_the_pair_and_the_step():
    """The uniform's words are md_reference.philox4x32_10((r, step low, step high, 2), key): the twin's decision flips between
    delta = log(u) (1 + 1e-9) (rejected) and log(u) (1 - 1e-9) (accepted) with u from the pure-Python Philox -- for seeds and
    steps with high words, and pairs other than 0.  u = 1 cannot be rejected: delta = 0 is accepted."""
    for seed, step, r in [(0, 0, 0), ((7 << 32) + 5, 3, 1), (12345, (1 << 32) + 6, 4), ((1 << 63) + 9, (5 << 32) + 1, 3), (2, 40, 0)]:
        w = pair_words(seed, step, r)
        assert w == philox4x32_10((r, step & 0xFFFFFFFF, step >> 32, 2), (seed & 0xFFFFFFFF, seed >> 32))
        log_u = math.log(pair_uniform(seed, step, r))
        assert log_u < 0.0
        assert not _decision_of_the_twin(seed, step, r, log_u * (1.0 + 1e-9)), (seed, step, r)
        assert _decision_of_the_twin(seed, step, r, log_u * (1.0 - 1e-9)), (seed, step, r)
        # the neighbouring streams and counters give other uniforms: the bracket would not hold for them
        other = philox4x32_10((r, step & 0xFFFFFFFF, step >> 32, 1), (seed & 0xFFFFFFFF, seed >> 32))
        assert other != w
    assert _decision_of_the_twin(0, 0, 0, 0.0)


def test_a_decision_does_not_depend_on_the_atoms_noise():
    """The same energies through a ladder of 3-atom replicas that advances (streams 0 and 1 consumed for every atom) and
    through one of 7-atom replicas that never advances: the same decisions, rungs and counters."""
    R, steps, seed = 5, 16, (9 << 32) + 2
    rs = np.random.RandomState(5)
    energies = rs.normal(scale=0.4, size=(steps, R)).astype(np.float32)
    logs = []
    for n_rep, advance in ((3, True), (7, False)):
        host, _, frs = _pair(R, n_rep, 1, seed, LADDER5, rs_seed=n_rep)
        host.log_steps, host.log = steps, np.zeros((steps, R, 5))
        for step in range(steps):
            if advance:
                host.advance()
            host.finish(frs.normal(size=(R * n_rep, 3)).astype(np.float32), energies[step])
        logs.append((host.log[:, :, 3:].copy(), host.rung.copy(), host.attempts.copy(), host.accepts.copy()))
    for a, b in zip(*logs):
        assert np.array_equal(a, b)
    assert logs[0][3].sum() >= 3 and logs[0][3].sum() < logs[0][2].sum()


# ---- physics on a harmonic well: host twins only ------------------------------------------------------------------------------
T_WELL = np.array([300.0, 380.0, 480.0, 600.0])
K_WELL, N_REP, STEPS, INTERVAL, BLOCK = 1.0, 8, 40000, 5, 1000
_WELL = {}


def _well(interval):
    """40,000 steps of 4 replicas x 8 atoms in E = k/2 sum |x|^2 (energy and forces rounded to float32, made in numpy), open,
    m = 20 amu, dt = 1 fs, friction 0.05 /fs, through hermnet_host_md_advance + hermnet_host_remd_finish.  Computed once per
    interval: (log [steps,4,5], attempts, accepts)."""
    if interval not in _WELL:
        R, n = len(T_WELL), len(T_WELL) * N_REP
        rs = np.random.RandomState(17)
        t_atom = np.repeat(T_WELL, N_REP)
        x = rs.normal(size=(n, 3)) * np.sqrt(KB * t_atom / K_WELL)[:, None]
        v = rs.normal(size=(n, 3)) * np.sqrt(KB * t_atom / (20.0 * 103.642696562))[:, None]
        host = HostREMD(x, v, np.full(n, 20.0), 1.0, T_WELL, 0.05, interval, seed=2024, log_steps=STEPS)
        host.f_prev[:] = (-K_WELL * host.x).astype(np.float32)
        for _ in range(STEPS):
            host.advance()
            e = (0.5 * K_WELL * (host.x * host.x).reshape(R, -1).sum(axis=1)).astype(np.float32)
            host.finish((-K_WELL * host.x).astype(np.float32), e)
        assert host.state.tolist() == [STEPS, 0, 0, 0]
        _WELL[interval] = (host.log.copy(), host.attempts.copy(), host.accepts.copy())
    return _WELL[interval]


def _blocked(series):
    """(mean, standard error from the means of blocks of 1,000 steps)."""
    blocks = series.reshape(-1, BLOCK).mean(axis=1)
    return series.mean(), blocks.std(ddof=1) / math.sqrt(len(blocks))


def test_well_mean_energy_per_rung_equals_the_ladder_without_exchange():
    """The mean logged E_pot of the steps spent at rung r (12 kB T_r in theory) equals that of a second run of the same length
    with exchanges off -- DeviceMD's host arithmetic, replica r at T_r throughout -- within 5 blocked standard errors of the
    two runs combined.  A wrong sign of delta or a missing velocity rescale fails this."""
    log, _, _ = _well(INTERVAL)
    ref, ref_attempts, _ = _well(10 * STEPS)
    assert ref_attempts.sum() == 0 and np.all(ref[:, :, 3] == np.arange(4)) and np.all(ref[:, :, 4] == np.arange(4))
    for r in range(4):
        at_r = log[:, :, 3] == r
        assert np.all(at_r.sum(axis=1) == 1)                          # every step, exactly one replica holds rung r
        mean, se = _blocked(log[:, :, 0][at_r])
        mean0, se0 = _blocked(ref[:, r, 0])
        print("rung %d: E_pot %.5f +- %.5f with exchange, %.5f +- %.5f without, theory %.5f"
              % (r, mean, se, mean0, se0, 12 * KB * T_WELL[r]))
        assert abs(mean - mean0) <= 5.0 * math.hypot(se, se0), (r, mean, mean0, se, se0)
        assert abs(mean0 - 12 * KB * T_WELL[r]) <= 5.0 * se0            # (the reference itself is where theory puts it)


def test_well_acceptance_per_pair_equals_the_gamma_expectation():
    """The acceptance of pair r equals E[min(1, exp(delta))] over 10^6 independent draws E ~ Gamma(12, kB T) at the two
    temperatures, within 5 binomial standard errors of the attempt count, doubled for the correlation between successive
    attempts."""
    _, attempts, accepts = _well(INTERVAL)
    assert attempts.tolist() == [4000, 4000, 4000]
    rs = np.random.RandomState(1)
    beta = 1.0 / (KB * T_WELL)
    for r in range(3):
        ea, eb = rs.gamma(12.0, KB * T_WELL[r], 10 ** 6), rs.gamma(12.0, KB * T_WELL[r + 1], 10 ** 6)
        want = np.minimum(1.0, np.exp((beta[r] - beta[r + 1]) * (ea - eb))).mean()
        got = accepts[r] / attempts[r]
        margin = 2.0 * 5.0 * math.sqrt(want * (1.0 - want) / attempts[r])
        print("pair %d: acceptance %.4f, expected %.4f +- %.4f" % (r, got, want, margin))
        assert abs(got - want) <= margin, (r, got, want, margin)


def test_well_every_replica_visits_every_rung():
    log, _, _ = _well(INTERVAL)
    for g in range(4):
        assert sorted(set(log[:, g, 3].astype(int))) == [0, 1, 2, 3], g
