"""Shared by tests/test_remd_host.py and tests/test_remd_device.py: the numpy transcription of the replica-exchange finish
(hermnet_amd/csrc/remd_step.h and md_finish.h, operation by operation), the host-made ladder constants exactly as
hermnet_amd/remd.py makes them, and a thin wrapper that runs the library's host twins (hermnet_host_md_advance,
hermnet_host_remd_finish) on numpy arrays."""
import math
import types

import numpy as np

from md_reference import AMU, KB, M32, HostMD, NumpyMD, _p, advance_np, host_noise, philox4x32_10


def ladder(temperatures, masses_rep, dt, friction):
    """(beta [R], up [R-1], down [R-1], sigma_table [R, n_rep]) of hermnet_amd/remd.py: DeviceREMD._own_state."""
    t = np.asarray(temperatures, dtype=np.float64)
    c1 = math.exp(-float(friction) * dt)
    m = np.asarray(masses_rep, dtype=np.float64) * AMU
    table = np.sqrt(KB * t[:, None] * (1.0 - c1 * c1) / m[None, :])
    return 1.0 / (KB * t), np.sqrt(t[1:] / t[:-1]), np.sqrt(t[:-1] / t[1:]), np.ascontiguousarray(table)


def pair_words(seed, step, r):
    """The four words of pair r's uniform: key (seed low, seed high), counter (r, step low, step high, 2)."""
    return philox4x32_10((r, step & M32, (step >> 32) & M32, 2), (seed & M32, (seed >> 32) & M32))


def pair_uniform(seed, step, r):
    w = pair_words(seed, step, r)
    return (float(((w[0] >> 5) << 26) | (w[1] >> 6)) + 1.0) * (1.0 / 9007199254740992.0)


def attempt_of(step, interval):
    """The attempt's index at the end of the committed step `step` (0-based), -1: none."""
    return (step + 1) // interval - 1 if (step + 1) % interval == 0 else -1


def decide(seed, step, interval, beta, energy32, replica_at):
    """remd_decide's pairs: a list of (r, ga, gb, delta, log u, accepted) of the attempt at the end of `step` (empty: none)."""
    a, R, out = attempt_of(step, interval), len(beta), []
    if a < 0:
        return out
    e = np.asarray(energy32, dtype=np.float32)
    for r in range(R - 1):
        if r % 2 != a % 2:
            continue
        ga, gb = int(replica_at[r]), int(replica_at[r + 1])
        delta = (beta[r] - beta[r + 1]) * (np.float64(e[ga]) - np.float64(e[gb]))
        log_u = math.log(pair_uniform(seed, step, r))
        out.append((r, ga, gb, float(delta), log_u, bool(delta >= 0.0 or log_u < delta)))
    return out


def canonical_sum(terms):
    """hn_canonical_sums<1,-1>: lane l of 256 adds terms l, l + 256, ... from 0.0, then the tree m = 128, ..., 1."""
    t = np.asarray(terms, dtype=np.float64)
    rows = np.zeros((-(-max(len(t), 1) // 256)) * 256)
    rows[:len(t)] = t
    part = np.zeros(256)
    for row in rows.reshape(-1, 256):        # (the padding adds +0.0: no change)
        part = part + row
    m = 128
    while m >= 1:
        part[:m] = part[:m] + part[m:2 * m]
        m //= 2
    return part[0]


class _Ladder(object):
    """What NumpyREMD and HostREMD share: the ladder's constants and state in the layout of include/hermnet_hip.h."""

    def _make_ladder(self, masses, dt, temperatures, friction, interval, log_steps):
        R = self.R = len(temperatures)
        self.n_rep = self.n // R
        self.interval = int(interval)
        self.beta, self.up, self.down, self.sigma_table = ladder(temperatures, np.asarray(masses)[:self.n_rep], dt, friction)
        self.rung, self.replica_at = np.arange(R, dtype=np.int64), np.arange(R, dtype=np.int64)
        self.rung_new, self.vscale = np.arange(R, dtype=np.int64), np.ones(R)
        self.outcome = np.zeros(R - 1, dtype=np.int64)
        self.attempts, self.accepts = np.zeros(R - 1, dtype=np.int64), np.zeros(R - 1, dtype=np.int64)
        self.log_steps = log_steps
        self.log = np.full((log_steps, R, 5), -7.0)

    def snapshot(self):
        names = ("x", "v", "image", "f_prev", "pos32", "sigma", "rung", "replica_at", "attempts", "accepts", "log", "state")
        return types.SimpleNamespace(**{k: getattr(self, k).copy() for k in names})


class HostREMD(_Ladder, HostMD):
    """hermnet_host_md_advance + hermnet_host_remd_finish on numpy arrays."""

    def __init__(self, x, v, masses, dt, temperatures, friction, interval, seed=0, log_steps=64, cell=None):
        R = len(temperatures)
        batch = np.repeat(np.arange(R), len(x) // R)
        HostMD.__init__(self, x, v, masses, dt, cell=cell, batch=batch, friction=friction, temperature=temperatures, seed=seed,
                        log_steps=log_steps, num_graphs=R)
        self._make_ladder(masses, dt, temperatures, friction, interval, log_steps)

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20, expect=0):
        f, e, tot = self._evaluation(f32, energy, total)
        rc = self.lib.hermnet_host_remd_finish(
            self.n, self.B, _p(self.graph_ptr), _p(f), _p(e), _p(tot), capacity, self.interval, self.seed, *self._finish_atoms(),
            _p(self.beta), _p(self.up), _p(self.down), _p(self.sigma_table), _p(self.sigma), _p(self.rung), _p(self.replica_at),
            _p(self.rung_new), _p(self.vscale), _p(self.outcome), _p(self.attempts), _p(self.accepts), *self._finish_tail())
        assert rc == expect, rc


class NumpyREMD(_Ladder, NumpyMD):
    """The reference: md_advance_one (the noise of the library's host form) and the replica-exchange finish in numpy float64,
    operation by operation.  `decisions`: every pair it decided, (step, r, ga, gb, delta, log u, accepted)."""

    def __init__(self, x, v, masses, dt, temperatures, friction, interval, seed=0, log_steps=64, cell=None):
        R = len(temperatures)
        NumpyMD.__init__(self, x, v, masses, dt, cell=cell, batch=np.repeat(np.arange(R), len(x) // R), friction=friction,
                         temperature=temperatures, seed=seed, num_graphs=R)
        self.decisions = []
        self._make_ladder(masses, dt, temperatures, friction, interval, log_steps)

    def advance(self):
        step, code, mode = (int(w) for w in self.state[[0, 1, 3]])
        if code != 0:
            return self.pos32
        if mode == 0:
            self.x0[:], self.v0[:], self.image0[:] = self.x, self.v, self.image
            xi = host_noise(self.seed, step, self.n)[1]
            advance_np(self.x, self.v, self.image, self.f_prev, self.kick, self.dt, self.c1_atom, self.sigma, xi, self.cell, self.inv)
        self.pos32 = self.x.astype(np.float32)
        return self.pos32

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20):
        if self.state[1] != 0:
            return
        step, code, mode, f, e = self._begin_finish(f32, energy, total, capacity, self.R)
        if code == 0 and mode == 0:
            # remd_decide
            self.rung_new, self.vscale = self.rung.copy(), np.ones(self.R)
            self.outcome[:] = 0
            for r, ga, gb, delta, log_u, yes in decide(self.seed, step, self.interval, self.beta, e, self.replica_at):
                self.decisions.append((step, r, ga, gb, delta, log_u, yes))
                self.outcome[r] = 2 if yes else 1
                if yes:
                    self.rung_new[ga], self.rung_new[gb] = r + 1, r
                    self.vscale[ga], self.vscale[gb] = self.up[r], self.down[r]
            # remd_apply_replica
            for g in range(self.R):
                lo, hi = g * self.n_rep, (g + 1) * self.n_rep
                self.log[step % self.log_steps, g] = (np.float64(e[g]), canonical_sum(self.ke_atom[lo:hi]), float(total[0]),
                                                      float(self.rung[g]), float(self.rung_new[g]))
                if self.rung_new[g] != self.rung[g]:
                    self.v[lo:hi] = self.v[lo:hi] * self.vscale[g]
                    self.sigma[lo:hi] = self.sigma_table[self.rung_new[g]]
            # remd_commit
            self.rung = self.rung_new.copy()
            self.replica_at[self.rung_new] = np.arange(self.R)
            self.attempts += self.outcome != 0
            self.accepts += self.outcome == 2
        self._commit(step, code, mode)
