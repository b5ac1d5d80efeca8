"""Shared by tests/test_swapmc_host.py and tests/test_swapmc_device.py: the numpy transcription of the species-swap protocol
(hermnet_amd/csrc/swapmc_step.h around md_step.h / md_finish.h, operation by operation), the candidate tables made
independently of hermnet_amd/swapmc.py, and a thin wrapper that runs the library's host twins (hermnet_host_swapmc_advance /
_finish) on numpy arrays."""
import math
import types

import numpy as np

from md_reference import KB, M32, HostMD, NumpyMD, _p, advance_np, host_noise, philox4x32_10
from remd_reference import canonical_sum


def tables(z, masses, batch, num_graphs):
    """(cand int32, cand_ptr int32 [B, S+1], S): per graph the atoms of finite mass sorted by (species index, atom); species
    index = rank of the atomic number among the batch's.  Plain loops."""
    species = sorted(set(int(v) for v in z))
    S = max(1, len(species))
    cand, ptr = [], np.zeros((num_graphs, S + 1), dtype=np.int32)
    for g in range(num_graphs):
        for k in range(S):
            ptr[g, k] = len(cand)
            cand += [i for i in range(len(z)) if batch[i] == g and np.isfinite(masses[i]) and species and int(z[i]) == species[k]]
        ptr[g, S] = len(cand)
    return np.array(cand, dtype=np.int32), ptr, S


def trial_words(seed, t, g):
    """The four words of graph g's trial t: key (seed low, seed high), counter (g, t low, t high, 3)."""
    return philox4x32_10((g, t & M32, (t >> 32) & M32, 3), (seed & M32, (seed >> 32) & M32))


def pick_pair(seed, t, g, cand, ptr):
    """swapmc_pick: (i, j) of graph g at trial t from its row `ptr` [S+1] of cand_ptr, or None where it is not tried."""
    w = trial_words(seed, t, g)
    S, base = len(ptr) - 1, int(ptr[0])
    m = int(ptr[S]) - base
    if m <= 0:
        return None
    at = (w[0] * m) >> 32
    s = [k for k in range(S) if int(ptr[k]) - base <= at < int(ptr[k + 1]) - base][0]
    m_s = int(ptr[s + 1]) - int(ptr[s])
    if m - m_s == 0:
        return None
    k = (w[1] * (m - m_s)) >> 32
    q = k if k < int(ptr[s]) - base else k + m_s
    return int(cand[base + at]), int(cand[base + q])


def trial_uniform(seed, t, g):
    w = trial_words(seed, t, g)
    return (float(((w[2] >> 5) << 26) | (w[3] >> 6)) + 1.0) * (1.0 / 9007199254740992.0)


def decide(seed, t, g, beta_g, energy32_g, e_ref_g):
    """swapmc_decide's arithmetic for one tried graph: (d, delta, log u, accepted)."""
    d = np.float64(np.float32(energy32_g)) - np.float64(e_ref_g)
    delta = -np.float64(beta_g) * d
    log_u = math.log(trial_uniform(seed, t, g))
    return float(d), float(delta), log_u, bool(delta >= 0.0 or log_u < delta)


class _Swaps(object):
    """What NumpySwapMC and HostSwapMC share: the swaps' constants and state in the layout of include/hermnet_hip.h."""

    def _make_swaps(self, z, masses, interval, swaps, mc_temperature, swap_rows, B):
        self.interval, self.swaps, self.swap_rows = int(interval), int(swaps), int(swap_rows)
        t = np.broadcast_to(np.asarray(mc_temperature, dtype=np.float64).reshape(-1), (B,)) if np.ndim(mc_temperature) else \
            np.full(B, float(mc_temperature))
        self.beta = 1.0 / (KB * t)
        self.cand, self.cand_ptr, self.S = tables(z, masses, self.batch, B)
        self.num_cand = len(self.cand)
        self.e_ref = np.zeros(B)
        self.mc = np.zeros(2, dtype=np.int64)
        self.attempts, self.accepts = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        self.swap_log = np.full((self.swap_rows, B, 4), -7.0)
        self.pair = np.full((B, 2), -1, dtype=np.int32)
        self.dval, self.outcome = np.zeros(B), np.zeros(B, dtype=np.int64)

    def kind(self):
        """What the next replay is: "halted", "prime", "trial" or "md"."""
        if self.state[1] != 0:
            return "halted"
        return "prime" if self.state[3] != 0 else ("trial" if self.mc[1] > 0 else "md")

    def snapshot(self):
        names = ("x", "v", "image", "f_prev", "pos32", "e_ref", "mc", "attempts", "accepts", "swap_log", "log", "state")
        return types.SimpleNamespace(**{k: getattr(self, k).copy() for k in names})


class HostSwapMC(_Swaps, HostMD):
    """hermnet_host_swapmc_advance + hermnet_host_swapmc_finish on numpy arrays."""

    def __init__(self, x, v, z, masses, dt, interval, swaps, mc_temperature, cell=None, batch=None, friction=None,
                 temperature=None, seed=0, log_steps=64, swap_rows=64, num_graphs=None):
        HostMD.__init__(self, x, v, masses, dt, cell=cell, batch=batch, friction=friction, temperature=temperature, seed=seed,
                        log_steps=log_steps, num_graphs=num_graphs)
        self._make_swaps(z, masses, interval, swaps, mc_temperature, swap_rows, self.B)

    def _tables(self):
        return _p(self.cand), _p(self.cand_ptr), self.S, self.num_cand

    def advance(self, expect=0):
        rc = self.lib.hermnet_host_swapmc_advance(
            self.n, self.B, self.flags, self.dt, self.seed, _p(self.x), _p(self.v), _p(self.x0), _p(self.v0), _p(self.image),
            _p(self.image0), _p(self.f_prev), _p(self.kick), _p(self.c1), _p(self.sigma), _p(self.batch), _p(self.cell),
            _p(self.inv), _p(self.pos32), _p(self.state), _p(self.mc), _p(self.graph_ptr), *self._tables())
        assert rc == expect, rc
        return self.pos32

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20, expect=0):
        f, e, tot = self._evaluation(f32, energy, total)
        rc = self.lib.hermnet_host_swapmc_finish(
            self.n, self.B, _p(self.graph_ptr), _p(self.batch), _p(f), _p(e), _p(tot), capacity, self.interval, self.swaps,
            self.seed, *self._finish_atoms(), _p(self.beta), _p(self.e_ref), _p(self.mc), *self._tables(), _p(self.pair),
            _p(self.dval), _p(self.outcome), _p(self.attempts), _p(self.accepts), _p(self.swap_log), self.swap_rows,
            *self._finish_tail())
        assert rc == expect, rc


class NumpySwapMC(_Swaps, NumpyMD):
    """The reference: md_advance_one (the noise of the library's host form), md_finish.h's skeleton and swapmc_step.h in
    numpy float64, operation by operation.  `decisions`: every tried graph, (t, g, i, j, d, delta, log u, accepted)."""

    def __init__(self, x, v, z, masses, dt, interval, swaps, mc_temperature, cell=None, batch=None, friction=None,
                 temperature=None, seed=0, log_steps=64, swap_rows=64, num_graphs=None):
        NumpyMD.__init__(self, x, v, masses, dt, cell=cell, batch=batch, friction=friction, temperature=temperature, seed=seed,
                         num_graphs=num_graphs)
        self.B = int(num_graphs) if num_graphs is not None else int(self.batch[-1]) + 1
        self.graph_ptr = np.searchsorted(self.batch, np.arange(self.B + 1))
        self.log_steps, self.log = log_steps, np.full((log_steps, self.B, 3), -7.0)
        self.decisions = []
        self._make_swaps(z, masses, interval, swaps, mc_temperature, swap_rows, self.B)

    def _exchange(self, i, j):
        """swapmc_exchange."""
        self.x[[i, j]], self.image[[i, j]] = self.x[[j, i]], self.image[[j, i]]
        self.pos32[[i, j]] = self.x[[i, j]].astype(np.float32)

    def _pairs(self, t):
        return [pick_pair(self.seed, t, g, self.cand, self.cand_ptr[g]) for g in range(self.B)]

    def advance(self):
        kind = self.kind()
        step, t = int(self.state[0]), int(self.mc[0])
        if kind == "halted":
            return self.pos32
        if kind == "trial":
            for pair in self._pairs(t):
                if pair is not None:
                    self._exchange(*pair)
            return self.pos32
        if kind == "md":
            self.x0[:], self.v0[:], self.image0[:] = self.x, self.v, self.image
            xi = host_noise(self.seed, step, self.n)[1] if self.c1_atom is not None else None
            advance_np(self.x, self.v, self.image, self.f_prev, self.kick, self.dt, self.c1_atom, self.sigma, xi, self.cell, self.inv)
        self.pos32 = self.x.astype(np.float32)
        return self.pos32

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20):
        kind = self.kind()
        if kind == "halted":
            return
        if kind != "trial":
            step, code, mode, f, e = self._begin_finish(f32, energy, total, capacity, self.B)
            if code == 0:
                self.e_ref = e.astype(np.float64)
                if mode == 0:
                    for g in range(self.B):
                        lo, hi = self.graph_ptr[g], self.graph_ptr[g + 1]
                        self.log[step % self.log_steps, g] = (np.float64(e[g]), canonical_sum(self.ke_atom[lo:hi]), float(total[0]))
            self._commit(step, code, mode)
            if code == 0 and mode == 0 and (step + 1) % self.interval == 0:
                self.mc[1] = self.swaps
            return
        step, t, left = int(self.state[0]), int(self.mc[0]), int(self.mc[1])
        f = np.array(f32, dtype=np.float32)
        e = np.zeros(self.B, dtype=np.float32) if energy is None else np.array(energy, dtype=np.float32)
        code = (int(total[1]) & 255) | (4 if int(total[0]) > capacity else 0) | (0 if np.all(np.isfinite(e)) else 256)
        pairs = self._pairs(t)
        if code != 0:                                     # void: everyone back, the halt recorded, t and left stay
            for pair in pairs:
                if pair is not None:
                    self._exchange(*pair)
            self.state[1], self.state[2] = code, step
            return
        for g, pair in enumerate(pairs):
            row = self.swap_log[t % self.swap_rows, g]
            if pair is None:
                row[:] = (-1.0, -1.0, 0.0, 0.0)
                continue
            d, delta, log_u, yes = decide(self.seed, t, g, self.beta[g], e[g], self.e_ref[g])
            self.decisions.append((t, g, pair[0], pair[1], d, delta, log_u, yes))
            row[:] = (float(pair[0]), float(pair[1]), d, 2.0 if yes else 1.0)
            self.attempts[g] += 1
            if yes:
                lo, hi = self.graph_ptr[g], self.graph_ptr[g + 1]
                self.f_prev[lo:hi] = f[lo:hi]
                self.e_ref[g] = np.float64(e[g])
                self.accepts[g] += 1
            else:
                self._exchange(*pair)
        self.mc[0], self.mc[1] = t + 1, left - 1
