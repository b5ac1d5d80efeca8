"""Shared by tests/test_nhc_host.py and tests/test_nhc_device.py: the numpy / Python float64 transcription of the Nose-Hoover
chain step (hermnet_amd/csrc/nhc_step.h around md_step.h / md_finish.h, operation by operation: Python's float +, * round
once each, like the contraction-free C), the chains' tables made independently of hermnet_amd/nhc.py, a thin wrapper that
runs the library's host twins (hermnet_host_nhc_advance / _finish) on numpy arrays, and the coupled anharmonic system of
the conservation and sampling tests."""
import math
import types

import numpy as np

from md_reference import AMU, KB, HostMD, NumpyMD, _p, advance_np
from metad_reference import _COEFFS, LN2_HI, LN2_LO, LOG2E
from remd_reference import canonical_sum


def py_exp(a):
    """mt_exp (csrc/metad_step.h) on one Python float."""
    if not (a >= -745.0):
        return 0.0
    k = math.floor(a * LOG2E + 0.5)
    r = (a - k * LN2_HI) - k * LN2_LO
    p = _COEFFS[0]
    for c in _COEFFS[1:]:
        p = p * r + c
    return math.ldexp(p, k)


def weights(order):
    if order == 1:
        return [1.0]
    if order == 3:
        w = 1.0 / (2.0 - 2.0 ** (1.0 / 3.0))
        return [w, 1.0 - 2.0 * w, w]
    w = 1.0 / (4.0 - 4.0 ** (1.0 / 3.0))
    return [w, w, 1.0 - 4.0 * w, w, w]


def tables(temperature, tau, dof, dt, chain, order, substeps):
    """(delta [order], kt [B], dof_kt [B], q [B,M], inv_q [B,M]) in plain loops."""
    B = len(temperature)
    delta = np.array([w * (0.5 * dt) / float(substeps) for w in weights(order)])
    kt, dof_kt = np.zeros(B), np.zeros(B)
    q, inv_q = np.zeros((B, chain)), np.zeros((B, chain))
    for g in range(B):
        kt[g] = KB * float(temperature[g])
        dof_kt[g] = float(dof[g]) * kt[g]
        if math.isfinite(tau[g]):
            for j in range(chain):
                q[g, j] = (dof_kt[g] if j == 0 else kt[g]) * (float(tau[g]) * float(tau[g]))
                inv_q[g, j] = 1.0 / q[g, j]
    return delta, kt, dof_kt, q, inv_q


def half_step(delta, substeps, kt, dof_kt, q, inv_q, xi, v, k2):
    """nhc_half_step on Python lists xi, v (in place) and the float k2: (s, k2)."""
    M = len(xi)

    def force(j):
        if j == 0:
            return (k2 - dof_kt) * inv_q[0]
        return (q[j - 1] * (v[j - 1] * v[j - 1]) - kt) * inv_q[j]

    s = 1.0
    for _ in range(substeps):
        for d in delta:
            d2, d4 = 0.5 * d, 0.25 * d
            v[M - 1] = v[M - 1] + force(M - 1) * d2
            for j in range(M - 2, -1, -1):
                e = py_exp(-(d4 * v[j + 1]))
                v[j] = (v[j] * e + force(j) * d2) * e
            a = py_exp(-(d * v[0]))
            s = s * a
            k2 = (k2 * a) * a
            for j in range(M):
                xi[j] = xi[j] + d * v[j]
            for j in range(M - 1):
                e = py_exp(-(d4 * v[j + 1]))
                v[j] = (v[j] * e + force(j) * d2) * e
            v[M - 1] = v[M - 1] + force(M - 1) * d2
    return s, k2


def chain_energy(kt, dof_kt, q, xi, v):
    """nhc_energy."""
    e = dof_kt * xi[0]
    for j in range(1, len(xi)):
        e = e + kt * xi[j]
    for j in range(len(xi)):
        e = e + 0.5 * (q[j] * (v[j] * v[j]))
    return e


class _Chains(object):
    """What NumpyNHC and HostNHC share: the chains' constants and state in the layout of include/hermnet_hip.h."""

    def _make_chains(self, temperature, tau, dof, chain, order, substeps, B, log_steps):
        per = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1), (B,)).copy()
        self.chain, self.order, self.substeps = int(chain), int(order), int(substeps)
        self.dof = per(dof)
        self.delta, self.kt, self.dof_kt, self.q, self.inv_q = tables(per(temperature), per(tau), self.dof, self.dt, self.chain,
                                                                      self.order, self.substeps)
        self.xi, self.v_xi = np.zeros((B, self.chain)), np.zeros((B, self.chain))
        self.xi0, self.v_xi0 = np.full((B, self.chain), -7.0), np.full((B, self.chain), -7.0)
        self.scale = np.ones((B, 2))
        self.log_steps, self.log = log_steps, np.full((log_steps, B, 4), -7.0)

    def snapshot(self):
        names = ("x", "v", "image", "f_prev", "pos32", "xi", "v_xi", "scale", "log", "state")
        return types.SimpleNamespace(**{k: getattr(self, k).copy() for k in names})


class HostNHC(_Chains, HostMD):
    """hermnet_host_nhc_advance + hermnet_host_nhc_finish on numpy arrays."""

    def __init__(self, x, v, masses, dt, temperature, tau, dof, chain=3, order=3, substeps=1, cell=None, batch=None,
                 log_steps=64, num_graphs=None):
        HostMD.__init__(self, x, v, masses, dt, cell=cell, batch=batch, log_steps=log_steps, num_graphs=num_graphs)
        self._make_chains(temperature, tau, dof, chain, order, substeps, self.B, log_steps)

    def _chains(self):
        return (self.chain, self.order, self.substeps, _p(self.delta), _p(self.kt), _p(self.dof_kt), _p(self.q), _p(self.inv_q),
                _p(self.xi), _p(self.v_xi), _p(self.xi0), _p(self.v_xi0), _p(self.scale))

    def advance(self, expect=0):
        rc = self.lib.hermnet_host_nhc_advance(
            self.n, self.B, self.flags, self.dt, _p(self.x), _p(self.v), _p(self.x0), _p(self.v0), _p(self.image),
            _p(self.image0), _p(self.f_prev), _p(self.kick), _p(self.batch), _p(self.cell), _p(self.inv), _p(self.pos32),
            _p(self.state), _p(self.graph_ptr), _p(self.half_mass), *self._chains())
        assert rc == expect, rc
        return self.pos32

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20, expect=0):
        f, e, tot = self._evaluation(f32, energy, total)
        rc = self.lib.hermnet_host_nhc_finish(self.n, self.B, _p(self.graph_ptr), _p(self.batch), _p(f), _p(e), _p(tot), capacity,
                                              *self._finish_atoms(), *self._chains(), *self._finish_tail())
        assert rc == expect, rc


class NumpyNHC(_Chains, NumpyMD):
    """The reference: nhc_step.h around md_advance_one and md_finish.h's skeleton, operation by operation."""

    def __init__(self, x, v, masses, dt, temperature, tau, dof, chain=3, order=3, substeps=1, cell=None, batch=None,
                 log_steps=64, num_graphs=None):
        NumpyMD.__init__(self, x, v, masses, dt, cell=cell, batch=batch, num_graphs=num_graphs)
        self.B = int(num_graphs) if num_graphs is not None else int(self.batch[-1]) + 1
        self.graph_ptr = np.searchsorted(self.batch, np.arange(self.B + 1))
        self._make_chains(temperature, tau, dof, chain, order, substeps, self.B, log_steps)

    def _half(self, g, e_kin, slot):
        """nhc_graph_one; returns s."""
        xi, v = self.xi[g].tolist(), self.v_xi[g].tolist()
        s, _ = half_step(self.delta.tolist(), self.substeps, float(self.kt[g]), float(self.dof_kt[g]), self.q[g].tolist(),
                         self.inv_q[g].tolist(), xi, v, 2.0 * float(e_kin))
        self.xi[g], self.v_xi[g], self.scale[g, slot] = xi, v, s
        return s

    def advance(self):
        if self.state[1] != 0:
            return self.pos32
        if self.state[3] == 0:
            v = self.v
            ke = self.half_mass * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            self.xi0[:], self.v_xi0[:] = self.xi, self.v_xi
            for g in range(self.B):
                self._half(g, canonical_sum(ke[self.graph_ptr[g]:self.graph_ptr[g + 1]]), 0)
            self.x0[:], self.v0[:], self.image0[:] = self.x, self.v, self.image
            self.v[:] = self.v * self.scale[self.batch, 0][:, None]
            advance_np(self.x, self.v, self.image, self.f_prev, self.kick, self.dt, None, None, None, self.cell, self.inv)
        self.pos32 = self.x.astype(np.float32)
        return self.pos32

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20):
        if self.state[1] != 0:
            return
        step, code, mode, f, e = self._begin_finish(f32, energy, total, capacity, self.B)
        if mode == 0 and code != 0:
            self.xi[:], self.v_xi[:] = self.xi0, self.v_xi0
        elif mode == 0:
            for g in range(self.B):
                k = canonical_sum(self.ke_atom[self.graph_ptr[g]:self.graph_ptr[g + 1]])
                s = self._half(g, k, 1)
                e_nhc = chain_energy(float(self.kt[g]), float(self.dof_kt[g]), self.q[g].tolist(), self.xi[g].tolist(),
                                     self.v_xi[g].tolist())
                self.log[step % self.log_steps, g] = (np.float64(e[g]), (float(k) * s) * s, float(total[0]), e_nhc)
            self.v[:] = self.v * self.scale[self.batch, 1][:, None]
        self._commit(step, code, mode)


# ---- the coupled anharmonic system of the conservation and sampling tests --------------------------------------------------------
class Wells(object):
    """n atoms of unequal masses, each in an ANISOTROPIC quartic well c4 (sum_k alpha_k u_k^2)^2 around its own site (u = x -
    site; alpha in [0.5, 1.5] per atom and axis), neighbours on a ring coupled by harmonic springs k |u_i - u_{i+1}|^2 / 2:
    anharmonic, coupled, no conserved momentum (dof = 3 n).  (In isotropic wells every atom nearly keeps its own angular
    momentum, and the chain then samples Var(E_kin) 5 to 20 % too wide on runs of this length: not ergodic enough.)
    Evaluated in float64 at the float32 coordinates an advance hands out; energy and forces are returned in float32."""

    def __init__(self, n=16, c4=30.0, k=2.0):
        rs = np.random.RandomState(7)
        self.n, self.c4, self.k = n, c4, k
        self.sites = np.stack([1.5 * np.arange(n), np.zeros(n), np.zeros(n)], axis=1)
        self.alpha = rs.uniform(0.5, 1.5, (n, 3))
        self.masses = rs.uniform(10.0, 40.0, n)

    def evaluate(self, pos32):
        u = pos32.astype(np.float64) - self.sites
        r2 = (self.alpha * u * u).sum(axis=1)
        d = u - np.roll(u, -1, axis=0)
        e = self.c4 * (r2 * r2).sum() + 0.5 * self.k * (d * d).sum()
        f = -4.0 * self.c4 * r2[:, None] * self.alpha * u - self.k * (d - np.roll(d, 1, axis=0))
        return f.astype(np.float32), np.array([e], dtype=np.float32)

    def start(self, temperature, seed):
        """(x, v): the sites, and Maxwell-Boltzmann velocities at 2 T (half of it becomes potential energy)."""
        rs = np.random.RandomState(seed)
        v = rs.standard_normal((self.n, 3)) * np.sqrt(KB * 2.0 * temperature / (self.masses * AMU))[:, None]
        return self.sites.copy(), v


def run_wells(driver, wells, steps):
    """Prime, then `steps` time steps of `driver` (a HostNHC or NumpyNHC with log_steps >= steps) in the wells: the log."""
    driver.state[3] = 1
    for _ in range(steps + 1):
        f, e = wells.evaluate(driver.advance())
        driver.finish(f, e)
    assert driver.state.tolist() == [steps, 0, 0, 0]
    return driver.log[:steps, 0].copy()
