"""Shared by tests/test_pimd_host.py and tests/test_pimd_device.py: `NumpyPIMD`, the numpy transcription of the ring-polymer
step (hermnet_amd/csrc/pimd_step.h and md_finish.h, operation by operation: numpy's elementwise float64 +, * and floor round
once each, like the contraction-free C), and `HostPIMD`, a thin wrapper that runs the library's host twins
(hermnet_host_pimd_advance / _finish) on numpy arrays.  Both take the host-made tables of hermnet_amd/pimd.py: ring_tables."""
import types

import numpy as np

from hermnet_amd.pimd import ring_tables
from md_reference import AMU, KB, LANGEVIN, HostMD, _p, _State, host_noise
from remd_reference import canonical_sum

FIELDS = ("x", "v", "image", "f_prev", "pos32", "centroid", "log", "state", "x0", "v0", "image0")


def estimators(log, beads, n_free, temperature):
    """hermnet_amd/pimd.py: DevicePIMD.estimators on a log [rows,P,5]: (potential, kinetic_primitive, kinetic_virial,
    ring_energy)."""
    kt = KB * temperature
    return (log[:, :, 0].sum(axis=1) / beads, 1.5 * n_free * beads * kt - log[:, :, 3].sum(axis=1) / beads,
            1.5 * n_free * kt - log[:, :, 4].sum(axis=1) / (2.0 * beads), (log[:, :, 1] + log[:, :, 3] + log[:, :, 0]).sum(axis=1))


class _Ring(object):
    def _make_ring(self, beads, masses, dt, temperature, tau0, pile_lambda, thermostat, log_steps):
        self.P, self.n_rep = beads, self.n // beads
        self.temperature, self.thermostat = temperature, thermostat
        self.tables = tb = ring_tables(beads, dt, temperature, np.asarray(masses, dtype=np.float64)[:self.n_rep] * AMU, tau0,
                                       pile_lambda, thermostat)
        self.cmat, self.cs, self.sw, self.ws, self.c1, self.sigma = tb.cmat, tb.cs, tb.sw, tb.ws, tb.c1, tb.sigma
        self.spring_c, self.inv_beads = tb.spring_c, tb.inv_beads
        self.centroid = np.zeros((self.n_rep, 3))
        self.log_steps = log_steps
        self.log = np.full((log_steps, beads, 5), -7.0)
        self.n_free = int(np.count_nonzero(np.isfinite(np.asarray(masses, dtype=np.float64)[:self.n_rep])))

    def snapshot(self):
        return types.SimpleNamespace(**{k: getattr(self, k).copy() for k in FIELDS})

    def estimators(self, rows=None):
        return estimators(self.log[:rows], self.P, self.n_free, self.temperature)


class HostPIMD(_Ring, HostMD):
    """hermnet_host_pimd_advance + hermnet_host_pimd_finish on numpy arrays.  x [P n_rep, 3]: bead j's atoms are rows
    j n_rep .. (j+1) n_rep; masses [P n_rep] (amu); cell [3,3] or None."""

    def __init__(self, beads, x, v, masses, dt, temperature, tau0=100.0, pile_lambda=1.0, thermostat=True, seed=0, log_steps=64,
                 cell=None):
        batch = np.repeat(np.arange(beads), len(x) // beads)
        cells = None if cell is None else np.tile(np.asarray(cell, dtype=np.float32).reshape(1, 3, 3), (beads, 1, 1))
        HostMD.__init__(self, x, v, masses, dt, cell=cells, batch=batch, seed=seed, log_steps=log_steps, num_graphs=beads)
        if thermostat:
            self.flags |= LANGEVIN
        self._make_ring(beads, masses, dt, temperature, tau0, pile_lambda, thermostat, log_steps)

    def advance(self, expect=0):
        rc = self.lib.hermnet_host_pimd_advance(
            self.n, self.B, self.flags, self.seed, self.inv_beads, _p(self.x), _p(self.v), _p(self.x0), _p(self.v0),
            _p(self.image), _p(self.image0), _p(self.f_prev), _p(self.kick), _p(self.cmat), _p(self.cs), _p(self.sw), _p(self.ws),
            _p(self.c1), _p(self.sigma), _p(self.cell), _p(self.inv), _p(self.pos32), _p(self.centroid), _p(self.state))
        assert rc == expect, rc
        return self.pos32

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20, expect=0):
        f, e, tot = self._evaluation(f32, energy, total)
        rc = self.lib.hermnet_host_pimd_finish(
            self.n, self.B, _p(self.graph_ptr), _p(f), _p(e), _p(tot), capacity, *self._finish_atoms(), _p(self.spring_c),
            _p(self.centroid), *self._finish_tail())
        assert rc == expect, rc


class NumpyPIMD(_Ring, _State):
    """The reference: pimd_step.h's phases and the finish in numpy float64, operation by operation.  The Gaussians are those
    of the library's host form (`host_noise`), or `gaussians(step)` [P n_rep, 3] where one is given."""

    def __init__(self, beads, x, v, masses, dt, temperature, tau0=100.0, pile_lambda=1.0, thermostat=True, seed=0, log_steps=64,
                 cell=None, gaussians=None):
        self._make_state(x, v)
        m = np.asarray(masses, dtype=np.float64) * AMU
        self.dt, self.seed, self.gaussians = float(dt), seed, gaussians
        self.kick, self.half_mass = 0.5 * self.dt / m, np.where(np.isfinite(m), 0.5 * m, 0.0)
        self.cell = self.inv = None
        if cell is not None:
            c = np.tile(np.asarray(cell, dtype=np.float32).reshape(1, 3, 3), (beads, 1, 1)).astype(np.float64)
            self.cell, self.inv = c[0], np.linalg.inv(c)[0]
        self._make_ring(beads, masses, dt, temperature, tau0, pile_lambda, thermostat, log_steps)

    def _flight(self, q, v):
        cs, sw, ws = (t[:, None, None] for t in (self.cs, self.sw, self.ws))
        return cs * q + sw * v, cs * v - ws * q

    def advance(self):
        step, code, mode = (int(w) for w in self.state[[0, 1, 3]])
        if code != 0:
            return self.pos32
        if mode == 0:
            P, nr, C = self.P, self.n_rep, self.cmat
            self.x0[:], self.v0[:], self.image0[:] = self.x, self.v, self.image
            X, V, I = self.x.reshape(P, nr, 3), self.v.reshape(P, nr, 3), self.image.reshape(P, nr, 3)
            F = self.f_prev.astype(np.float64).reshape(P, nr, 3)
            kick = self.kick[:nr]
            free = kick != 0.0
            xb, vb = X[:, free], V[:, free] + kick[free][None, :, None] * F[:, free]          # B
            q, u = np.zeros_like(xb), np.zeros_like(vb)
            for j in range(P):                                                                # to modes
                q = q + C[j, :, None, None] * xb[j][None]
                u = u + C[j, :, None, None] * vb[j][None]
            q, u = self._flight(q, u)                                                         # A
            if self.thermostat:
                xi = self.gaussians(step) if self.gaussians is not None else host_noise(self.seed, step, self.n)[1]
                xi = np.asarray(xi).reshape(P, nr, 3)[:, free]
                u = self.c1[:, None, None] * u + self.sigma[:, free, None] * xi               # O
                q, u = self._flight(q, u)                                                     # A
            xn, vn = np.zeros_like(q), np.zeros_like(u)
            for k in range(P):                                                                # back to beads
                xn = xn + C[:, k, None, None] * q[k][None]
                vn = vn + C[:, k, None, None] * u[k][None]
            X[:, free], V[:, free] = xn, vn
            c = np.zeros((nr, 3))
            for j in range(P):
                c = c + X[j]
            c = c * self.inv_beads
            if self.cell is not None:                                                         # the wrap by the centroid
                cell, inv = self.cell, self.inv
                s = (c[:, 0:1] * inv[0][None, :] + c[:, 1:2] * inv[1][None, :]) + c[:, 2:3] * inv[2][None, :]
                with np.errstate(invalid="ignore"):
                    fl = np.floor(s)
                    n = np.where((fl >= -1073741824.0) & (fl <= 1073741824.0) & free[:, None], fl, 0.0)
                shift = (n[:, 0:1] * cell[0][None, :] + n[:, 1:2] * cell[1][None, :]) + n[:, 2:3] * cell[2][None, :]
                c[free] = (c - shift)[free]
                X[:] = X - shift[None]
                I += n.astype(np.int32)[None]
            self.centroid = c
        self.pos32 = self.x.astype(np.float32)
        return self.pos32

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20):
        if self.state[1] != 0:
            return
        P, nr = self.P, self.n_rep
        step, code, mode, f, e = self._begin_finish(f32, energy, total, capacity, P)
        if code == 0 and mode == 0:
            X, F = self.x.reshape(P, nr, 3), f.astype(np.float64).reshape(P, nr, 3)
            free = self.half_mass[:nr] != 0.0
            for j in range(P):                                       # pimd_log_bead
                d, r, g = X[j] - X[(j + 1) % P], X[j] - self.centroid, F[j]
                spring = self.spring_c * ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                vir = (r[:, 0] * g[:, 0] + r[:, 1] * g[:, 1]) + r[:, 2] * g[:, 2]
                ke = self.ke_atom[j * nr:(j + 1) * nr]
                self.log[step % self.log_steps, j] = (np.float64(e[j]), canonical_sum(np.where(free, ke, 0.0)), float(total[0]),
                                                      canonical_sum(np.where(free, spring, 0.0)),
                                                      canonical_sum(np.where(free, vir, 0.0)))
        self._commit(step, code, mode)
