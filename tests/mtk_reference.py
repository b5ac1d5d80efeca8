"""Shared by tests/test_mtk_host.py and tests/test_mtk_device.py: the numpy / Python float64 transcription of the MTK
barostat step (hermnet_amd/csrc/mtk_step.h, operation by operation: Python's float +, * round once each, like the
contraction-free C), the barostat's tables made independently of hermnet_amd/mtk.py, a thin wrapper that runs the library's
host twins (hermnet_host_mtk_advance / _finish) on numpy arrays, and the pair-potential system of the conservation,
reversibility and sampling tests."""
import math
import types

import numpy as np

from md_reference import AMU, KB, NONFINITE, HostMD, NumpyMD, _p
from nhc_reference import _Chains, chain_energy, half_step, py_exp
from remd_reference import canonical_sum

ISOTROPIC, AXES = 0, 1
STATE_FIELDS = ("x", "v", "x0", "v0", "image", "image0", "f_prev", "pos32", "xi", "v_xi", "xi0", "v_xi0", "scale", "log", "state",
                "xi_b", "v_xi_b", "scale_b", "v_cell", "cell64", "cell32", "inv_cell", "w_prev", "factors", "backup", "flag",
                "refused")


def sinhc(x):
    """mtk_sinhc on one Python float."""
    y = x * x
    p = 1.0 / 39916800.0
    for c in (1.0 / 362880.0, 1.0 / 5040.0, 1.0 / 120.0, 1.0 / 6.0, 1.0):
        p = p * y + c
    return p


def det3(c):
    """npt_det3 on a list of 9 Python floats."""
    return (c[0] * (c[4] * c[8] - c[5] * c[7]) + c[1] * (c[5] * c[6] - c[3] * c[8])) + c[2] * (c[3] * c[7] - c[4] * c[6])


def inverse3(c):
    """npt_inverse3."""
    det = det3(c)
    adj = [c[4] * c[8] - c[5] * c[7], c[2] * c[7] - c[1] * c[8], c[1] * c[5] - c[2] * c[4],
           c[5] * c[6] - c[3] * c[8], c[0] * c[8] - c[2] * c[6], c[2] * c[3] - c[0] * c[5],
           c[3] * c[7] - c[4] * c[6], c[1] * c[6] - c[0] * c[7], c[0] * c[4] - c[1] * c[3]]
    return [t / det for t in adj]


def baro_tables(temperature, tau, taup, dof, pressure, coupling, mask, chain):
    """(par [B,5], dof_kt_b [B], q_b [B,M], inv_q_b [B,M]) in plain loops; coupling: ISOTROPIC or AXES, mask: the bits."""
    B = len(temperature)
    par, dof_kt_b = np.zeros((B, 5)), np.zeros(B)
    q, inv_q = np.zeros((B, chain)), np.zeros((B, chain))
    dof_b = 1.0 if coupling == ISOTROPIC else float(sum((mask >> k) & 1 for k in range(3)))
    for g in range(B):
        kt = KB * float(temperature[g])
        d, tp = float(dof[g]), float(taup[g])
        if math.isfinite(tp):
            w = (d + 3.0) * kt * (tp * tp)
            if coupling == AXES:
                w = w / 3.0
            par[g, 0], par[g, 1] = w, 1.0 / w
        par[g, 2], par[g, 3], par[g, 4] = 1.0 + 3.0 / d, 1.0 / d, float(pressure[g])
        dof_kt_b[g] = dof_b * kt
        if math.isfinite(tp) and math.isfinite(tau[g]):
            for j in range(chain):
                q[g, j] = (dof_kt_b[g] if j == 0 else kt) * (tp * tp)
                inv_q[g, j] = 1.0 / q[g, j]
    return par, dof_kt_b, q, inv_q


class _Baro(object):
    """What NumpyMTK and HostMTK share: the barostat's constants and state in the layout of include/hermnet_hip.h."""

    def _make_baro(self, temperature, tau, taup, dof, pressure, coupling, mask, max_strain, cell, B, log_steps):
        per = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1), (B,)).copy()
        M = self.chain
        self.coupling = {"isotropic": ISOTROPIC, "axes": AXES}[coupling]
        self.mask = 7 if self.coupling == ISOTROPIC else sum(1 << k for k, on in enumerate(mask) if on)
        self.max_strain = float(max_strain)
        self.par, self.dof_kt_b, self.q_b, self.inv_q_b = baro_tables(per(temperature), per(tau), per(taup), per(dof),
                                                                      per(pressure), self.coupling, self.mask, M)
        self.xi_b, self.v_xi_b, self.scale_b = np.zeros((B, M)), np.zeros((B, M)), np.ones((B, 2))
        self.v_cell = np.zeros((B, 3))
        self.cell64 = np.array(cell, dtype=np.float64).reshape(B, 9)
        self.cell32 = np.ascontiguousarray(self.cell64.astype(np.float32))
        self.inv_cell = np.ascontiguousarray(np.linalg.inv(self.cell32.astype(np.float64).reshape(B, 3, 3))).reshape(B, 9)
        self.w_prev = np.zeros((B, 9), dtype=np.float32)
        self.factors, self.backup = np.ones((B, 12)), np.full((B, 2 * M + 30), -7.0)
        self.flag, self.refused = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        self.e_code = np.zeros(B, dtype=np.float32)
        self.log_steps, self.log = log_steps, np.full((log_steps, B, 7), -7.0)

    def snapshot(self):
        return types.SimpleNamespace(**{k: getattr(self, k).copy() for k in STATE_FIELDS})

    def volume(self):
        return np.array([abs(det3(c.tolist())) for c in self.cell64])

    def flip(self):
        """Time reversal: every velocity of the extended system changes its sign."""
        for a in (self.v, self.v_cell, self.v_xi, self.v_xi_b):
            a *= -1.0


class HostMTK(_Baro, _Chains, HostMD):
    """hermnet_host_mtk_advance + hermnet_host_mtk_finish on numpy arrays."""

    def __init__(self, x, v, masses, dt, temperature, tau, dof, cell, pressure=0.0, taup=1000.0, coupling="isotropic",
                 mask=(1, 1, 1), max_strain=1e-2, chain=3, order=3, substeps=1, batch=None, log_steps=64, num_graphs=None,
                 wrap=True):
        HostMD.__init__(self, x, v, masses, dt, cell=cell, batch=batch, log_steps=log_steps, num_graphs=num_graphs)
        if not wrap:
            self.flags = 0
        self._make_chains(temperature, tau, dof, chain, order, substeps, self.B, log_steps)
        self._make_baro(temperature, tau, taup, dof, pressure, coupling, mask, max_strain, cell, self.B, log_steps)

    def _chains(self):
        return (self.chain, self.order, self.substeps, _p(self.delta), _p(self.kt), _p(self.dof_kt), _p(self.q), _p(self.inv_q),
                _p(self.xi), _p(self.v_xi), _p(self.xi0), _p(self.v_xi0), _p(self.scale))

    def _baro(self):
        return (self.coupling, self.mask, self.max_strain, _p(self.par), _p(self.dof_kt_b), _p(self.q_b), _p(self.inv_q_b),
                _p(self.xi_b), _p(self.v_xi_b), _p(self.scale_b), _p(self.v_cell), _p(self.cell64), _p(self.cell32),
                _p(self.inv_cell), _p(self.w_prev), _p(self.factors), _p(self.backup), _p(self.flag), _p(self.refused),
                _p(self.e_code))

    def advance(self, expect=0):
        rc = self.lib.hermnet_host_mtk_advance(
            self.n, self.B, self.flags, self.dt, _p(self.x), _p(self.v), _p(self.x0), _p(self.v0), _p(self.image),
            _p(self.image0), _p(self.f_prev), _p(self.kick), _p(self.batch), _p(self.pos32), _p(self.state), _p(self.graph_ptr),
            _p(self.half_mass), *self._chains(), *self._baro())
        assert rc == expect, rc
        return self.pos32

    def finish(self, f32, energy=None, virial=None, total=(0, 0), capacity=1 << 20, expect=0):
        f, e, tot = self._evaluation(f32, energy, total)
        w = np.zeros((self.B, 9), dtype=np.float32) if virial is None else np.ascontiguousarray(virial, dtype=np.float32)
        rc = self.lib.hermnet_host_mtk_finish(self.n, self.B, _p(self.graph_ptr), _p(self.batch), _p(f), _p(e), _p(w), _p(tot),
                                              capacity, self.dt, *self._finish_atoms(), *self._chains(), *self._baro(),
                                              *self._finish_tail())
        assert rc == expect, rc


class NumpyMTK(_Baro, _Chains, NumpyMD):
    """The reference: mtk_step.h, operation by operation."""

    def __init__(self, x, v, masses, dt, temperature, tau, dof, cell, pressure=0.0, taup=1000.0, coupling="isotropic",
                 mask=(1, 1, 1), max_strain=1e-2, chain=3, order=3, substeps=1, batch=None, log_steps=64, num_graphs=None,
                 wrap=True):
        NumpyMD.__init__(self, x, v, masses, dt, cell=None, batch=batch, num_graphs=num_graphs)
        self.B = int(num_graphs) if num_graphs is not None else int(self.batch[-1]) + 1
        self.graph_ptr = np.searchsorted(self.batch, np.arange(self.B + 1))
        self.wrap = wrap
        self._make_chains(temperature, tau, dof, chain, order, substeps, self.B, log_steps)
        self._make_baro(temperature, tau, taup, dof, pressure, coupling, mask, max_strain, cell, self.B, log_steps)

    # ---- per graph ------------------------------------------------------------------------------------------------------------
    def _rate2(self, vg):
        """mtk_rate2."""
        if self.coupling == ISOTROPIC:
            return vg[0] * vg[0]
        s = 0.0
        for k in range(3):
            if self.mask & (1 << k):
                s = s + vg[k] * vg[k]
        return s

    def _baro_half(self, g, vg, slot):
        """mtk_baro_half on the list vg (in place); the barostat's chain is read and written."""
        xi, v = self.xi_b[g].tolist(), self.v_xi_b[g].tolist()
        k2 = float(self.par[g, 0]) * self._rate2(vg)
        s, _ = half_step(self.delta.tolist(), self.substeps, float(self.kt[g]), float(self.dof_kt_b[g]), self.q_b[g].tolist(),
                         self.inv_q_b[g].tolist(), xi, v, k2)
        self.xi_b[g], self.v_xi_b[g], self.scale_b[g, slot] = xi, v, s
        for k in range(3):
            vg[k] = vg[k] * s

    def _particles_half(self, g, e_kin, slot):
        """nhc_graph_one without the backup: (s, what the chain left of K2)."""
        xi, v = self.xi[g].tolist(), self.v_xi[g].tolist()
        s, k2 = half_step(self.delta.tolist(), self.substeps, float(self.kt[g]), float(self.dof_kt[g]), self.q[g].tolist(),
                          self.inv_q[g].tolist(), xi, v, 2.0 * float(e_kin))
        self.xi[g], self.v_xi[g], self.scale[g, slot] = xi, v, s
        return s, k2

    def _kick_baro(self, g, hdt, k2, kaa, w, vol, vg):
        """mtk_kick_baro; w: the virial as 9 Python floats."""
        par = self.par[g].tolist()
        inv_w, p0 = par[1], par[4]
        if inv_w == 0.0:
            return
        if self.coupling == ISOTROPIC:
            trw = (w[0] + w[4]) + w[8]
            gf = ((par[2] * k2 + trw) - (3.0 * p0) * vol) * inv_w
            vg[0] = vg[1] = vg[2] = vg[0] + hdt * gf
            return
        for k in range(3):
            if self.mask & (1 << k):
                gf = (((kaa[k] + w[4 * k]) - p0 * vol) + k2 * par[3]) * inv_w
                vg[k] = vg[k] + hdt * gf

    def _make_factors(self, g, vg):
        """mtk_make_factors: (refused?, the twelve)."""
        dt = self.dt
        hdt, qdt, inv_dof = 0.5 * dt, 0.25 * dt, float(self.par[g, 3])
        f = [1.0] * 12
        bad = any(not (abs(vg[k] * dt) <= self.max_strain) for k in range(3))
        if not bad:
            total = (vg[0] + vg[1]) + vg[2]
            for k in range(3):
                rho = vg[k] + total * inv_dof
                xa, xb, xr = rho * hdt, rho * qdt, vg[k] * hdt
                f[k] = py_exp(-xa)
                f[3 + k] = py_exp(-xb) * sinhc(xb)
                f[6 + k] = py_exp(vg[k] * dt)
                f[9 + k] = py_exp(xr) * sinhc(xr)
            bad = not all(math.isfinite(t) for t in f)
        return (1, [1.0] * 12) if bad else (0, f)

    def _sums(self, g, ke):
        """mtk_kinetic_sums from the per-atom kinetic energies `ke` and v."""
        lo, hi = self.graph_ptr[g], self.graph_ptr[g + 1]
        m, v = (2.0 * self.half_mass)[lo:hi], self.v[lo:hi]
        return float(canonical_sum(ke[lo:hi])), [float(canonical_sum((m * v[:, k]) * v[:, k])) for k in range(3)]

    def _open(self, g, e_kin, kaa_in):
        """mtk_open_one."""
        self.backup[g] = np.concatenate([self.xi_b[g], self.v_xi_b[g], self.v_cell[g], self.cell64[g],
                                         self.cell32[g].astype(np.float64), self.inv_cell[g]])
        vg, cell = self.v_cell[g].tolist(), self.cell64[g].tolist()
        self._baro_half(g, vg, 0)
        s, k2 = self._particles_half(g, e_kin, 0)
        kaa = [(t * s) * s for t in kaa_in]
        self._kick_baro(g, 0.5 * self.dt, k2, kaa, [float(t) for t in self.w_prev[g]], abs(det3(cell)), vg)
        self.v_cell[g] = vg
        self.flag[g], f = self._make_factors(g, vg)
        self.factors[g] = f
        if f[6] == 1.0 and f[7] == 1.0 and f[8] == 1.0:
            return
        new = [cell[3 * i + k] * f[6 + k] for i in range(3) for k in range(3)]
        self.cell64[g] = new
        self.cell32[g] = np.array(new, dtype=np.float64).astype(np.float32)
        self.inv_cell[g] = inverse3([float(t) for t in self.cell32[g]])

    # ---- the two halves ---------------------------------------------------------------------------------------------------------
    def advance(self):
        if self.state[1] != 0:
            return self.pos32
        if self.state[3] == 0:
            v = self.v
            ke = self.half_mass * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            self.xi0[:], self.v_xi0[:] = self.xi, self.v_xi
            for g in range(self.B):
                e_kin, kaa = self._sums(g, ke)
                self._open(g, e_kin, kaa)
            self.x0[:], self.v0[:], self.image0[:] = self.x, self.v, self.image
            fac = self.factors[self.batch]
            v = self.v * self.scale[self.batch, 0][:, None]
            v = v * fac[:, 0:3] + (self.kick[:, None] * self.f_prev.astype(np.float64)) * fac[:, 3:6]
            x = self.x * fac[:, 6:9] + (self.dt * v) * fac[:, 9:12]
            if self.wrap:
                cell = self.cell32.astype(np.float64).reshape(-1, 3, 3)[self.batch]
                inv = self.inv_cell.reshape(-1, 3, 3)[self.batch]
                s = (x[:, 0:1] * inv[:, 0, :] + x[:, 1:2] * inv[:, 1, :]) + x[:, 2:3] * inv[:, 2, :]
                with np.errstate(invalid="ignore"):
                    fl = np.floor(s)
                    n = np.where((fl >= -1073741824.0) & (fl <= 1073741824.0), fl, 0.0)
                x = x - ((n[:, 0:1] * cell[:, 0, :] + n[:, 1:2] * cell[:, 1, :]) + n[:, 2:3] * cell[:, 2, :])
                self.image += n.astype(np.int32)
            self.x[:], self.v[:] = x, v
        self.pos32 = self.x.astype(np.float32)
        return self.pos32

    def finish(self, f32, energy=None, virial=None, total=(0, 0), capacity=1 << 20):
        if self.state[1] != 0:
            return
        B, M = self.B, self.chain
        step, mode = int(self.state[0]), int(self.state[3])
        f = np.array(f32, dtype=np.float32)
        e = np.zeros(B, dtype=np.float32) if energy is None else np.array(energy, dtype=np.float32)
        w = np.zeros((B, 9), dtype=np.float32) if virial is None else np.array(virial, dtype=np.float32).reshape(B, 9)
        code = int(total[1]) & 255
        if int(total[0]) > capacity:
            code |= 4
        if not np.all(np.isfinite(e)):
            code |= NONFINITE
        if (mode == 0 and self.flag.any()) or not np.all(np.isfinite(w)):       # mtk_code
            code |= NONFINITE
        if mode != 0:
            if code == 0:
                self.f_prev, self.w_prev = f.copy(), w.copy()
        elif code != 0:
            self.x[:], self.image[:], self.v[:] = self.x0, self.image0, self.v0
            self.pos32 = self.x0.astype(np.float32)
            self.xi[:], self.v_xi[:] = self.xi0, self.v_xi0
            bk = self.backup
            self.xi_b[:], self.v_xi_b[:], self.v_cell[:] = bk[:, :M], bk[:, M:2 * M], bk[:, 2 * M:2 * M + 3]
            self.cell64[:], self.cell32[:] = bk[:, 2 * M + 3:2 * M + 12], bk[:, 2 * M + 12:2 * M + 21].astype(np.float32)
            self.inv_cell[:] = bk[:, 2 * M + 21:2 * M + 30]
            self.refused += (self.flag != 0)
        else:
            fac = self.factors[self.batch]
            v = self.v * fac[:, 0:3] + (self.kick[:, None] * f.astype(np.float64)) * fac[:, 3:6]
            self.v[:] = v
            self.f_prev = f.copy()
            self.ke_atom = self.half_mass * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            for g in range(B):
                self._close(g, step, float(e[g]), [float(t) for t in w[g]], float(total[0]))
            self.w_prev = w.copy()
            self.v[:] = self.v * self.scale[self.batch, 1][:, None]
        self._commit(step, code, mode)

    def _close(self, g, step, energy, w, found):
        """mtk_close_one."""
        e_kin, kaa = self._sums(g, self.ke_atom)
        vol = abs(det3(self.cell64[g].tolist()))
        vg = self.v_cell[g].tolist()
        self._kick_baro(g, 0.5 * self.dt, 2.0 * e_kin, kaa, w, vol, vg)
        s, _ = self._particles_half(g, e_kin, 1)
        self._baro_half(g, vg, 1)
        self.v_cell[g] = vg
        par = self.par[g].tolist()
        trk = ((kaa[0] * s) * s + (kaa[1] * s) * s) + (kaa[2] * s) * s
        trw = (w[0] + w[4]) + w[8]
        e_nhc = (chain_energy(float(self.kt[g]), float(self.dof_kt[g]), self.q[g].tolist(), self.xi[g].tolist(),
                              self.v_xi[g].tolist())
                 + chain_energy(float(self.kt[g]), float(self.dof_kt_b[g]), self.q_b[g].tolist(), self.xi_b[g].tolist(),
                                self.v_xi_b[g].tolist()))
        self.log[step % self.log_steps, g] = (energy, (e_kin * s) * s, found, e_nhc, ((trk + trw) / vol) / 3.0, vol,
                                              par[4] * vol + 0.5 * (par[0] * self._rate2(vg)))


def conserved_log(log):
    """Columns 0 + 1 + 3 + 6 of a log [rows,7] (hermnet_amd.mtk.conserved on one graph)."""
    return ((log[:, 0] + log[:, 1]) + log[:, 3]) + log[:, 6]


# ---- the pair-potential system of the conservation, reversibility and sampling tests ------------------------------------------------
class Pairs(object):
    """n atoms of unequal masses in a periodic (triclinic) cell with the smooth short-range pair potential u(r) = eps (1 - (r /
    rc)^2)^3 for r < rc (twice continuously differentiable at rc, finite at 0: soft spheres), minimum image over the 27
    neighbouring cells, evaluated in numpy float64 at the float32 coordinates and the float32 cell an advance hands out;
    energy, forces and the virial W = sum_pairs d (x) f (npt_step.h's sign: P = (sum m v v + W) / V) are rounded to float32 as
    a step's outputs are."""

    def __init__(self, n=32, eps=0.4, rc=3.2, cell=None, seed=11):
        rs = np.random.RandomState(seed)
        self.n, self.eps, self.rc = n, eps, rc
        self.cell = np.diag([7.4, 7.4, 7.4]) if cell is None else np.asarray(cell, dtype=np.float64)
        self.masses = rs.uniform(12.0, 40.0, n)
        self.frac = rs.uniform(0.0, 1.0, (n, 3))
        self.shifts = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64)

    def evaluate(self, pos32, cell32):
        x, cell = pos32.astype(np.float64), np.asarray(cell32, dtype=np.float64).reshape(3, 3)
        d = x[:, None, :] - x[None, :, :]                                    # [n,n,3]: from j to i
        d = d[:, :, None, :] + (self.shifts @ cell)[None, None, :, :]       # [n,n,27,3]
        r2 = (d * d).sum(axis=-1)
        t = 1.0 - r2 / (self.rc * self.rc)
        inside = (r2 < self.rc * self.rc) & (r2 > 0.0)
        t = np.where(inside, t, 0.0)
        e = 0.5 * self.eps * (t ** 3).sum()
        # f_i = -du/dr d/r = eps 6 t^2 / rc^2 d
        fpair = (6.0 * self.eps / (self.rc * self.rc)) * (t * t)[..., None] * d
        f = fpair.sum(axis=(1, 2))
        w = 0.5 * np.einsum("ijsa,ijsb->ab", d, fpair)
        return f.astype(np.float32), np.array([e], dtype=np.float32), w.astype(np.float32).reshape(1, 9)

    def start(self, temperature, seed):
        """(x, v): the random sites, and Maxwell-Boltzmann velocities at T with the centre of mass at rest."""
        rs = np.random.RandomState(seed)
        m = self.masses * AMU
        v = rs.standard_normal((self.n, 3)) * np.sqrt(KB * temperature / m)[:, None]
        v -= (m[:, None] * v).sum(axis=0) / m.sum()
        return self.frac @ self.cell, v


def run_pairs(driver, pairs, steps, prime=True):
    """(Prime, then) `steps` time steps of `driver` (a HostMTK / NumpyMTK of one graph with log_steps >= steps) in the pair
    potential, evaluated in the cell each advance leaves: the log."""
    first = int(driver.state[0])
    if prime:
        driver.state[3] = 1
    for _ in range(steps + (1 if prime else 0)):
        pos = driver.advance()
        f, e, w = pairs.evaluate(pos, driver.cell32[0])
        driver.finish(f, e, w)
    assert driver.state.tolist() == [first + steps, 0, 0, 0], driver.state
    return driver.log[np.arange(first, first + steps) % driver.log_steps, 0].copy()
