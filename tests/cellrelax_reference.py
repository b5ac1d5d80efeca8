"""Shared by tests/test_cellrelax_host.py and tests/test_cellrelax_device.py: the numpy float64 transcription of the cell
relaxation's arithmetic (hermnet_amd/csrc/cellrelax_step.h, operation by operation; FIRE itself and the canonical sums are
those of relax_reference.py), a thin wrapper that runs the library's host twins (hermnet_host_cellrelax_advance / _finish)
on numpy arrays, `same_state` that compares the two bit for bit, a textbook FIRE over an (n+3, 3) array of generalised
coordinates written the way ASE's UnitCellFilter does it (numpy's own linear algebra, numpy's own sums), and a float64
Lennard-Jones for triclinic cells with forces and virial.

An evaluation is a function (pos32 [N,3] float32, cell32 [B,3,3] float32) -> (energy [B] f32, forces [N,3] f32, virial [B,3,3]
f32): what the captured step returns for the float32 inputs the advance wrote."""
import ctypes

import numpy as np

from hermnet_amd import _lib
from npt_reference import det3, inverse3
from relax_reference import ASTART, FA, FDEC, FINC, NMIN, WRAP, _p, bits, canonical_max, canonical_sum, dot3, graph_ptr_of

HYDROSTATIC, CONSTANT_VOLUME = 1, 2


def mask9(mask):
    """None, 3x3 or Voigt 6 (xx, yy, zz, yz, xz, xy) -> the nine entry-wise factors."""
    if mask is None:
        return np.ones(9)
    m = np.asarray(mask, dtype=np.float64)
    if m.shape == (6,):
        m = np.array([[m[0], m[5], m[4]], [m[5], m[1], m[3]], [m[4], m[3], m[2]]])
    return np.ascontiguousarray(m.reshape(9))


def default_cell_factor(batch, B):
    return np.maximum(np.bincount(batch, minlength=B).astype(np.float64), 1.0)


# ---- cellrelax_step.h, operation by operation -----------------------------------------------------------------------------------
def cell_np(G, cf, C0):
    """cellrelax_cell: (F, F^-1, C, cell32, det F), all flat [9]."""
    G, C0 = np.asarray(G).reshape(9), np.asarray(C0).reshape(9)
    F = G / cf
    C = np.zeros(9)
    for i in range(3):
        for j in range(3):
            C[3 * i + j] = (C0[3 * i] * F[3 * j] + C0[3 * i + 1] * F[3 * j + 1]) + C0[3 * i + 2] * F[3 * j + 2]
    return F, inverse3(F), C, C.astype(np.float32), det3(F)


def to_cart_np(q, F):
    """cellrelax_to_cart on [m,3]: x = q F^T."""
    return np.stack([(q[:, 0] * F[3 * j] + q[:, 1] * F[3 * j + 1]) + q[:, 2] * F[3 * j + 2] for j in range(3)], axis=1)


def atom_force_np(f, F):
    """cellrelax_atom_force on [m,3]: fq = f F."""
    return np.stack([(f[:, 0] * F[j] + f[:, 1] * F[3 + j]) + f[:, 2] * F[6 + j] for j in range(3)], axis=1)


def cell_force_np(w32, C, Finv, cf, p, mask, flags):
    """cellrelax_cell_force: (fG [9], volume, pressure, stress [9])."""
    w = np.asarray(w32, dtype=np.float32).reshape(9).astype(np.float64)
    det = det3(C)
    vol = -det if det < 0.0 else det
    sw = np.array([0.5 * (w[3 * i + j] + w[3 * j + i]) for i in range(3) for j in range(3)])
    pv = p * vol
    s = np.array([sw[k] - pv if k % 4 == 0 else sw[k] for k in range(9)])
    with np.errstate(divide="ignore", invalid="ignore"):
        stress = -sw / vol
        a = np.zeros(9)
        for i in range(3):
            for j in range(3):
                a[3 * i + j] = (s[3 * i] * Finv[3 * j] + s[3 * i + 1] * Finv[3 * j + 1]) + s[3 * i + 2] * Finv[3 * j + 2]
        if flags & HYDROSTATIC:
            t = ((a[0] + a[4]) + a[8]) / 3.0
            a = np.array([t if k % 4 == 0 else 0.0 for k in range(9)])
        a = a * mask
        if flags & CONSTANT_VOLUME:
            t = ((a[0] + a[4]) + a[8]) / 3.0
            for k in range(3):
                a[4 * k] = a[4 * k] - t
        return a / cf, vol, (((sw[0] + sw[4]) + sw[8]) / 3.0) / vol, stress


def _dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


class NumpyCellRelax(object):
    """cellrelax_step.h + the step logic of cellrelax_kernels.hip in numpy float64.  advance() -> (pos32, cell32) to
    evaluate; finish(f32, w32, energy, total, capacity) takes that evaluation's forces and virial."""

    def __init__(self, x, cell, batch=None, num_graphs=None, fixed=None, fmax=0.05, dt=0.1, dtmax=1.0, maxstep=0.2, wrap=True,
                 mask=None, hydrostatic_strain=False, constant_volume=False, scalar_pressure=0.0, cell_factor=None):
        n = len(x)
        self.x = np.array(x, dtype=np.float64).reshape(n, 3)
        self.q, self.q0, self.x0, self.v = self.x.copy(), self.x.copy(), self.x.copy(), np.zeros((n, 3))
        self.image, self.image0 = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 3), dtype=np.int32)
        self.batch = np.zeros(n, dtype=np.int64) if batch is None else np.asarray(batch, dtype=np.int64)
        B = self.B = int(num_graphs) if num_graphs is not None else (int(self.batch[-1]) + 1 if n else 1)
        self.ptr = graph_ptr_of(self.batch, B)
        self.fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
        self.fmax = np.broadcast_to(np.asarray(fmax, dtype=np.float64), (B,)).copy()
        self.dt0, self.dtmax, self.maxstep, self.wrap = float(dt), float(dtmax), float(maxstep), bool(wrap)
        self.cell0 = np.array(cell, dtype=np.float64).reshape(B, 9)
        self.inv0 = np.stack([inverse3(c) for c in self.cell0])
        self.cf = default_cell_factor(self.batch, B) if cell_factor is None else \
            np.broadcast_to(np.asarray(cell_factor, dtype=np.float64), (B,)).copy()
        self.p = np.broadcast_to(np.asarray(scalar_pressure, dtype=np.float64), (B,)).copy()
        self.mask = mask9(mask)
        self.flags = (HYDROSTATIC if hydrostatic_strain else 0) | (CONSTANT_VOLUME if constant_volume else 0)
        eye = np.eye(3).reshape(9)
        self.rows = self.cf[:, None] * eye[None]
        self.rows0, self.rows_v = self.rows.copy(), np.zeros((B, 9))
        self.deform, self.deform_inv = np.tile(eye, (B, 1)), np.tile(eye, (B, 1))
        self.det_f, self.cell64 = np.ones(B), self.cell0.copy()
        self.cell32 = self.cell0.astype(np.float32)
        self.obs = np.zeros((B, 11))
        self.dt, self.a, self.scale = np.full(B, self.dt0), np.full(B, ASTART), np.zeros(B)
        self.fnorm, self.energy = np.full(B, np.inf), np.zeros(B)
        self.nsteps, self.fresh = np.zeros(B, dtype=np.int64), np.ones(B, dtype=np.int64)
        self.converged, self.conv_step = np.zeros(B, dtype=np.int64), np.full(B, -1, dtype=np.int64)
        self.f = np.zeros((n, 3), dtype=np.float32)
        self.step, self.halt_code, self.halt_step, self.done = 0, 0, 0, 0
        self.pos32 = self.x.astype(np.float32)
        self.log = []                         # one [B,6] row per completed evaluation
        self.modes = []                       # per evaluation [B]: 'fresh', 'mix', 'stop', 'freeze', 'frozen'
        self.clamped = []                     # per evaluation [B] bool
        self.cell_led = []                    # per evaluation [B] bool: the largest generalised force was a cell row's

    def _cell_from_rows(self, g):
        (self.deform[g], self.deform_inv[g], self.cell64[g], self.cell32[g], self.det_f[g]) = \
            cell_np(self.rows[g], self.cf[g], self.cell0[g])

    def advance(self):
        if self.halt_code == 0:
            for g in range(self.B):
                if self.converged[g]:
                    continue
                self.rows0[g] = self.rows[g]
                self.rows[g] = self.rows[g] + self.scale[g] * self.rows_v[g]
                self._cell_from_rows(g)
                a, b = self.ptr[g], self.ptr[g + 1]
                self.q0[a:b], self.x0[a:b], self.image0[a:b] = self.q[a:b], self.x[a:b], self.image[a:b]
                free = ~self.fixed[a:b]
                q, image = self.q[a:b][free], self.image[a:b][free]
                q = q + self.scale[g] * self.v[a:b][free]
                if self.wrap:
                    cell, inv = self.cell0[g].reshape(3, 3), self.inv0[g].reshape(3, 3)
                    s = (q[:, 0:1] * inv[0] + q[:, 1:2] * inv[1]) + q[:, 2:3] * inv[2]
                    with np.errstate(invalid="ignore"):
                        fl = np.floor(s)
                        nn = np.where((fl >= -1073741824.0) & (fl <= 1073741824.0), fl, 0.0)
                    q = q - ((nn[:, 0:1] * cell[0] + nn[:, 1:2] * cell[1]) + nn[:, 2:3] * cell[2])
                    image = image + nn.astype(np.int32)
                self.q[a:b][free], self.image[a:b][free] = q, image
                self.x[a:b] = to_cart_np(self.q[a:b], self.deform[g])
            self.pos32 = self.x.astype(np.float32)
        return self.pos32, self.cell32.reshape(self.B, 3, 3)

    def finish(self, f32, w32, energy=None, total=(0, 0), capacity=1 << 40):
        if self.halt_code != 0 or self.done:
            return
        B = self.B
        f32 = np.asarray(f32, dtype=np.float32).reshape(-1, 3)
        w32 = np.asarray(w32, dtype=np.float32).reshape(B, 9)
        e = np.zeros(B, dtype=np.float32) if energy is None else np.asarray(energy, dtype=np.float32).reshape(B)
        code = int(total[1]) & 255
        if int(total[0]) > capacity:
            code |= 4
        if not np.all(np.isfinite(e)) or not np.all(np.isfinite(w32)) or not np.all(self.det_f > 0.0):
            code |= 256
        if code:
            for g in range(B):
                if not self.converged[g]:
                    a, b = self.ptr[g], self.ptr[g + 1]
                    self.q[a:b], self.x[a:b], self.image[a:b] = self.q0[a:b], self.x0[a:b], self.image0[a:b]
                    self.rows[g] = self.rows0[g]
                    det = self.det_f[g]
                    self._cell_from_rows(g)
                    self.det_f[g] = det
            self.pos32 = self.x.astype(np.float32)
            self.halt_code, self.halt_step = code, self.step
            return
        modes, clamped, led = [], [], []
        for g in range(B):
            a, b = self.ptr[g], self.ptr[g + 1]
            if self.converged[g]:
                modes.append("frozen")
                clamped.append(False)
                led.append(False)
                continue
            held = self.fixed[a:b]
            F = self.deform[g]
            f = atom_force_np(np.where(held[:, None], 0.0, f32[a:b].astype(np.float64)), F)
            v = self.v[a:b]
            f2 = dot3(f, f)
            s = [canonical_sum(dot3(f, v)), canonical_sum(f2), canonical_sum(dot3(v, v)), canonical_max(f2)]
            atoms_fm2 = s[3]
            fG, vol, pr, stress = cell_force_np(w32[g], self.cell64[g], self.deform_inv[g], self.cf[g], self.p[g], self.mask,
                                                self.flags)
            vG = self.rows_v[g].copy()
            for r in range(3):                                       # the rows' terms, in row order
                fr, vr = fG[3 * r:3 * r + 3], vG[3 * r:3 * r + 3]
                r2 = _dot(fr, fr)
                s[0] = s[0] + _dot(fr, vr)
                s[1] = s[1] + r2
                s[2] = s[2] + _dot(vr, vr)
                s[3] = r2 if r2 > s[3] else s[3]
            P, ff, vv, fm2 = s
            led.append(bool(fm2 > atoms_fm2))
            self.energy[g] = np.float64(e[g]) + self.p[g] * vol
            self.obs[g, 0], self.obs[g, 1], self.obs[g, 2:] = vol, pr, stress
            self.fnorm[g] = np.sqrt(fm2)
            self.f[a:b] = f32[a:b]
            if fm2 < self.fmax[g] * self.fmax[g]:
                self.converged[g], self.conv_step[g], self.scale[g] = 1, self.step, 0.0
                self.v[a:b] = 0.0
                self.rows_v[g] = 0.0
                modes.append("freeze")
                clamped.append(False)
                continue
            if self.fresh[g]:
                self.fresh[g], self.dt[g], self.a[g], self.nsteps[g] = 0, self.dt0, ASTART, 0
                modes.append("fresh")
            elif P > 0.0:
                keep = 1.0 - self.a[g]
                cf_ = (self.a[g] / np.sqrt(ff)) * np.sqrt(vv) if ff > 0.0 else 0.0
                v = keep * v + cf_ * f
                vG = keep * vG + cf_ * fG
                if self.nsteps[g] > NMIN:
                    grown = self.dt[g] * FINC
                    self.dt[g] = grown if grown < self.dtmax else self.dtmax
                    self.a[g] = self.a[g] * FA
                self.nsteps[g] += 1
                modes.append("mix")
            else:
                v, vG = np.zeros_like(v), np.zeros(9)
                self.a[g], self.dt[g], self.nsteps[g] = ASTART, self.dt[g] * FDEC, 0
                modes.append("stop")
            v = v + self.dt[g] * f
            v = np.where(held[:, None], 0.0, v)
            vG = vG + self.dt[g] * fG
            self.v[a:b], self.rows_v[g] = v, vG
            ss = canonical_sum(dot3(v, v))
            for r in range(3):
                ss = ss + _dot(vG[3 * r:3 * r + 3], vG[3 * r:3 * r + 3])
            nd = self.dt[g] * np.sqrt(ss)
            clamped.append(bool(nd > self.maxstep))
            self.scale[g] = self.dt[g] * (self.maxstep / nd) if nd > self.maxstep else self.dt[g]
        self.log.append(np.stack([self.energy, self.fnorm, self.dt, np.full(B, float(total[0])), self.obs[:, 0], self.obs[:, 1]],
                                 axis=1).copy())
        self.modes.append(modes)
        self.clamped.append(clamped)
        self.cell_led.append(led)
        self.step += 1
        if np.all(self.converged != 0):
            self.done = 1


# ---- the host twins ----------------------------------------------------------------------------------------------------------
class HostCellRelax(object):
    """The library's host twins on numpy arrays (the state layout of include/hermnet_hip.h)."""

    def __init__(self, x, cell, batch=None, num_graphs=None, fixed=None, fmax=0.05, dt=0.1, dtmax=1.0, maxstep=0.2, wrap=True,
                 mask=None, hydrostatic_strain=False, constant_volume=False, scalar_pressure=0.0, cell_factor=None, log_steps=512):
        n = self.n = len(x)
        self.lib = _lib.load()
        self.x = np.array(x, dtype=np.float64).reshape(n, 3)
        self.q, self.q0, self.x0, self.v = self.x.copy(), self.x.copy(), self.x.copy(), np.zeros((n, 3))
        self.image, self.image0 = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 3), dtype=np.int32)
        self.f_prev = np.zeros((n, 3), dtype=np.float32)
        self.batch = np.zeros(n, dtype=np.int64) if batch is None else np.ascontiguousarray(batch, dtype=np.int64)
        B = self.B = int(num_graphs) if num_graphs is not None else (int(self.batch[-1]) + 1 if n else 1)
        self.graph_ptr = graph_ptr_of(self.batch, B)
        self.fixed = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.uint8)
        self.fmax = np.ascontiguousarray(np.broadcast_to(np.asarray(fmax, dtype=np.float64), (B,)))
        self.dt, self.dtmax, self.maxstep = float(dt), float(dtmax), float(maxstep)
        self.flags = WRAP if wrap else 0
        self.cell0 = np.ascontiguousarray(np.array(cell, dtype=np.float64).reshape(B, 9))
        self.inv0 = np.ascontiguousarray(np.stack([inverse3(c) for c in self.cell0]))
        self.cf = default_cell_factor(self.batch, B) if cell_factor is None else \
            np.ascontiguousarray(np.broadcast_to(np.asarray(cell_factor, dtype=np.float64), (B,)))
        self.p = np.ascontiguousarray(np.broadcast_to(np.asarray(scalar_pressure, dtype=np.float64), (B,)))
        self.mask = mask9(mask)
        self.cell_flags = (HYDROSTATIC if hydrostatic_strain else 0) | (CONSTANT_VOLUME if constant_volume else 0)
        eye = np.eye(3).reshape(9)
        self.rows = np.ascontiguousarray(self.cf[:, None] * eye[None])
        self.rows0, self.rows_v = self.rows.copy(), np.zeros((B, 9))
        self.deform, self.deform_inv = np.tile(eye, (B, 1)), np.tile(eye, (B, 1))
        self.det_f, self.cell64 = np.ones(B), self.cell0.copy()
        self.cell32 = self.cell0.astype(np.float32)
        self.obs = np.zeros((B, 11))
        self.pos32 = self.x.astype(np.float32)
        self.gf = np.zeros((B, 5))
        self.gf[:, 0], self.gf[:, 1], self.gf[:, 3] = self.dt, ASTART, np.inf
        self.gi = np.zeros((B, 4), dtype=np.int64)
        self.gi[:, 1], self.gi[:, 3] = 1, -1
        self.gf_new, self.gi_new = self.gf.copy(), self.gi.copy()
        self.log_steps = log_steps
        self.log = np.full((log_steps, B, 6), -7.0)
        self.state = np.zeros(4, dtype=np.int64)

    def advance_args(self):
        return (self.n, self.B, self.flags, _p(self.q), _p(self.q0), _p(self.x), _p(self.x0), _p(self.v), _p(self.image),
                _p(self.image0), _p(self.fixed), _p(self.batch), _p(self.cell0), _p(self.inv0), _p(self.cf), _p(self.rows),
                _p(self.rows0), _p(self.rows_v), _p(self.deform), _p(self.deform_inv), _p(self.det_f), _p(self.cell64),
                _p(self.cell32), _p(self.pos32), _p(self.state), _p(self.gf), _p(self.gi))

    def advance(self):
        assert self.lib.hermnet_host_cellrelax_advance(*self.advance_args()) == 0
        return self.pos32, self.cell32.reshape(self.B, 3, 3)

    def finish_args(self, f, e, w, tot, capacity):
        return (self.n, self.B, self.cell_flags, _p(self.graph_ptr), _p(f), _p(e), _p(w), _p(tot), capacity, self.dt, self.dtmax,
                self.maxstep, float(self.fmax[0]), _p(self.fmax), _p(self.p), _p(self.mask), _p(self.cell0), _p(self.inv0),
                _p(self.cf), _p(self.q), _p(self.q0), _p(self.x), _p(self.x0), _p(self.v), _p(self.image), _p(self.image0),
                _p(self.f_prev), _p(self.fixed), _p(self.pos32), _p(self.rows), _p(self.rows0), _p(self.rows_v), _p(self.deform),
                _p(self.deform_inv), _p(self.det_f), _p(self.cell64), _p(self.cell32), _p(self.obs), _p(self.gf), _p(self.gi),
                _p(self.gf_new), _p(self.gi_new), _p(self.log), self.log_steps, _p(self.state))

    def finish(self, f32, w32, energy=None, total=(0, 0), capacity=1 << 40):
        f = np.ascontiguousarray(f32, dtype=np.float32)
        w = np.ascontiguousarray(w32, dtype=np.float32).reshape(self.B, 9)
        e = np.zeros(self.B, dtype=np.float32) if energy is None else np.ascontiguousarray(energy, dtype=np.float32)
        tot = np.array(total, dtype=np.int64)
        assert self.lib.hermnet_host_cellrelax_finish(*self.finish_args(f, e, w, tot, capacity)) == 0


def same_state(host, ref):
    """A HostCellRelax (or anything with its arrays) against a NumpyCellRelax, bit for bit."""
    B = ref.B
    for name in ("q", "x", "v", "rows", "rows_v", "deform", "cell64", "obs"):
        assert np.array_equal(bits(np.asarray(getattr(host, name)).reshape(-1)), bits(getattr(ref, name).reshape(-1))), name
    # (a singular F makes an inverse of inf / nan: the same ones)
    assert np.array_equal(np.asarray(host.deform_inv).reshape(B, 9), ref.deform_inv, equal_nan=True)
    assert np.array_equal(np.asarray(host.image), ref.image) and np.array_equal(np.asarray(host.pos32), ref.pos32)
    assert np.array_equal(np.asarray(host.cell32).reshape(B, 9), ref.cell32)
    gf, gi = np.asarray(host.gf), np.asarray(host.gi)
    assert np.array_equal(bits(gf[:, 0]), bits(ref.dt)) and np.array_equal(bits(gf[:, 1]), bits(ref.a))
    assert np.array_equal(bits(gf[:, 2]), bits(ref.scale)) and np.array_equal(bits(gf[:, 3]), bits(ref.fnorm))
    assert np.array_equal(bits(gf[:, 4]), bits(ref.energy))
    assert np.array_equal(gi[:, 0], ref.nsteps) and np.array_equal(gi[:, 1], ref.fresh)
    assert np.array_equal(gi[:, 2], ref.converged) and np.array_equal(gi[:, 3], ref.conv_step)
    assert np.asarray(host.state).tolist() == [ref.step, ref.halt_code, ref.halt_step, ref.done]


def drive(opt, evaluate, evaluations, until_done=False, every=None):
    """`evaluations` x (advance, evaluate, finish) on a Host- or NumpyCellRelax; returns the evaluations made."""
    for k in range(evaluations):
        pos32, cell32 = opt.advance()
        e, f, w = evaluate(pos32, cell32)
        opt.finish(f, w, energy=e)
        if every is not None:
            every(k)
        if until_done and (opt.state[3] if hasattr(opt, "state") else opt.done):
            return k + 1
    return evaluations


# ---- textbook FIRE on ASE's UnitCellFilter (one structure) ----------------------------------------------------------------------
def textbook_cell_fire(x, cell, evaluate, fmax=0.05, dt=0.1, dtmax=1.0, maxstep=0.2, cap=400, mask=None, hydrostatic_strain=False,
                       constant_volume=False, scalar_pressure=0.0, cell_factor=None):
    """ASE's optimize/fire.py FIRE.step on ase.constraints.UnitCellFilter's get_positions / get_forces / set_positions,
    written with numpy's own linear algebra and sums.  Returns (evaluations until the largest generalised force < fmax or
    None, [(positions, cell) at which forces and stress were evaluated], [enthalpy per evaluation])."""
    n = len(x)
    cell0 = np.array(cell, dtype=np.float64).reshape(3, 3)
    cf = float(n) if cell_factor is None else float(cell_factor)
    m = mask9(mask).reshape(3, 3)
    r = np.concatenate([np.array(x, dtype=np.float64), cf * np.eye(3)])      # get_positions at F = I
    v, a, nsteps, path, enthalpy = None, ASTART, 0, [], []
    for k in range(cap):
        F = r[n:] / cf                                                     # set_positions
        c = cell0 @ F.T
        pos = r[:n] @ F.T
        path.append((pos.copy(), c.copy()))
        e, f32, w32 = evaluate(pos.astype(np.float32), c.astype(np.float32).reshape(1, 3, 3))
        vol = abs(np.linalg.det(c))
        w = np.asarray(w32, dtype=np.float64).reshape(3, 3)
        stress = -0.5 * (w + w.T) / vol
        enthalpy.append(float(np.asarray(e).reshape(-1)[0]) + scalar_pressure * vol)
        virial = -vol * (stress + scalar_pressure * np.eye(3))             # get_forces
        virial = np.linalg.solve(F, virial.T).T
        if hydrostatic_strain:
            virial = np.eye(3) * (np.trace(virial) / 3.0)
        virial = virial * m
        if constant_volume:
            virial = virial - np.eye(3) * (np.trace(virial) / 3.0)
        f = np.concatenate([np.asarray(f32, dtype=np.float64).reshape(n, 3) @ F, virial / cf])
        if (f ** 2).sum(axis=1).max() < fmax ** 2:
            return k + 1, path, enthalpy
        if v is None:
            v = np.zeros_like(r)
        else:
            vf = np.vdot(f, v)
            if vf > 0.0:
                v = (1.0 - a) * v + a * f / np.sqrt(np.vdot(f, f)) * np.sqrt(np.vdot(v, v))
                if nsteps > NMIN:
                    dt = min(dt * FINC, dtmax)
                    a *= FA
                nsteps += 1
            else:
                v[:] *= 0.0
                a = ASTART
                dt *= FDEC
                nsteps = 0
        v += dt * f
        dr = dt * v
        normdr = np.sqrt(np.vdot(dr, dr))
        if normdr > maxstep:
            dr = maxstep * dr / normdr
        r = r + dr
    return None, path, enthalpy


# ---- Lennard-Jones in float64 for triclinic cells: energy, forces, virial ------------------------------------------------------
SIGMA, EPS, RC = 2.5, 0.4, 6.0
FCC_A0 = 2.0 ** (1.0 / 6.0) * SIGMA * np.sqrt(2.0) * 0.9712     # the fcc lattice constant near LJ's minimum with this cutoff
_SHIFTS = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64)


def lj_one(pos, cell):
    """(energy, forces [n,3], virial [3,3]) of one periodic structure, float64: pairs within RC among the minimum image and
    its 26 neighbours (valid while the cell's heights exceed RC).  virial W = sum over pairs of r_ij (x) f_ij, so that the
    stress is -W / V."""
    p, c = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(cell, dtype=np.float64).reshape(3, 3)
    if len(p) == 0:
        return 0.0, np.zeros((0, 3)), np.zeros((3, 3))
    d = p[:, None, :] - p[None, :, :]
    s = d @ np.linalg.inv(c)
    d = (s - np.round(s)) @ c
    energy, f, w = 0.0, np.zeros_like(p), np.zeros((3, 3))
    for sh in _SHIFTS @ c:
        e = d + sh
        r2 = (e ** 2).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            s6 = (SIGMA * SIGMA / r2) ** 3
            inside = (r2 > 0.0) & (r2 < RC * RC)
            g = np.where(inside, 24.0 * EPS * (2.0 * s6 * s6 - s6) / r2, 0.0)
            energy += 0.5 * np.where(inside, 4.0 * EPS * (s6 * s6 - s6), 0.0).sum()
        ge = g[:, :, None] * e
        f += ge.sum(1)
        w += 0.5 * np.einsum("ija,ijb->ab", e, ge)
    return energy, f, w


def lj_evaluation(ptr):
    """The evaluation (module docstring) of a batch whose graph g holds atoms ptr[g]:ptr[g+1]; float32 results."""
    B = len(ptr) - 1

    def evaluate(pos32, cell32):
        out = [lj_one(pos32[ptr[g]:ptr[g + 1]], np.asarray(cell32).reshape(B, 3, 3)[g]) for g in range(B)]
        return (np.array([o[0] for o in out], dtype=np.float32), np.concatenate([o[1] for o in out]).astype(np.float32),
                np.stack([o[2] for o in out]).astype(np.float32))

    return evaluate


def lj_fcc(reps, seed, rattle=0.08, strain=None, outside=False):
    """(coordinates, cell [3,3]) of an fcc block of reps cubic cells near LJ's minimum, the cell then deformed by the 3x3
    `strain` (cell <- cell (I + strain), atoms with it), the atoms rattled; `outside`: every third atom starts lattice
    vectors away from the cell."""
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    grid = np.array([[i, j, k] for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])])
    x = (grid[:, None, :] + base[None]).reshape(-1, 3) * FCC_A0
    cell = np.diag(np.array(reps, dtype=np.float64) * FCC_A0)
    if strain is not None:
        d = np.eye(3) + np.asarray(strain, dtype=np.float64)
        x, cell = x @ d, cell @ d
    x = x + np.random.RandomState(seed).uniform(-rattle, rattle, x.shape)
    if outside:
        x[::3] += np.array([2, -1, 1]) @ cell
    return x, cell
