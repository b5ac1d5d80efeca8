"""Shared by tests/test_relax_host.py and tests/test_relax_device.py: the numpy float64 transcription of the relaxation's
arithmetic (hermnet_amd/csrc/relax_step.h, operation by operation, the per-graph sums in resident_step.h's canonical order:
lane partials as an explicit loop over the rows of a zero-padded [-1,256] reshape, then the explicit fold), a thin wrapper
that runs the library's host twins (hermnet_host_relax_advance / _finish) on numpy arrays, a plain vectorised FIRE that
follows ASE's published `FIRE.step`, and two analytic force fields x -> float32 forces."""
import ctypes

import numpy as np

from hermnet_amd import _lib
from md_reference import bits  # noqa: F401

WRAP = 2
NMIN, FINC, FDEC, ASTART, FA = 5, 1.1, 0.5, 0.1, 0.99


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def graph_ptr_of(batch, B):
    return np.searchsorted(batch, np.arange(B + 1)).astype(np.int32)


# ---- the canonical reduction ------------------------------------------------------------------------------------------------
def _lanes(terms):
    """terms [m] of one graph's atoms -> [rows,256], zero-padded: row r holds atoms 256 r ... 256 r + 255."""
    m = len(terms)
    rows = max(1, -(-m // 256))
    t = np.zeros(rows * 256)
    t[:m] = terms
    return t.reshape(rows, 256)


def canonical_sum(terms):
    part = np.zeros(256)
    for row in _lanes(terms):             # lane l: 0.0 + t[l] + t[l+256] + ...  (the padding adds +0.0: no change)
        part = part + row
    m = 128
    while m >= 1:
        part[:m] = part[:m] + part[m:2 * m]
        m //= 2
    return part[0]


def canonical_max(terms):
    part = np.zeros(256)
    for row in _lanes(terms):
        part = np.where(row > part, row, part)
    m = 128
    while m >= 1:
        part[:m] = np.where(part[m:2 * m] > part[:m], part[m:2 * m], part[:m])
        m //= 2
    return part[0]


def dot3(p, q):
    return (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]


# ---- the numpy transcription ------------------------------------------------------------------------------------------------
class NumpyRelax(object):
    """relax_step.h + the step logic of relax_kernels.hip in numpy float64.  advance() -> the float32 coordinates to
    evaluate; finish(f32, energy, total, capacity) takes that evaluation's forces."""

    def __init__(self, x, cell=None, batch=None, num_graphs=None, fixed=None, fmax=0.05, dt=0.1, dtmax=1.0, maxstep=0.2,
                 wrap=True):
        n = len(x)
        self.x = np.array(x, dtype=np.float64).reshape(n, 3)
        self.x0, self.v = self.x.copy(), np.zeros((n, 3))
        self.image, self.image0 = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 3), dtype=np.int32)
        self.batch = np.zeros(n, dtype=np.int64) if batch is None else np.asarray(batch, dtype=np.int64)
        self.B = int(num_graphs) if num_graphs is not None else (int(self.batch[-1]) + 1 if n else 1)
        self.ptr = graph_ptr_of(self.batch, self.B)
        self.fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
        self.fmax = np.broadcast_to(np.asarray(fmax, dtype=np.float64), (self.B,)).copy()
        self.dt0, self.dtmax, self.maxstep = float(dt), float(dtmax), float(maxstep)
        self.cell = self.inv = None
        if cell is not None and wrap:
            c = np.asarray(cell, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3)
            self.cell, self.inv = c, np.linalg.inv(c)
        B = self.B
        self.dt, self.a, self.scale = np.full(B, self.dt0), np.full(B, ASTART), np.zeros(B)
        self.fnorm, self.energy = np.full(B, np.inf), np.zeros(B)
        self.nsteps, self.fresh = np.zeros(B, dtype=np.int64), np.ones(B, dtype=np.int64)
        self.converged, self.conv_step = np.zeros(B, dtype=np.int64), np.full(B, -1, dtype=np.int64)
        self.f = np.zeros((n, 3), dtype=np.float32)
        self.step, self.halt_code, self.halt_step, self.done = 0, 0, 0, 0
        self.pos32 = self.x.astype(np.float32)
        self.log = []                         # one [B,4] row per completed evaluation
        self.modes = []                       # per evaluation [B]: 'fresh', 'mix', 'stop', 'freeze', 'frozen'
        self.clamped = []                     # per evaluation [B] bool

    def advance(self):
        if self.halt_code == 0:
            for g in range(self.B):
                if self.converged[g]:
                    continue
                a, b = self.ptr[g], self.ptr[g + 1]
                self.x0[a:b], self.image0[a:b] = self.x[a:b], self.image[a:b]
                free = ~self.fixed[a:b]
                x, image = self.x[a:b][free], self.image[a:b][free]
                x = x + self.scale[g] * self.v[a:b][free]
                if self.cell is not None:
                    cell, inv = self.cell[g], self.inv[g]
                    s = (x[:, 0:1] * inv[0] + x[:, 1:2] * inv[1]) + x[:, 2:3] * inv[2]
                    with np.errstate(invalid="ignore"):
                        fl = np.floor(s)
                        nn = np.where((fl >= -1073741824.0) & (fl <= 1073741824.0), fl, 0.0)
                    x = x - ((nn[:, 0:1] * cell[0] + nn[:, 1:2] * cell[1]) + nn[:, 2:3] * cell[2])
                    image = image + nn.astype(np.int32)
                self.x[a:b][free], self.image[a:b][free] = x, image
            self.pos32 = self.x.astype(np.float32)
        return self.pos32

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 40):
        if self.halt_code != 0 or self.done:
            return
        f32 = np.asarray(f32, dtype=np.float32).reshape(-1, 3)
        e = np.zeros(self.B, dtype=np.float32) if energy is None else np.asarray(energy, dtype=np.float32).reshape(self.B)
        code = int(total[1]) & 255
        if int(total[0]) > capacity:
            code |= 4
        if not np.all(np.isfinite(e)):
            code |= 256
        if code:
            for g in range(self.B):
                if not self.converged[g]:
                    a, b = self.ptr[g], self.ptr[g + 1]
                    self.x[a:b], self.image[a:b] = self.x0[a:b], self.image0[a:b]
            self.pos32 = self.x.astype(np.float32)
            self.halt_code, self.halt_step = code, self.step
            return
        modes, clamped = [], []
        for g in range(self.B):
            a, b = self.ptr[g], self.ptr[g + 1]
            if self.converged[g]:
                modes.append("frozen")
                clamped.append(False)
                continue
            held = self.fixed[a:b]
            f = np.where(held[:, None], 0.0, f32[a:b].astype(np.float64))
            v = self.v[a:b]
            f2 = dot3(f, f)
            P, ff, vv, fm2 = canonical_sum(dot3(f, v)), canonical_sum(f2), canonical_sum(dot3(v, v)), canonical_max(f2)
            self.energy[g] = np.float64(e[g])
            self.fnorm[g] = np.sqrt(fm2)
            self.f[a:b] = f32[a:b]
            if fm2 < self.fmax[g] * self.fmax[g]:
                self.converged[g], self.conv_step[g], self.scale[g] = 1, self.step, 0.0
                self.v[a:b] = 0.0
                modes.append("freeze")
                clamped.append(False)
                continue
            if self.fresh[g]:
                self.fresh[g], self.dt[g], self.a[g], self.nsteps[g] = 0, self.dt0, ASTART, 0
                modes.append("fresh")
            elif P > 0.0:
                keep = 1.0 - self.a[g]
                cf = (self.a[g] / np.sqrt(ff)) * np.sqrt(vv) if ff > 0.0 else 0.0
                v = keep * v + cf * f
                if self.nsteps[g] > NMIN:
                    grown = self.dt[g] * FINC
                    self.dt[g] = grown if grown < self.dtmax else self.dtmax
                    self.a[g] = self.a[g] * FA
                self.nsteps[g] += 1
                modes.append("mix")
            else:
                v = np.zeros_like(v)
                self.a[g], self.dt[g], self.nsteps[g] = ASTART, self.dt[g] * FDEC, 0
                modes.append("stop")
            v = v + self.dt[g] * f
            v = np.where(held[:, None], 0.0, v)
            self.v[a:b] = v
            nd = self.dt[g] * np.sqrt(canonical_sum(dot3(v, v)))
            clamped.append(bool(nd > self.maxstep))
            self.scale[g] = self.dt[g] * (self.maxstep / nd) if nd > self.maxstep else self.dt[g]
        self.log.append(np.stack([self.energy, self.fnorm, self.dt, np.full(self.B, float(total[0]))], axis=1).copy())
        self.modes.append(modes)
        self.clamped.append(clamped)
        self.step += 1
        if np.all(self.converged != 0):
            self.done = 1


# ---- the host twins ----------------------------------------------------------------------------------------------------------
class HostRelax(object):
    """The library's host twins on numpy arrays (the state layout of include/hermnet_hip.h)."""

    def __init__(self, x, cell=None, batch=None, num_graphs=None, fixed=None, fmax=0.05, dt=0.1, dtmax=1.0, maxstep=0.2,
                 wrap=True, log_steps=256):
        n = self.n = len(x)
        self.lib = _lib.load()
        self.x = np.array(x, dtype=np.float64).reshape(n, 3)
        self.x0, self.v = self.x.copy(), np.zeros((n, 3))
        self.image, self.image0 = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 3), dtype=np.int32)
        self.f_prev = np.zeros((n, 3), dtype=np.float32)
        self.batch = np.zeros(n, dtype=np.int64) if batch is None else np.ascontiguousarray(batch, dtype=np.int64)
        self.B = int(num_graphs) if num_graphs is not None else (int(self.batch[-1]) + 1 if n else 1)
        self.graph_ptr = graph_ptr_of(self.batch, self.B)
        self.fixed = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.uint8)
        self.fmax = np.ascontiguousarray(np.broadcast_to(np.asarray(fmax, dtype=np.float64), (self.B,)))
        self.dt, self.dtmax, self.maxstep = float(dt), float(dtmax), float(maxstep)
        self.flags, self.cell, self.inv = 0, None, None
        if cell is not None and wrap:
            self.cell = np.ascontiguousarray(np.asarray(cell, dtype=np.float32).reshape(-1, 9))
            self.inv = np.ascontiguousarray(np.linalg.inv(self.cell.astype(np.float64).reshape(-1, 3, 3)))
            self.flags = WRAP
        self.pos32 = self.x.astype(np.float32)
        self.gf = np.zeros((self.B, 5))
        self.gf[:, 0], self.gf[:, 1], self.gf[:, 3] = self.dt, ASTART, np.inf
        self.gi = np.zeros((self.B, 4), dtype=np.int64)
        self.gi[:, 1], self.gi[:, 3] = 1, -1
        self.gf_new, self.gi_new = self.gf.copy(), self.gi.copy()
        self.log_steps = log_steps
        self.log = np.full((log_steps, self.B, 4), -7.0)
        self.state = np.zeros(4, dtype=np.int64)

    def advance(self):
        rc = self.lib.hermnet_host_relax_advance(self.n, self.B, self.flags, _p(self.x), _p(self.x0), _p(self.v), _p(self.image),
                                                 _p(self.image0), _p(self.fixed), _p(self.batch), _p(self.cell), _p(self.inv),
                                                 _p(self.pos32), _p(self.state), _p(self.gf), _p(self.gi))
        assert rc == 0
        return self.pos32

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 40):
        f = np.ascontiguousarray(f32, dtype=np.float32)
        e = np.zeros(self.B, dtype=np.float32) if energy is None else np.ascontiguousarray(energy, dtype=np.float32)
        tot = np.array(total, dtype=np.int64)
        rc = self.lib.hermnet_host_relax_finish(self.n, self.B, _p(self.graph_ptr), _p(f), _p(e), _p(tot), capacity, self.dt,
                                                self.dtmax, self.maxstep, float(self.fmax[0]), _p(self.fmax), _p(self.x),
                                                _p(self.v), _p(self.x0), _p(self.image), _p(self.image0), _p(self.f_prev),
                                                _p(self.fixed), _p(self.pos32), _p(self.gf), _p(self.gi), _p(self.gf_new),
                                                _p(self.gi_new), _p(self.log), self.log_steps, _p(self.state))
        assert rc == 0


def same_state(host, ref):
    """A HostRelax (or anything with its arrays) against a NumpyRelax, bit for bit."""
    assert np.array_equal(bits(host.x), bits(ref.x)) and np.array_equal(bits(host.v), bits(ref.v))
    assert np.array_equal(host.image, ref.image) and np.array_equal(host.pos32, ref.pos32)
    assert np.array_equal(bits(host.gf[:, 0]), bits(ref.dt)) and np.array_equal(bits(host.gf[:, 1]), bits(ref.a))
    assert np.array_equal(bits(host.gf[:, 2]), bits(ref.scale)) and np.array_equal(bits(host.gf[:, 3]), bits(ref.fnorm))
    assert np.array_equal(host.gi[:, 0], ref.nsteps) and np.array_equal(host.gi[:, 1], ref.fresh)
    assert np.array_equal(host.gi[:, 2], ref.converged) and np.array_equal(host.gi[:, 3], ref.conv_step)
    assert host.state.tolist() == [ref.step, ref.halt_code, ref.halt_step, ref.done]


# ---- textbook FIRE (ASE's optimize/fire.py: FIRE.step, one structure) -------------------------------------------------------
def textbook_fire(x, force, fmax=0.05, dt=0.1, dtmax=1.0, maxstep=0.2, cap=200):
    """Returns (evaluations until max |f_i| < fmax or None, [positions at which the forces were evaluated])."""
    r = np.array(x, dtype=np.float64)
    v, a, nsteps, path = None, ASTART, 0, []
    for k in range(cap):
        path.append(r.copy())
        f = force(r.astype(np.float32)).astype(np.float64)
        if (f ** 2).sum(axis=1).max() < fmax ** 2:
            return k + 1, path
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
    return None, path


# ---- analytic force fields: x float32 -> f float32 -------------------------------------------------------------------------------
def wells(n, seed, amplitude, cell=None, outside=False):
    """(start coordinates, force): f = -k (x - x*) per component, k uniform in [1, 10] eV/A^2, the start rattled by
    `amplitude` around x*.  With `cell` the displacement from x* is taken to the minimum image, so wrapped coordinates
    feel the same well."""
    rs = np.random.RandomState(seed)
    c = np.diag([12.0, 12.0, 12.0]) if cell is None else np.asarray(cell, dtype=np.float64)
    centre = rs.uniform(0.2, 0.8, (n, 3)) @ c
    k = rs.uniform(1.0, 10.0, (n, 3))
    x = centre + rs.uniform(-amplitude, amplitude, (n, 3))
    if outside:
        x[::3] += np.array([2, -1, 1]) @ c
    inv = np.linalg.inv(c)

    def force(pos32):
        d = pos32.astype(np.float64) - centre
        if cell is not None:
            d = d - np.round(d @ inv) @ c
        return (-k * d).astype(np.float32)

    return x, force


def lennard_jones(reps, seed, rattle=0.15, sigma=2.5, eps=0.4, rc=6.0):
    """(start coordinates, cell, force): periodic Lennard-Jones on an fcc cell at 0.98 of the equilibrium spacing, rattled."""
    a0 = 0.98 * 2.0 ** (1.0 / 6.0) * sigma * np.sqrt(2.0)
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    grid = np.array([[i, j, k] for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])])
    x = (grid[:, None, :] + base[None]).reshape(-1, 3) * a0
    box = np.array(reps, dtype=np.float64) * a0
    x = x + np.random.RandomState(seed).uniform(-rattle, rattle, x.shape)
    shifts = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]) * box

    def force(pos32):
        p = pos32.astype(np.float64)
        d = p[:, None, :] - p[None, :, :]
        d = d - np.round(d / box) * box                       # minimum image, then its 26 neighbours (box < 2 rc)
        f = np.zeros_like(p)
        for s in shifts:
            e = d + s
            r2 = (e ** 2).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                s6 = (sigma * sigma / r2) ** 3
                w = np.where((r2 > 0.0) & (r2 < rc * rc), 24.0 * eps * (2.0 * s6 * s6 - s6) / r2, 0.0)
            f += (w[:, :, None] * e).sum(1)
        return f.astype(np.float32)

    return x, np.diag(box), force
