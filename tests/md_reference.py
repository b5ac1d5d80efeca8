"""Shared by tests/test_md_host.py and tests/test_md_device.py: a pure-Python Philox4x32-10, the numpy float64
transcription of the integrator's per-atom arithmetic (hermnet_amd/csrc/md_step.h, operation by operation: numpy's
elementwise float64 +, * and floor round once each, like the contraction-free C), and a thin wrapper that runs the
library's host twins (hermnet_host_md_advance / _finish / _noise) on numpy arrays."""
import ctypes
import math

import numpy as np

from hermnet_amd import _lib

AMU = 103.642696562
KB = 8.617333262e-5
LANGEVIN, WRAP, CAPACITY_BIT, NONFINITE = 1, 2, 4, 256
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def noise_words(seed, step, atom):
    """The eight words of (seed, step, atom): counters (atom, step low, step high, stream 0 / 1), key (seed low, seed high)."""
    key = (seed & M32, (seed >> 32) & M32)
    return (philox4x32_10((atom, step & M32, (step >> 32) & M32, 0), key) +
            philox4x32_10((atom, step & M32, (step >> 32) & M32, 1), key))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_noise(seed, step, n):
    """(words [n,8] uint32, gaussians [n,3] float64) of the library's host form."""
    words, gauss = np.zeros((n, 8), dtype=np.uint32), np.zeros((n, 3), dtype=np.float64)
    assert _lib.load().hermnet_host_md_noise(seed, step, n, _p(words), _p(gauss)) == 0
    return words, gauss


def coefficients(masses, dt, batch, friction=None, temperature=None, num_graphs=None):
    """(kick, half_mass, c1 [B] or None, sigma [N] or None) exactly as hermnet_amd/md.py makes them."""
    m = np.asarray(masses, dtype=np.float64) * AMU
    kick = 0.5 * dt / m
    half_mass = np.where(np.isfinite(m), 0.5 * m, 0.0)
    if friction is None:
        return kick, half_mass, None, None
    t = np.asarray(temperature, dtype=np.float64)
    B = int(num_graphs) if num_graphs is not None else int(batch[-1]) + 1
    t = np.broadcast_to(t.reshape(-1) if t.ndim else t, (B,)).astype(np.float64)
    c1 = math.exp(-float(friction) * dt)
    return kick, half_mass, np.full(B, c1), np.sqrt(KB * t[batch] * (1.0 - c1 * c1) / m)


# ---- the numpy transcription ------------------------------------------------------------------------------------------------
def advance_np(x, v, image, f32, kick, dt, c1_atom=None, sigma=None, xi=None, cell=None, inv=None):
    """md_advance_atom + md_wrap_atom on whole arrays, in place.  cell [N,3,3] float64 (per atom), inv likewise."""
    f = f32.astype(np.float64)
    k = kick[:, None]
    v[:] = v + k * f
    if c1_atom is None:
        x[:] = x + dt * v
    else:
        h = 0.5 * dt
        x[:] = x + h * v
        v[:] = c1_atom[:, None] * v + sigma[:, None] * xi
        x[:] = x + h * v
    if cell is not None:
        s = (x[:, 0:1] * inv[:, 0, :] + x[:, 1:2] * inv[:, 1, :]) + x[:, 2:3] * inv[:, 2, :]
        with np.errstate(invalid="ignore"):
            fl = np.floor(s)
            n = np.where((fl >= -1073741824.0) & (fl <= 1073741824.0), fl, 0.0)
        x[:] = x - ((n[:, 0:1] * cell[:, 0, :] + n[:, 1:2] * cell[:, 1, :]) + n[:, 2:3] * cell[:, 2, :])
        image += n.astype(np.int32)


def finish_np(v, f32, kick, half_mass):
    """md_finish_atom on whole arrays, in place; returns the per-atom kinetic energies."""
    v[:] = v + kick[:, None] * f32.astype(np.float64)
    return half_mass * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


class _State(object):
    """The state arrays every reference and every wrapper of the MD family starts from (the layout of
    include/hermnet_hip.h)."""

    def _make_state(self, x, v):
        n = self.n = len(x)
        self.x, self.v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
        self.x0, self.v0 = np.zeros_like(self.x), np.zeros_like(self.v)
        self.image, self.image0 = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 3), dtype=np.int32)
        self.f_prev = np.zeros((n, 3), dtype=np.float32)
        self.pos32 = self.x.astype(np.float32)
        self.ke_atom = np.zeros(n, dtype=np.float64)
        self.state = np.zeros(4, dtype=np.int64)
        return n

    # md_finish.h's skeleton in numpy, for the references whose finish keeps the protocol (NumpyREMD, NumpyPIMD)
    def _begin_finish(self, f32, energy, total, capacity, B):
        """hn_step_code, then md_finish_one on every atom: (step, code, mode, forces, energies)."""
        step, mode = int(self.state[0]), int(self.state[3])
        f = np.array(f32, dtype=np.float32)
        e = np.zeros(B, dtype=np.float32) if energy is None else np.array(energy, dtype=np.float32)
        code = int(total[1]) & 255
        if int(total[0]) > capacity:
            code |= CAPACITY_BIT
        if not np.all(np.isfinite(e)):
            code |= NONFINITE
        if mode != 0:
            if code == 0:
                self.f_prev = f.copy()
        elif code != 0:
            self.x[:], self.image[:], self.v[:] = self.x0, self.image0, self.v0
            self.pos32 = self.x0.astype(np.float32)
        else:
            self.ke_atom = finish_np(self.v, f, self.kick, self.half_mass)
            self.f_prev = f.copy()
        return step, code, mode, f, e

    def _commit(self, step, code, mode):
        """md_commit."""
        if code != 0:
            self.state[1], self.state[2] = code, step
        elif mode == 0:
            self.state[0] = step + 1
        if mode != 0:
            self.state[3] = 0


class NumpyMD(_State):
    """The reference trajectory: numpy float64 velocity Verlet / BAOAB with the noise of the library's host form."""

    def __init__(self, x, v, masses, dt, cell=None, batch=None, friction=None, temperature=None, seed=0, num_graphs=None):
        n = self._make_state(x, v)
        self.batch = np.zeros(n, dtype=np.int64) if batch is None else np.asarray(batch, dtype=np.int64)
        self.dt, self.seed, self.step = float(dt), seed, 0
        self.kick, self.half_mass, c1, self.sigma = coefficients(masses, dt, self.batch, friction, temperature, num_graphs)
        self.c1_atom = None if c1 is None else c1[self.batch]
        self.cell = self.inv = None
        if cell is not None:
            c = np.asarray(cell, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3)
            self.cell, self.inv = c[self.batch], np.linalg.inv(c)[self.batch]
        self.f, self.ke = self.f_prev, None

    def advance(self):
        xi = host_noise(self.seed, self.step, len(self.x))[1] if self.c1_atom is not None else None
        advance_np(self.x, self.v, self.image, self.f, self.kick, self.dt, self.c1_atom, self.sigma, xi, self.cell, self.inv)
        return self.x.astype(np.float32)

    def finish(self, f32):
        self.f = np.array(f32, dtype=np.float32)
        self.ke = finish_np(self.v, self.f, self.kick, self.half_mass)
        self.step += 1


class HostMD(_State):
    """The library's host twins on numpy arrays (the state layout of include/hermnet_hip.h).  `_evaluation`, `_finish_atoms`
    and `_finish_tail` are what the finishes of the family's wrappers (HostNPT, HostREMD, HostPIMD) share."""

    def __init__(self, x, v, masses, dt, cell=None, batch=None, friction=None, temperature=None, seed=0, log_steps=64,
                 num_graphs=None):
        n = self._make_state(x, v)
        self.lib = _lib.load()
        self.batch = np.zeros(n, dtype=np.int64) if batch is None else np.ascontiguousarray(batch, dtype=np.int64)
        self.B = int(num_graphs) if num_graphs is not None else int(self.batch[-1]) + 1
        self.graph_ptr = np.searchsorted(self.batch, np.arange(self.B + 1)).astype(np.int32)
        self.dt, self.seed = float(dt), seed
        self.kick, self.half_mass, self.c1, self.sigma = coefficients(masses, dt, self.batch, friction, temperature, self.B)
        self.flags = LANGEVIN if friction is not None else 0
        self.cell = self.inv = None
        if cell is not None:
            self.cell = np.ascontiguousarray(np.asarray(cell, dtype=np.float32).reshape(-1, 9))
            self.inv = np.ascontiguousarray(np.linalg.inv(self.cell.astype(np.float64).reshape(-1, 3, 3)))
            self.flags |= WRAP
        self.log_steps = log_steps
        self.log = np.full((log_steps, self.B, 3), -7.0)

    def advance(self):
        rc = self.lib.hermnet_host_md_advance(self.n, self.B, self.flags, self.dt, self.seed, _p(self.x), _p(self.v), _p(self.x0),
                                              _p(self.v0), _p(self.image), _p(self.image0), _p(self.f_prev), _p(self.kick),
                                              _p(self.c1), _p(self.sigma), _p(self.batch), _p(self.cell), _p(self.inv),
                                              _p(self.pos32), _p(self.state))
        assert rc == 0
        return self.pos32

    def _evaluation(self, f32, energy, total):
        """(forces, energies -- zeros where none are given --, the list's (found, flags)) as the arrays a finish takes."""
        e = np.zeros(self.B, dtype=np.float32) if energy is None else np.ascontiguousarray(energy, dtype=np.float32)
        return np.ascontiguousarray(f32, dtype=np.float32), e, np.array(total, dtype=np.int64)

    def _finish_atoms(self):
        """The eleven per-atom pointers of every finish, x ... ke_atom."""
        return (_p(self.x), _p(self.v), _p(self.x0), _p(self.v0), _p(self.image), _p(self.image0), _p(self.f_prev),
                _p(self.kick), _p(self.half_mass), _p(self.pos32), _p(self.ke_atom))

    def _finish_tail(self):
        return _p(self.log), self.log_steps, _p(self.state)

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20):
        f, e, tot = self._evaluation(f32, energy, total)
        rc = self.lib.hermnet_host_md_finish(self.n, self.B, _p(self.graph_ptr), _p(f), _p(e), _p(tot), capacity,
                                             *self._finish_atoms(), *self._finish_tail())
        assert rc == 0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
