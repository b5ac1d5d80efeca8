"""Shared by tests/test_metad_host.py and tests/test_metad_device.py: the numpy float64 transcription of csrc/metad_step.h
(operation by operation: `np_exp` is mt_exp, `NumpyMetaD` the whole biased step) and thin wrappers that run the library's
host twins (hermnet_host_metad_bias / _cv / _exp) on numpy arrays.  The tables come from hermnet_amd/metad.py's own host
functions (`cv_tables`, `bias_tables`): what `DeviceMetaD` uploads."""
import types

import numpy as np

from hermnet_amd import _lib
from hermnet_amd.metad import COORDINATION, DISTANCE, bias_tables, cv_tables
from md_reference import HostMD, NumpyMD, _p, advance_np, host_noise

LOG2E, LN2_HI, LN2_LO = 1.44269504088896338700e+00, 6.93147180369123816490e-01, 1.90821492927058770002e-10
_COEFFS = [1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0,
           1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0]


def np_exp(a):
    """mt_exp on an array."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        live = a >= -745.0
    x = np.where(live, a, 0.0)
    k = np.floor(x * LOG2E + 0.5)
    r = (x - k * LN2_HI) - k * LN2_LO
    p = np.full_like(x, _COEFFS[0])
    for c in _COEFFS[1:]:
        p = p * r + c
    return np.where(live, np.ldexp(p, k.astype(np.int64)), 0.0)


def host_exp(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.zeros_like(a)
    assert _lib.load().hermnet_host_metad_exp(a.size, _p(a), _p(out)) == 0
    return out


def canonical_sums(terms):
    """hn_canonical_sums<C,-1> on terms [K,C]: lane l of 256 adds the terms l, l + 256, ... from 0.0, then the tree."""
    t = np.asarray(terms, dtype=np.float64)
    t = t.reshape(len(t), t.shape[1] if t.ndim > 1 else 1)
    rows = np.zeros(((-(-max(len(t), 1) // 256)) * 256, t.shape[1]))
    rows[:len(t)] = t
    part = np.zeros((256, t.shape[1]))
    for row in rows.reshape(-1, 256, t.shape[1]):        # (the padding adds +0.0: no change)
        part = part + row
    m = 128
    while m >= 1:
        part[:m] = part[:m] + part[m:2 * m]
        m //= 2
    return part[0]


def _fractional(x, inv):
    return (x[..., 0:1] * inv[0] + x[..., 1:2] * inv[1]) + x[..., 2:3] * inv[2]


def _min_image(si, sj, cell):
    """obs_min_image: (d from j to i, |d|^2)."""
    ds = si - sj
    ds = ds - np.floor(ds + 0.5)
    d = (ds[..., 0:1] * cell[0] + ds[..., 1:2] * cell[1]) + ds[..., 2:3] * cell[2]
    return d, (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _powi(w, k):
    r = np.ones_like(w)
    for _ in range(k):
        r = r * w
    return r


def switch_np(r2, par, p):
    """mt_switch: (st, g)."""
    w = r2 * par[0]
    wp1 = _powi(w, p - 1)
    sw = 1.0 / (1.0 + wp1 * w)
    return (sw - par[2]) * par[3], -(((float(p) * wp1) * (sw * sw)) * par[4])


def walker_cvs_np(tables, x, image, cell, inv):
    """One walker's CVs in numpy: (s [D], grad [D,n,3]) -- launch 1, the CV half of launch 2 and mt_cv_grad."""
    n, D = len(x), len(tables.kind)
    s, grad = np.zeros(D), np.zeros((D, n, 3))
    frac = _fractional(x, inv)
    for d in range(D):
        kind, p = (int(v) for v in tables.kind[d])
        par = tables.par[d]
        if kind == DISTANCE:
            wa, wb = tables.weight[d, 0], tables.weight[d, 1]
            im = image.astype(np.float64)
            u = x + ((im[:, 0:1] * cell[0] + im[:, 1:2] * cell[1]) + im[:, 2:3] * cell[2])
            c = canonical_sums(np.concatenate([wa[:, None] * u, wb[:, None] * u], axis=1))
            dv, r2 = _min_image(_fractional(c[None, :3], inv)[0], _fractional(c[None, 3:], inv)[0], cell)
            r = np.sqrt(r2)
            e = dv / r if r > 0.0 else np.zeros(3)
            s[d] = r
            grad[d] = (wa - wb)[:, None] * e
            continue
        assert kind == COORDINATION
        role = tables.role[d].astype(np.int64)
        in_a, in_b = (role & 1) != 0, (role & 2) != 0
        acc = np.zeros((n, 4))
        for j in range(n):                                   # ascending j: the order of every lane's sum
            dv, r2 = _min_image(frac, frac[j], cell)
            ab, ba = in_a & in_b[j], in_b & in_a[j]
            live = (np.arange(n) != j) & (ab | ba) & (r2 < par[1])
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                st, gr = switch_np(r2, par, p)
                c = np.where(ab & ba, 2.0, 1.0) * gr
                acc[:, 0] = np.where(live & ab, acc[:, 0] + st, acc[:, 0])
                for k in range(3):
                    acc[:, 1 + k] = np.where(live, acc[:, 1 + k] + c * dv[:, k], acc[:, 1 + k])
        acc = acc * par[5]
        s[d] = canonical_sums(acc[:, 0:1])[0]
        grad[d] = acc[:, 1:]
    return s, grad


def bias_np(bias, s, centres, heights):
    """(V, dV/ds [D]) at s over the hills: mt_hill_term in hn_canonical_sums' order."""
    D, K = len(s), len(heights)
    terms = np.zeros((K, 3))
    gk = np.array(heights, dtype=np.float64)
    dd = np.zeros((K, D))
    for d in range(D):
        dd[:, d] = s[d] - centres[:, d]
        gk = gk * np_exp(-((dd[:, d] * dd[:, d]) * bias.sigma_par[d, 0]))
    terms[:, 0] = gk
    for d in range(D):
        terms[:, 1 + d] = gk * (-(dd[:, d] * bias.sigma_par[d, 1]))
    sums = canonical_sums(terms)
    return sums[0], sums[1:1 + D]


class _Bias(object):
    """What HostMetaD and NumpyMetaD share: the tables and the stage's state in the layout of include/hermnet_hip.h."""

    def _make_bias(self, B, cvs, cell, height, sigma, pace, temperature, bias_factor, max_hills, hills, log_steps):
        self.B, self.n_rep, self.D = B, self.n // B, len(cvs)
        self.tables = cv_tables(cvs, self.n_rep, cell)
        self.bias = bias_tables(self.D, height, sigma, pace, temperature, bias_factor, max_hills, hills)
        K = len(self.bias.heights)
        self.hill_count = np.array([K], dtype=np.int64)
        self.hill_centres, self.hill_heights = np.zeros((max_hills, self.D)), np.zeros(max_hills)
        self.hill_centres[:K], self.hill_heights[:K] = self.bias.centres, self.bias.heights
        self.cv_atom, self.cv_walker = np.zeros((self.D, self.n, 6)), np.zeros((B, 16))
        self.forces_b, self.bias_forces = np.zeros((self.n, 3), dtype=np.float32), np.zeros((self.n, 3))
        self.cv_log = np.full((log_steps, B, self.D + 2), -7.0)
        self.cell32 = np.ascontiguousarray(np.broadcast_to(np.asarray(cell, dtype=np.float32).reshape(-1, 3, 3), (B, 3, 3)))
        self.inv64 = np.ascontiguousarray(np.linalg.inv(self.cell32.astype(np.float64)))

    def hills(self):
        K = int(self.hill_count[0])
        return self.hill_centres[:K].copy(), self.hill_heights[:K].copy()

    def snapshot(self):
        c, h = self.hills()
        return types.SimpleNamespace(hill_count=len(h), hill_centres=c, hill_heights=h, sigma=self.bias.sigma.copy(),
                                     bias_factor=self.bias.bias_factor)


def bias_args(o, f, e, tot, capacity):
    """hermnet_host_metad_bias's arguments on the arrays of `o` (a _Bias with x, image, graph_ptr, state); it fills o.forces_b."""
    t, b = o.tables, o.bias
    return (o.n, o.B, o.D, _p(o.graph_ptr), _p(o.x), _p(o.image), _p(o.cell32), _p(o.inv64), _p(t.kind), _p(t.par), _p(t.role),
            _p(t.weight), _p(b.sigma_par), b.height, b.inv_kt, b.pace, b.max_hills, _p(f), _p(e), _p(tot), capacity, _p(o.state),
            _p(o.cv_atom), _p(o.cv_walker), _p(o.hill_count), _p(o.hill_centres), _p(o.hill_heights), _p(o.forces_b),
            _p(o.bias_forces), _p(o.cv_log), o.log_steps)


def advance_args(o):
    """hermnet_host_md_advance's arguments on the arrays of the HostMD `o`."""
    return (o.n, o.B, o.flags, o.dt, o.seed, _p(o.x), _p(o.v), _p(o.x0), _p(o.v0), _p(o.image), _p(o.image0), _p(o.f_prev),
            _p(o.kick), _p(o.c1), _p(o.sigma), _p(o.batch), _p(o.cell), _p(o.inv), _p(o.pos32), _p(o.state))


def finish_args(o, f, e, tot, capacity):
    """hermnet_host_md_finish's arguments on the arrays of the HostMD `o`, reading the forces `f`."""
    return (o.n, o.B, _p(o.graph_ptr), _p(f), _p(e), _p(tot), capacity, *o._finish_atoms(), *o._finish_tail())


class HostMetaD(_Bias, HostMD):
    """hermnet_host_md_advance + hermnet_host_metad_bias + hermnet_host_md_finish on numpy arrays."""

    def __init__(self, B, x, v, masses, dt, cell, cvs, height, sigma, pace, temperature, friction=None, bias_factor=None,
                 max_hills=4096, hills=None, seed=0, log_steps=64, wrap=True):
        cells = np.broadcast_to(np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3), (B, 3, 3))
        HostMD.__init__(self, x, v, masses, dt, cell=cells if wrap else None, batch=np.repeat(np.arange(B), len(x) // B),
                        friction=friction, temperature=temperature, seed=seed, log_steps=log_steps, num_graphs=B)
        self._make_bias(B, cvs, cell, height, sigma, pace, temperature, bias_factor, max_hills, hills, log_steps)

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20):
        f, e, tot = self._evaluation(f32, energy, total)
        assert self.lib.hermnet_host_metad_bias(*bias_args(self, f, e, tot, capacity)) == 0
        assert self.lib.hermnet_host_md_finish(*finish_args(self, self.forces_b, e, tot, capacity)) == 0


def bound_step(host, forces, biased=True):
    """One time step of `host` (a HostMetaD, or with `biased=False` any HostMD) as a function without arguments, the twins'
    arguments bound once: advance, `forces(pos32, out)` fills the float32 forces in place, (bias,) finish.  For long runs."""
    lib, f = host.lib, np.zeros((host.n, 3), dtype=np.float32)
    e, tot = np.zeros(host.B, dtype=np.float32), np.zeros(2, dtype=np.int64)
    adv = advance_args(host)
    bias = bias_args(host, f, e, tot, 1 << 20) if biased else None
    fin = finish_args(host, host.forces_b if biased else f, e, tot, 1 << 20)
    keep = (f, e, tot)

    def step():
        assert lib.hermnet_host_md_advance(*adv) == 0
        forces(host.pos32, keep[0])
        if bias is not None:
            assert lib.hermnet_host_metad_bias(*bias) == 0
        assert lib.hermnet_host_md_finish(*fin) == 0
    return step


def host_cv(cvs, B, x, image, cell):
    """hermnet_host_metad_cv: (values [B,D], grads [D,N,3])."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, D = len(x), len(cvs)
    t = cv_tables(cvs, n // B, cell)
    cell32 = np.ascontiguousarray(np.broadcast_to(np.asarray(cell, dtype=np.float32).reshape(-1, 3, 3), (B, 3, 3)))
    inv = np.ascontiguousarray(np.linalg.inv(cell32.astype(np.float64)))
    ptr = (np.arange(B + 1) * (n // B)).astype(np.int32)
    image = np.ascontiguousarray(image, dtype=np.int32)
    cv_atom, cv_walker, values, grads = np.zeros((D, n, 6)), np.zeros((B, 16)), np.zeros((B, D)), np.zeros((D, n, 3))
    rc = _lib.load().hermnet_host_metad_cv(n, B, D, _p(ptr), _p(x), _p(image), _p(cell32), _p(inv), _p(t.kind), _p(t.par),
                                           _p(t.role), _p(t.weight), _p(cv_atom), _p(cv_walker), _p(values), _p(grads))
    assert rc == 0, rc
    return values, grads


class NumpyMetaD(_Bias, NumpyMD):
    """The reference: md_advance_one (the noise of the library's host form), the bias stage of csrc/metad_step.h and
    md_finish.h's skeleton in numpy float64, operation by operation."""

    def __init__(self, B, x, v, masses, dt, cell, cvs, height, sigma, pace, temperature, friction=None, bias_factor=None,
                 max_hills=4096, hills=None, seed=0, log_steps=64, wrap=True):
        cells = np.broadcast_to(np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3), (B, 3, 3))
        NumpyMD.__init__(self, x, v, masses, dt, cell=cells if wrap else None, batch=np.repeat(np.arange(B), len(x) // B),
                         friction=friction, temperature=temperature, seed=seed, num_graphs=B)
        self.log_steps = log_steps
        self._make_bias(B, cvs, cell, height, sigma, pace, temperature, bias_factor, max_hills, hills, log_steps)

    def advance(self):
        step, code, mode = (int(w) for w in self.state[[0, 1, 3]])
        if code != 0:
            return self.pos32
        if mode == 0:
            self.x0[:], self.v0[:], self.image0[:] = self.x, self.v, self.image
            xi = host_noise(self.seed, step, self.n)[1] if self.c1_atom is not None else None
            advance_np(self.x, self.v, self.image, self.f_prev, self.kick, self.dt, self.c1_atom, self.sigma, xi, self.cell, self.inv)
        self.pos32 = self.x.astype(np.float32)
        return self.pos32

    def _stage(self, f32, energy, total, capacity):
        """The four launches: self.forces_b, and on a committing step the row and the deposit."""
        step, mode = int(self.state[0]), int(self.state[3])
        f = np.array(f32, dtype=np.float32)
        e = np.zeros(self.B, dtype=np.float32) if energy is None else np.array(energy, dtype=np.float32)
        void = (int(total[1]) & 255) != 0 or int(total[0]) > capacity or not np.all(np.isfinite(e))
        if void:
            self.forces_b = f.copy()
            return
        b, K = self.bias, int(self.hill_count[0])
        due = mode == 0 and (step + 1) % b.pace == 0
        new = []
        for g in range(self.B):
            lo, hi = g * self.n_rep, (g + 1) * self.n_rep
            cell, inv = self.cell32[g].astype(np.float64), self.inv64[g]
            s, grad = walker_cvs_np(self.tables, self.x[lo:hi], self.image[lo:hi], cell, inv)
            big_v, dv = bias_np(b, s, self.hill_centres[:K], self.hill_heights[:K])
            h = 0.0
            if due:
                h = b.height * float(np_exp(-(big_v * b.inv_kt))) if b.inv_kt != 0.0 else b.height
                new.append((s.copy(), h))
            nb = np.zeros((self.n_rep, 3))
            for d in range(self.D):
                nb = nb + dv[d] * grad[d]
            self.bias_forces[lo:hi] = -nb
            self.forces_b[lo:hi] = (f[lo:hi].astype(np.float64) - nb).astype(np.float32)
            if mode == 0:
                self.cv_log[step % self.log_steps, g] = list(s) + [big_v, h]
        for g, (s, h) in enumerate(new):
            if K + g < b.max_hills:
                self.hill_centres[K + g], self.hill_heights[K + g] = s, h
        if due:
            self.hill_count[0] = min(K + self.B, b.max_hills)

    def finish(self, f32, energy=None, total=(0, 0), capacity=1 << 20):
        if self.state[1] != 0:
            return
        self._stage(f32, energy, total, capacity)
        step, code, mode, _, _ = self._begin_finish(self.forces_b, energy, total, capacity, self.B)
        self._commit(step, code, mode)
