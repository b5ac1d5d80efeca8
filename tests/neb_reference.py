"""Shared by tests/test_neb_host.py and tests/test_neb_device.py: `NumpyNEB`, the numpy float64 transcription of the
nudged elastic band's arithmetic (hermnet_amd/csrc/neb_step.h, operation by operation; the per-image sums in
resident_step.h's canonical order through tests/relax_reference.py, the folds over a band's images as explicit loops), and
`HostNEB`, a thin wrapper that runs the library's host twins (hermnet_host_relax_advance, hermnet_host_neb_finish) on numpy
arrays in the state layout of include/hermnet_hip.h."""
import numpy as np

from hermnet_amd import _lib
from relax_reference import ASTART, FA, FDEC, FINC, NMIN, _p, bits, canonical_max, canonical_sum, dot3  # noqa: F401


def layout(sizes, images):
    """Bands of images[k] images of sizes[k] atoms each: (graph_ptr [B+1], band_ptr [K+1], band_of [B]) int32, batch [N]."""
    per_image = np.repeat(np.asarray(sizes, dtype=np.int64), images)
    graph_ptr = np.concatenate([[0], np.cumsum(per_image)]).astype(np.int32)
    band_ptr = np.concatenate([[0], np.cumsum(images)]).astype(np.int32)
    band_of = np.repeat(np.arange(len(images)), images).astype(np.int32)
    batch = np.repeat(np.arange(len(per_image)), per_image).astype(np.int64)
    return graph_ptr, band_ptr, band_of, batch


def tangent_coef(Em, E0, Ep):
    """(c1, c2) of the improved tangent T = c2 t2 + c1 t1."""
    if Ep > E0 > Em:
        return 0.0, 1.0
    if Ep < E0 < Em:
        return 1.0, 0.0
    dp, dm = abs(Ep - E0), abs(Em - E0)
    hi, lo = (dp, dm) if dp > dm else (dm, dp)
    return (lo, hi) if Ep > Em else (hi, lo)


def tangent_branch(Em, E0, Ep):
    """The name of the branch `tangent_coef` takes (for the tests that ask that all occur)."""
    if Ep > E0 > Em:
        return "rising"
    if Ep < E0 < Em:
        return "falling"
    if Ep == Em:
        return "equal"
    return "maximum" if E0 >= max(Em, Ep) else "minimum"


class _Common(object):
    def _layout(self, x, graph_ptr, band_ptr, fixed, k, fmax):
        self.n = n = len(x)
        self.graph_ptr = np.ascontiguousarray(graph_ptr, dtype=np.int32)
        self.band_ptr = np.ascontiguousarray(band_ptr, dtype=np.int32)
        self.B, self.K = len(self.graph_ptr) - 1, len(self.band_ptr) - 1
        self.band_of = np.repeat(np.arange(self.K), np.diff(self.band_ptr)).astype(np.int32)
        self.batch = np.repeat(np.arange(self.B), np.diff(self.graph_ptr)).astype(np.int64)
        self.fixed = np.zeros(n, dtype=np.uint8) if fixed is None else np.ascontiguousarray(fixed, dtype=np.uint8)
        self.k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.float64), (self.K,)))
        self.fmax = np.ascontiguousarray(np.broadcast_to(np.asarray(fmax, dtype=np.float64), (self.K,)))
        self.x = np.array(x, dtype=np.float64).reshape(n, 3)
        self.x0, self.v = self.x.copy(), np.zeros((n, 3))
        self.image, self.image0 = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 3), dtype=np.int32)
        self.pos32 = self.x.astype(np.float32)
        self.f_prev = np.zeros((n, 3), dtype=np.float32)
        B = self.B
        interior = np.ones(B, dtype=bool)
        interior[self.band_ptr[:-1]] = interior[self.band_ptr[1:] - 1] = False
        self.interior = interior
        self.gf = np.zeros((B, 5))
        self.gf[:, 0], self.gf[:, 1], self.gf[:, 3] = self.dt0, ASTART, np.inf
        self.gi = np.zeros((B, 4), dtype=np.int64)
        self.gi[:, 1], self.gi[:, 3] = 1, -1
        self.gi[~interior, 1], self.gi[~interior, 2] = 0, 1          # end points: converged, scale 0, for ever
        self.obs = np.zeros((B, 4))
        self.climber = np.full(self.K, -1, dtype=np.int64)
        self.g = np.zeros((n, 3))
        self.state = np.zeros(4, dtype=np.int64)

    def interior_of(self, k):
        return range(self.band_ptr[k] + 1, self.band_ptr[k + 1] - 1)


class NumpyNEB(_Common):
    """neb_step.h in numpy float64.  advance() -> the float32 coordinates to evaluate; finish(f32, energy, total, capacity)
    takes that evaluation's forces and energies.  The state has the host twin's layout (gf, gi, obs, climber, state), so the
    two compare array by array; `log` is a list of [B,4] rows, `branches` the tangent branch of every interior image per
    evaluation."""

    def __init__(self, x, graph_ptr, band_ptr, fixed=None, k=0.1, fmax=0.05, climb=True, dt=0.1, dtmax=1.0, maxstep=0.2):
        self.dt0, self.dtmax, self.maxstep, self.climb = float(dt), float(dtmax), float(maxstep), bool(climb)
        self._layout(x, graph_ptr, band_ptr, fixed, k, fmax)
        self.log, self.branches = [], []

    def advance(self):
        """hermnet_relax_advance without the wrap: per atom of an image that is not converged x0 = x, x += scale v."""
        if self.state[1] == 0:
            for g in range(self.B):
                if self.gi[g, 2]:
                    continue
                a, b = self.graph_ptr[g], self.graph_ptr[g + 1]
                self.x0[a:b], self.image0[a:b] = self.x[a:b], self.image[a:b]
                free = self.fixed[a:b] == 0
                self.x[a:b][free] = self.x[a:b][free] + self.gf[g, 2] * self.v[a:b][free]
            self.pos32 = self.x.astype(np.float32)
        return self.pos32

    def _image_force(self, g, k, f32, e, top):
        """First launch, interior image g of band k: g into self.g, obs; returns the image's four partial sums."""
        gp = self.graph_ptr
        a, b, m = gp[g], gp[g + 1], gp[g + 1] - gp[g]
        am, ap = gp[g - 1], gp[g + 1]
        held = self.fixed[a:b] != 0
        c1, c2 = tangent_coef(np.float64(e[g - 1]), np.float64(e[g]), np.float64(e[g + 1]))
        x = self.x[a:b]
        t1 = np.where(held[:, None], 0.0, x - self.x[am:am + m])
        t2 = np.where(held[:, None], 0.0, self.x[ap:ap + m] - x)
        T = c2 * t2 + c1 * t1
        F = np.where(held[:, None], 0.0, f32[a:b].astype(np.float64))
        t1t1, t2t2, TT, FT = (canonical_sum(dot3(p, q)) for p, q in ((t1, t1), (t2, t2), (T, T), (F, T)))
        inv = 0.0 if TT == 0.0 else 1.0 / np.sqrt(TT)
        ft = FT * inv
        seg = np.sqrt(t2t2)
        spring = self.k[k] * (seg - np.sqrt(t1t1))
        par = -2.0 * ft if g == top else spring - ft
        gg = F + par * (T * inv)
        self.g[a:b] = gg
        v = self.v[a:b]
        g2 = dot3(gg, gg)
        part = (canonical_sum(dot3(gg, v)), canonical_sum(g2), canonical_sum(dot3(v, v)), canonical_max(g2))
        self.obs[g] = (np.float64(e[g]), np.sqrt(part[3]), seg, ft)
        return part

    def finish(self, f32, energy, total=(0, 0), capacity=1 << 40):
        if self.state[1] != 0 or self.state[3] != 0:
            return
        f32 = np.asarray(f32, dtype=np.float32).reshape(-1, 3)
        e = np.asarray(energy, dtype=np.float32).reshape(self.B)
        step = int(self.state[0])
        code = int(total[1]) & 255
        if int(total[0]) > capacity:
            code |= 4
        if not np.all(np.isfinite(e)):
            code |= 256
        bands = [(k, self.band_ptr[k] + 1) for k in range(self.K)]
        moving = [k for k, lead in bands if not self.gi[lead, 2]]
        if code:
            for k in moving:
                for g in self.interior_of(k):
                    a, b = self.graph_ptr[g], self.graph_ptr[g + 1]
                    self.x[a:b], self.image[a:b] = self.x0[a:b], self.image0[a:b]
            self.pos32 = self.x.astype(np.float32)
            self.state[1], self.state[2] = code, step
            return
        branches = {}
        for k in moving:
            blo, bhi, lead = self.band_ptr[k], self.band_ptr[k + 1], self.band_ptr[k] + 1
            inner = list(self.interior_of(k))
            top = -1
            if self.climb:
                for j in inner:
                    if top < 0 or e[j] > e[top]:
                        top = j
            for g in (blo, bhi - 1):
                self.obs[g] = (np.float64(e[g]), 0.0, 0.0, 0.0)
            # first launch: every image's force and partials
            s = [0.0, 0.0, 0.0, 0.0]
            parts = {}
            for g in inner:
                parts[g] = self._image_force(g, k, f32, e, top)
                branches[g] = tangent_branch(np.float64(e[g - 1]), np.float64(e[g]), np.float64(e[g + 1]))
            # second launch: the fold in ascending image order from 0.0, FIRE's decision, the velocities
            for g in inner:
                for c in range(3):
                    s[c] = s[c] + parts[g][c]
                s[3] = parts[g][3] if parts[g][3] > s[3] else s[3]
            P, ff, vv, fm2 = s
            dt, a_, scale, fnorm = self.gf[lead, :4]
            nsteps, fresh, converged, conv_step = self.gi[lead]
            fnorm = np.sqrt(fm2)
            mode, keep, cf = "keep", 0.0, 0.0
            if fm2 < self.fmax[k] * self.fmax[k]:
                converged, conv_step, scale, mode = 1, step, 0.0, "freeze"
            elif fresh:
                fresh, dt, a_, nsteps = 0, self.dt0, ASTART, 0
            elif P > 0.0:
                mode, keep = "mix", 1.0 - a_
                cf = (a_ / np.sqrt(ff)) * np.sqrt(vv) if ff > 0.0 else 0.0
                if nsteps > NMIN:
                    grown = dt * FINC
                    dt = grown if grown < self.dtmax else self.dtmax
                    a_ = a_ * FA
                nsteps += 1
            else:
                mode, a_, dt, nsteps = "stop", ASTART, dt * FDEC, 0
            csum = 0.0
            for g in inner:
                a, b = self.graph_ptr[g], self.graph_ptr[g + 1]
                held = self.fixed[a:b] != 0
                v, f = self.v[a:b], self.g[a:b]
                if mode == "freeze":
                    v = np.zeros_like(v)
                else:
                    if mode == "mix":
                        v = keep * v + cf * f
                    elif mode == "stop":
                        v = np.zeros_like(v)
                    v = v + dt * f
                    v = np.where(held[:, None], 0.0, v)
                self.v[a:b] = v
                self.f_prev[a:b] = f32[a:b]
                csum = csum + canonical_sum(dot3(v, v))
            # third launch: the clamp, the band's state into its interior images' rows
            if not converged:
                nd = dt * np.sqrt(csum)
                scale = dt * (self.maxstep / nd) if nd > self.maxstep else dt
            for g in inner:
                self.gf[g] = (dt, a_, scale, fnorm, np.float64(e[g]))
                self.gi[g] = (nsteps, fresh, converged, conv_step)
            self.climber[k] = -1 if top < 0 else top - blo
        row = np.stack([self.obs[:, 0], self.obs[:, 1], self.gf[self.band_ptr[:-1][self.band_of] + 1, 0],
                        np.full(self.B, float(total[0]))], axis=1)
        self.log.append(row.copy())
        self.branches.append(branches)
        self.state[0] = step + 1
        if all(self.gi[lead, 2] for _, lead in bands):
            self.state[3] = 1


class HostNEB(_Common):
    """The library's host twins on numpy arrays."""

    def __init__(self, x, graph_ptr, band_ptr, fixed=None, k=0.1, fmax=0.05, climb=True, dt=0.1, dtmax=1.0, maxstep=0.2,
                 log_steps=256):
        self.lib = _lib.load()
        self.dt0, self.dtmax, self.maxstep, self.climb = float(dt), float(dtmax), float(maxstep), int(bool(climb))
        self._layout(x, graph_ptr, band_ptr, fixed, k, fmax)
        self.isum, self.csum = np.zeros((self.B, 4)), np.zeros(self.B)
        self.bf_new, self.bi_new = np.zeros((self.K, 5)), np.zeros((self.K, 4), dtype=np.int64)
        self.climber_new = np.full(self.K, -1, dtype=np.int64)
        self.log_steps = log_steps
        self.log = np.full((log_steps, self.B, 4), -7.0)

    def advance(self):
        rc = self.lib.hermnet_host_relax_advance(self.n, self.B, 0, _p(self.x), _p(self.x0), _p(self.v), _p(self.image),
                                                 _p(self.image0), _p(self.fixed), _p(self.batch), None, None, _p(self.pos32),
                                                 _p(self.state), _p(self.gf), _p(self.gi))
        assert rc == 0
        return self.pos32

    def finish_args(self, f, e, tot, capacity):
        return [self.n, self.B, self.K, self.climb, _p(self.graph_ptr), _p(self.band_ptr), _p(self.band_of), _p(f), _p(e),
                _p(tot), capacity, self.dt0, self.dtmax, self.maxstep, _p(self.k), _p(self.fmax), _p(self.x), _p(self.v),
                _p(self.x0), _p(self.image), _p(self.image0), _p(self.f_prev), _p(self.fixed), _p(self.pos32), _p(self.gf),
                _p(self.gi), _p(self.obs), _p(self.climber), _p(self.g), _p(self.isum), _p(self.csum), _p(self.bf_new),
                _p(self.bi_new), _p(self.climber_new), _p(self.log), self.log_steps, _p(self.state)]

    def finish(self, f32, energy, total=(0, 0), capacity=1 << 40):
        f = np.ascontiguousarray(f32, dtype=np.float32)
        e = np.ascontiguousarray(energy, dtype=np.float32)
        tot = np.array(total, dtype=np.int64)
        rc = self.lib.hermnet_host_neb_finish(*self.finish_args(f, e, tot, capacity))
        assert rc == 0


STATE_F64 = ("x", "x0", "v", "gf", "obs", "g")
STATE_INT = ("image", "image0", "pos32", "f_prev", "gi", "climber", "state")


def same_state(host, ref):
    """A HostNEB (or anything with its arrays) against a NumpyNEB, bit for bit."""
    for name in STATE_F64:
        assert np.array_equal(bits(getattr(host, name)), bits(getattr(ref, name))), name
    for name in STATE_INT:
        assert np.array_equal(getattr(host, name), getattr(ref, name)), name
