"""Shared by tests/test_npt_host.py and tests/test_npt_device.py: the numpy float64 transcription of the barostat's
arithmetic (hermnet_amd/csrc/npt_step.h, operation by operation; the six kinetic sums in resident_step.h's canonical order
through relax_reference.canonical_sum), a reference trajectory `NumpyNPT` (md_reference.NumpyMD plus the barostat) and a thin
wrapper `HostNPT` that runs the library's host twins (hermnet_host_md_advance / hermnet_host_md_finish_npt) on numpy arrays."""
import numpy as np

from md_reference import HostMD, NumpyMD, _p, bits, finish_np  # noqa: F401
from relax_reference import canonical_sum

ISOTROPIC, AXES, FULL = 0, 1, 2
COUPLING = {"isotropic": ISOTROPIC, "axes": AXES, "full": FULL}
XX, YY, ZZ, XY, XZ, YZ = range(6)


def mask_bits(mask):
    return sum(1 << k for k, on in enumerate(mask) if on)


def coupling_constant(dt, taup, compressibility, B):
    """c [B] = (dt / taup) compressibility / 3, as hermnet_amd/md.py makes it."""
    taup = np.broadcast_to(np.asarray(taup, dtype=np.float64), (B,))
    comp = np.broadcast_to(np.asarray(compressibility, dtype=np.float64), (B,))
    return (float(dt) / taup) * comp / 3.0


# ---- npt_step.h ---------------------------------------------------------------------------------------------------------------
def kinetic_sums(v, half_mass):
    """npt_kinetic_terms through hn_canonical_sums<6>: K over (xx, yy, zz, xy, xz, yz) of one graph's atoms."""
    m = 2.0 * half_mass
    mx, my, mz = m * v[:, 0], m * v[:, 1], m * v[:, 2]
    terms = [mx * v[:, 0], my * v[:, 1], mz * v[:, 2], mx * v[:, 1], mx * v[:, 2], my * v[:, 2]]
    return np.array([canonical_sum(t) for t in terms])


def det3(c):
    c = np.asarray(c, dtype=np.float64).reshape(9)
    return (c[0] * (c[4] * c[8] - c[5] * c[7]) + c[1] * (c[5] * c[6] - c[3] * c[8])) + c[2] * (c[3] * c[7] - c[4] * c[6])


def inverse3(c):
    c = np.asarray(c, dtype=np.float64).reshape(9)
    det = det3(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([(c[4] * c[8] - c[5] * c[7]) / det, (c[2] * c[7] - c[1] * c[8]) / det, (c[1] * c[5] - c[2] * c[4]) / det,
                         (c[5] * c[6] - c[3] * c[8]) / det, (c[0] * c[8] - c[2] * c[6]) / det, (c[2] * c[3] - c[0] * c[5]) / det,
                         (c[3] * c[7] - c[4] * c[6]) / det, (c[1] * c[6] - c[0] * c[7]) / det, (c[0] * c[4] - c[1] * c[3]) / det])


def _strain(c, target, p, max_strain):
    """npt_strain: (the clamped entry of I - mu, did the clamp act?)."""
    e = c * (target - p)
    if e > max_strain:
        return max_strain, True
    if e < -max_strain:
        return -max_strain, True
    return e, False


def graph_np(kin, w32, c, p0, coupling, mask, max_strain, cell):
    """npt_graph for one graph: kin [6], w32 [9] float32, cell [9] float64 -> dict(mu, cell, cell32, inv, e_kin, pressure,
    volume, acted)."""
    one, half = np.float64(1.0), np.float64(0.5)
    c, p0, max_strain = np.float64(c), np.float64(p0), np.float64(max_strain)
    cell = np.asarray(cell, dtype=np.float64).reshape(9)
    w = np.asarray(w32, dtype=np.float32).reshape(9).astype(np.float64)
    det = det3(cell)
    vol = -det if det < 0.0 else det
    p = np.zeros(9)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p[0] = (kin[XX] + half * (w[0] + w[0])) / vol
        p[4] = (kin[YY] + half * (w[4] + w[4])) / vol
        p[8] = (kin[ZZ] + half * (w[8] + w[8])) / vol
        p[1] = p[3] = (kin[XY] + half * (w[1] + w[3])) / vol
        p[2] = p[6] = (kin[XZ] + half * (w[2] + w[6])) / vol
        p[5] = p[7] = (kin[YZ] + half * (w[5] + w[7])) / vol
        pressure = ((p[0] + p[4]) + p[8]) / np.float64(3.0)
    e_kin = half * ((kin[XX] + kin[YY]) + kin[ZZ])
    bad = not np.all(np.isfinite(p))
    mu, acted = np.eye(3).reshape(9), bad
    if not bad:
        if coupling == ISOTROPIC:
            e, hit = _strain(c, p0, pressure, max_strain)
            acted |= hit
            for k in range(3):
                mu[4 * k] = one - e
        elif coupling == AXES:
            for k in range(3):
                if mask & (1 << k):
                    e, hit = _strain(c, p0, p[4 * k], max_strain)
                    acted |= hit
                    mu[4 * k] = one - e
        else:
            for a in range(3):
                for b in range(3):
                    e, hit = _strain(c, p0 if a == b else np.float64(0.0), p[3 * a + b], max_strain)
                    acted |= hit
                    mu[3 * a + b] = (one if a == b else np.float64(0.0)) - e
    new = np.zeros(9)
    for i in range(3):
        for j in range(3):
            new[3 * i + j] = (cell[3 * i] * mu[j] + cell[3 * i + 1] * mu[3 + j]) + cell[3 * i + 2] * mu[6 + j]
    cell32 = new.astype(np.float32)
    return dict(mu=mu, cell=new, cell32=cell32, inv=inverse3(cell32.astype(np.float64)), e_kin=e_kin, pressure=pressure,
                volume=vol, acted=bool(acted))


def scale_np(x, mu):
    """npt_scale_atom on [m,3] coordinates: x mu (row vectors)."""
    mu = mu.reshape(3, 3)
    return (x[:, 0:1] * mu[0] + x[:, 1:2] * mu[1]) + x[:, 2:3] * mu[2]


# ---- the reference trajectory -------------------------------------------------------------------------------------------------
class NumpyNPT(NumpyMD):
    """NumpyMD plus the barostat: `advance()` -> the float32 coordinates to evaluate (and `cell32`, the float32 cells to
    evaluate them in); `finish(f32, virial32, energy, edges)` takes that evaluation's forces and virial."""

    def __init__(self, x, v, masses, dt, cell, pressure, compressibility, taup, coupling="isotropic", mask=(1, 1, 1),
                 max_strain=1e-2, batch=None, num_graphs=None, **kw):
        NumpyMD.__init__(self, x, v, masses, dt, cell=cell, batch=batch, num_graphs=num_graphs, **kw)
        self.B = int(num_graphs) if num_graphs is not None else int(self.batch[-1]) + 1
        self.ptr = np.searchsorted(self.batch, np.arange(self.B + 1))
        self.cell64 = np.array(cell, dtype=np.float64).reshape(self.B, 9)
        self.cell32 = self.cell64.astype(np.float32)
        self.inv64 = np.stack([inverse3(c) for c in self.cell32.astype(np.float64)])
        self._per_atom()
        self.p0 = np.broadcast_to(np.asarray(pressure, dtype=np.float64), (self.B,)).copy()
        self.c = coupling_constant(dt, taup, compressibility, self.B)
        self.coupling, self.mask, self.max_strain = COUPLING[coupling], mask_bits(mask), float(max_strain)
        self.mu = np.tile(np.eye(3).reshape(9), (self.B, 1))
        self.clamped = np.zeros(self.B, dtype=np.int64)
        self.log = []

    def _per_atom(self):
        """What NumpyMD's wrap reads: the widened float32 cell and its inverse, per atom."""
        self.cell = self.cell32.astype(np.float64).reshape(self.B, 3, 3)[self.batch]
        self.inv = self.inv64.reshape(self.B, 3, 3)[self.batch]

    def finish(self, f32, virial32, energy=None, edges=0):
        self.f = np.array(f32, dtype=np.float32)
        finish_np(self.v, self.f, self.kick, self.half_mass)
        w = np.asarray(virial32, dtype=np.float32).reshape(self.B, 9)
        e = np.zeros(self.B, dtype=np.float32) if energy is None else np.asarray(energy, dtype=np.float32).reshape(self.B)
        row = np.zeros((self.B, 5))
        for g in range(self.B):
            a, b = self.ptr[g], self.ptr[g + 1]
            kin = kinetic_sums(self.v[a:b], self.half_mass[a:b])
            r = graph_np(kin, w[g], self.c[g], self.p0[g], self.coupling, self.mask, self.max_strain, self.cell64[g])
            self.cell64[g], self.cell32[g], self.inv64[g], self.mu[g] = r["cell"], r["cell32"], r["inv"], r["mu"]
            self.clamped[g] += int(r["acted"])
            self.x[a:b] = scale_np(self.x[a:b], r["mu"])
            row[g] = (np.float64(e[g]), r["e_kin"], float(edges), r["pressure"], r["volume"])
        self._per_atom()
        self.log.append(row)
        self.step += 1


# ---- the host twins -----------------------------------------------------------------------------------------------------------
class HostNPT(HostMD):
    """The library's host twins on numpy arrays: HostMD's advance, hermnet_host_md_finish_npt as the finish."""

    def __init__(self, x, v, masses, dt, cell, pressure, compressibility, taup, coupling="isotropic", mask=(1, 1, 1),
                 max_strain=1e-2, log_steps=64, **kw):
        HostMD.__init__(self, x, v, masses, dt, cell=cell, log_steps=log_steps, **kw)
        B = self.B
        self.cell64 = np.array(cell, dtype=np.float64).reshape(B, 9)
        self.cell = np.ascontiguousarray(self.cell64.astype(np.float32))                # cell32: what advance wraps with
        self.inv = np.stack([inverse3(c) for c in self.cell.astype(np.float64)])
        self.mu = np.tile(np.eye(3).reshape(9), (B, 1))
        self.clamped = np.zeros(B, dtype=np.int64)
        self.p0 = np.broadcast_to(np.asarray(pressure, dtype=np.float64), (B,)).copy()
        self.c = np.ascontiguousarray(coupling_constant(dt, taup, compressibility, B))
        self.coupling, self.mask, self.max_strain = COUPLING[coupling], mask_bits(mask), float(max_strain)
        self.log = np.full((log_steps, B, 5), -7.0)

    def finish(self, f32, virial32, energy=None, total=(0, 0), capacity=1 << 20):
        f, e, tot = self._evaluation(f32, energy, total)
        w = np.ascontiguousarray(virial32, dtype=np.float32).reshape(self.B, 9)
        rc = self.lib.hermnet_host_md_finish_npt(
            self.n, self.B, _p(self.graph_ptr), _p(self.batch), _p(f), _p(e), _p(w), _p(tot), capacity, self.coupling, self.mask,
            self.max_strain, _p(self.p0), _p(self.c), *self._finish_atoms(), _p(self.cell64), _p(self.cell), _p(self.inv),
            _p(self.mu), _p(self.clamped), *self._finish_tail())
        assert rc == 0
