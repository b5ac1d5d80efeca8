"""The MD observers of hermnet_amd/csrc/observe_step.h twice over: `NumpyFrames`, `NumpyRDF`, `NumpyMSD` transcribe the header
operation by operation in numpy float64; `HostFrames`, `HostRDF`, `HostMSD` hold the same arrays and call the library's host
twins (hermnet_host_observe_*).  Both kinds are offered a configuration with `offer(state, ...)` -- one observer launch of a
replay -- and keep `obs`, their rings and counts as numpy arrays of the same names, so a test compares them field by field."""
import ctypes

import numpy as np

from hermnet_amd import _lib
from hermnet_amd.observe import pair_counts, rdf_edges, rdf_fits, rdf_work, species_of  # noqa: F401


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def state_words(step, code=0):
    return np.array([step, code, 0, 0], dtype=np.int64)


def _cells(cell, B):
    """[B,3,3] float32 of a cell given as [3,3] or [B,3,3] (None stays None)."""
    return None if cell is None else np.ascontiguousarray(np.asarray(cell, dtype=np.float32).reshape(B, 3, 3))


class _Words(object):
    def _start(self, stride):
        self.stride = int(stride)
        self.obs = np.array([-1, 0, 0, 0], dtype=np.int64)

    def due(self, state):
        return state[1] == 0 and state[0] % self.stride == 0 and state[0] > self.obs[0]

    def commit(self, state):
        self.obs[0] = state[0]
        self.obs[1] += 1


# ---- frames -------------------------------------------------------------------------------------------------------------------
class NumpyFrames(_Words):
    def __init__(self, n, num_graphs, stride, frames, velocities=False, images=False, periodic=True):
        self._start(stride)
        self.n, self.B, self.frames = n, num_graphs, frames
        self.steps = np.zeros(frames, dtype=np.int64)
        self.positions = np.zeros((frames, n, 3), dtype=np.float32)
        self.velocities = np.zeros((frames, n, 3), dtype=np.float32) if velocities else None
        self.images = np.zeros((frames, n, 3), dtype=np.int32) if images else None
        self.cells = np.zeros((frames, num_graphs, 3, 3), dtype=np.float32) if periodic else None

    def offer(self, state, x, v=None, image=None, cell=None):
        if not self.due(state):
            return
        slot = self.obs[1] % self.frames
        self.positions[slot] = np.asarray(x, dtype=np.float64).astype(np.float32)
        if self.velocities is not None:
            self.velocities[slot] = np.asarray(v, dtype=np.float64).astype(np.float32)
        if self.images is not None:
            self.images[slot] = image
        if self.cells is not None:
            self.cells[slot] = _cells(cell, self.B)
        self.steps[slot] = state[0]
        self.commit(state)


class HostFrames(NumpyFrames):
    def offer(self, state, x, v=None, image=None, cell=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        v = None if self.velocities is None else np.ascontiguousarray(v, dtype=np.float64)
        image = None if self.images is None else np.ascontiguousarray(image, dtype=np.int32)
        cell = _cells(cell, self.B) if self.cells is not None else None
        _lib.call("hermnet_host_observe_frames", self.n, self.B, self.stride, self.frames, _p(x), _p(v), _p(image), _p(cell),
                  _p(state), _p(self.obs), _p(self.steps), _p(self.positions), _p(self.velocities), _p(self.images), _p(self.cells))


# ---- mean-squared displacement ------------------------------------------------------------------------------------------------
def canonical_sums(terms, lo, hi):
    """csrc/resident_step.h: hn_canonical_sums over the rows lo..hi-1 of `terms` [n,K] (rows that add nothing hold 0.0:
    a lane's partial starts at +0.0 and never becomes -0.0, so adding 0.0 leaves its bits)."""
    K = terms.shape[1]
    rows = -(-(hi - lo) // 256)
    padded = np.zeros((max(rows, 0) * 256, K))
    padded[:hi - lo] = terms[lo:hi]
    part = np.zeros((256, K))
    for chunk in padded.reshape(-1, 256, K):
        part = part + chunk
    m = 128
    while m >= 1:
        part[:m] = part[:m] + part[m:2 * m]
        m //= 2
    return part[0]


class NumpyMSD(_Words):
    def __init__(self, z, graph_ptr, stride, rows, periodic=True):
        self._start(stride)
        self.kinds, self.species = species_of(z)
        self.ptr = np.asarray(graph_ptr, dtype=np.int32)
        self.n, self.B, self.S, self.rows, self.periodic = len(self.species), len(self.ptr) - 1, len(self.kinds), rows, periodic
        self.steps = np.zeros(rows, dtype=np.int64)
        self.sums = np.zeros((rows, self.B, self.S, 4))
        self.x_origin = np.zeros((self.n, 3))
        self.image_origin = np.zeros((self.n, 3), dtype=np.int32)

    def offer(self, state, x, image, cell=None):
        if not self.due(state):
            return
        x, image = np.asarray(x, dtype=np.float64), np.asarray(image, dtype=np.int32)
        if self.obs[1] == 0:
            self.x_origin[:], self.image_origin[:] = x, image
        slot = self.obs[1] % self.rows
        d = x - self.x_origin
        if self.periodic:
            di = (image - self.image_origin).astype(np.float64)
            c = _cells(cell, self.B).astype(np.float64)[np.repeat(np.arange(self.B), np.diff(self.ptr))]      # [N,3,3]
            d = d + ((di[:, 0:1] * c[:, 0, :] + di[:, 1:2] * c[:, 1, :]) + di[:, 2:3] * c[:, 2, :])
        terms = np.concatenate([d, ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]], axis=1)
        for g in range(self.B):
            for s in range(self.S):
                mine = np.where((self.species == s)[:, None], terms, 0.0)
                self.sums[slot, g, s] = canonical_sums(mine, int(self.ptr[g]), int(self.ptr[g + 1]))
        self.steps[slot] = state[0]
        self.commit(state)


class HostMSD(NumpyMSD):
    def offer(self, state, x, image, cell=None):
        x, image = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(image, dtype=np.int32)
        cell = _cells(cell, self.B) if self.periodic else None
        _lib.call("hermnet_host_observe_msd", self.n, self.B, self.S, self.stride, self.rows, _p(self.ptr), _p(self.species),
                  _p(x), _p(image), _p(cell), _p(state), _p(self.obs), _p(self.steps), _p(self.x_origin), _p(self.image_origin),
                  _p(self.sums))


# ---- radial distribution function -----------------------------------------------------------------------------------------------
def pair_r2(x, cell, inv):
    """r^2 [n,n] of one graph by observe_step.h's definition: x [n,3] float64, cell / inv [3,3] float64 (None: open)."""
    x = np.asarray(x, dtype=np.float64)
    if cell is None:
        s = x
    else:
        s = np.stack([(x[:, 0] * inv[0, k] + x[:, 1] * inv[1, k]) + x[:, 2] * inv[2, k] for k in range(3)], axis=1)
    ds = s[:, None, :] - s[None, :, :]
    if cell is None:
        d = ds
    else:
        ds = ds - np.floor(ds + 0.5)
        d = np.stack([(ds[..., 0] * cell[0, j] + ds[..., 1] * cell[1, j]) + ds[..., 2] * cell[2, j] for j in range(3)], axis=-1)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


class NumpyRDF(_Words):
    def __init__(self, z, graph_ptr, r_max, bins, stride=1, slots=None, periodic=True):
        self._start(stride)
        self.kinds, self.species = species_of(z)
        self.ptr = np.asarray(graph_ptr, dtype=np.int32)
        self.n, self.B, self.S = len(self.species), len(self.ptr) - 1, len(self.kinds)
        self.P, self.bins, self.r_max, self.periodic = self.S * (self.S + 1) // 2, int(bins), float(r_max), periodic
        self.slots = self.B if slots is None else int(slots)
        self.edges, self.edge2 = rdf_edges(r_max, bins)
        self.work = np.ascontiguousarray(rdf_work(self.ptr))
        self.counts = np.zeros((self.slots, self.P, self.bins), dtype=np.int64)
        self.samples = np.zeros(self.slots, dtype=np.int64)
        self.skipped = np.zeros(self.slots, dtype=np.int64)
        self.volume_sum = np.zeros(self.slots)
        per_graph = np.stack([np.bincount(self.species[a:b], minlength=self.S) for a, b in zip(self.ptr[:-1], self.ptr[1:])])
        self.n_pairs = pair_counts(per_graph)

    def pair_index(self, a, b):
        return a * self.S - a * (a - 1) // 2 + (b - a)

    def offer(self, state, x, cell=None, inv=None, slot_of=None):
        """cell: the float32 cell [B,3,3] (or [3,3]); inv: ITS float64 inverse as the driver holds it."""
        if not self.due(state):
            return
        x = np.asarray(x, dtype=np.float64)
        cells = _cells(cell, self.B).astype(np.float64) if self.periodic else None
        invs = np.asarray(inv, dtype=np.float64).reshape(self.B, 3, 3) if self.periodic else None
        fits = rdf_fits(self.r_max, invs) if self.periodic else np.ones(self.B, dtype=bool)
        for g in range(self.B):
            slot = g if slot_of is None else int(slot_of[g])
            if not fits[g]:
                self.skipped[slot] += 1
                continue
            lo, hi = int(self.ptr[g]), int(self.ptr[g + 1])
            sp = self.species[lo:hi]
            for first in range(0, hi - lo, 512):          # rows in blocks: [512, n] at a time
                rows = slice(first, min(first + 512, hi - lo))
                if self.periodic:
                    r2 = _rows_r2(x[lo:hi], rows, cells[g], invs[g])
                else:
                    r2 = _rows_r2(x[lo:hi], rows, None, None)
                b = np.searchsorted(self.edge2, r2, side="right") - 1          # edge2[b] <= r2 < edge2[b+1]
                i, j = np.nonzero((np.arange(hi - lo)[None, :] > np.arange(rows.start, rows.stop)[:, None]) & (b < self.bins) & (b >= 0))
                za, zb = sp[rows][i], sp[j]
                pair = self.pair_index(np.minimum(za, zb), np.maximum(za, zb))
                np.add.at(self.counts[slot], (pair, b[i, j]), 1)
            self.samples[slot] += 1
            if self.periodic:
                c = cells[g].reshape(9)
                det = (c[0] * (c[4] * c[8] - c[5] * c[7]) + c[1] * (c[5] * c[6] - c[3] * c[8])) + c[2] * (c[3] * c[7] - c[4] * c[6])
                self.volume_sum[slot] = self.volume_sum[slot] + abs(det)
        self.commit(state)


def _rows_r2(x, rows, cell, inv):
    """pair_r2's rows `rows` (atom i of the rows against every atom j)."""
    if cell is None:
        s = x
    else:
        s = np.stack([(x[:, 0] * inv[0, k] + x[:, 1] * inv[1, k]) + x[:, 2] * inv[2, k] for k in range(3)], axis=1)
    ds = s[rows, None, :] - s[None, :, :]
    if cell is None:
        d = ds
    else:
        ds = ds - np.floor(ds + 0.5)
        d = np.stack([(ds[..., 0] * cell[0, j] + ds[..., 1] * cell[1, j]) + ds[..., 2] * cell[2, j] for j in range(3)], axis=-1)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


class HostRDF(NumpyRDF):
    def offer(self, state, x, cell=None, inv=None, slot_of=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        cell = _cells(cell, self.B) if self.periodic else None
        inv = np.ascontiguousarray(np.asarray(inv, dtype=np.float64).reshape(self.B, 3, 3)) if self.periodic else None
        slot_of = None if slot_of is None else np.ascontiguousarray(slot_of, dtype=np.int64)
        _lib.call("hermnet_host_observe_rdf", self.n, self.B, self.S, self.bins, self.slots, self.stride, self.r_max * self.r_max,
                  _p(self.ptr), _p(self.species), _p(x), _p(cell), _p(inv), _p(slot_of), _p(self.edge2), _p(self.work),
                  len(self.work), _p(state), _p(self.obs), _p(self.counts), _p(self.samples), _p(self.skipped),
                  _p(self.volume_sum))
