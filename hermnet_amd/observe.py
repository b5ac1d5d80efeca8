"""MD observers: trajectory frames, radial distribution functions and mean-squared displacements taken INSIDE the replayed
step of a device-resident MD driver.

`DeviceMD` and the drivers built on it make one hipGraph replay one time step, and `run(n)` never stops -- but what a run
leaves behind is the log ring and the final state; a configuration in between costs a `fetch()` (a synchronisation and a
download) and an analysis on the host per sample.  An observer is a small set of kernels behind the driver's finish
(csrc/observe_kernels.hip; the definitions are csrc/observe_step.h) that, every `stride` committed steps, records a frame
into a device ring, adds to a species-resolved pair histogram, or appends a row of displacement sums:

    md = DeviceMD(model, z, cell, pos, masses, dt,
                  observers=[Frames(stride=10, frames=256), RDF(r_max=6.0, bins=120, stride=5), MSD(stride=5, rows=1024)])
    md.run(2000)
    s = md.fetch()              # still ONE packed copy and one synchronisation
    s.observers[0]              # Frames: steps [k], positions [k,N,3] f32, cell [k,B,3,3] f32 (, velocities, images)
    s.observers[1]              # RDF: counts [slots,P,bins] int64, samples, skipped [slots], pairs, r, g [slots,P,bins]
    s.observers[2]              # MSD: steps [k], sums [k,B,S,4], msd [k,B,S], msd_drift_corrected [k,B,S], species

`observers=` is a keyword of `DeviceMD`, `DeviceNPT`, `DeviceREMD` and `DevicePIMD` (not of the relaxation and NEB drivers).
An observer object serves one driver.

Protocol (csrc/observe_step.h): an observer's kernels follow the driver's commit, and a sample is due iff the halt code is
0, the step is a multiple of `stride` and later than the observer's last sample.  So the start configuration is sampled as
step 0 (with the velocities given to the constructor; `maxwell_boltzmann()` behind it is not seen by that frame), a void
step, a halted or a parked replay record nothing, and a resumed run's observers equal an uninterrupted run's.  `run(n)`
refuses, as it does for log rows, when a ring (`frames`, `rows`) could overwrite entries not fetched yet; the host counts
the multiples of `stride` in the steps the pending replays can reach, which void steps can only make fewer.  A `fetch()`
carries only the ring entries not fetched yet.  Everything travels in the packed copy as float64: the histogram's counts
are exact below 2^53.

`RDF`: all pairs i < j of a graph by the minimum image in float64, binned by comparisons against squared edges made on the
host -- device, host twin and tests/observe_reference.py count the same integers.  Rounding the fractional difference finds
the nearest image of every vector shorter than half the smallest cell height, so the constructor refuses a larger `r_max`,
and under a barostat the kernel checks every sample: a graph whose cell has shrunk below 2 r_max skips that sample (counted
in `skipped`), it never records wrong counts.  `g = counts <V> / (n_pairs shell samples)`: 1 for an ideal gas.  Slots are
graphs; with `by_rung=True` (`DeviceREMD` alone) a replica adds to the slot of the rung it holds behind the step's exchange,
so a histogram belongs to a temperature.  `MSD`: d = (x - x_o) + (image - image_o) cell against the origin stored at the
first sample, with the CURRENT cell (under a barostat: a convention); per graph and species the sums of d and |d|^2."""
import math
import types

import numpy as np
import torch

from . import _lib

MAX_BINS = 1024                           # csrc/observe_step.h: HN_OBS_RDF_MAX_BINS
MAX_HIST = 8192                           # ... HN_OBS_RDF_MAX_HIST: species pairs x bins, the LDS histogram's budget
TILE = 256                                # ... HN_OBS_TILE


def species_of(atomic_number):
    """(the sorted distinct atomic numbers [S], each atom's index among them [N] int32)."""
    z = np.asarray(atomic_number, dtype=np.int64).reshape(-1)
    kinds = np.unique(z)
    return kinds, np.searchsorted(kinds, z).astype(np.int32)


def species_pairs(kinds):
    """The species pairs (Za, Zb), a <= b, in the order of the histograms (csrc/observe_step.h: obs_pair_index)."""
    return [(int(kinds[a]), int(kinds[b])) for a in range(len(kinds)) for b in range(a, len(kinds))]


def rdf_edges(r_max, bins):
    """(the bin edges [bins+1], their squares: what the kernels compare r^2 against), float64."""
    r = np.arange(int(bins) + 1, dtype=np.float64) * float(r_max) / int(bins)
    return r, r * r


def rdf_work(graph_ptr):
    """The work list [W,3] int32 = (graph, tile_i, tile_j >= tile_i) over the 256-atom tiles of every graph."""
    work = [(g, i, j) for g in range(len(graph_ptr) - 1)
            for i in range(-(-int(graph_ptr[g + 1] - graph_ptr[g]) // TILE)) for j in range(i, -(-int(graph_ptr[g + 1] - graph_ptr[g]) // TILE))]
    return np.asarray(work, dtype=np.int32).reshape(-1, 3)


def rdf_fits(r_max, inv):
    """[B] bool: r_max^2 |column k of inv|^2 <= 1/4 for k = 0, 1, 2 -- r_max is at most half of every cell height (the
    kernel's own check, operation by operation)."""
    inv = np.asarray(inv, dtype=np.float64).reshape(-1, 3, 3)
    q = (inv[:, 0, :] * inv[:, 0, :] + inv[:, 1, :] * inv[:, 1, :]) + inv[:, 2, :] * inv[:, 2, :]
    return np.all((float(r_max) * float(r_max)) * q <= 0.25, axis=1)


def pair_counts(species_count):
    """[.., P] pairs of every species pair from [.., S] atoms per species: N_a N_b, N_a (N_a - 1) / 2 for a = b."""
    c = np.asarray(species_count, dtype=np.int64)
    S = c.shape[-1]
    return np.stack([c[..., a] * (c[..., a] - 1) // 2 if a == b else c[..., a] * c[..., b]
                     for a in range(S) for b in range(a, S)], axis=-1)


def rdf_g(counts, samples, volume_sum, n_pairs, r_max, bins):
    """g [slots,P,bins] = counts <V> / (n_pairs shell samples), <V> = volume_sum / samples; NaN where a slot has no sample or
    a species pair no pair."""
    r, _ = rdf_edges(r_max, bins)
    shell = 4.0 * math.pi / 3.0 * (r[1:] ** 3 - r[:-1] ** 3)
    samples = np.asarray(samples, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_v = np.asarray(volume_sum, dtype=np.float64) / samples
        return (np.asarray(counts, dtype=np.float64) * mean_v[:, None, None]
                / (np.asarray(n_pairs, dtype=np.float64)[:, :, None] * shell[None, None, :] * samples[:, None, None]))


class _Observer(object):
    """What the three observers share: the stride, the obs words on the device, what the host knows of them (as of the last
    fetch) and the count of samples that can be due."""

    __slots__ = ("stride", "obs", "_last", "_taken", "_bound")

    def _init(self, stride):
        if int(stride) != stride or int(stride) < 1:
            raise ValueError("%s: stride must be an integer >= 1" % type(self).__name__)
        self.stride = int(stride)         # a sample every that many committed steps
        self.obs = None                   # [4] int64 on the device = (last sampled step, samples taken, 0, 0); the commit kernel
        self._last, self._taken = -1, 0   # obs[0], obs[1] as of the last fetch
        self._bound = False               # `_bind`: an observer serves one driver

    def _bind_words(self, driver):
        if self._bound:
            raise ValueError("%s: this observer already serves a driver -- make one per driver" % type(self).__name__)
        self._bound = True
        self.obs = torch.tensor([-1, 0, 0, 0], dtype=torch.int64).to(driver.device)

    def _unfetched(self, driver, n=0):
        """The most samples taken since the last fetch once the pending replays and `n` more are through: the multiples of
        `stride` in (last sampled step, the step they can reach]."""
        reach = driver._logged + driver._pending + int(n)
        return max(0, reach // self.stride - (self._last // self.stride if self._last >= 0 else -1))

    def _check_run(self, driver, n):
        """Rings only: refuse a run that could overwrite entries not fetched yet."""

    def _ring(self, ring):
        """The ring indices of the samples not fetched yet (as many as `_unfetched` allows), on the device."""
        k = min(self._k, ring)
        return (torch.arange(k, device=self.obs.device) + self._taken) % ring

    def _words(self, h):
        """Read the obs words at the head of `h`; returns how many samples were taken since the last fetch."""
        last, taken = int(h[0]), int(h[1])
        k = taken - self._taken
        self._last, self._taken = last, taken
        return k


def _cell_ptr(step):
    return None if step.cell is None else step.cell.data_ptr()


class Frames(_Observer):
    """A ring of `frames` trajectory frames, one every `stride` steps: float32 positions (the rounding of the wrapped
    float64 state) and the step's float32 cell; `velocities=True` adds float32 velocities, `images=True` the int32 image
    counts (positions + images @ cell is the unwrapped path).  Snapshot: `steps` [k], `positions` [k,N,3], `cell` [k,B,3,3]
    (None for open structures), `velocities`, `images` (None where not recorded) -- the k frames not fetched yet."""

    __slots__ = ("frames", "velocities", "images", "steps", "positions", "cells", "vel", "img", "_k")

    def __init__(self, stride=1, frames=256, velocities=False, images=False):
        self._init(stride)
        if int(frames) < 1:
            raise ValueError("Frames: frames >= 1")
        self.frames, self.velocities, self.images = int(frames), bool(velocities), bool(images)

    def _bind(self, driver, cell):
        self._bind_words(driver)
        n, B, dev, F = driver.n, driver.num_graphs, driver.device, self.frames
        self.steps = torch.zeros(F, dtype=torch.int64, device=dev)                   # the step of every slot; the commit kernel
        self.positions = torch.zeros(F, n, 3, dtype=torch.float32, device=dev)      # the ring; the frame kernel
        self.cells = None if cell is None else torch.zeros(F, B, 3, 3, dtype=torch.float32, device=dev)
        self.vel = torch.zeros(F, n, 3, dtype=torch.float32, device=dev) if self.velocities else None
        self.img = torch.zeros(F, n, 3, dtype=torch.int32, device=dev) if self.images else None
        self._k = 0                       # `_parts`: the entries the packed copy carries

    def _launch(self, driver, step):
        P = _lib.ptr
        if (step.cell is None) != (self.cells is None):
            raise RuntimeError("Frames: the captured step's cell changed its kind")
        _lib.call("hermnet_observe_frames", driver.n, driver.num_graphs, self.stride, self.frames, P(driver.x),
                  P(driver.v) if self.velocities else None, P(driver.image) if self.images else None, _cell_ptr(step),
                  P(driver.state), P(self.obs), P(self.steps), P(self.positions), P(self.vel), P(self.img), P(self.cells),
                  torch.cuda.current_stream(driver.device).cuda_stream)

    def _check_run(self, driver, n):
        if self._unfetched(driver, n) > self.frames:
            raise RuntimeError("%s.run(%d) would overwrite frames not fetched yet (up to %d due, frames=%d): fetch() first"
                               % (type(driver).__name__, n, self._unfetched(driver, n), self.frames))

    def _parts(self, driver):
        self._k = self._unfetched(driver)
        idx = self._ring(self.frames)
        rings = [self.steps, self.positions, self.cells, self.vel, self.img]
        return [self.obs.double()] + [t.index_select(0, idx).double().reshape(-1) for t in rings if t is not None]

    def _read(self, driver, h):
        """The snapshot's entry and the elements of `h` it used."""
        n, B, cap = driver.n, driver.num_graphs, min(self._k, self.frames)
        k = self._words(h)
        assert 0 <= k <= cap, (k, cap)
        o = 4
        take = lambda width: h[o:o + cap * width].reshape(cap, width)[:k]
        s = types.SimpleNamespace(steps=take(1).reshape(k).astype(np.int64), cell=None, velocities=None, images=None)
        o += cap
        s.positions = take(3 * n).astype(np.float32).reshape(k, n, 3)
        o += cap * 3 * n
        if self.cells is not None:
            s.cell = take(9 * B).astype(np.float32).reshape(k, B, 3, 3)
            o += cap * 9 * B
        if self.vel is not None:
            s.velocities = take(3 * n).astype(np.float32).reshape(k, n, 3)
            o += cap * 3 * n
        if self.img is not None:
            s.images = take(3 * n).astype(np.int32).reshape(k, n, 3)
            o += cap * 3 * n
        return s, o


class RDF(_Observer):
    """Species-resolved radial distribution functions up to `r_max` (A) in `bins` bins, a sample every `stride` steps (the
    module docstring).  ValueError: `r_max` above half the smallest cell height of a graph; more than 1024 bins or more than
    8192 histogram cells (species pairs x bins: the kernel's LDS budget); `by_rung` with a driver that has no rungs.

    Snapshot (cumulative since the construction): `counts` [slots,P,bins] int64, `samples`, `skipped` [slots], `volume_sum`
    [slots], `pairs` [(Za, Zb), ...] (a <= b, sorted atomic numbers), `edges` [bins+1], `r` [bins] (bin centres), `n_pairs`
    [slots,P] and `g` [slots,P,bins] float64 (None for open structures, which have no volume)."""

    __slots__ = ("r_max", "bins", "by_rung", "kinds", "species", "work", "edge2", "counts", "samples", "skipped", "volume_sum",
                 "n_pairs", "periodic")

    def __init__(self, r_max, bins, stride=1, by_rung=False):
        self._init(stride)
        self.r_max, self.bins, self.by_rung = float(r_max), int(bins), bool(by_rung)
        if not (self.r_max > 0.0 and math.isfinite(self.r_max)) or not (1 <= self.bins <= MAX_BINS):
            raise ValueError("RDF: r_max > 0 and 1 <= bins <= %d" % MAX_BINS)

    def _bind(self, driver, cell):
        B, dev = driver.num_graphs, driver.device
        if self.by_rung and getattr(driver, "rung", None) is None:
            raise ValueError("RDF(by_rung=True): %s has no rungs -- DeviceREMD alone" % type(driver).__name__)
        self.kinds, species = species_of(driver.z.cpu().numpy())
        S = len(self.kinds)
        if S * (S + 1) // 2 * self.bins > MAX_HIST:
            raise ValueError("RDF: %d species pairs x %d bins = %d histogram cells -- at most %d"
                             % (S * (S + 1) // 2, self.bins, S * (S + 1) // 2 * self.bins, MAX_HIST))
        self.periodic = cell is not None
        if self.periodic:
            c32 = torch.as_tensor(cell).detach().float().cpu().numpy().astype(np.float64).reshape(B, 3, 3)
            fits = rdf_fits(self.r_max, np.linalg.inv(c32))
            if not np.all(fits):
                raise ValueError("RDF: r_max = %g A is more than half the smallest cell height of graph %d (rounding the "
                                 "fractional difference is the minimum image only below it)" % (self.r_max, int(np.argmin(fits))))
        self._bind_words(driver)
        ptr = driver.graph_ptr.cpu().numpy()
        per_graph = np.stack([np.bincount(species[ptr[g]:ptr[g + 1]], minlength=S) for g in range(B)])
        self.n_pairs = pair_counts(per_graph)             # [slots,P] on the host (by_rung: the replicas are copies of one system)
        self.species = torch.from_numpy(species).to(dev)  # [N] int32
        self.work = torch.from_numpy(rdf_work(ptr)).to(dev)          # [W,3] int32
        self.edge2 = torch.from_numpy(rdf_edges(self.r_max, self.bins)[1]).to(dev)      # [bins+1] f64
        self.counts = torch.zeros(B, S * (S + 1) // 2, self.bins, dtype=torch.int64, device=dev)    # the pair kernel's integer adds
        self.samples = torch.zeros(B, dtype=torch.int64, device=dev)                 # the commit kernel
        self.skipped = torch.zeros(B, dtype=torch.int64, device=dev)                 # the commit kernel
        self.volume_sum = torch.zeros(B, dtype=torch.float64, device=dev)            # the commit kernel

    def _launch(self, driver, step):
        P = _lib.ptr
        if (step.cell is None) == self.periodic:
            raise RuntimeError("RDF: the captured step's cell changed its kind")
        inv = None if step.cell is None else driver._inverse_of(step.cell).data_ptr()
        _lib.call("hermnet_observe_rdf", driver.n, driver.num_graphs, len(self.kinds), self.bins, driver.num_graphs, self.stride,
                  self.r_max * self.r_max, P(driver.graph_ptr), P(self.species), P(driver.x), _cell_ptr(step), inv,
                  P(driver.rung) if self.by_rung else None, P(self.edge2), P(self.work), int(self.work.shape[0]),
                  P(driver.state), P(self.obs), P(self.counts), P(self.samples), P(self.skipped), P(self.volume_sum),
                  torch.cuda.current_stream(driver.device).cuda_stream)

    def _parts(self, driver):
        return [self.obs.double(), self.counts.double().reshape(-1), self.samples.double(), self.skipped.double(), self.volume_sum]

    def _read(self, driver, h):
        B, bins = driver.num_graphs, self.bins
        P = self.counts.shape[1]
        self._words(h)
        o = 4
        s = types.SimpleNamespace(counts=h[o:o + B * P * bins].astype(np.int64).reshape(B, P, bins))
        o += B * P * bins
        s.samples, s.skipped = h[o:o + B].astype(np.int64), h[o + B:o + 2 * B].astype(np.int64)
        s.volume_sum = h[o + 2 * B:o + 3 * B].copy()
        o += 3 * B
        s.pairs, s.n_pairs = species_pairs(self.kinds), self.n_pairs
        s.edges = rdf_edges(self.r_max, bins)[0]
        s.r = 0.5 * (s.edges[1:] + s.edges[:-1])
        s.g = rdf_g(s.counts, s.samples, s.volume_sum, s.n_pairs, self.r_max, bins) if self.periodic else None
        return s, o


class MSD(_Observer):
    """A ring of `rows` rows of displacement sums, one every `stride` steps, against the origin stored at the first sample
    (the module docstring).  Snapshot -- the k rows not fetched yet --: `steps` [k], `sums` [k,B,S,4] = (sum d_x, sum d_y,
    sum d_z, sum |d|^2) per graph and species, `msd` [k,B,S] = sum |d|^2 / n_s, `msd_drift_corrected` = msd - |sum d / n_s|^2,
    `species` [S] (the sorted atomic numbers) and `n_species` [B,S]."""

    __slots__ = ("rows", "kinds", "species", "n_species", "steps", "sums", "x_origin", "image_origin", "_k")

    def __init__(self, stride=1, rows=1024):
        self._init(stride)
        if int(rows) < 1:
            raise ValueError("MSD: rows >= 1")
        self.rows = int(rows)

    def _bind(self, driver, cell):
        self._bind_words(driver)
        B, dev = driver.num_graphs, driver.device
        self.kinds, species = species_of(driver.z.cpu().numpy())
        S, ptr = len(self.kinds), driver.graph_ptr.cpu().numpy()
        self.n_species = np.stack([np.bincount(species[ptr[g]:ptr[g + 1]], minlength=S) for g in range(B)])   # [B,S], host
        self.species = torch.from_numpy(species).to(dev)  # [N] int32
        self.steps = torch.zeros(self.rows, dtype=torch.int64, device=dev)           # the commit kernel
        self.sums = torch.zeros(self.rows, B, S, 4, dtype=torch.float64, device=dev)            # the sums kernel
        self.x_origin = torch.zeros_like(driver.x)        # the sums kernel, at the first sample
        self.image_origin = torch.zeros_like(driver.image)
        self._k = 0

    def _launch(self, driver, step):
        P = _lib.ptr
        _lib.call("hermnet_observe_msd", driver.n, driver.num_graphs, len(self.kinds), self.stride, self.rows, P(driver.graph_ptr),
                  P(self.species), P(driver.x), P(driver.image), _cell_ptr(step), P(driver.state), P(self.obs), P(self.steps),
                  P(self.x_origin), P(self.image_origin), P(self.sums), torch.cuda.current_stream(driver.device).cuda_stream)

    def _check_run(self, driver, n):
        if self._unfetched(driver, n) > self.rows:
            raise RuntimeError("%s.run(%d) would overwrite MSD rows not fetched yet (up to %d due, rows=%d): fetch() first"
                               % (type(driver).__name__, n, self._unfetched(driver, n), self.rows))

    def _parts(self, driver):
        self._k = self._unfetched(driver)
        idx = self._ring(self.rows)
        return [self.obs.double(), self.steps.index_select(0, idx).double(), self.sums.index_select(0, idx).reshape(-1)]

    def _read(self, driver, h):
        B, S, cap = driver.num_graphs, len(self.kinds), min(self._k, self.rows)
        k = self._words(h)
        assert 0 <= k <= cap, (k, cap)
        s = types.SimpleNamespace(steps=h[4:4 + cap][:k].astype(np.int64), species=self.kinds.copy(), n_species=self.n_species)
        s.sums = h[4 + cap:4 + cap + cap * B * S * 4].reshape(cap, B, S, 4)[:k].copy()
        s.msd, s.msd_drift_corrected = msd_of(s.sums, self.n_species)
        return s, 4 + cap + cap * B * S * 4


def msd_of(sums, n_species):
    """(msd, drift-corrected msd) [k,B,S] from the sums [k,B,S,4] and the atoms per graph and species [B,S]; NaN where a graph
    has no atom of a species."""
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.asarray(n_species, dtype=np.float64)[None]
        msd = sums[..., 3] / n
        drift = sums[..., :3] / n[..., None]
        return msd, msd - ((drift[..., 0] * drift[..., 0] + drift[..., 1] * drift[..., 1]) + drift[..., 2] * drift[..., 2])
