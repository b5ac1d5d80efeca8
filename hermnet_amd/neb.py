"""Device-resident nudged elastic band: climbing-image NEB with improved tangents for one band or several, INSIDE the
replayed hipGraph.

A band of images is a batch of replicas, which is what `GraphedBatchMDStep` evaluates in one step.  A host-driven NEB is
that step, a `fetch()`, then the NEB projection and the optimiser in numpy -- per force evaluation.  `DeviceNEB` keeps all
of it on the device: `hermnet_relax_advance` in front of the search, unchanged, and `hermnet_neb_finish`
(csrc/neb_kernels.hip; the definition is csrc/neb_step.h) behind the force backward, so that one replay IS one force
evaluation of every image, the projection, and one step of FIRE on every band:

    neb = DeviceNEB(model, z, cells, pos, batch=batch, num_graphs=B, k=0.1, climb=True, fmax=0.05)
    neb.run(50)                 # 50 replays enqueued; returns at once
    s = neb.fetch()             # ONE packed device-to-host copy: s.converged [K], s.climbing_image [K], s.energy [B], ...
    s = neb.run_until(500)      # ... or: chunks of replays until every band has converged

The method is Henkelman & Jonsson's improved tangent (J. Chem. Phys. 113, 9978) with a climbing image, ASE's
`NEB(method="improvedtangent", climb=...)`, under ASE's FIRE with ASE's defaults, applied to each band AS A WHOLE: its sums
run over all interior images.  Unlike the relaxation's, the graphs are coupled: an image's force needs its neighbours'
coordinates and energies.  The sums take one documented order without atomics (per image the canonical order of
csrc/resident_step.h, then over the band's images in ascending order), so the device, the library's host twin and a numpy
transcription agree bit for bit (tests/test_neb_host.py, tests/test_neb_device.py).

NO WRAP.  The driver always advances without the wrap and has no `wrap` argument: displacements between neighbouring
images are then plain differences, and a band stays continuous in the coordinates it was given.  The neighbour search copes
with coordinates a few cells outside.  The images given must be continuous themselves: neighbouring periodic images whose
displacement has a fractional component beyond 0.5 are refused.

Halt protocol, `resume()`, `PARKED`: `DeviceRelax`'s (a void step returns the coordinates, leaves velocities and band state).

Out of scope: wrapping and minimum-image tangents, ASE's `aseneb` / `eb` / `spline` methods, IDPP interpolation, variable
springs, atom shards, HTNet, bands whose cell varies."""
import numpy as np
import torch

from . import _lib
from ._resident import host_f64, per_graph
from .relax import DeviceRelax


def interpolate(first, last, n_images):
    """Linear interpolation in float64: [n_images, n, 3] from `first` to `last` inclusive ([n,3] arrays, or anything with
    `positions`)."""
    a, b = (host_f64(getattr(p, "positions", p)).reshape(-1, 3) for p in (first, last))
    if a.shape != b.shape or int(n_images) < 2:
        raise ValueError("neb.interpolate: two end points of one shape, n_images >= 2")
    t = np.arange(int(n_images), dtype=np.float64) / (int(n_images) - 1)
    return a[None] + t[:, None, None] * (b - a)[None]


class DeviceNEB(DeviceRelax):
    """See the module docstring.  model, atomic_number [N], pos [N,3], `batch` [N] with `num_graphs` = B, `fixed` [N],
    `dt`, `dtmax`, `maxstep`, `capacity`, `log_steps`, `reference_compat`: `DeviceRelax`'s; the B graphs are the images.
    `cell` [B,3,3], or None for open structures.  `band_ptr` [K+1] splits the images into K bands (default: one band); a band
    has 3 images or more, all of one atom count and one `atomic_number`; bands may differ in both.  A band's first and last
    image are its end points: they are evaluated with the rest (the tangents need their energies) and never move.  `k`
    (spring constant, eV/A^2) and `fmax` (eV/A, on the largest NEB force of the band's interior images): scalars or [K].
    `climb`: the interior image of largest energy in an evaluation (ties: the lowest index) climbs -- its force along the
    tangent is reversed and it feels no spring.  There is no `wrap` argument: coordinates are never wrapped.  A band whose
    largest NEB force is below its `fmax` converges and freezes while the others go on.

    ValueError, naming the band: fewer than 3 images, images that differ in atom count or atomic numbers, periodic
    neighbouring images whose displacement has a fractional component beyond 0.5 (not continuous across a cell face).

    `fetch()`: the base's snapshot (`forces`: the model's, as accepted; `velocities`: FIRE's), `done`; per band [K]
    `converged`, `converged_step`, `fmax` (the largest |g_a| of the band's last evaluation while it moved), `dt`, `a`,
    `scale`, `nsteps`, `climbing_image` (index within the band, -1: none); per image [B] `energy`, `image_fmax`, `segment`
    (|x_(i+1) - x_i|) and `tangential_force` (F.tau; the three are 0 on end points); `log` [rows,B,4] = (E_pot, the image's
    max |g_a|, the band's dt, edges found) per evaluation."""

    __slots__ = ("k", "climb", "band_ptr", "band_of", "num_bands", "_band_ptr_h", "obs", "climber", "climber_new", "g", "isum",
                 "csum")
    LOG_WIDTH = 4

    def __init__(self, model, atomic_number, cell, pos, batch=None, num_graphs=None, band_ptr=None, k=0.1, climb=True, fmax=0.05,
                 fixed=None, dt=0.1, dtmax=1.0, maxstep=0.2, capacity=None, log_steps=4096, reference_compat=False, device=None):
        self.dt, self.dtmax, self.maxstep = float(dt), float(dtmax), float(maxstep)
        if not (self.dt > 0.0 and self.dtmax > 0.0 and self.maxstep > 0.0) or int(log_steps) < 1:
            raise ValueError("DeviceNEB: dt, dtmax, maxstep > 0 and log_steps >= 1")
        if batch is None:
            raise ValueError("DeviceNEB: batch= and num_graphs= are required (the graphs of the batch are the images)")
        self.climb = bool(climb)          # a climbing image per band
        self._start(model, atomic_number, cell, pos, batch, num_graphs, capacity, log_steps, False, reference_compat, device,
                    fmax=fmax, fixed=fixed, k=k, band_ptr=band_ptr, cell_given=cell)
        self._unpark()

    def _bands(self, band_ptr, cell_given):
        """`band_ptr` on the host, checked against the images (the class docstring's refusals)."""
        B, ptr = self.num_graphs, np.searchsorted(self._batch_h, np.arange(self.num_graphs + 1))
        bp = np.array([0, B], dtype=np.int64) if band_ptr is None else np.asarray(torch.as_tensor(band_ptr).cpu(), dtype=np.int64)
        if bp.ndim != 1 or len(bp) < 2 or bp[0] != 0 or bp[-1] != B or np.any(np.diff(bp) < 0):
            raise ValueError("DeviceNEB: band_ptr must be [K+1], non-decreasing, from 0 to num_graphs")
        z, x = self.z.cpu().numpy(), self.x.cpu().numpy()
        cells = None if cell_given is None else host_f64(torch.as_tensor(cell_given).detach().float()).reshape(B, 3, 3)
        for k, count in enumerate(np.diff(bp)):
            if count < 3:
                raise ValueError("DeviceNEB: band %d has %d images -- a band is two end points and one image or more between "
                                 "them" % (k, count))
        for k, (lo, hi) in enumerate(zip(bp[:-1], bp[1:])):
            first = z[ptr[lo]:ptr[lo + 1]]
            for g in range(lo + 1, hi):
                mine = z[ptr[g]:ptr[g + 1]]
                if len(mine) != len(first) or np.any(mine != first):
                    raise ValueError("DeviceNEB: band %d: image %d differs from image %d in atom count or atomic numbers"
                                     % (k, g - lo, 0))
                if cells is not None:
                    d = x[ptr[g]:ptr[g + 1]] - x[ptr[g - 1]:ptr[g]]
                    if len(d) and np.abs(d @ np.linalg.inv(cells[g - 1])).max() > 0.5:
                        raise ValueError("DeviceNEB: band %d: images %d and %d are not continuous across a cell face (a "
                                         "fractional displacement beyond 0.5) -- unwrap the band; the driver never wraps"
                                         % (k, g - lo - 1, g - lo))
        return bp

    def _own_state(self, fmax, fixed, k, band_ptr, cell_given):
        bp = self._bands(band_ptr, cell_given)
        B, K, dev, n = self.num_graphs, len(bp) - 1, self.device, self.n
        fm, kk = per_graph(fmax, K), per_graph(k, K)
        if not np.all(fm > 0.0) or not (np.all(kk >= 0.0) and np.all(np.isfinite(kk))):
            raise ValueError("DeviceNEB: fmax must be positive, k finite and not negative")
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.num_bands, self._band_ptr_h = K, bp                    # bands; band_ptr on the host
        self.band_ptr = put(bp.astype(np.int32))                    # [K+1] int32
        self.band_of = put(np.repeat(np.arange(K), np.diff(bp)).astype(np.int32))     # [B] int32: the band of an image
        self.fmax, self._fmax0, self.k = put(fm), None, put(kk)     # thresholds and spring constants [K] f64
        self.x0.copy_(self.x)             # end points are never backed up: their x0 is this copy for good
        self.fixed = None                 # [N] uint8, 1 where the atom is held; None: no atom is
        if fixed is not None:
            self.fixed = put((host_f64(fixed).reshape(n) != 0).astype(np.uint8))
        # per image relax_step.h's rows: an interior image's is its band's FIRE state (the first interior image's is read);
        # an end point's says converged, scale 0 from the start, and is never written: advance leaves it alone
        gf = np.zeros((B, 5))
        gf[:, 0], gf[:, 1], gf[:, 3] = self.dt, 0.1, np.inf
        gi = np.zeros((B, 4), dtype=np.int64)
        gi[:, 1], gi[:, 3] = 1, -1
        ends = np.concatenate([bp[:-1], bp[1:] - 1])
        gi[ends, 1], gi[ends, 2] = 0, 1
        self.gf, self.gi = put(gf), put(gi)                                              # finish's last kernel
        self.gf_new = torch.zeros(K, 5, dtype=torch.float64, device=dev)                 # the band's new state (scratch);
        self.gi_new = torch.zeros(K, 4, dtype=torch.int64, device=dev)                   # finish's second kernel
        self.climber_new = torch.full((K,), -1, dtype=torch.int64, device=dev)
        self.climber = torch.full((K,), -1, dtype=torch.int64, device=dev)               # finish's last kernel
        self.obs = torch.zeros(B, 4, dtype=torch.float64, device=dev)    # (energy, max |g_a|, |t2|, ft); finish's first kernel
        self.g = torch.zeros(n, 3, dtype=torch.float64, device=dev)      # the NEB force (scratch); finish's first kernel
        self.isum = torch.zeros(B, 4, dtype=torch.float64, device=dev)   # an image's partial sums (scratch); first kernel
        self.csum = torch.zeros(B, dtype=torch.float64, device=dev)      # an image's clamp sum (scratch); second kernel

    # ---- the finish hook (the advance is DeviceRelax's, which never wraps here: `wrap` is False) ----------------------------------
    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        _lib.call("hermnet_neb_finish", self.n, self.num_graphs, self.num_bands, int(self.climb), P(self.graph_ptr),
                  P(self.band_ptr), P(self.band_of), P(forces), P(energy), P(total), int(step.capacity), self.dt, self.dtmax,
                  self.maxstep, P(self.k), P(self.fmax), P(self.x), P(self.v), P(self.x0), P(self.image), P(self.image0),
                  P(self.f_prev), P(self.fixed), P(step.pos), P(self.gf), P(self.gi), P(self.obs), P(self.climber), P(self.g),
                  P(self.isum), P(self.csum), P(self.gf_new), P(self.gi_new), P(self.climber_new), P(self.log), self.log_steps,
                  P(self.state), torch.cuda.current_stream(self.device).cuda_stream)

    # ---- the packed fetch's own part ------------------------------------------------------------------------------------------
    def _fetch_extras(self):
        return [self.gf, self.gi, self.obs, self.climber]

    def _read_extras(self, s, word, h):
        B, K = self.num_graphs, self.num_bands
        gf, gi = h[:5 * B].reshape(B, 5), h[5 * B:9 * B].reshape(B, 4).astype(np.int64)
        obs = h[9 * B:13 * B].reshape(B, 4)
        lead = self._band_ptr_h[:-1] + 1                            # the image that carries its band's state
        s.done = bool(word)
        s.dt, s.a, s.scale, s.fmax = (gf[lead, c].copy() for c in range(4))
        s.nsteps, s.converged, s.converged_step = gi[lead, 0].copy(), gi[lead, 2] != 0, gi[lead, 3].copy()
        s.climbing_image = h[13 * B:13 * B + K].astype(np.int64)
        s.energy, s.image_fmax, s.segment, s.tangential_force = (obs[:, c].copy() for c in range(4))

    # ---- ASE hand-off (duck-typed) ------------------------------------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, images, model, device="cuda:0", **kw):
        """`images`: the list of one band's images, end points included (or of several bands', with `band_ptr=`): anything
        with `positions`, `numbers`, `cell`, `pbc`; all periodic in three directions, or all open."""
        if not isinstance(images, (list, tuple)):
            raise ValueError("DeviceNEB.from_atoms: a list of images")
        return super().from_atoms(images, model, device=device, **kw)
