"""Device-resident relaxation: FIRE for a batch of structures INSIDE the replayed hipGraph, each structure converging on
its own.

A host-driven relaxation is `GraphedMDStep(pos)`, `fetch()`, an optimiser step on the host -- per force evaluation, a round
trip of the order of the device step itself for cells of 100-1000 atoms; and a batch of structures has no driver at all
(an optimiser that takes one structure relaxes a batch one at a time, or in lock-step until the slowest has converged).
`DeviceRelax` puts two small entry points around the captured step (csrc/relax_kernels.hip: `hermnet_relax_advance` in
front of the search, `hermnet_relax_finish` behind the force backward), so that one replay IS one force evaluation of the
optimiser for every structure of the batch:

    rx = DeviceRelax(model, z, cells, pos, batch=batch, num_graphs=B, fmax=0.05)
    rx.run(50)                  # 50 replays enqueued; returns at once: no synchronisation, no upload, no download
    s = rx.fetch()              # ONE packed device-to-host copy + one synchronisation: s.converged [B], s.positions, ...
    s = rx.run_until(500)       # ... or: chunks of replays until every structure has converged

The optimiser is ASE's FIRE with ASE's defaults (dt 0.1, dtmax 1.0, maxstep 0.2 A, Nmin 5, finc 1.1, fdec 0.5, astart 0.1,
fa 0.99, fmax 0.05 eV/A), applied to every graph independently: a graph whose largest force falls below its `fmax` freezes
-- its coordinates are never written again -- while the others keep going; once all have converged the replays change
nothing.  Coordinates and velocities are float64 on the device, the model's float32 input is the rounding of x.  The
per-graph sums that steer the trajectory (F.v, |F|^2, |v|^2, max |F_i|^2) are taken in one documented order without atomics
(csrc/resident_step.h), so the device, the library's host twins and a numpy transcription agree bit for bit
(tests/test_relax_host.py, tests/test_relax_device.py).

Halt protocol: the resident drivers' (`_resident.ResidentDriver`, csrc/resident_step.h).  A step whose neighbour list is
incomplete or whose energy is not finite is VOID: coordinates and images return to the start of the step, velocities and
the optimiser's state stay, the halt is recorded, no log row is written and later replays change nothing.  `resume()`
recaptures (with a larger capacity where the list overflowed) and clears the halt; the next replay repeats the void move.

Out of scope: cell relaxation, atom shards, HTNet, constraints other than `fixed` atoms, optimisers other than FIRE."""
import numpy as np
import torch

from . import _lib
from ._resident import HN_MD_WRAP, ResidentDriver, host_f64, per_graph


def _members(atoms):
    return list(atoms) if isinstance(atoms, (list, tuple)) else [atoms]


class DeviceRelax(ResidentDriver):
    """See the module docstring.  model: HVNet in eval(), parameters not requiring grad, on the GPU.  atomic_number [N],
    cell [3,3] (`batch` None) or [B,3,3] (None: a batch of open structures), pos [N,3].  `fixed` [N] bool: atoms that are
    held -- they count as f = 0 in the convergence test and in FIRE's sums, and never move.  `batch` [N] int64
    non-decreasing with `num_graphs`: a batch of structures (`GraphedBatchMDStep`).  `fmax` (eV/A): a scalar or [B].  `dt`,
    `dtmax`, `maxstep`: FIRE's start and largest time step and the longest move of a structure per evaluation (A).
    `capacity`, `reference_compat`: as for the graphed steps.  `log_steps`: rows of the log ring -- `run` refuses to
    overwrite rows not fetched yet.  `wrap`: coordinates are wrapped into the cell as they move, `images` counts the lattice
    vectors removed.  The coordinates given are those of the first force evaluation.

    `fetch()`: the base's snapshot (`step`: evaluations completed; `velocities`: FIRE's), `done` (every graph has
    converged), per graph `converged` [B] bool, `converged_step` [B] (the evaluation's index, -1: not yet), `fmax` [B] (max
    |f_i| of the graph's last evaluation while it moved; inf before the first), `energy` [B] and the optimiser state `dt`,
    `a`, `scale`, `nsteps` [B]; `log` [rows,B,4] = (E_pot, max |f_i|, dt, edges found) per evaluation.
    `resume()`: a void step leaves velocities and optimiser state alone, so the next replay repeats the move it had made."""

    __slots__ = ("dt", "dtmax", "maxstep", "fmax", "_fmax0", "fixed", "gf", "gi", "gf_new", "gi_new")
    LOG_WIDTH = 4

    def __init__(self, model, atomic_number, cell, pos, fixed=None, batch=None, num_graphs=None, fmax=0.05, dt=0.1, dtmax=1.0,
                 maxstep=0.2, capacity=None, log_steps=4096, wrap=True, reference_compat=False, device=None):
        self.dt, self.dtmax, self.maxstep = float(dt), float(dtmax), float(maxstep)      # FIRE's start / largest dt, longest move
        if not (self.dt > 0.0 and self.dtmax > 0.0 and self.maxstep > 0.0) or int(log_steps) < 1:
            raise ValueError("DeviceRelax: dt, dtmax, maxstep > 0 and log_steps >= 1")
        self._start(model, atomic_number, cell, pos, batch, num_graphs, capacity, log_steps, wrap, reference_compat, device,
                    fmax=fmax, fixed=fixed)
        self._unpark()

    def _own_state(self, fmax, fixed):
        B, dev = self.num_graphs, self.device
        fm = per_graph(fmax, B)
        if not np.all(fm > 0.0):
            raise ValueError("DeviceRelax: fmax must be positive")
        self.fmax, self._fmax0 = torch.from_numpy(fm).to(dev), float(fm[0])     # the thresholds [B] f64, and the first on the host
        self.x0.copy_(self.x)             # (the first advance backs x up anyway)
        self.fixed = None                 # [N] uint8, 1 where the atom is held; None: no atom is
        if fixed is not None:
            self.fixed = torch.from_numpy((host_f64(fixed).reshape(self.n) != 0).astype(np.uint8)).to(dev)
        # per-graph state: (dt, a, scale, fnorm, energy) and (nsteps, fresh, converged, conv_step); scale 0 and fresh 1: the
        # first replay evaluates the start coordinates and starts FIRE from v = 0
        gf = np.zeros((B, 5))
        gf[:, 0], gf[:, 1], gf[:, 3] = self.dt, 0.1, np.inf
        gi = np.zeros((B, 4), dtype=np.int64)
        gi[:, 1], gi[:, 3] = 1, -1
        self.gf, self.gi = torch.from_numpy(gf).to(dev), torch.from_numpy(gi).to(dev)    # finish's last kernel
        self.gf_new, self.gi_new = self.gf.clone(), self.gi.clone()                      # finish's per-graph kernel (scratch)

    # ---- the two hooks of the capture ---------------------------------------------------------------------------------------
    def _advance(self, step):
        P = _lib.ptr
        wrap, cell, inv = self._cell_args(step)
        _lib.call("hermnet_relax_advance", self.n, self.num_graphs, HN_MD_WRAP if wrap else 0, P(self.x), P(self.x0), P(self.v),
                  P(self.image), P(self.image0), P(self.fixed), P(self.batch), cell, inv, P(self._pos_input(step)),
                  P(self.state), P(self.gf), P(self.gi), torch.cuda.current_stream(self.device).cuda_stream)

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        _lib.call("hermnet_relax_finish", self.n, self.num_graphs, P(self.graph_ptr), P(forces), P(energy), P(total),
                  int(step.capacity), self.dt, self.dtmax, self.maxstep, self._fmax0, P(self.fmax), P(self.x), P(self.v),
                  P(self.x0), P(self.image), P(self.image0), P(self.f_prev), P(self.fixed), P(step.pos), P(self.gf), P(self.gi),
                  P(self.gf_new), P(self.gi_new), P(self.log), self.log_steps, P(self.state),
                  torch.cuda.current_stream(self.device).cuda_stream)

    def _unpark(self):
        """Parked while the capture was made: nothing has moved, so the halt words are cleared and that is all."""
        self.state[1:3].zero_()

    # ---- the packed fetch's own part ------------------------------------------------------------------------------------------
    def _fetch_extras(self):
        return [self.gf, self.gi]

    def _read_extras(self, s, word, h):
        B = self.num_graphs
        gf, gi = h[:5 * B].reshape(B, 5), h[5 * B:].reshape(B, 4).astype(np.int64)
        s.done = bool(word)
        s.dt, s.a, s.scale, s.fmax, s.energy = (gf[:, k].copy() for k in range(5))
        s.nsteps, s.converged, s.converged_step = gi[:, 0].copy(), gi[:, 2] != 0, gi[:, 3].copy()

    # ---- running --------------------------------------------------------------------------------------------------------------
    def run_until(self, max_steps, chunk=32):
        """`run(chunk)` and `fetch()` until every graph has converged, a halt, or `max_steps` evaluations in all; returns the
        last snapshot (`done`, `halted` and `step` say which)."""
        chunk = max(1, min(int(chunk), self.log_steps))
        s = self.fetch()
        while not (s.done or s.halted) and s.step < max_steps:
            self.run(min(chunk, max_steps - s.step))
            s = self.fetch()
        return s

    # ---- ASE hand-off (duck-typed: ASE itself is not needed) --------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, atoms, model, device="cuda:0", **kw):
        """`atoms`: one structure or a list of them (one batch), anything with `positions`, `numbers`, `cell`, `pbc`.  The
        members of a list are all periodic (pbc in all three directions) or all open."""
        dev = torch.device(device)
        ms = _members(atoms)
        periodic = [bool(np.all(np.asarray(m.pbc))) for m in ms]
        if len(set(periodic)) != 1 or (not periodic[0] and any(np.any(np.asarray(m.pbc)) for m in ms)):
            raise RuntimeError("DeviceRelax.from_atoms: structures that are all periodic in three directions, or all open")
        pos = np.concatenate([np.asarray(m.positions, dtype=np.float64).reshape(-1, 3) for m in ms])
        z = torch.as_tensor(np.concatenate([np.asarray(m.numbers).reshape(-1) for m in ms])).to(dev)
        cells = np.stack([np.asarray(m.cell, dtype=np.float64).reshape(3, 3) for m in ms]) if periodic[0] else None
        if not isinstance(atoms, (list, tuple)):
            if cells is None:
                raise RuntimeError("DeviceRelax.from_atoms: one structure must be periodic (open structures: a list)")
            return cls(model, z, torch.from_numpy(cells[0]).float().to(dev), pos, device=dev, **kw)
        batch = torch.from_numpy(np.repeat(np.arange(len(ms)), [len(m.positions) for m in ms])).to(dev)
        cell = None if cells is None else torch.from_numpy(cells).float().to(dev)
        return cls(model, z, cell, pos, batch=batch, num_graphs=len(ms), device=dev, **kw)

    def to_atoms(self, atoms, snapshot=None):
        """Write the positions (wrapped) of `snapshot` (default: a fetch()) into `atoms` (one structure, or the list the
        batch was made of); returns the snapshot."""
        s = snapshot if snapshot is not None else self.fetch()
        ms = _members(atoms)
        ptr = np.searchsorted(self._batch_h, np.arange(self.num_graphs + 1))
        if len(ms) != self.num_graphs or any(len(m.positions) != b - a for m, a, b in zip(ms, ptr[:-1], ptr[1:])):
            raise ValueError("DeviceRelax.to_atoms: the structures do not match the batch")
        for m, a, b in zip(ms, ptr[:-1], ptr[1:]):
            m.positions = s.positions[a:b].copy()
        return s
