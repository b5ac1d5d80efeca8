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
(csrc/relax_step.h), so the device, the library's host twins and a numpy transcription agree bit for bit
(tests/test_relax_host.py, tests/test_relax_device.py).

Halt protocol: `DeviceMD`'s.  A step whose neighbour list is incomplete or whose energy is not finite is VOID: coordinates
and images return to the start of the step, velocities and the optimiser's state stay, the halt is recorded, no log row is
written and later replays change nothing.  `resume()` recaptures (with a larger capacity where the list overflowed) and
clears the halt; the next replay repeats the void move.

Out of scope: cell relaxation, atom shards, HTNet, constraints other than `fixed` atoms, optimisers other than FIRE."""
import types

import numpy as np
import torch

from . import _lib
from ._resident import PARKED, after_halt, cell_args, f64, fetch_packed

HN_MD_WRAP = 2                            # include/hermnet_hip.h


def _members(atoms):
    return list(atoms) if isinstance(atoms, (list, tuple)) else [atoms]


class DeviceRelax(object):
    """See the module docstring.  model: HVNet in eval(), parameters not requiring grad, on the GPU.  atomic_number [N],
    cell [3,3] (`batch` None) or [B,3,3] (None: a batch of open structures), pos [N,3].  `fixed` [N] bool: atoms that are
    held -- they count as f = 0 in the convergence test and in FIRE's sums, and never move.  `batch` [N] int64
    non-decreasing with `num_graphs`: a batch of structures (`GraphedBatchMDStep`).  `fmax` (eV/A): a scalar or [B].  `dt`,
    `dtmax`, `maxstep`: FIRE's start and largest time step and the longest move of a structure per evaluation (A).
    `capacity`, `reference_compat`: as for the graphed steps.  `log_steps`: rows of the log ring -- `run` refuses to
    overwrite rows not fetched yet.  `wrap`: coordinates are wrapped into the cell as they move, `images` counts the lattice
    vectors removed.  The coordinates given are those of the first force evaluation."""

    def __init__(self, model, atomic_number, cell, pos, fixed=None, batch=None, num_graphs=None, fmax=0.05, dt=0.1, dtmax=1.0,
                 maxstep=0.2, capacity=None, log_steps=4096, wrap=True, reference_compat=False, device=None):
        from .graph import GraphedBatchMDStep, GraphedMDStep
        dev = torch.device(device) if device is not None else (pos.device if torch.is_tensor(pos) else torch.device("cuda:0"))
        if dev.type != "cuda":
            raise RuntimeError("DeviceRelax needs GPU tensors")
        self.device, self.model = dev, model
        self.lib = _lib.load()
        self.dt, self.dtmax, self.maxstep, self.log_steps = float(dt), float(dtmax), float(maxstep), int(log_steps)
        self.wrap, self.inv_cell, self._inv_of = bool(wrap), None, None
        if not (self.dt > 0.0 and self.dtmax > 0.0 and self.maxstep > 0.0) or self.log_steps < 1:
            raise ValueError("DeviceRelax: dt, dtmax, maxstep > 0 and log_steps >= 1")
        self.z = torch.as_tensor(atomic_number).long().to(dev)
        n = self.n = int(self.z.numel())
        self.num_graphs = 1 if batch is None else int(num_graphs if num_graphs is not None else int(torch.as_tensor(batch)[-1]) + 1)
        B = self.num_graphs
        fm = np.asarray(fmax.detach().cpu() if torch.is_tensor(fmax) else fmax, dtype=np.float64)
        fm = np.ascontiguousarray(np.broadcast_to(fm.reshape(-1) if fm.ndim else fm, (B,)))
        if not np.all(fm > 0.0):
            raise ValueError("DeviceRelax: fmax must be positive")
        self.fmax, self._fmax0 = torch.from_numpy(fm.copy()).to(dev), float(fm[0])
        self.x = f64(pos, dev, (n, 3))
        self.x0 = self.x.clone()
        self.v = torch.zeros(n, 3, dtype=torch.float64, device=dev)
        self.image = torch.zeros(n, 3, dtype=torch.int32, device=dev)
        self.image0 = torch.zeros_like(self.image)
        self.f_prev = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        self.fixed = None
        if fixed is not None:
            held = np.asarray(fixed.detach().cpu() if torch.is_tensor(fixed) else fixed).astype(bool).reshape(n)
            self.fixed = torch.from_numpy(held.astype(np.uint8)).to(dev)
        batch_h = np.zeros(n, dtype=np.int64) if batch is None else np.asarray(torch.as_tensor(batch).cpu(), dtype=np.int64)
        if batch_h.shape != (n,) or np.any(np.diff(batch_h) < 0) or (n and (batch_h[0] < 0 or batch_h[-1] >= B)):
            raise ValueError("DeviceRelax: batch must be [N], non-decreasing, in [0, num_graphs)")
        self._batch_h = batch_h
        self.graph_ptr = torch.from_numpy(np.searchsorted(batch_h, np.arange(B + 1)).astype(np.int32)).to(dev)
        # per-graph state: (dt, a, scale, fnorm, energy) and (nsteps, fresh, converged, conv_step); scale 0 and fresh 1: the
        # first replay evaluates the start coordinates and starts FIRE from v = 0
        gf = np.zeros((B, 5))
        gf[:, 0], gf[:, 1], gf[:, 3] = self.dt, 0.1, np.inf
        gi = np.zeros((B, 4), dtype=np.int64)
        gi[:, 1], gi[:, 3] = 1, -1
        self.gf, self.gi = torch.from_numpy(gf).to(dev), torch.from_numpy(gi).to(dev)
        self.gf_new, self.gi_new = self.gf.clone(), self.gi.clone()
        self.log = torch.zeros(self.log_steps, B, 4, dtype=torch.float64, device=dev)
        self.state = torch.tensor([0, PARKED, 0, 0], dtype=torch.int64).to(dev)
        # the captured step: advance -> the graphed step's own _eager() -> finish
        cell_t = None if cell is None else torch.as_tensor(cell).detach().float().to(dev).contiguous()
        hooks = (self._advance, self._finish)
        self.batch = None
        p32 = self.x.float()
        if batch is None:
            if cell_t is None:
                raise RuntimeError("DeviceRelax: one structure needs a periodic cell (open structures: batch=, cell=None)")
            self.step = GraphedMDStep(model, self.z, cell_t.reshape(3, 3), p32, capacity=capacity,
                                      reference_compat=reference_compat, hooks=hooks)
        else:
            self.batch = torch.from_numpy(batch_h).to(dev)
            self.step = GraphedBatchMDStep(model, self.z, cell_t, p32, self.batch, B, capacity=capacity,
                                           reference_compat=reference_compat, hooks=hooks)
        self._logged = self._pending = 0
        self._host = None
        self.state[1:3].zero_()               # parked while the capture was made: nothing has moved

    # ---- the two hooks of the capture ---------------------------------------------------------------------------------------
    def _advance(self, step):
        P = _lib.ptr
        wrap, cell, inv = cell_args(self, step)
        if step.pos.dtype != torch.float32 or not step.pos.is_contiguous() or step.pos.numel() != 3 * self.n:
            raise RuntimeError("DeviceRelax: the step's coordinate input must be a contiguous float32 [N,3]")
        _lib.check(self.lib.hermnet_relax_advance(
            self.n, self.num_graphs, HN_MD_WRAP if wrap else 0, P(self.x), P(self.x0), P(self.v), P(self.image), P(self.image0),
            P(self.fixed), P(self.batch), cell, inv, P(step.pos), P(self.state), P(self.gf), P(self.gi),
            torch.cuda.current_stream(self.device).cuda_stream), "hermnet_relax_advance")

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = out[0], out[1], out[-2]
        if (energy.dtype != torch.float32 or not energy.is_contiguous() or energy.numel() != self.num_graphs
                or forces.dtype != torch.float32 or not forces.is_contiguous() or forces.numel() != 3 * self.n
                or total.dtype != torch.int64 or total.numel() != 2):
            raise RuntimeError("DeviceRelax: unexpected outputs of the captured step")
        _lib.check(self.lib.hermnet_relax_finish(
            self.n, self.num_graphs, P(self.graph_ptr), P(forces), P(energy), P(total), int(step.capacity), self.dt, self.dtmax,
            self.maxstep, self._fmax0, P(self.fmax), P(self.x), P(self.v), P(self.x0), P(self.image), P(self.image0), P(self.f_prev),
            P(self.fixed), P(step.pos), P(self.gf), P(self.gi), P(self.gf_new), P(self.gi_new), P(self.log), self.log_steps,
            P(self.state), torch.cuda.current_stream(self.device).cuda_stream), "hermnet_relax_finish")

    # ---- running --------------------------------------------------------------------------------------------------------------
    @property
    def capacity(self):
        return self.step.capacity

    def stale(self):
        return self.step.stale()

    def run(self, n):
        """Enqueue `n` force evaluations (replays) back to back and return at once: no synchronisation, no copy."""
        n = int(n)
        if n < 0:
            raise ValueError("run(n): n >= 0")
        if self.step.stale():
            raise RuntimeError("DeviceRelax: the model's weight copies were rebuilt after the capture -- resume() recaptures")
        if self._pending + n > self.log_steps:
            raise RuntimeError("DeviceRelax.run(%d) would overwrite log rows not fetched yet (%d pending, log_steps=%d): "
                               "fetch() first" % (n, self._pending, self.log_steps))
        replay = self.step.graph.replay
        for _ in range(n):
            replay()
        self._pending += n

    def fetch(self):
        """Everything a caller wants on the host through ONE packed device-to-host copy and one synchronisation: `step`
        (evaluations completed), `halted`, `halt_code` (list flags in the low bits, 4 = more pairs than capacity, 256 = an
        energy that is not finite), `halt_step`, `done` (every graph has converged), per graph `converged` [B] bool,
        `converged_step` [B] (the evaluation's index, -1: not yet), `fmax` [B] (max |f_i| of the graph's last evaluation
        while it moved; inf before the first) and `energy` [B]; `positions` [N,3] float64 (wrapped), `images` [N,3] int32,
        `velocities` [N,3] float64 (FIRE's), `forces` [N,3] float32, the per-graph optimiser state `dt`, `a`, `scale`,
        `nsteps` [B], and `log` [rows,B,4] float64 = (E_pot, max |f_i|, dt, edges found) of the evaluations completed since
        the last fetch."""
        n, B, rows = self.n, self.num_graphs, self._pending
        idx = (torch.arange(rows, device=self.device) + self._logged) % self.log_steps
        packed = torch.cat([self.state.double(), self.gf.reshape(-1), self.gi.double().reshape(-1), self.x.reshape(-1),
                            self.image.double().reshape(-1), self.v.reshape(-1), self.f_prev.double().reshape(-1),
                            self.log.index_select(0, idx).reshape(-1)])
        h = fetch_packed(self, packed, 4 + 9 * B + 12 * n + self.log_steps * B * 4)
        step, code, halt_step, done = int(h[0]), int(h[1]), int(h[2]), int(h[3])
        rows_done = max(0, min(rows, step - self._logged))
        s = types.SimpleNamespace(step=step, halted=code != 0, halt_code=code, halt_step=halt_step if code else None,
                                  done=bool(done))
        gf, gi = h[4:4 + 5 * B].reshape(B, 5), h[4 + 5 * B:4 + 9 * B].reshape(B, 4).astype(np.int64)
        s.dt, s.a, s.scale, s.fmax, s.energy = (gf[:, k].copy() for k in range(5))
        s.nsteps, s.converged, s.converged_step = gi[:, 0].copy(), gi[:, 2] != 0, gi[:, 3].copy()
        o = 4 + 9 * B
        s.positions = h[o:o + 3 * n].reshape(n, 3).copy()
        s.images = h[o + 3 * n:o + 6 * n].astype(np.int32).reshape(n, 3)
        s.velocities = h[o + 6 * n:o + 9 * n].reshape(n, 3).copy()
        s.forces = h[o + 9 * n:o + 12 * n].astype(np.float32).reshape(n, 3)
        s.log = h[o + 12 * n:].reshape(rows, B, 4)[:rows_done].copy()
        self._logged, self._pending = step, 0
        after_halt(self, code, halt_step)
        return s

    def run_until(self, max_steps, chunk=32):
        """`run(chunk)` and `fetch()` until every graph has converged, a halt, or `max_steps` evaluations in all; returns the
        last snapshot (`done`, `halted` and `step` say which)."""
        chunk = max(1, min(int(chunk), self.log_steps))
        s = self.fetch()
        while not (s.done or s.halted) and s.step < max_steps:
            self.run(min(chunk, max_steps - s.step))
            s = self.fetch()
        return s

    def resume(self):
        """After a halt (or a stale capture): a new capture -- with a larger capacity where the list had outgrown it --,
        halt cleared.  Coordinates, velocities and the optimiser's state are those of the last completed evaluation, so the
        next replay repeats the move the void step had made."""
        self.state[1].fill_(PARKED)               # the capture's warm-up runs and its first replay must not move anything
        self.step.recapture()
        self.state[1:3].zero_()

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
