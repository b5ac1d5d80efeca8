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

`DeviceCellRelax` is `DeviceRelax` on atoms AND cell (its class docstring): ASE's UnitCellFilter under the same FIRE, the
captured step carries the virial kernels and `hermnet_cellrelax_advance` writes the cell the search reads.

Out of scope: atom shards, HTNet, constraints other than `fixed` atoms, optimisers other than FIRE; for the cell: separate
thresholds for forces and stress, ASE's ExpCellFilter / FrechetCellFilter."""
import numpy as np
import torch

from . import _lib
from ._resident import HN_MD_WRAP, ResidentDriver, host_f64, per_graph
from .md import _det3, _inverse3


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
    OPEN_REFUSED = None       # from_atoms: the message that refuses a structure not periodic in all three directions, if any
    CELLS_FLOAT64 = False     # from_atoms: the cells go on as float64 on the host; else as the step's float32, on the device

    @classmethod
    def from_atoms(cls, atoms, model, device="cuda:0", **kw):
        """`atoms`: one structure or a list of them (one batch), anything with `positions`, `numbers`, `cell`, `pbc`.  The
        members of a list are all periodic (pbc in all three directions) or all open (`DeviceCellRelax`: all periodic, and
        their cells are kept in float64)."""
        dev = torch.device(device)
        ms = _members(atoms)
        periodic = [bool(np.all(np.asarray(m.pbc))) for m in ms]
        if cls.OPEN_REFUSED and not all(periodic):
            raise RuntimeError(cls.OPEN_REFUSED)
        if len(set(periodic)) != 1 or (not periodic[0] and any(np.any(np.asarray(m.pbc)) for m in ms)):
            raise RuntimeError("DeviceRelax.from_atoms: structures that are all periodic in three directions, or all open")
        pos = np.concatenate([np.asarray(m.positions, dtype=np.float64).reshape(-1, 3) for m in ms])
        z = torch.as_tensor(np.concatenate([np.asarray(m.numbers).reshape(-1) for m in ms])).to(dev)
        cells = np.stack([np.asarray(m.cell, dtype=np.float64).reshape(3, 3) for m in ms]) if periodic[0] else None
        if cells is not None and not cls.CELLS_FLOAT64:
            cells = torch.from_numpy(cells).float().to(dev)
        if not isinstance(atoms, (list, tuple)):
            if cells is None:
                raise RuntimeError("DeviceRelax.from_atoms: one structure must be periodic (open structures: a list)")
            return cls(model, z, cells[0], pos, device=dev, **kw)
        batch = torch.from_numpy(np.repeat(np.arange(len(ms)), [len(m.positions) for m in ms])).to(dev)
        return cls(model, z, cells, pos, batch=batch, num_graphs=len(ms), device=dev, **kw)

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


def _mask9(mask):
    """`mask` (None, 3x3 or Voigt 6: xx, yy, zz, yz, xz, xy) as the nine entry-wise factors, float64 on the host."""
    if mask is None:
        return np.ones(9)
    m = host_f64(mask)
    if m.shape == (6,):
        m = np.array([[m[0], m[5], m[4]], [m[5], m[1], m[3]], [m[4], m[3], m[2]]])
    if m.shape != (3, 3) or not np.all(np.isfinite(m)):
        raise ValueError("DeviceCellRelax: mask is 3x3 or Voigt 6, with finite entries")
    return np.ascontiguousarray(m.reshape(9))


class DeviceCellRelax(DeviceRelax):
    """`DeviceRelax` that relaxes the CELL with the atoms: ASE's `UnitCellFilter` under ASE's FIRE inside the replayed step,
    for one structure or a batch, each structure with its own cell and converging on its own.  One replay is one force-and-
    stress evaluation followed by one FIRE step on the n + 3 generalised rows of every graph (csrc/cellrelax_step.h is the
    definition): with C0 the cell given (float64) and F the deformation gradient (I at the start), the cell is C = C0 F^T,
    the coordinates q_i = x_i F^-T and the three rows `cell_factor` F; the forces f_i F and proj(S F^-T) / `cell_factor`
    with S = sym(W) - p V I from the step's own virial W.  `cell` is required (float64 is kept); `mask` (3x3 or Voigt 6,
    default all ones) multiplies the cell's force entry-wise, `hydrostatic_strain` keeps F a multiple of I,
    `constant_volume` removes the trace, `scalar_pressure` p (eV/A^3, a scalar or [B]) makes the objective the enthalpy E +
    p V, `cell_factor` (a scalar or [B]) defaults to each graph's atom count (1 for an empty graph).  `fmax` is ASE's single
    threshold on the largest generalised force, `maxstep` bounds the whole generalised move.  Everything else is
    `DeviceRelax`'s; `fixed` atoms keep q, so they ride the cell affinely.

    Float64 is the truth: the step's float32 cell and coordinates are roundings of C and x, as in `DeviceNPT`.  The cell
    moves BEFORE the evaluation, so a void step takes it back with the atoms; a step is also void (halt code 256) on a
    virial that is not finite or det F <= 0.  A converged graph is never written again, its cell included.

    `fetch()`: `DeviceRelax`'s, where `energy` [B] is the enthalpy, `fmax` [B] the largest generalised force, `velocities`
    those of q; and `cell` [B,3,3] float64, `deform_grad` [B,3,3], `volume` [B], `stress` [B,3,3] (-sym(W) / V of the
    graph's last evaluation while it moved), `cell_velocity` [B,3,3]; `log` [rows,B,6] = (enthalpy, max generalised force,
    dt, edges found, volume, pressure tr W / 3V) per evaluation."""

    __slots__ = ("scalar_pressure", "cell_factor", "flags", "_mask_h", "_cell_given", "q", "q0", "cell0", "rows", "rows0",
                 "rows_v", "deform", "deform_inv", "det_f", "cell64", "obs", "p0", "cf")
    LOG_WIDTH = 6

    def __init__(self, model, atomic_number, cell, pos, mask=None, hydrostatic_strain=False, constant_volume=False,
                 scalar_pressure=0.0, cell_factor=None, **kw):
        if cell is None:
            raise RuntimeError("DeviceCellRelax: periodic cells are required (cell=None, open structures, have no cell to relax)")
        self._mask_h = _mask9(mask)                       # the nine factors on the host: the entry points read them at the call
        self.flags = ((_lib.HN_CELLRELAX_HYDROSTATIC if hydrostatic_strain else 0)
                      | (_lib.HN_CELLRELAX_CONSTANT_VOLUME if constant_volume else 0))
        self.scalar_pressure, self.cell_factor = scalar_pressure, cell_factor     # as given
        self._cell_given = cell                           # `_own_state` makes cell0 of it
        super().__init__(model, atomic_number, cell, pos, **kw)

    def _own_state(self, fmax, fixed):
        super()._own_state(fmax, fixed)
        B, dev = self.num_graphs, self.device
        cell = host_f64(self._cell_given).reshape(B, 3, 3).copy()
        self._cell_given = None
        if not (np.all(np.isfinite(cell)) and np.all(_det3(cell) != 0.0)):
            raise ValueError("DeviceCellRelax: cells must be finite and not singular")
        count = np.bincount(self._batch_h, minlength=B).astype(np.float64)
        cf = np.maximum(count, 1.0) if self.cell_factor is None else per_graph(self.cell_factor, B)
        if not (np.all(cf > 0.0) and np.all(np.isfinite(cf))):
            raise ValueError("DeviceCellRelax: cell_factor must be positive")
        p0 = per_graph(self.scalar_pressure, B)
        eye = np.tile(np.eye(3), (B, 1, 1))
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        self.q, self.q0 = self.x.clone(), self.x.clone()  # q = x F^-T [N,3] f64 (F = I): the state; advance, void finish
        self.cell0 = put(cell)                            # C0 [B,3,3] f64: constant
        self.inv_cell = put(_inverse3(cell))              # its inverse (adjugate over determinant): what q is wrapped with
        self.cf, self.p0 = put(cf), put(p0)               # cell_factor, pressure [B]
        self.rows = put(cf[:, None, None] * eye)          # G = cell_factor F [B,3,3]; advance, void finish
        self.rows0 = self.rows.clone()                    # G at the start of the step; advance
        self.rows_v = torch.zeros_like(self.rows)         # the rows' velocities; finish
        self.deform, self.deform_inv = put(eye), put(eye)  # F, F^-1; advance, void finish
        self.det_f = torch.ones(B, dtype=torch.float64, device=dev)      # det F of the last advance; advance
        self.cell64 = put(cell)                           # C = C0 F^T: the truth; advance, void finish
        self.obs = torch.zeros(B, 11, dtype=torch.float64, device=dev)   # (V, tr W / 3V, stress [9]); finish

    def _step_options(self, single):
        return dict(stress=True, variable_cell=True) if single else dict(stress=True)

    def _inverse_of(self, cell):
        return self.inv_cell              # device state: the constant inverse of C0 (q is wrapped in the reference frame)

    def _cell_input(self, step):
        """The step's float32 cell tensor, checked: advance writes it."""
        cell = step.cell
        if cell is None or cell.dtype != torch.float32 or not cell.is_contiguous() or cell.numel() != 9 * self.num_graphs:
            raise RuntimeError("DeviceCellRelax: the step's cell must be a contiguous float32 [B,3,3]")
        return cell

    # ---- the two hooks of the capture ---------------------------------------------------------------------------------------
    def _advance(self, step):
        P = _lib.ptr
        _lib.call("hermnet_cellrelax_advance", self.n, self.num_graphs, HN_MD_WRAP if self.wrap else 0, P(self.q), P(self.q0),
                  P(self.x), P(self.x0), P(self.v), P(self.image), P(self.image0), P(self.fixed), P(self.batch), P(self.cell0),
                  P(self.inv_cell), P(self.cf), P(self.rows), P(self.rows0), P(self.rows_v), P(self.deform), P(self.deform_inv),
                  P(self.det_f), P(self.cell64), P(self._cell_input(step)), P(self._pos_input(step)), P(self.state), P(self.gf),
                  P(self.gi), torch.cuda.current_stream(self.device).cuda_stream)

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        virial, B = out[2], self.num_graphs
        if virial.dtype != torch.float32 or not virial.is_contiguous() or virial.numel() != 9 * B:
            raise RuntimeError("DeviceCellRelax: the captured step must return a contiguous float32 virial [B,3,3]")
        _lib.call("hermnet_cellrelax_finish", self.n, B, self.flags, P(self.graph_ptr), P(forces), P(energy), P(virial),
                  P(total), int(step.capacity), self.dt, self.dtmax, self.maxstep, self._fmax0, P(self.fmax), P(self.p0),
                  self._mask_h.ctypes.data, P(self.cell0), P(self.inv_cell), P(self.cf), P(self.q), P(self.q0), P(self.x),
                  P(self.x0), P(self.v), P(self.image), P(self.image0), P(self.f_prev), P(self.fixed), P(step.pos), P(self.rows),
                  P(self.rows0), P(self.rows_v), P(self.deform), P(self.deform_inv), P(self.det_f), P(self.cell64),
                  P(self._cell_input(step)), P(self.obs), P(self.gf), P(self.gi), P(self.gf_new), P(self.gi_new), P(self.log),
                  self.log_steps, P(self.state), torch.cuda.current_stream(self.device).cuda_stream)

    # ---- the packed fetch's own part ------------------------------------------------------------------------------------------
    def _fetch_extras(self):
        return super()._fetch_extras() + [self.cell64, self.deform, self.rows_v, self.obs]

    def _read_extras(self, s, word, h):
        B = self.num_graphs
        super()._read_extras(s, word, h[:9 * B])
        m = h[9 * B:]
        s.cell, s.deform_grad, s.cell_velocity = (m[9 * B * k:9 * B * (k + 1)].reshape(B, 3, 3).copy() for k in range(3))
        obs = m[27 * B:].reshape(B, 11)
        s.stress = obs[:, 2:].reshape(B, 3, 3).copy()
        s.volume = np.abs(_det3(s.cell))

    # ---- ASE hand-off: DeviceRelax.from_atoms, with these two rules ------------------------------------------------------------
    OPEN_REFUSED = ("DeviceCellRelax.from_atoms: periodic structures (pbc in all three directions): an open structure has no "
                    "cell to relax")
    CELLS_FLOAT64 = True                  # `_own_state` makes cell0 of them

    def to_atoms(self, atoms, snapshot=None):
        """`DeviceRelax.to_atoms`, and each member's cell -- written first and without moving the atoms: the positions are
        already those of the relaxed cell.  One structure, or the list the batch was made of."""
        s = snapshot if snapshot is not None else self.fetch()
        ms = _members(atoms)
        if len(ms) != self.num_graphs:
            raise ValueError("DeviceCellRelax.to_atoms: the structures do not match the batch")
        for g, m in enumerate(ms):
            if hasattr(m, "set_cell"):
                m.set_cell(s.cell[g].copy(), scale_atoms=False)
            else:
                m.cell = s.cell[g].copy()
        return super().to_atoms(atoms, s)
