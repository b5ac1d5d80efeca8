"""Device-resident MD: velocity Verlet (NVE) and Langevin (BAOAB) steps INSIDE the replayed hipGraph.

`graph.GraphedMDStep` / `GraphedBatchMDStep` replay search + relation build + forward + force backward as one launch, but
a host-driven loop still uploads the coordinates, downloads the forces and integrates on the host every step -- for a
108-atom cell that round trip is of the order of the whole device step.  `DeviceMD` puts two small kernels around the
captured step (csrc/md_kernels.hip: `hermnet_md_advance` in front of the search, `hermnet_md_finish` behind the force
backward), so that one replay IS one time step:

    md = DeviceMD(model, z, cell, pos, masses, dt=1.0)                  # NVE; friction=, temperature= : Langevin
    md.run(1000)                # 1000 replays enqueued; returns at once: no synchronisation, no upload, no download
    s = md.fetch()              # ONE packed device-to-host copy + one synchronisation

Units are those of tools/md_nve.py: eV, Angstrom, amu, fs, K.  Coordinates and velocities are float64 on the device (a drift
of dt v ~ 1e-3 A added to a float32 coordinate of 30 A loses three digits every step); the model's float32 input is the
rounding of x.  The per-atom arithmetic is contraction-free IEEE, identical on the device, in the library's host twins and
in a numpy float64 transcription (tests/test_md_host.py, tests/test_md_device.py).

Halt protocol: a step whose neighbour list is incomplete (list flags; more pairs than `capacity`) or whose energy is not
finite (the stale-weight guard answers with NaN) is VOID -- coordinates, velocities and images return to the start of the
step, the halt code and step are recorded, no log row is written, and every later replay changes nothing.  `fetch()` reports
it; `resume()` recaptures (with a larger capacity where the list overflowed), re-evaluates the forces and clears the halt.

Out of scope: barostats / NPT (the cell is constant during `run`), constraints other than an infinite mass (= a fixed
atom), atom shards, HTNet, more than one time step per replay."""
import math
import types

import numpy as np
import torch

from . import _lib
from ._resident import HALT_CAPACITY, HALT_NONFINITE, PARKED as _PARKED, after_halt, cell_args, f64 as _f64, fetch_packed  # noqa: F401

AMU_A2_FS2_TO_EV = 103.642696562         # 1 amu A^2 / fs^2 in eV (tools/md_nve.py)
KB = 8.617333262e-5                       # eV / K
ASE_TIME_FS = math.sqrt(AMU_A2_FS2_TO_EV)   # ASE's time unit in fs: v [A/fs] = v_ase / 10.18051

HN_MD_LANGEVIN, HN_MD_WRAP = 1, 2        # include/hermnet_hip.h
# HALT_NONFINITE, HALT_CAPACITY (halt codes) and _PARKED (the halt code while a capture is made): _resident.py


class DeviceMD(object):
    """See the module docstring.  model: HVNet in eval(), parameters not requiring grad, on the GPU.  atomic_number [N],
    cell [3,3] (`batch` None) or [B,3,3], pos [N,3], masses [N] in amu (inf: the atom never moves), dt in fs.
    `friction=None`: NVE; `friction` (1/fs) with `temperature` (K, a scalar or [B]: replicas at different temperatures):
    Langevin, noise from Philox4x32-10 keyed by `seed` (it depends on seed, step and atom alone).  `batch` [N] int64
    non-decreasing with `num_graphs`: a batch of structures (`GraphedBatchMDStep`).  `capacity`, `reference_compat`: as for
    the graphed steps.  `log_steps`: rows of the observables ring -- `run` refuses to overwrite rows not fetched yet.
    `wrap`: coordinates are wrapped into the (triclinic) cell every step, `images` counts the lattice vectors removed
    (positions + images @ cell is the unwrapped path).  The coordinates given are used as they are for the first force
    evaluation."""

    def __init__(self, model, atomic_number, cell, pos, masses, dt, velocities=None, temperature=None, friction=None, seed=0,
                 batch=None, num_graphs=None, capacity=None, log_steps=4096, wrap=True, reference_compat=False,
                 device=None):
        from .graph import GraphedBatchMDStep, GraphedMDStep
        dev = torch.device(device) if device is not None else (pos.device if torch.is_tensor(pos) else torch.device("cuda:0"))
        if dev.type != "cuda":
            raise RuntimeError("DeviceMD needs GPU tensors")
        self.device, self.model = dev, model
        self.lib = _lib.load()
        self.dt, self.seed, self.log_steps = float(dt), int(seed) & (2 ** 64 - 1), int(log_steps)
        self.wrap, self.inv_cell, self._inv_of = bool(wrap), None, None
        if not (self.dt > 0.0) or self.log_steps < 1:
            raise ValueError("DeviceMD: dt > 0 and log_steps >= 1")
        self.z = torch.as_tensor(atomic_number).long().to(dev)
        n = self.n = int(self.z.numel())
        self.num_graphs = 1 if batch is None else int(num_graphs if num_graphs is not None else int(torch.as_tensor(batch)[-1]) + 1)
        B = self.num_graphs
        self.x = _f64(pos, dev, (n, 3))
        self.v = torch.zeros(n, 3, dtype=torch.float64, device=dev)
        self.x0, self.v0 = torch.zeros_like(self.x), torch.zeros_like(self.v)
        self.image = torch.zeros(n, 3, dtype=torch.int32, device=dev)
        self.image0 = torch.zeros_like(self.image)
        self.f_prev = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        self.ke_atom = torch.zeros(n, dtype=torch.float64, device=dev)
        self.log = torch.zeros(self.log_steps, B, 3, dtype=torch.float64, device=dev)
        self.state = torch.tensor([0, _PARKED, 0, 0], dtype=torch.int64).to(dev)
        # coefficients: everything that needs exp / sqrt / a division, once, in float64 on the host
        m = np.asarray(masses.detach().cpu() if torch.is_tensor(masses) else masses, dtype=np.float64).reshape(n)
        if not np.all(m > 0.0):
            raise ValueError("DeviceMD: masses must be positive (inf: a fixed atom)")
        self._m = m * AMU_A2_FS2_TO_EV                                    # eV fs^2 / A^2
        self._free = np.isfinite(self._m)
        batch_h = np.zeros(n, dtype=np.int64) if batch is None else np.asarray(torch.as_tensor(batch).cpu(), dtype=np.int64)
        if batch_h.shape != (n,) or np.any(np.diff(batch_h) < 0) or (n and (batch_h[0] < 0 or batch_h[-1] >= B)):
            raise ValueError("DeviceMD: batch must be [N], non-decreasing, in [0, num_graphs)")
        self._batch_h = batch_h
        self.graph_ptr = torch.from_numpy(np.searchsorted(batch_h, np.arange(B + 1)).astype(np.int32)).to(dev)
        self.kick = torch.from_numpy(0.5 * self.dt / self._m).to(dev)
        self.half_mass = torch.from_numpy(np.where(self._free, 0.5 * self._m, 0.0)).to(dev)
        self.flags = 0
        self.c1 = self.sigma = None
        if friction is not None:
            if temperature is None:
                raise ValueError("DeviceMD: Langevin dynamics (friction=) needs a temperature")
            t = np.asarray(temperature.detach().cpu() if torch.is_tensor(temperature) else temperature, dtype=np.float64)
            t = np.broadcast_to(t.reshape(-1) if t.ndim else t, (B,)).astype(np.float64)
            c1 = math.exp(-float(friction) * self.dt)
            self.c1 = torch.full((B,), c1, dtype=torch.float64).to(dev)
            self.sigma = torch.from_numpy(np.sqrt(KB * t[batch_h] * (1.0 - c1 * c1) / self._m)).to(dev)
            self.flags |= HN_MD_LANGEVIN
        self.temperature, self.friction = temperature, friction
        # the captured step: advance -> the graphed step's own _eager() -> finish
        cell_t = None if cell is None else torch.as_tensor(cell).detach().float().to(dev).contiguous()
        hooks = (self._advance, self._finish)
        self.batch = None
        p32 = self.x.float()
        if batch is None:
            if cell_t is None:
                raise RuntimeError("DeviceMD: one structure needs a periodic cell (open structures: batch=, cell=None)")
            self.step = GraphedMDStep(model, self.z, cell_t.reshape(3, 3), p32, capacity=capacity,
                                      reference_compat=reference_compat, hooks=hooks)
        else:
            self.batch = torch.from_numpy(batch_h).to(dev)
            self.step = GraphedBatchMDStep(model, self.z, cell_t, p32, self.batch, B, capacity=capacity,
                                           reference_compat=reference_compat, hooks=hooks)
        self._logged = self._pending = 0
        self._host = None
        if velocities is not None:
            self.set_velocities(velocities)
        self._prime()

    # ---- the two hooks of the capture ---------------------------------------------------------------------------------------
    def _cell_args(self, step):
        """(flags, cell pointer, inverse-cell pointer): the cell is the tensor the search reads; its inverse is made here."""
        wrap, cell, inv = cell_args(self, step)
        return (self.flags | HN_MD_WRAP) if wrap else (self.flags & ~HN_MD_WRAP), cell, inv

    def _advance(self, step):
        P = _lib.ptr
        flags, cell, inv = self._cell_args(step)
        if step.pos.dtype != torch.float32 or not step.pos.is_contiguous() or step.pos.numel() != 3 * self.n:
            raise RuntimeError("DeviceMD: the step's coordinate input must be a contiguous float32 [N,3]")
        _lib.check(self.lib.hermnet_md_advance(
            self.n, self.num_graphs, flags, self.dt, self.seed, P(self.x), P(self.v), P(self.x0), P(self.v0), P(self.image),
            P(self.image0), P(self.f_prev), P(self.kick), P(self.c1), P(self.sigma), P(self.batch), cell, inv, P(step.pos),
            P(self.state), torch.cuda.current_stream(self.device).cuda_stream), "hermnet_md_advance")

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = out[0], out[1], out[-2]
        if (energy.dtype != torch.float32 or not energy.is_contiguous() or energy.numel() != self.num_graphs
                or forces.dtype != torch.float32 or not forces.is_contiguous() or forces.numel() != 3 * self.n
                or total.dtype != torch.int64 or total.numel() != 2):
            raise RuntimeError("DeviceMD: unexpected outputs of the captured step")
        _lib.check(self.lib.hermnet_md_finish(
            self.n, self.num_graphs, P(self.graph_ptr), P(forces), P(energy), P(total), int(step.capacity), P(self.x), P(self.v),
            P(self.x0), P(self.v0), P(self.image), P(self.image0), P(self.f_prev), P(self.kick), P(self.half_mass), P(step.pos),
            P(self.ke_atom), P(self.log), self.log_steps, P(self.state),
            torch.cuda.current_stream(self.device).cuda_stream), "hermnet_md_finish")

    def _prime(self):
        """Clear the halt and evaluate the forces of the current coordinates with the captured graph (mode word 1: no kick,
        no log row, no step)."""
        self.state[1:3].zero_()
        self.state[3].fill_(1)
        self.step.graph.replay()

    # ---- running --------------------------------------------------------------------------------------------------------------
    @property
    def capacity(self):
        return self.step.capacity

    def stale(self):
        return self.step.stale()

    def run(self, n):
        """Enqueue `n` time steps (replays) back to back and return at once: no synchronisation, no copy."""
        n = int(n)
        if n < 0:
            raise ValueError("run(n): n >= 0")
        if self.step.stale():
            raise RuntimeError("DeviceMD: the model's weight copies were rebuilt after the capture -- resume() recaptures")
        if self._pending + n > self.log_steps:
            raise RuntimeError("DeviceMD.run(%d) would overwrite log rows not fetched yet (%d pending, log_steps=%d): fetch() "
                               "first" % (n, self._pending, self.log_steps))
        replay = self.step.graph.replay
        for _ in range(n):
            replay()
        self._pending += n

    def fetch(self):
        """Everything a caller wants on the host through ONE packed device-to-host copy and one synchronisation: `step`,
        `halted`, `halt_code` (list flags in the low bits, 4 = more pairs than capacity, 256 = an energy that is not finite),
        `halt_step`, `positions` [N,3] float64 (wrapped), `images` [N,3] int32, `velocities` [N,3] float64 (A/fs), `forces`
        [N,3] float32 (the last accepted ones), and `log` [rows,B,3] float64 = (E_pot, E_kin, edges found) of the steps
        completed since the last fetch."""
        n, B, rows = self.n, self.num_graphs, self._pending
        idx = (torch.arange(rows, device=self.device) + self._logged) % self.log_steps
        packed = torch.cat([self.state.double(), self.x.reshape(-1), self.image.double().reshape(-1), self.v.reshape(-1),
                            self.f_prev.double().reshape(-1), self.log.index_select(0, idx).reshape(-1)])
        h = fetch_packed(self, packed, 4 + 12 * n + self.log_steps * B * 3)
        step, code, halt_step = int(h[0]), int(h[1]), int(h[2])
        done = max(0, min(rows, step - self._logged))
        o = 4
        s = types.SimpleNamespace(step=step, halted=code != 0, halt_code=code, halt_step=halt_step if code else None)
        s.positions = h[o:o + 3 * n].reshape(n, 3).copy()
        s.images = h[o + 3 * n:o + 6 * n].astype(np.int32).reshape(n, 3)
        s.velocities = h[o + 6 * n:o + 9 * n].reshape(n, 3).copy()
        s.forces = h[o + 9 * n:o + 12 * n].astype(np.float32).reshape(n, 3)
        s.log = h[o + 12 * n:].reshape(rows, B, 3)[:done].copy()
        self._logged, self._pending = step, 0
        after_halt(self, code, halt_step)
        return s

    def resume(self):
        """After a halt (or a stale capture): a new capture -- with a larger capacity where the list had outgrown it --, the
        forces of the current coordinates, halt cleared.  The state is that of the last completed step; the noise of a step
        depends on (seed, step, atom) alone, so the run continues as if it had never stopped."""
        self.state[1].fill_(_PARKED)              # the capture's warm-up runs and its first replay must not integrate
        self.step.recapture()
        self._prime()

    # ---- velocities -----------------------------------------------------------------------------------------------------------
    def set_velocities(self, v):
        """v [N,3] in A/fs (atoms of infinite mass keep v = 0)."""
        v = np.array(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64).reshape(self.n, 3)
        v[~self._free] = 0.0
        self.v.copy_(torch.from_numpy(v))

    def maxwell_boltzmann(self, temperature, seed=0):
        """Velocities drawn from the Maxwell-Boltzmann distribution at `temperature` (K; a scalar or [B])."""
        t = np.asarray(temperature.detach().cpu() if torch.is_tensor(temperature) else temperature, dtype=np.float64)
        t = np.broadcast_to(t.reshape(-1) if t.ndim else t, (self.num_graphs,))[self._batch_h]
        xi = np.random.RandomState(seed).standard_normal((self.n, 3))
        with np.errstate(divide="ignore"):
            self.set_velocities(xi * np.sqrt(KB * t / self._m)[:, None])

    def zero_momentum(self):
        """Remove every graph's centre-of-mass velocity (atoms of infinite mass are not counted and keep v = 0)."""
        m = torch.from_numpy(np.where(self._free, self._m, 0.0)).to(self.device)
        b = self.batch if self.batch is not None else torch.zeros(self.n, dtype=torch.long, device=self.device)
        B = self.num_graphs
        p = torch.zeros(B, 3, dtype=torch.float64, device=self.device).index_add_(0, b, self.v * m[:, None])
        mt = torch.zeros(B, dtype=torch.float64, device=self.device).index_add_(0, b, m)
        vcm = p / mt.clamp_min(1e-300)[:, None]
        self.v.sub_(vcm[b] * (m > 0).double()[:, None])

    # ---- ASE hand-off (duck-typed: ASE itself is not needed) --------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, atoms, model, dt, device="cuda:0", **kw):
        """`atoms`: anything with `positions`, `numbers`, `cell`, `pbc`, `get_masses()`, `get_velocities()` (ASE units: A and
        A / (10.18051 fs))."""
        if not np.all(np.asarray(atoms.pbc)):
            raise RuntimeError("DeviceMD.from_atoms: a periodic structure (pbc in all three directions)")
        dev = torch.device(device)
        v = atoms.get_velocities()
        return cls(model, torch.as_tensor(np.asarray(atoms.numbers)).to(dev),
                   torch.as_tensor(np.asarray(atoms.cell, dtype=np.float64).reshape(3, 3)).float().to(dev),
                   np.asarray(atoms.positions, dtype=np.float64), np.asarray(atoms.get_masses(), dtype=np.float64), dt,
                   velocities=None if v is None else np.asarray(v, dtype=np.float64) / ASE_TIME_FS, device=dev, **kw)

    def to_atoms(self, atoms, snapshot=None):
        """Write positions (wrapped) and velocities (ASE units) of `snapshot` (default: a fetch()) into `atoms`; returns
        the snapshot."""
        s = snapshot if snapshot is not None else self.fetch()
        atoms.positions = s.positions.copy()
        atoms.set_velocities(s.velocities * ASE_TIME_FS)
        return s
