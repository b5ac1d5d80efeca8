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

Halt protocol (the resident drivers': `_resident.ResidentDriver`, csrc/resident_step.h): a step whose neighbour list is
incomplete (list flags; more pairs than `capacity`) or whose energy is not finite (the stale-weight guard answers with NaN)
is VOID -- coordinates, velocities and images return to the start of the
step, the halt code and step are recorded, no log row is written, and every later replay changes nothing.  `fetch()` reports
it; `resume()` recaptures (with a larger capacity where the list overflowed), re-evaluates the forces and clears the halt.

Out of scope: barostats / NPT (the cell is constant during `run`), constraints other than an infinite mass (= a fixed
atom), atom shards, HTNet, more than one time step per replay."""
import math

import numpy as np
import torch

from . import _lib
from ._resident import HALT_CAPACITY, HALT_NONFINITE, HN_MD_LANGEVIN, HN_MD_WRAP, ResidentDriver, host_f64, per_graph  # noqa: F401

AMU_A2_FS2_TO_EV = 103.642696562         # 1 amu A^2 / fs^2 in eV (tools/md_nve.py)
KB = 8.617333262e-5                       # eV / K
ASE_TIME_FS = math.sqrt(AMU_A2_FS2_TO_EV)   # ASE's time unit in fs: v [A/fs] = v_ase / 10.18051


class DeviceMD(ResidentDriver):
    """See the module docstring.  model: HVNet in eval(), parameters not requiring grad, on the GPU.  atomic_number [N],
    cell [3,3] (`batch` None) or [B,3,3], pos [N,3], masses [N] in amu (inf: the atom never moves), dt in fs.
    `friction=None`: NVE; `friction` (1/fs) with `temperature` (K, a scalar or [B]: replicas at different temperatures):
    Langevin, noise from Philox4x32-10 keyed by `seed` (it depends on seed, step and atom alone).  `batch` [N] int64
    non-decreasing with `num_graphs`: a batch of structures (`GraphedBatchMDStep`).  `capacity`, `reference_compat`: as for
    the graphed steps.  `log_steps`: rows of the observables ring -- `run` refuses to overwrite rows not fetched yet.
    `wrap`: coordinates are wrapped into the (triclinic) cell every step, `images` counts the lattice vectors removed
    (positions + images @ cell is the unwrapped path).  The coordinates given are used as they are for the first force
    evaluation.

    `fetch()`: the base's snapshot, `velocities` in A/fs, `log` [rows,B,3] = (E_pot, E_kin, edges found) per time step.
    `resume()`: the noise of a step depends on (seed, step, atom) alone, so a resumed run equals an uninterrupted one."""

    __slots__ = ("dt", "seed", "temperature", "friction", "flags", "_m", "_free", "v0", "ke_atom", "kick", "half_mass", "c1",
                 "sigma")
    LOG_WIDTH = 3

    def __init__(self, model, atomic_number, cell, pos, masses, dt, velocities=None, temperature=None, friction=None, seed=0,
                 batch=None, num_graphs=None, capacity=None, log_steps=4096, wrap=True, reference_compat=False,
                 device=None):
        self.dt = float(dt)                               # the time step in fs
        self.seed = int(seed) & (2 ** 64 - 1)             # the noise's key
        if not (self.dt > 0.0) or int(log_steps) < 1:
            raise ValueError("DeviceMD: dt > 0 and log_steps >= 1")
        self.temperature, self.friction = temperature, friction       # as given
        self._start(model, atomic_number, cell, pos, batch, num_graphs, capacity, log_steps, wrap, reference_compat, device,
                    masses=masses)
        if velocities is not None:
            self.set_velocities(velocities)
        self._unpark()

    def _own_state(self, masses):
        """Coefficients: everything that needs exp / sqrt / a division, once, in float64 on the host."""
        n, B, dev = self.n, self.num_graphs, self.device
        m = host_f64(masses).reshape(n)
        if not np.all(m > 0.0):
            raise ValueError("DeviceMD: masses must be positive (inf: a fixed atom)")
        self._m = m * AMU_A2_FS2_TO_EV                    # masses in eV fs^2 / A^2, on the host
        self._free = np.isfinite(self._m)                 # atoms of finite mass, on the host
        self.v0 = torch.zeros_like(self.v)                # v at the start of the step; advance
        self.ke_atom = torch.zeros(n, dtype=torch.float64, device=dev)    # per-atom kinetic energies; finish
        self.kick = torch.from_numpy(0.5 * self.dt / self._m).to(dev)     # dt / 2m [N]
        self.half_mass = torch.from_numpy(np.where(self._free, 0.5 * self._m, 0.0)).to(dev)   # m / 2 [N], 0 where fixed
        self.flags = 0                                    # HN_MD_LANGEVIN where a thermostat runs (the wrap bit: `_advance`)
        self.c1 = self.sigma = None                       # Langevin: exp(-friction dt) [B], sqrt(kB T (1 - c1^2) / m) [N]
        if self.friction is not None:
            if self.temperature is None:
                raise ValueError("DeviceMD: Langevin dynamics (friction=) needs a temperature")
            t = per_graph(self.temperature, B)
            c1 = math.exp(-float(self.friction) * self.dt)
            self.c1 = torch.full((B,), c1, dtype=torch.float64).to(dev)
            self.sigma = torch.from_numpy(np.sqrt(KB * t[self._batch_h] * (1.0 - c1 * c1) / self._m)).to(dev)
            self.flags |= HN_MD_LANGEVIN

    # ---- the two hooks of the capture ---------------------------------------------------------------------------------------
    def _advance(self, step):
        P = _lib.ptr
        wrap, cell, inv = self._cell_args(step)
        flags = (self.flags | HN_MD_WRAP) if wrap else (self.flags & ~HN_MD_WRAP)
        _lib.check(self.lib.hermnet_md_advance(
            self.n, self.num_graphs, flags, self.dt, self.seed, P(self.x), P(self.v), P(self.x0), P(self.v0), P(self.image),
            P(self.image0), P(self.f_prev), P(self.kick), P(self.c1), P(self.sigma), P(self.batch), cell, inv,
            P(self._pos_input(step)), P(self.state), torch.cuda.current_stream(self.device).cuda_stream), "hermnet_md_advance")

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        _lib.check(self.lib.hermnet_md_finish(
            self.n, self.num_graphs, P(self.graph_ptr), P(forces), P(energy), P(total), int(step.capacity), P(self.x), P(self.v),
            P(self.x0), P(self.v0), P(self.image), P(self.image0), P(self.f_prev), P(self.kick), P(self.half_mass), P(step.pos),
            P(self.ke_atom), P(self.log), self.log_steps, P(self.state),
            torch.cuda.current_stream(self.device).cuda_stream), "hermnet_md_finish")

    def _unpark(self):
        """Clear the halt and evaluate the forces of the current coordinates with the captured graph (mode word 1: no kick,
        no log row, no step): the first force evaluation, and the one behind a recapture."""
        self.state[1:3].zero_()
        self.state[3].fill_(1)
        self.step.graph.replay()

    # ---- velocities -----------------------------------------------------------------------------------------------------------
    def set_velocities(self, v):
        """v [N,3] in A/fs (atoms of infinite mass keep v = 0)."""
        v = host_f64(v).reshape(self.n, 3).copy()
        v[~self._free] = 0.0
        self.v.copy_(torch.from_numpy(v))

    def maxwell_boltzmann(self, temperature, seed=0):
        """Velocities drawn from the Maxwell-Boltzmann distribution at `temperature` (K; a scalar or [B])."""
        t = per_graph(temperature, self.num_graphs)[self._batch_h]
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
