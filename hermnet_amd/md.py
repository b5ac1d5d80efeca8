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

`DeviceNPT` is `DeviceMD` with a Berendsen barostat inside the replay (its class docstring): the captured step carries the
virial kernels, and `hermnet_md_finish_npt` scales the cell and the coordinates at the end of every committed step.

Out of scope: for `DeviceMD` the cell is constant during `run` (barostat: `DeviceNPT`); for both, constraints other than an
infinite mass (= a fixed atom), atom shards, HTNet, more than one time step per replay."""
import math
import types

import numpy as np
import torch

from . import _lib
from ._resident import HALT_CAPACITY, HALT_NONFINITE, HN_MD_LANGEVIN, HN_MD_WRAP, ResidentDriver, host_f64, per_graph  # noqa: F401

AMU_A2_FS2_TO_EV = 103.642696562         # 1 amu A^2 / fs^2 in eV (tools/md_nve.py)
KB = 8.617333262e-5                       # eV / K
ASE_TIME_FS = math.sqrt(AMU_A2_FS2_TO_EV)   # ASE's time unit in fs: v [A/fs] = v_ase / 10.18051
GPA = 1.0 / 160.2176634                   # 1 GPa in eV / A^3
HN_MD_BARO = {"isotropic": _lib.HN_MD_BARO_ISOTROPIC, "axes": _lib.HN_MD_BARO_AXES, "full": _lib.HN_MD_BARO_FULL}


def stack_atoms(members, who, noun, device, cells_float64=False):
    """The list `members` of ASE-like structures (anything with `positions`, `numbers`, `cell`, `pbc`, `get_masses()`,
    `get_velocities()`; ASE units: A and A / (10.18051 fs)) as one batch for the MD drivers: a namespace of `z` [N] and
    `batch` [N] on `device`, `cell` [B,3,3] (None: every member is open; float64 on the host where `cells_float64`, else the
    step's float32 on the device), `pos` [N,3], `masses` [N] and `velocities` [N,3] in A/fs (None: no member has any; zeros
    for a member without) float64 on the host, and `counts`, the members' atom counts.  RuntimeError in the name of `who`
    unless the `noun` ("replicas", "beads", ...) are all periodic in three directions or all open."""
    periodic = [bool(np.all(np.asarray(a.pbc))) for a in members]
    if not all(periodic) and any(np.any(np.asarray(a.pbc)) for a in members):
        raise RuntimeError("%s: %s periodic in all three directions, or all open" % (who, noun))
    counts = [len(a.positions) for a in members]
    cell = None
    if all(periodic):
        cell = np.stack([np.asarray(a.cell, dtype=np.float64).reshape(3, 3) for a in members])
        if not cells_float64:
            cell = torch.as_tensor(cell).float().to(device)
    vel = [a.get_velocities() for a in members]
    v = None
    if any(u is not None for u in vel):
        v = np.concatenate([np.zeros((c, 3)) if u is None else np.asarray(u, dtype=np.float64) for u, c in zip(vel, counts)])
        v = v / ASE_TIME_FS
    return types.SimpleNamespace(
        z=torch.as_tensor(np.concatenate([np.asarray(a.numbers) for a in members])).to(device), cell=cell,
        pos=np.concatenate([np.asarray(a.positions, dtype=np.float64) for a in members]),
        masses=np.concatenate([np.asarray(a.get_masses(), dtype=np.float64) for a in members]), velocities=v,
        batch=torch.as_tensor(np.repeat(np.arange(len(members)), counts)).to(device), counts=counts)


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
    `resume()`: the noise of a step depends on (seed, step, atom) alone, so a resumed run equals an uninterrupted one.
    `observers`: a list of `observe.Frames` / `RDF` / `MSD` -- what they record arrives as `observers` [list] of the snapshot,
    in the same packed copy (hermnet_amd/observe.py)."""

    __slots__ = ("dt", "seed", "temperature", "friction", "flags", "_m", "_free", "v0", "ke_atom", "kick", "half_mass", "c1",
                 "sigma")
    LOG_WIDTH = 3

    def __init__(self, model, atomic_number, cell, pos, masses, dt, velocities=None, temperature=None, friction=None, seed=0,
                 batch=None, num_graphs=None, capacity=None, log_steps=4096, wrap=True, reference_compat=False,
                 device=None, observers=None):
        self.dt = float(dt)                               # the time step in fs
        self.seed = int(seed) & (2 ** 64 - 1)             # the noise's key
        if not (self.dt > 0.0) or int(log_steps) < 1:
            raise ValueError("DeviceMD: dt > 0 and log_steps >= 1")
        self.temperature, self.friction = temperature, friction       # as given
        self._start(model, atomic_number, cell, pos, batch, num_graphs, capacity, log_steps, wrap, reference_compat, device,
                    observers=observers, masses=masses)
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
    # (the blocks of arguments every driver of the family passes, in the order of the C boundary)
    def _advance_atoms(self):
        """The advance's eight per-atom pointers, x ... kick."""
        P = _lib.ptr
        return (P(self.x), P(self.v), P(self.x0), P(self.v0), P(self.image), P(self.image0), P(self.f_prev), P(self.kick))

    def _advance_cell(self, step):
        """(flags with the wrap bit as the step's cell says, cell pointer, inverse-cell pointer)."""
        wrap, cell, inv = self._cell_args(step)
        return (self.flags | HN_MD_WRAP) if wrap else (self.flags & ~HN_MD_WRAP), cell, inv

    def _finish_atoms(self, step):
        """The finish's eleven per-atom pointers, x ... ke_atom; pos32 is the step's coordinate input."""
        P = _lib.ptr
        return (P(self.x), P(self.v), P(self.x0), P(self.v0), P(self.image), P(self.image0), P(self.f_prev), P(self.kick),
                P(self.half_mass), P(step.pos), P(self.ke_atom))

    def _finish_tail(self):
        """What ends every finish: log, log_steps, state, stream."""
        return _lib.ptr(self.log), self.log_steps, _lib.ptr(self.state), torch.cuda.current_stream(self.device).cuda_stream

    def _advance(self, step):
        P = _lib.ptr
        flags, cell, inv = self._advance_cell(step)
        _lib.call("hermnet_md_advance", self.n, self.num_graphs, flags, self.dt, self.seed, *self._advance_atoms(), P(self.c1),
                  P(self.sigma), P(self.batch), cell, inv, P(self._pos_input(step)), P(self.state),
                  torch.cuda.current_stream(self.device).cuda_stream)

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        _lib.call("hermnet_md_finish", self.n, self.num_graphs, P(self.graph_ptr), P(forces), P(energy), P(total),
                  int(step.capacity), *self._finish_atoms(step), *self._finish_tail())

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
    CELLS_FLOAT64 = False     # from_atoms: the cell goes on as float64 on the host; else as the step's float32, on the device

    @classmethod
    def from_atoms(cls, atoms, model, dt, device="cuda:0", **kw):
        """`atoms`: one periodic structure -- what `stack_atoms` takes (`DeviceNPT`: its cell is kept in float64)."""
        dev = torch.device(device)
        s = stack_atoms([atoms], cls.__name__ + ".from_atoms", "a structure", dev, cls.CELLS_FLOAT64)
        if s.cell is None:
            raise RuntimeError("%s.from_atoms: a periodic structure (pbc in all three directions)" % cls.__name__)
        return cls(model, s.z, s.cell[0], s.pos, s.masses, dt, velocities=s.velocities, device=dev, **kw)

    @staticmethod
    def _write_atoms(atoms, positions, velocities):
        """`positions` (A) and `velocities` (A/fs) into `atoms`, in ASE's units."""
        atoms.positions = positions.copy()
        atoms.set_velocities(velocities * ASE_TIME_FS)

    def to_atoms(self, atoms, snapshot=None):
        """Write positions (wrapped) and velocities (ASE units) of `snapshot` (default: a fetch()) into `atoms`; returns
        the snapshot."""
        s = snapshot if snapshot is not None else self.fetch()
        self._write_atoms(atoms, s.positions, s.velocities)
        return s


def same_copies(name, noun, atomic_number, cell, masses, batch_h, B):
    """The atom count of one of the B graphs of a batch that must be copies of ONE system (`noun`: "replica", "bead");
    ValueError in the name of the driver `name` for copies that differ in atom count, atomic numbers, masses or cell."""
    z, m = np.asarray(torch.as_tensor(atomic_number).cpu()).reshape(-1), host_f64(masses).reshape(-1)
    if len(batch_h) != len(z) or len(m) != len(z) or np.any(np.diff(batch_h) < 0):
        raise ValueError("%s: atomic_number, masses and batch are [N], batch non-decreasing" % name)
    ptr = np.searchsorted(batch_h, np.arange(B + 1))
    differs = "%s: %s %%d differs from %s 0 in " % (name, noun, noun)
    for g in range(1, B):
        mine, first = slice(ptr[g], ptr[g + 1]), slice(ptr[0], ptr[1])
        if ptr[g + 1] - ptr[g] != ptr[1] - ptr[0]:
            raise ValueError((differs + "atom count (%d, %d): the %ss are copies of one system")
                             % (g, ptr[g + 1] - ptr[g], ptr[1] - ptr[0], noun))
        if np.any(z[mine] != z[first]):
            raise ValueError((differs + "atomic numbers") % g)
        if np.any(m[mine] != m[first]):
            raise ValueError((differs + "masses") % g)
    if cell is not None:
        c = host_f64(cell).reshape(-1, 3, 3)
        if len(c) != B:
            raise ValueError("%s: cell is [B,3,3], one per %s" % (name, noun))
        for g in range(1, B):
            if np.any(c[g] != c[0]):
                raise ValueError((differs + "cell") % g)
    return int(ptr[1] - ptr[0])


class CopiesMD(DeviceMD):
    """What the drivers of B copies of ONE system share (`remd.DeviceREMD`: the replicas of a ladder; `pimd.DevicePIMD`: the
    beads of a ring): copy g's atoms are the rows g n_rep .. (g + 1) n_rep of the batch.  The subclass's constructor sets
    `n_rep` (from `same_copies`) in front of `DeviceMD`'s."""

    __slots__ = ("n_rep",)

    def _write_member(self, atoms, snapshot, g):
        """Positions and velocities of copy `g` of `snapshot` into `atoms` (ASE units)."""
        mine = slice(g * self.n_rep, (g + 1) * self.n_rep)
        self._write_atoms(atoms, snapshot.positions[mine], snapshot.velocities[mine])


def _det3(c):
    """csrc/npt_step.h: npt_det3 on [B,3,3] float64, operation by operation."""
    c = c.reshape(-1, 9)
    return ((c[:, 0] * (c[:, 4] * c[:, 8] - c[:, 5] * c[:, 7]) + c[:, 1] * (c[:, 5] * c[:, 6] - c[:, 3] * c[:, 8]))
            + c[:, 2] * (c[:, 3] * c[:, 7] - c[:, 4] * c[:, 6]))


def _inverse3(c):
    """csrc/npt_step.h: npt_inverse3 (adjugate over determinant) on [B,3,3] float64: the inverse the kernels themselves
    make after every scaling, so a run's first wrap and its later ones use one definition."""
    c = c.reshape(-1, 9)
    det = _det3(c)
    a = [c[:, k] for k in range(9)]
    adj = [a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
           a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
           a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]]
    return np.stack([t / det for t in adj], axis=1).reshape(-1, 3, 3)


class DeviceNPT(DeviceMD):
    """`DeviceMD` at constant pressure: a Berendsen barostat INSIDE the replayed step, for one structure or a batch
    (replicas at different pressures and temperatures in one capture).  Everything `DeviceMD` takes, and `pressure` (the
    target, eV/A^3; `GPA` converts), `compressibility` (A^3/eV), `taup` (fs) -- scalars or [B] --, `coupling`:

        "isotropic"  mu = (1 - c (P0 - P)) I                            (ASE's NPTBerendsen)
        "axes"       mu = diag(1 - c (P0 - P_kk)) where `mask[k]`, 1 elsewhere      (ASE's Inhomogeneous_NPTBerendsen,
                     applied to Cartesian components, so it is valid for triclinic cells too)
        "full"       mu_ab = delta_ab - c (P0 delta_ab - P_ab)

    with c = (dt / taup) compressibility / 3 and P_ab = (sum m v_a v_b + sym(W)_ab) / V from the step's own virial W (stress
    = -sym(W) / V) and the kinetic tensor.  With `friction=None` it is velocity Verlet plus barostat, with `friction` the
    usual Langevin NPT.  One force evaluation per step: the scaling ends a committed step (cell <- cell mu, x <- x mu for
    every atom, held ones too; images and velocities stay) and the next replay's search reads the new cell.  The float64
    cell is the truth; the step's float32 cell is its rounding, as the float32 coordinates are of x.  Two safety conditions
    that are not physics: every entry of mu - I is clamped to +-`max_strain`, and a pressure that is not finite gives mu = I
    -- a scaled cell cannot be taken back by a later void step.  `cell` may be given in float64.

    `fetch()`: `DeviceMD`'s, `log` [rows,B,5] = (E_pot, E_kin, edges found, pressure, volume) per time step -- the pressure
    that step's scaling was made from, the volume before it --, `cell` [B,3,3] float64, `volume` [B], `mu` [B,3,3] (the last
    scaling) and `clamped` [B] (how often a safety condition acted).  A void step, a prime and the parked replays of a capture
    never scale, so halt and `resume()` are `DeviceMD`'s.

    Out of scope: stochastic cell rescaling (a barostat that samples the correct ensemble: `mtk.DeviceMTK`), velocity
    scaling, atom shards, HTNet, open structures (they have no volume).  (Relaxing a cell, under pressure too:
    `relax.DeviceCellRelax`.)"""

    __slots__ = ("pressure", "compressibility", "taup", "coupling", "mask", "max_strain", "cell64", "mu", "clamped", "p0",
                 "coupling_c", "_cell_given")
    LOG_WIDTH = 5

    def __init__(self, model, atomic_number, cell, pos, masses, dt, pressure=0.0, compressibility=None, taup=1000.0,
                 coupling="isotropic", mask=(1, 1, 1), max_strain=1e-2, **kw):
        if cell is None:
            raise RuntimeError("DeviceNPT: a barostat needs periodic cells (cell=None, open structures, have no volume)")
        if compressibility is None:
            raise ValueError("DeviceNPT: compressibility= (A^3/eV) is required")
        if coupling not in HN_MD_BARO:
            raise ValueError("DeviceNPT: coupling is one of %s" % sorted(HN_MD_BARO))
        self.pressure, self.compressibility, self.taup = pressure, compressibility, taup     # as given
        self.coupling = coupling                          # "isotropic", "axes" or "full"
        self.mask = sum(1 << k for k, on in enumerate(tuple(mask)) if on)      # "axes": bit k = direction k is coupled
        self.max_strain = float(max_strain)               # the largest |mu - I| entry of one step
        if len(tuple(mask)) != 3 or not (self.max_strain > 0.0):
            raise ValueError("DeviceNPT: mask has three entries and max_strain > 0")
        self._cell_given = cell                           # `_own_state` makes cell64 of it
        super().__init__(model, atomic_number, cell, pos, masses, dt, **kw)

    def _own_state(self, masses):
        super()._own_state(masses)
        B, dev = self.num_graphs, self.device
        taup, comp = per_graph(self.taup, B), per_graph(self.compressibility, B)
        if not (np.all(taup > 0.0) and np.all(comp >= 0.0)):
            raise ValueError("DeviceNPT: taup > 0 and compressibility >= 0")
        cell = host_f64(self._cell_given).reshape(B, 3, 3).copy()
        self._cell_given = None
        self.cell64 = torch.from_numpy(cell).to(dev)      # the cell [B,3,3] f64: the truth; finish
        self.inv_cell = torch.from_numpy(_inverse3(cell.astype(np.float32).astype(np.float64))).to(dev)   # of the f32 cell; finish
        self.mu = torch.eye(3, dtype=torch.float64, device=dev).repeat(B, 1, 1).contiguous()   # the last scaling; finish
        self.clamped = torch.zeros(B, dtype=torch.int64, device=dev)      # safety conditions that acted; finish
        self.p0 = torch.from_numpy(per_graph(self.pressure, B)).to(dev)   # the targets [B]
        self.coupling_c = torch.from_numpy((self.dt / taup) * comp / 3.0).to(dev)     # (dt / taup) compressibility / 3 [B]

    def _step_options(self, single):
        return dict(stress=True, variable_cell=True) if single else dict(stress=True)

    def _inverse_of(self, cell):
        return self.inv_cell              # device state: finish rewrites it with the cell

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        virial, cell, B = out[2], step.cell, self.num_graphs
        if virial.dtype != torch.float32 or not virial.is_contiguous() or virial.numel() != 9 * B:
            raise RuntimeError("DeviceNPT: the captured step must return a contiguous float32 virial [B,3,3]")
        if cell is None or cell.dtype != torch.float32 or not cell.is_contiguous() or cell.numel() != 9 * B:
            raise RuntimeError("DeviceNPT: the step's cell must be a contiguous float32 [B,3,3]")
        _lib.call("hermnet_md_finish_npt", self.n, B, P(self.graph_ptr), P(self.batch), P(forces), P(energy), P(virial),
                  P(total), int(step.capacity), HN_MD_BARO[self.coupling], self.mask, self.max_strain, P(self.p0),
                  P(self.coupling_c), *self._finish_atoms(step), P(self.cell64), P(cell), P(self.inv_cell), P(self.mu),
                  P(self.clamped), *self._finish_tail())

    def resume(self):
        """`DeviceMD.resume`, and the last accepted forces stay: they are those of the configuration BEFORE the last scaling
        (one force evaluation per step), which the recapture's evaluation of the scaled configuration must not replace --
        the next step's first kick is the one an uninterrupted run makes.  (After a change of weights that one half kick
        still uses the old weights' forces.)"""
        f = self.f_prev.clone()
        super().resume()
        self.f_prev.copy_(f)

    # ---- the packed fetch's own part ------------------------------------------------------------------------------------------
    def _fetch_extras(self):
        return [self.cell64, self.mu, self.clamped]

    def _read_extras(self, s, word, h):
        B = self.num_graphs
        s.cell, s.mu = h[:9 * B].reshape(B, 3, 3).copy(), h[9 * B:18 * B].reshape(B, 3, 3).copy()
        s.clamped = h[18 * B:19 * B].astype(np.int64)
        s.volume = np.abs(_det3(s.cell))

    # ---- ASE hand-off ---------------------------------------------------------------------------------------------------------
    CELLS_FLOAT64 = True                  # `_own_state` makes cell64 of it

    def to_atoms(self, atoms, snapshot=None):
        """`DeviceMD.to_atoms`, and the cell (one structure) -- written first and without moving the atoms: the positions
        are already those of the scaled cell."""
        s = snapshot if snapshot is not None else self.fetch()
        if self.num_graphs != 1:
            raise ValueError("DeviceNPT.to_atoms: one structure (a batch: take `cell` and `positions` of the snapshot)")
        if hasattr(atoms, "set_cell"):
            atoms.set_cell(s.cell[0].copy(), scale_atoms=False)
        else:
            atoms.cell = s.cell[0].copy()
        return super().to_atoms(atoms, s)
