"""Device-resident ring-polymer path-integral MD (PIMD, RPMD, TRPMD): the harmonic springs between the beads of a ring
polymer integrated INSIDE the replayed hipGraph.

`GraphedBatchMDStep` evaluates P copies of a system in one replay, but the beads of a ring polymer are coupled by springs,
and a host-driven loop leaves the replay every step to propagate them in normal modes.  `DevicePIMD` keeps that on the
device: `hermnet_pimd_advance` (csrc/pimd_kernels.hip; the definition is csrc/pimd_step.h) takes the place of
`hermnet_md_advance` in front of the search, and `hermnet_pimd_finish` is `hermnet_md_finish` with a wider log row, so one
replay IS one time step of the ring polymer and has exactly the launches of a `DeviceMD` replay:

    pimd = DevicePIMD.from_atoms(atoms, model, dt=0.5, temperature=300.0, beads=8)      # PILE-L thermostat, tau0 = 100 fs
    pimd.maxwell_boltzmann()    # at P T
    pimd.run(1000)              # 1000 replays enqueued; returns at once
    s = pimd.fetch()            # s.log [rows,P,5] = (E_pot_j, E_kin_j, edges found, spring_j, vir_j) per step and bead
    e = pimd.estimators(s)      # e.potential, e.kinetic_primitive, e.kinetic_virial, e.ring_energy [rows], e.centroid

The convention is Ceriotti, Parrinello, Markland and Manolopoulos, J. Chem. Phys. 133, 124104 (2010): the P beads are the P
graphs of the batch, all the same system of n_rep atoms (atom a of bead j is row j n_rep + a); every bead feels the full
model potential and the extended system is sampled at P T; omega_P = P kB T / hbar, springs 1/2 m omega_P^2 |q_j - q_(j+1)|^2
cyclic in j; normal modes through the real orthogonal C (`ring_tables`), omega_k = 2 omega_P sin(k pi / P).  The splitting is
BAOAB (Liu, Li and Liu, J. Chem. Phys. 145, 024103 (2016)): kick, exact free flight of every mode over dt/2, the PILE-L
thermostat v~ = c1_k v~ + sigma xi (gamma_k = 2 pile_lambda omega_k for k >= 1, gamma_0 = 1 / tau0), the flight again, the
second kick behind the force evaluation.  `thermostat=False` is plain RPMD -- no noise is drawn and the two half flights
are one flight over dt, so one bead is velocity Verlet as `DeviceMD` writes it --; `tau0=None` with the thermostat on
leaves the centroid mode free: TRPMD.  Everything that needs cos, sin, exp, sqrt or a division is made once on the host in
float64 (`ring_tables`); the kernels, their host twins and tests/pimd_reference.py only add, multiply and floor, so all
three agree bit for bit.  The noise depends on (seed, step, mode n_rep + atom) alone: a resumed run equals an uninterrupted
one.

Wrapping is by the centroid: every bead of an atom loses the same lattice vectors, so the beads of an atom always hold
equal images, the springs need no minimum image, and beads may sit slightly outside the cell (the search wraps on its own).

Halt protocol, `resume()`, `run`, `zero_momentum`: `DeviceMD`'s.

Out of scope: GLE / PIGLET thermostats, ring contraction, an NPT ring polymer, several rings in one batch, more than 128
beads, atom shards, HTNet."""
import math
import types

import numpy as np
import torch

from . import _lib
from ._resident import HN_MD_LANGEVIN, host_f64
from .md import KB, CopiesMD, same_copies, stack_atoms

HBAR = 0.6582119569                       # eV fs
MAX_BEADS = 128                           # csrc/pimd_step.h: HN_PIMD_MAX_BEADS (a tile is 256 / P atoms x P lanes)


def ring_matrix(beads):
    """The real orthogonal normal-mode matrix C [P,P], C[j][k]: q~_k = sum_j C[j][k] q_j."""
    P = int(beads)
    c = np.zeros((P, P))
    j = np.arange(P, dtype=np.float64)
    for k in range(P):
        if k == 0:
            c[:, k] = math.sqrt(1.0 / P)
        elif 2 * k < P:
            c[:, k] = math.sqrt(2.0 / P) * np.cos(2.0 * math.pi * j * k / P)
        elif 2 * k == P:
            c[:, k] = math.sqrt(1.0 / P) * (1.0 - 2.0 * (np.arange(P) % 2))
        else:
            c[:, k] = math.sqrt(2.0 / P) * np.sin(2.0 * math.pi * j * k / P)
    return c


def ring_tables(beads, dt, temperature, mass, tau0=100.0, pile_lambda=1.0, thermostat=True):
    """The host-made tables of one ring polymer, float64: a namespace of `cmat` [P,P], `omega` [P] (1/fs), `cs`, `sw`, `ws`,
    `c1` [P], `sigma` [P, n_rep], `inv_beads`, `spring_c` [n_rep] and `omega_p`.  `mass` [n_rep] in eV fs^2 / A^2 (inf: a
    held atom).  The free flight's tables are those of dt/2 with a thermostat and of dt without (the module docstring)."""
    P, dt, t = int(beads), float(dt), float(temperature)
    m = np.asarray(mass, dtype=np.float64).reshape(-1)
    omega_p = P * KB * t / HBAR
    k = np.arange(P, dtype=np.float64)
    omega = 2.0 * omega_p * np.sin(k * math.pi / P)
    omega[0] = 0.0
    flight = 0.5 * dt if thermostat else dt
    cs, sn = np.cos(omega * flight), np.sin(omega * flight)
    sw = np.full(P, flight)
    sw[1:] = sn[1:] / omega[1:]
    ws = omega * sn
    c1 = np.ones(P)
    if thermostat:
        gamma = 2.0 * float(pile_lambda) * omega
        gamma[0] = 0.0 if tau0 is None else 1.0 / float(tau0)
        c1 = np.array([math.exp(-g * dt) for g in gamma])
    with np.errstate(divide="ignore"):
        sigma = np.sqrt(KB * (P * t) * (1.0 - c1 * c1)[:, None] / m[None, :])
    spring_c = np.where(np.isfinite(m), 0.5 * m * omega_p * omega_p, 0.0)
    return types.SimpleNamespace(cmat=ring_matrix(P), omega=omega, cs=cs, sw=sw, ws=ws, c1=c1,
                                 sigma=np.ascontiguousarray(sigma), inv_beads=1.0 / P, spring_c=spring_c, omega_p=omega_p)


class DevicePIMD(CopiesMD):
    """See the module docstring.  model, atomic_number [N], cell [B,3,3] (None: open structures; [3,3] with `batch=None`), pos
    [N,3], masses [N], dt, `batch` [N] with `num_graphs` = P, `seed`, `velocities`, `capacity`, `log_steps`, `wrap`,
    `reference_compat`, `device`: `DeviceMD`'s; the P graphs are the beads, a single structure with `batch=None` is P = 1.
    `temperature` (K, one number): the physical temperature T -- the beads move at P T.  `tau0` (fs; None: the centroid is
    not thermostatted), `pile_lambda`, `thermostat`: the module docstring's.

    ValueError, with the reason: beads that differ in atom count, atomic numbers, masses or cell; more than 128 beads; a
    temperature, `tau0` or `pile_lambda` that is not positive and finite; `friction=` (the thermostat is PILE-L: `tau0=`,
    `pile_lambda=`, `thermostat=`) or a per-graph `temperature` (the beads of one ring share one T).

    `fetch()`: `DeviceMD`'s snapshot, `log` [rows,P,5] = (E_pot_j, E_kin_j, edges found, spring_j, vir_j) per time step with
    spring_j = sum_a 1/2 m_a omega_P^2 |x_(j,a) - x_(j+1,a)|^2 and vir_j = sum_a (x_(j,a) - centroid_a) . f_(j,a)."""

    __slots__ = ("beads", "tau0", "pile_lambda", "thermostat", "tables", "cmat", "cs", "sw", "ws", "pc1", "psigma",
                 "spring_c", "centroid")
    LOG_WIDTH = 5

    def __init__(self, model, atomic_number, cell, pos, masses, dt, temperature, tau0=100.0, pile_lambda=1.0, thermostat=True,
                 batch=None, num_graphs=None, seed=0, **kw):
        if "friction" in kw:
            raise ValueError("DevicePIMD: there is no friction= -- the thermostat is PILE-L: tau0= (fs, the centroid's; None: "
                             "TRPMD), pile_lambda= (the internal modes') and thermostat=False (RPMD)")
        t = host_f64(temperature)
        if t.size != 1:
            raise ValueError("DevicePIMD: temperature= is one number, the physical temperature of the ring polymer (its beads "
                             "move at P T); a per-graph temperature belongs to DeviceMD / DeviceREMD")
        t = float(t.reshape(-1)[0])
        positive = lambda a: math.isfinite(a) and a > 0.0
        if not positive(t):
            raise ValueError("DevicePIMD: temperature must be positive and finite")
        if tau0 is not None and not positive(float(tau0)):
            raise ValueError("DevicePIMD: tau0 must be positive and finite (None: no centroid thermostat, TRPMD)")
        if not positive(float(pile_lambda)):
            raise ValueError("DevicePIMD: pile_lambda must be positive and finite")
        z = torch.as_tensor(atomic_number).reshape(-1)
        if batch is None:
            P, self.n_rep = 1, int(z.numel())
        else:
            batch_h = np.asarray(torch.as_tensor(batch).cpu(), dtype=np.int64).reshape(-1)
            P = int(num_graphs if num_graphs is not None else batch_h[-1] + 1)
            if P > MAX_BEADS:
                raise ValueError("DevicePIMD: %d beads -- at most %d" % (P, MAX_BEADS))
            self.n_rep = same_copies("DevicePIMD", "bead", atomic_number, cell, masses, batch_h, P)
        self.beads = P                                    # P
        self.tau0 = None if tau0 is None else float(tau0)
        self.pile_lambda, self.thermostat = float(pile_lambda), bool(thermostat)
        super().__init__(model, atomic_number, cell, pos, masses, dt, temperature=t, friction=None, seed=seed, batch=batch,
                         num_graphs=None if batch is None else P, **kw)

    def _own_state(self, masses):
        """`DeviceMD`'s kick and half_mass, then the ring's tables: what needs cos / sin / exp / sqrt / a division, once, in
        float64 on the host."""
        super()._own_state(masses)
        dev = self.device
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        tb = self.tables = ring_tables(self.beads, self.dt, self.temperature, self._m[:self.n_rep], self.tau0, self.pile_lambda,
                                       self.thermostat)   # on the host
        self.cmat, self.cs, self.sw, self.ws = put(tb.cmat), put(tb.cs), put(tb.sw), put(tb.ws)
        self.pc1, self.psigma = put(tb.c1), put(tb.sigma)                 # [P], [P, n_rep]: the O step's
        self.spring_c = put(tb.spring_c)                                  # [n_rep]: 1/2 m omega_P^2
        self.centroid = torch.zeros(self.n_rep, 3, dtype=torch.float64, device=dev)   # the wrapped centroids; advance
        if self.thermostat:
            self.flags |= HN_MD_LANGEVIN

    # ---- the two hooks of the capture ---------------------------------------------------------------------------------------
    def _advance(self, step):
        P = _lib.ptr
        flags, cell, inv = self._advance_cell(step)
        _lib.call("hermnet_pimd_advance", self.n, self.num_graphs, flags, self.seed, self.tables.inv_beads,
                  *self._advance_atoms(), P(self.cmat), P(self.cs), P(self.sw), P(self.ws), P(self.pc1), P(self.psigma), cell, inv,
                  P(self._pos_input(step)), P(self.centroid), P(self.state), torch.cuda.current_stream(self.device).cuda_stream)

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        _lib.call("hermnet_pimd_finish", self.n, self.num_graphs, P(self.graph_ptr), P(forces), P(energy), P(total),
                  int(step.capacity), *self._finish_atoms(step), P(self.spring_c), P(self.centroid), *self._finish_tail())

    # ---- velocities, estimators -------------------------------------------------------------------------------------------------
    def maxwell_boltzmann(self, temperature=None, seed=0):
        """`DeviceMD.maxwell_boltzmann`; the default is P T, the temperature the beads move at."""
        super().maxwell_boltzmann(self.beads * self.temperature if temperature is None else temperature, seed)

    def estimators(self, snapshot):
        """Per logged step of `snapshot` (a `fetch()`), with N the atoms of finite mass and P the beads: `potential` = mean_j
        E_pot_j, `kinetic_primitive` = (3N/2) P kB T - (1/P) sum_j spring_j, `kinetic_virial` = (3N/2) kB T - (1/2P) sum_j
        vir_j, `ring_energy` = sum_j (E_kin_j + spring_j + E_pot_j) -- what RPMD conserves -- [rows] each, and `centroid`
        [n_rep,3], the mean over the beads of the snapshot's positions."""
        log, P, kt = snapshot.log, self.beads, KB * self.temperature
        n_free = int(np.count_nonzero(self._free[:self.n_rep]))
        return types.SimpleNamespace(
            potential=log[:, :, 0].sum(axis=1) / P,
            kinetic_primitive=1.5 * n_free * P * kt - log[:, :, 3].sum(axis=1) / P,
            kinetic_virial=1.5 * n_free * kt - log[:, :, 4].sum(axis=1) / (2.0 * P),
            ring_energy=(log[:, :, 1] + log[:, :, 3] + log[:, :, 0]).sum(axis=1),
            centroid=snapshot.positions.reshape(P, self.n_rep, 3).sum(axis=0) / P)

    # ---- ASE hand-off (duck-typed) ------------------------------------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, atoms, model, dt, temperature, beads=None, device="cuda:0", **kw):
        """`atoms`: one structure, replicated into `beads` graphs, or the list of the P beads (then `beads` is None or P) --
        anything with `positions`, `numbers`, `cell`, `pbc`, `get_masses()`, `get_velocities()` (ASE units); periodic in all
        three directions, or open."""
        if isinstance(atoms, (list, tuple)):
            images = list(atoms)
            if not images or (beads is not None and int(beads) != len(images)):
                raise ValueError("DevicePIMD.from_atoms: a list of the P beads (beads=%r, %d given)" % (beads, len(images)))
        else:
            if beads is None or int(beads) < 1:
                raise ValueError("DevicePIMD.from_atoms: beads >= 1")
            images = [atoms] * int(beads)
        dev = torch.device(device)
        s = stack_atoms(images, "DevicePIMD.from_atoms", "beads", dev)
        return cls(model, s.z, s.cell, s.pos, s.masses, dt, temperature, batch=s.batch, num_graphs=len(images),
                   velocities=s.velocities, device=dev, **kw)

    def to_atoms(self, images, snapshot=None):
        """Write positions (wrapped by the centroid) and velocities (ASE units) of `snapshot` (default: a fetch()) into the
        list `images`, entry j taking bead j.  Returns the snapshot."""
        s = snapshot if snapshot is not None else self.fetch()
        if not isinstance(images, (list, tuple)) or len(images) != self.beads:
            raise ValueError("DevicePIMD.to_atoms: a list of %d beads" % self.beads)
        for j, atoms in enumerate(images):
            self._write_member(atoms, s, j)
        return s

    def centroid_atoms(self, atoms, snapshot=None):
        """Write the centroid's positions and velocities (the means over the beads; ASE units) of `snapshot` (default: a
        fetch()) into `atoms`.  Returns the snapshot."""
        s = snapshot if snapshot is not None else self.fetch()
        mean = lambda a: a.reshape(self.beads, self.n_rep, 3).sum(axis=0) / self.beads
        self._write_atoms(atoms, mean(s.positions), mean(s.velocities))
        return s
