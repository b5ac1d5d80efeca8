"""Device-resident temperature replica exchange (parallel tempering): the exchanges of a ladder of Langevin replicas INSIDE
the replayed hipGraph.

`DeviceMD(..., friction=, temperature=[B], batch=)` runs B Langevin replicas at B temperatures in one capture, but cannot
exchange them: a host-driven ladder stops every few steps, fetches the energies, decides in numpy, rescales the velocities
and uploads new thermostat coefficients.  `DeviceREMD` keeps all of it on the device.  The front of the step is `DeviceMD`'s,
unchanged; `hermnet_remd_finish` (csrc/remd_kernels.hip; the definition is csrc/remd_step.h) takes the place of
`hermnet_md_finish` behind the force backward, so `run(n)` stays free of synchronisation across exchanges:

    remd = DeviceREMD(model, z, cells, pos, masses, dt=1.0, temperatures=[300, 330, 363, 400], friction=0.01,
                      exchange_interval=10, batch=batch, num_graphs=4)
    remd.maxwell_boltzmann(remd.temperatures)
    remd.run(1000)              # 1000 replays, 100 attempts; returns at once
    s = remd.fetch()            # s.rung [B], s.temperature [B], s.attempts / s.accepts [B-1], s.log [rows,B,5]

One ladder of R = B replicas of the same system.  `rung[g]` is the rung replica g holds, `replica_at[r]` its inverse; both
start as the identity.  Replicas stay where they are in the batch: temperatures travel.  The committed step with 0-based
index `step` ends with an attempt when (step + 1) % exchange_interval == 0; attempt a = (step + 1) / exchange_interval - 1
tries the neighbouring pairs (r, r+1) with r % 2 == a % 2.  Pair r is accepted iff delta = (beta_r - beta_(r+1)) (E_a - E_b)
>= 0 or log(u) < delta, with the step's own float32 energies in float64 and u from Philox4x32-10 keyed by `seed` at the
counter (r, step, stream 2) -- streams 0 and 1 are the atoms' noise.  A decision is a function of (seed, step, r, energies,
assignment) alone, so a run is reproducible however it is split, halted and resumed.  An accepted pair swaps rungs, the
velocities of the replica that goes up are multiplied by sqrt(T_(r+1) / T_r), of the one that goes down by its inverse, and
each atom's Langevin `sigma` becomes its new rung's.  A ladder that never exchanges is bit for bit `DeviceMD` with
`temperature=temperatures`.  A void step, a prime and a parked or halted replay attempt nothing.

Halt protocol, `resume()`, `run`, `maxwell_boltzmann`, `zero_momentum`: `DeviceMD`'s.

Out of scope: NPT ladders, Hamiltonian exchange, several ladders in one batch, non-neighbour pairs, atom shards, HTNet."""
import numpy as np
import torch

from . import _lib
from ._resident import host_f64
from .md import KB, CopiesMD, same_copies, stack_atoms


class DeviceREMD(CopiesMD):
    """See the module docstring.  model, atomic_number [N], cell [B,3,3] (None: open structures), pos [N,3], masses [N], dt,
    `batch` [N] with `num_graphs` = B, `seed`, `velocities`, `capacity`, `log_steps`, `wrap`, `reference_compat`, `device`:
    `DeviceMD`'s; the B graphs are the replicas.  `temperatures` [B] (K): the ladder, rung r at temperatures[r], replica g
    starts on rung g.  `friction` (1/fs): the Langevin thermostat's.  `exchange_interval`: an attempt every that many steps.

    ValueError, with the reason: `friction=None` (an exchange needs a thermostat: without one nothing would hold a replica at
    its new temperature); fewer than 2 replicas; `len(temperatures) != B` or a temperature that is not positive and finite;
    `exchange_interval < 1`; replicas that differ in atom count, atomic numbers, masses or cell.

    `fetch()`: `DeviceMD`'s snapshot, `log` [rows,B,5] = (E_pot, E_kin, edges found, the rung held during the step, the rung
    held behind the step's exchange) per time step -- E_kin is taken before any rescaling --, `rung` [B], `replica_at` [B],
    `temperature` [B] = temperatures[rung], `attempts` and `accepts` [B-1] per pair (r, r+1)."""

    __slots__ = ("temperatures", "exchange_interval", "sigma_table", "beta", "up", "down", "rung", "replica_at",
                 "rung_new", "vscale", "outcome", "attempts", "accepts")
    LOG_WIDTH = 5

    def __init__(self, model, atomic_number, cell, pos, masses, dt, temperatures, friction, exchange_interval, batch=None,
                 num_graphs=None, seed=0, **kw):
        if "temperature" in kw:
            raise ValueError("DeviceREMD: temperatures= is the ladder (there is no temperature=)")
        if friction is None:
            raise ValueError("DeviceREMD: friction=None -- an exchange needs a thermostat (Langevin) that holds a replica at "
                             "the temperature it was given")
        if batch is None:
            raise ValueError("DeviceREMD: a ladder needs 2 replicas or more: batch= and num_graphs= are required (the graphs "
                             "of the batch are the replicas)")
        batch_h = np.asarray(torch.as_tensor(batch).cpu(), dtype=np.int64).reshape(-1)
        B = int(num_graphs if num_graphs is not None else batch_h[-1] + 1)
        if B < 2:
            raise ValueError("DeviceREMD: a ladder needs 2 replicas or more (num_graphs = %d)" % B)
        t = host_f64(temperatures).reshape(-1).copy()
        if len(t) != B:
            raise ValueError("DeviceREMD: %d temperatures for %d replicas -- one per replica" % (len(t), B))
        if not np.all(np.isfinite(t) & (t > 0.0)):
            raise ValueError("DeviceREMD: temperatures must be positive and finite")
        if int(exchange_interval) != exchange_interval or int(exchange_interval) < 1:
            raise ValueError("DeviceREMD: exchange_interval must be an integer >= 1")
        self.temperatures = t                             # the ladder [R] in K, on the host
        self.exchange_interval = int(exchange_interval)   # steps between two attempts
        self.n_rep = same_copies("DeviceREMD", "replica", atomic_number, cell, masses, batch_h, B)   # atoms of one replica
        super().__init__(model, atomic_number, cell, pos, masses, dt, temperature=t, friction=friction, seed=seed, batch=batch,
                         num_graphs=B, **kw)

    def _own_state(self, masses):
        """`DeviceMD`'s coefficients (sigma of the identity assignment), then the ladder: what needs a division or a square
        root, once, in float64 on the host."""
        super()._own_state(masses)
        B, dev, t = self.num_graphs, self.device, self.temperatures
        c1 = float(self.c1[0])
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        with np.errstate(divide="ignore"):
            table = np.sqrt(KB * t[:, None] * (1.0 - c1 * c1) / self._m[None, :self.n_rep])
        self.sigma_table = put(table)                     # [R, n_rep] f64: DeviceMD's sigma of one replica at every rung
        self.beta = put(1.0 / (KB * t))                   # [R] f64
        self.up = put(np.sqrt(t[1:] / t[:-1]))            # [R-1] f64: the velocity factor of the replica that goes up ...
        self.down = put(np.sqrt(t[:-1] / t[1:]))          # ... and of the one that comes down
        self.rung = torch.arange(B, dtype=torch.int64, device=dev)                  # the rung a replica holds [B]; finish's last kernel
        self.replica_at = torch.arange(B, dtype=torch.int64, device=dev)            # its inverse [R]; finish's last kernel
        self.attempts = torch.zeros(B - 1, dtype=torch.int64, device=dev)           # tried pairs; finish's last kernel
        self.accepts = torch.zeros(B - 1, dtype=torch.int64, device=dev)            # accepted pairs; finish's last kernel
        self.rung_new = torch.arange(B, dtype=torch.int64, device=dev)              # scratch; finish's second kernel
        self.vscale = torch.ones(B, dtype=torch.float64, device=dev)                # scratch; finish's second kernel
        self.outcome = torch.zeros(B - 1, dtype=torch.int64, device=dev)            # scratch; finish's second kernel
        # (sigma [N], DeviceMD's: finish's third kernel rewrites a replica's entries when its rung changes)

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        _lib.call("hermnet_remd_finish", self.n, self.num_graphs, P(self.graph_ptr), P(forces), P(energy), P(total),
                  int(step.capacity), self.exchange_interval, self.seed, *self._finish_atoms(step), P(self.beta), P(self.up),
                  P(self.down), P(self.sigma_table), P(self.sigma), P(self.rung), P(self.replica_at), P(self.rung_new),
                  P(self.vscale), P(self.outcome), P(self.attempts), P(self.accepts), *self._finish_tail())

    # ---- the packed fetch's own part ------------------------------------------------------------------------------------------
    def _fetch_extras(self):
        return [self.rung, self.replica_at, self.attempts, self.accepts]

    def _read_extras(self, s, word, h):
        B = self.num_graphs
        s.rung, s.replica_at = h[:B].astype(np.int64), h[B:2 * B].astype(np.int64)
        s.attempts, s.accepts = h[2 * B:3 * B - 1].astype(np.int64), h[3 * B - 1:4 * B - 2].astype(np.int64)
        s.temperature = self.temperatures[s.rung]

    # ---- ASE hand-off (duck-typed) ------------------------------------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, replicas, model, dt, temperatures, friction, exchange_interval, device="cuda:0", **kw):
        """`replicas`: the list of the ladder's replicas in batch order -- what `md.stack_atoms` takes; all periodic in three
        directions, or all open."""
        if not isinstance(replicas, (list, tuple)) or len(replicas) < 2:
            raise ValueError("DeviceREMD.from_atoms: a list of 2 replicas or more")
        dev = torch.device(device)
        s = stack_atoms(replicas, "DeviceREMD.from_atoms", "replicas", dev)
        return cls(model, s.z, s.cell, s.pos, s.masses, dt, temperatures, friction, exchange_interval, batch=s.batch,
                   num_graphs=len(replicas), velocities=s.velocities, device=dev, **kw)

    def to_atoms(self, replicas, by_rung=False, snapshot=None):
        """Write positions (wrapped) and velocities (ASE units) of `snapshot` (default: a fetch()) into the list `replicas`:
        entry k takes replica k of the batch, or with `by_rung` the replica that holds rung k (ladder order: entry k is at
        temperatures[k]).  Returns the snapshot."""
        s = snapshot if snapshot is not None else self.fetch()
        if len(replicas) != self.num_graphs:
            raise ValueError("DeviceREMD.to_atoms: a list of %d replicas" % self.num_graphs)
        for k, atoms in enumerate(replicas):
            self._write_member(atoms, s, int(s.replica_at[k]) if by_rung else k)
        return s
