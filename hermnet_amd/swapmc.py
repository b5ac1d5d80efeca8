"""Device-resident hybrid Monte Carlo / MD: canonical species swaps between the steps of a replayed MD run, INSIDE the
replayed hipGraph.

Solid-state interdiffusion without vacancies is far beyond MD time scales, so chemical short-range order, segregation and
ordering transitions of an alloy are sampled with species swaps interleaved with MD (LAMMPS: `fix atom/swap`).  A host-driven
swap loop stops the replay for every trial -- fetch, decide in numpy, upload -- and rebuilds the atom set, because `z` is baked
into every capture.  `DeviceSwapMD` needs none of that, by one observation: in a fixed composition, exchanging the species of
atoms i and j is the same move as exchanging their COORDINATES.  `z`, the atom set, the row layout, `kick`, `half_mass`,
`sigma`, the species-resolved observers and the whole captured step stay exactly as they are:

    md = DeviceSwapMD(model, z, cell, pos, masses, dt=1.0, swap_interval=10, swaps=4, temperature=800.0, friction=0.01)
    md.run(md.replays_for(1000))    # 1000 time steps and the 396 trials between them; returns at once
    s = md.fetch()                  # s.swap_trials, s.swap_attempts / s.swap_accepts [B], s.energy_ref [B], s.swap_log

The cycle: the prime; then `swap_interval` committed MD steps (`DeviceMD`'s velocity Verlet or Langevin step, unchanged);
then `swaps` trial replays; and again.  `hermnet_swapmc_advance` / `hermnet_swapmc_finish` (csrc/swapmc_kernels.hip; the
definition is csrc/swapmc_step.h) take the place of `hermnet_md_advance` / `hermnet_md_finish` in the capture's two hooks and
branch on `state` and on the words mc = (t, left): t trials committed so far, left still due in this block.  A replay is a
prime where the mode word says so, else a trial where left > 0, else an MD step.  The commit sets left = swaps behind the
committed MD step that makes step % swap_interval == 0 and counts a committed trial; a prime leaves both words alone.

A trial replay makes one trial in EVERY graph of the batch (graphs may be different systems), each with its own pair, its
own beta = 1 / (kB `mc_temperature`) and its own decision.  Graph g's pair at trial t comes from Philox4x32-10 with the
driver's key at the counter (g, t, stream 3) -- streams 0 and 1 are the atoms' noise, stream 2 the replica exchange's: a
uniform first atom i among the graph's candidates (the atoms of finite mass: a fixed atom never swaps), then a uniform
partner j among the candidates of every OTHER species, both by a multiply-shift ((w m) >> 32) whose bias is at most
m / 2^32 for m candidates.  The proposal reads no coordinate, so it is symmetric.  A graph whose candidates are of one species
is not tried (outcome 0).  The move exchanges `x` and `image` of i and j; velocities stay with their atoms, so each atom keeps
its own mass and momentum, the move has dE_kin = 0 and detailed balance needs dE_pot alone -- nothing is rescaled.  Behind the
force backward d = E_new - energy_ref and the trial is accepted iff -beta d >= 0 or log(u) < -beta d.  Accepted: the forces of
g's atoms and energy_ref[g] are the new evaluation's.  Rejected: the pair is exchanged back, bit for bit.  A trial kicks
nobody, draws no atom's noise, writes no MD log row and does not advance `step`.

Halt protocol: `DeviceMD`'s.  A swap permutes coordinates, so the neighbour list's size cannot change in a trial: only an
energy that is not finite (the stale-weight guard) or the list's stale flags can void one.  A void trial exchanges every
graph's pair back, records the halt and leaves (t, left): after `resume()` -- whose prime leaves them alone too -- the same
trial is drawn again, and the resumed run equals an uninterrupted one.

`run(n)` keeps the base meaning: n replays of whichever kind is due (its room check is conservative for both rings);
`replays_for(md_steps)` answers how many replays the next `md_steps` time steps take.  Observers sample behind committed MD
steps only.  An accepted swap moves two atoms discontinuously: `MSD` reports those jumps as displacement; `Frames` and `RDF`
are unaffected.  `from_atoms` / `to_atoms`: `DeviceMD`'s for one structure; a list goes through `md.stack_atoms`.

Out of scope: semi-grand-canonical moves (the composition changes, the atom set must move), swaps under `DeviceNPT`,
`DeviceREMD` or `DevicePIMD`, restricting swaps to chosen species pairs, reusing the neighbour list across a trial (a trial
costs a full step), atom shards, HTNet."""
import numpy as np
import torch

from . import _lib
from ._resident import host_f64, per_graph
from .md import KB, DeviceMD, stack_atoms


def candidate_tables(z, free, batch_h, num_graphs):
    """(cand int32, cand_ptr int32 [B, S+1], S): per graph its atoms of finite mass (`free`) sorted by (species index, atom),
    and the absolute offsets of each species' range; species index = rank of the atomic number among those of the batch."""
    z = np.asarray(z, dtype=np.int64).reshape(-1)
    species = np.unique(z)
    S = max(1, len(species))
    index = np.searchsorted(species, z)
    atoms = np.nonzero(np.asarray(free, dtype=bool))[0]
    order = np.lexsort((atoms, index[atoms], batch_h[atoms]))
    cand = atoms[order].astype(np.int32)
    key = batch_h[cand] * S + index[cand]                 # ascending: (graph, species)
    ptr = np.searchsorted(key, np.arange(num_graphs * S + 1)).astype(np.int32)
    cand_ptr = np.stack([ptr[g * S:g * S + S + 1] for g in range(num_graphs)]) if num_graphs else np.zeros((0, S + 1), np.int32)
    return np.ascontiguousarray(cand), np.ascontiguousarray(cand_ptr, dtype=np.int32), S


class DeviceSwapMD(DeviceMD):
    """See the module docstring.  Everything `DeviceMD` takes (`friction=`, `temperature=`, `batch=`, `num_graphs=`, `seed=`,
    `observers=`, ...), and `swap_interval` (committed MD steps between two blocks of trials), `swaps` (trial replays of a
    block; 0: `DeviceMD` bit for bit), `mc_temperature` (K, a scalar or [B]; default: `temperature`), `swap_rows` (rows of the
    `swap_log` ring; default: `log_steps`).

    ValueError, with the reason: neither `mc_temperature` nor `temperature`; a temperature of the swaps that is not positive
    and finite; `swap_interval < 1`; `swaps < 0`; `swap_rows < 1`.

    `fetch()`: `DeviceMD`'s snapshot (`step` counts time steps, `log` holds the MD steps' rows), and `swap_trials` (t),
    `swaps_left`, `swap_attempts` / `swap_accepts` [B] (graphs tried / accepted), `energy_ref` [B] float64 (the energy of the
    current configuration) and `swap_log` [trials,B,4] = (i, j, d, outcome: 0 not tried, 1 rejected, 2 accepted) of the trials
    committed since the last fetch ((-1, -1, 0, 0) where not tried) -- all in the same packed copy."""

    __slots__ = ("swap_interval", "swaps", "mc_temperature", "swap_rows", "beta", "e_ref", "mc", "cand", "cand_ptr",
                 "num_species", "pair", "dval", "outcome", "attempts", "accepts", "swap_log", "_swap_logged", "_words")

    def __init__(self, model, atomic_number, cell, pos, masses, dt, swap_interval, swaps, mc_temperature=None, swap_rows=None,
                 **kw):
        t = mc_temperature if mc_temperature is not None else kw.get("temperature")
        if t is None:
            raise ValueError("DeviceSwapMD: the swaps need a temperature: mc_temperature= (K), or temperature= of the thermostat")
        if not np.all(np.isfinite(host_f64(t)) & (host_f64(t) > 0.0)):
            raise ValueError("DeviceSwapMD: the temperature of the swaps must be positive and finite")
        if int(swap_interval) != swap_interval or int(swap_interval) < 1:
            raise ValueError("DeviceSwapMD: swap_interval must be an integer >= 1")
        if int(swaps) != swaps or int(swaps) < 0:
            raise ValueError("DeviceSwapMD: swaps must be an integer >= 0")
        if swap_rows is not None and int(swap_rows) < 1:
            raise ValueError("DeviceSwapMD: swap_rows >= 1")
        self.swap_interval, self.swaps = int(swap_interval), int(swaps)       # MD steps between blocks; trials of a block
        self.mc_temperature = t                           # as given (K, a scalar or [B])
        self.swap_rows = None if swap_rows is None else int(swap_rows)        # rows of the swap ring (`_own_state`: log_steps)
        super().__init__(model, atomic_number, cell, pos, masses, dt, **kw)

    def _own_state(self, masses):
        """`DeviceMD`'s coefficients, then the swaps': beta and the candidate tables, once, on the host."""
        super()._own_state(masses)
        B, dev = self.num_graphs, self.device
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        if self.swap_rows is None:
            self.swap_rows = self.log_steps
        self.beta = put(1.0 / (KB * per_graph(self.mc_temperature, B)))       # [B] f64
        cand, cand_ptr, self.num_species = candidate_tables(self.z.cpu().numpy(), self._free, self._batch_h, B)
        self.cand, self.cand_ptr = put(cand), put(cand_ptr)                   # int32 [M], [B, S+1]
        self.e_ref = torch.zeros(B, dtype=torch.float64, device=dev)          # energy of the current configuration; finish's last kernel
        self.mc = torch.zeros(2, dtype=torch.int64, device=dev)               # (t, left); finish's last kernel
        self.attempts = torch.zeros(B, dtype=torch.int64, device=dev)         # tried; finish's last kernel
        self.accepts = torch.zeros(B, dtype=torch.int64, device=dev)          # accepted; finish's last kernel
        self.swap_log = torch.zeros(self.swap_rows, B, 4, dtype=torch.float64, device=dev)    # row t % swap_rows; finish's last kernel
        self.pair = torch.full((B, 2), -1, dtype=torch.int32, device=dev)     # scratch; finish's first kernel
        self.dval = torch.zeros(B, dtype=torch.float64, device=dev)           # scratch; finish's first kernel
        self.outcome = torch.zeros(B, dtype=torch.int64, device=dev)          # scratch; finish's first kernel
        self._swap_logged = 0             # `fetch`: the trial count its last snapshot stood at
        self._words = (0, 0)              # `fetch`: (step, left) of its last snapshot; `replays_for`

    def _tables(self):
        """The candidate tables' four arguments, in the order of the C boundary."""
        P = _lib.ptr
        return P(self.cand), P(self.cand_ptr), self.num_species, int(self.cand.numel())

    def _advance(self, step):
        P = _lib.ptr
        flags, cell, inv = self._advance_cell(step)
        _lib.call("hermnet_swapmc_advance", self.n, self.num_graphs, flags, self.dt, self.seed, *self._advance_atoms(),
                  P(self.c1), P(self.sigma), P(self.batch), cell, inv, P(self._pos_input(step)), P(self.state), P(self.mc),
                  P(self.graph_ptr), *self._tables(), torch.cuda.current_stream(self.device).cuda_stream)

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        _lib.call("hermnet_swapmc_finish", self.n, self.num_graphs, P(self.graph_ptr), P(self.batch), P(forces), P(energy),
                  P(total), int(step.capacity), self.swap_interval, self.swaps, self.seed, *self._finish_atoms(step),
                  P(self.beta), P(self.e_ref), P(self.mc), *self._tables(), P(self.pair), P(self.dval), P(self.outcome),
                  P(self.attempts), P(self.accepts), P(self.swap_log), self.swap_rows, *self._finish_tail())

    # ---- running --------------------------------------------------------------------------------------------------------------
    def run(self, n):
        """`DeviceMD.run`: `n` replays of whichever kind is due.  Refuses, as for the MD log, what could overwrite
        `swap_log` rows not fetched yet (every replay counted as a trial: conservative)."""
        if self._pending + int(n) > self.swap_rows:
            raise RuntimeError("DeviceSwapMD.run(%d) would overwrite swap_log rows not fetched yet (%d pending, swap_rows=%d): "
                               "fetch() first" % (int(n), self._pending, self.swap_rows))
        super().run(n)

    def replays_for(self, md_steps):
        """The replays that the next `md_steps` time steps take, from the words of the last `fetch()`: the trials still due in
        an open block, the steps, and the blocks of trials BETWEEN them -- the block behind the last of these steps is left
        for the next call.  RuntimeError with replays enqueued since that fetch (its words are stale)."""
        md_steps = int(md_steps)
        if md_steps < 0:
            raise ValueError("replays_for(md_steps): md_steps >= 0")
        if self._pending:
            raise RuntimeError("DeviceSwapMD.replays_for: %d replays were enqueued since the last fetch(): fetch() first"
                               % self._pending)
        if md_steps == 0:
            return 0
        step, left = self._words
        blocks = (step + md_steps - 1) // self.swap_interval - step // self.swap_interval
        return left + md_steps + self.swaps * blocks

    # ---- ASE hand-off (duck-typed) ------------------------------------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, atoms, model, dt, swap_interval, swaps, device="cuda:0", **kw):
        """`atoms`: one periodic structure (`DeviceMD.from_atoms`), or a list of structures -- what `md.stack_atoms` takes; all
        periodic in three directions, or all open -- that become the graphs of a batch."""
        if not isinstance(atoms, (list, tuple)):
            return super().from_atoms(atoms, model, dt, device=device, swap_interval=swap_interval, swaps=swaps, **kw)
        dev = torch.device(device)
        s = stack_atoms(list(atoms), "DeviceSwapMD.from_atoms", "structures", dev)
        return cls(model, s.z, s.cell, s.pos, s.masses, dt, swap_interval, swaps, batch=s.batch, num_graphs=len(atoms),
                   velocities=s.velocities, device=dev, **kw)

    def to_atoms(self, atoms, snapshot=None):
        """`DeviceMD.to_atoms`; a list takes the graphs of the batch in order.  (The species stay with their rows: after
        accepted swaps it is the positions that have changed places.)  Returns the snapshot."""
        if not isinstance(atoms, (list, tuple)):
            return super().to_atoms(atoms, snapshot)
        s = snapshot if snapshot is not None else self.fetch()
        if len(atoms) != self.num_graphs:
            raise ValueError("DeviceSwapMD.to_atoms: a list of %d structures" % self.num_graphs)
        ptr = np.searchsorted(self._batch_h, np.arange(self.num_graphs + 1))
        for g, member in enumerate(atoms):
            self._write_atoms(member, s.positions[ptr[g]:ptr[g + 1]], s.velocities[ptr[g]:ptr[g + 1]])
        return s

    # ---- the packed fetch's own part ------------------------------------------------------------------------------------------
    def _fetch_extras(self):
        idx = (torch.arange(self._pending, device=self.device) + self._swap_logged) % self.swap_rows
        return [self.mc, self.attempts, self.accepts, self.e_ref, self.swap_log.index_select(0, idx)]

    def _read_extras(self, s, word, h):
        B, rows = self.num_graphs, self._pending
        s.swap_trials, s.swaps_left = int(h[0]), int(h[1])
        s.swap_attempts, s.swap_accepts = h[2:2 + B].astype(np.int64), h[2 + B:2 + 2 * B].astype(np.int64)
        s.energy_ref = h[2 + 2 * B:2 + 3 * B].copy()
        done = max(0, min(rows, s.swap_trials - self._swap_logged))
        s.swap_log = h[2 + 3 * B:].reshape(rows, B, 4)[:done].copy()
        self._swap_logged, self._words = s.swap_trials, (s.step, s.swaps_left)
