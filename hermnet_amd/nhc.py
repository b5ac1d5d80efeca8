"""Device-resident NVT with Nose-Hoover chains: a deterministic, global, canonical thermostat INSIDE the replayed hipGraph.

`DeviceMD`'s only thermostat is Langevin, whose friction and noise act on every atom and damp exactly what the observers
measure inside the replay -- diffusion (`observe.MSD`) and velocity correlations (`observe.Frames`).  A Nose-Hoover chain
(Martyna, Klein, Tuckerman 1992; the integrator of Martyna, Tuckerman, Tobias, Klein 1996: LAMMPS's `fix nvt`) couples to a
graph through ONE number, its kinetic energy, and acts on it through ONE factor on its velocities, so the dynamics stay
deterministic and the momentum-conserving, time-reversible flow of NVE is only rescaled:

    md = DeviceNHC(model, z, cell, pos, masses, dt=1.0, temperature=300.0, tau=100.0)       # chain=3, order=3, substeps=1
    md.maxwell_boltzmann(300.0); md.zero_momentum()
    md.run(1000)
    s = md.fetch()                  # s.xi, s.v_xi [B,M], s.nhc_scale [B,2], s.temperature_now [B], s.log [rows,B,4]
    e = conserved(s)                # E_pot + E_kin + E_nhc per row and graph: constant up to the splitting error O(dt^2)

A time step is  NHC(dt/2) . kick(dt/2) . drift(dt) . [forces] . kick(dt/2) . NHC(dt/2).  `hermnet_nhc_advance` /
`hermnet_nhc_finish` (csrc/nhc_kernels.hip; the definition is csrc/nhc_step.h) take the place of `hermnet_md_advance` /
`hermnet_md_finish` in the capture's two hooks: two launches in front (the opening half step of every graph's chain by one
workgroup per graph, then `DeviceMD`'s NVE advance with the opening factor on v) and four behind (`DeviceMD`'s per-atom
finish, the closing half step with the log row, the closing factor on v, `DeviceMD`'s commit).  The chain's arithmetic is
IEEE +, x, floor, ldexp and the library's own exp alone, every division made here in float64, so device, host twins and
the numpy transcription (tests/nhc_reference.py) agree bit for bit.  The opening half step takes the kinetic energy from
the velocities as they stand, not from a number the last step left: `set_velocities`, `maxwell_boltzmann`, `zero_momentum`
and `resume()` need no bookkeeping.

Chain masses: Q_1 = dof kB T tau^2, Q_j = kB T tau^2.  `tau=inf` switches a graph's thermostat off: Q = 1/Q = 0, every
factor is exactly 1.0 and that graph's trajectory is `DeviceMD`'s NVE bit for bit.  `dof=None` counts 3 n_free - 3 for a
periodic graph without an atom of infinite mass -- its total momentum is conserved, so call `zero_momentum()` (a drifting
centre of mass is thermostatted as if it were heat) --, and 3 n_free for a graph that holds a fixed atom or is open.

Halt protocol: `DeviceMD`'s.  A void step returns the chain (xi, v_xi) to the start of the step with the atoms; a prime and
the parked replays of a capture leave it alone, so a resumed run equals an uninterrupted one, chain state included.

Out of scope: combination with `DeviceNPT` / `DeviceREMD` / `DevicePIMD` / `DeviceMetaD` / `DeviceSwapMD` (the MTK barostat
that stands on this: `mtk.DeviceMTK`), per-atom ("massive") chains, atom shards, HTNet."""
import numpy as np
import torch

from . import _lib
from ._resident import host_f64, per_graph
from .md import KB, DeviceMD

MAX_CHAIN = 8


def suzuki_yoshida(order):
    """The `order` (1, 3 or 5) Suzuki-Yoshida weights, float64."""
    if order == 1:
        return np.array([1.0])
    if order == 3:
        w = 1.0 / (2.0 - 2.0 ** (1.0 / 3.0))
        return np.array([w, 1.0 - 2.0 * w, w])
    if order == 5:
        w = 1.0 / (4.0 - 4.0 ** (1.0 / 3.0))
        return np.array([w, w, 1.0 - 4.0 * w, w, w])
    raise ValueError("DeviceNHC: order (the number of Suzuki-Yoshida weights) is one of 1, 3, 5")


def chain_tables(temperature, tau, dof, dt, chain, order, substeps):
    """What the kernels read, made once in float64 on the host: (delta [order] = w (dt / 2) / substeps, kt [B] = kB T, dof_kt
    [B], q [B,M], inv_q [B,M]); `temperature`, `tau`, `dof` are [B].  tau = inf: q = inv_q = 0."""
    kt = KB * np.asarray(temperature, dtype=np.float64)
    dof_kt = np.asarray(dof, dtype=np.float64) * kt
    tau = np.asarray(tau, dtype=np.float64)
    on = np.isfinite(tau)
    tau2 = np.where(on, tau, 1.0) ** 2
    q = np.repeat((kt * tau2)[:, None], chain, axis=1)
    q[:, 0] = dof_kt * tau2
    q = np.where(on[:, None], q, 0.0)
    with np.errstate(divide="ignore"):
        inv_q = np.where(on[:, None], 1.0 / q, 0.0)
    delta = suzuki_yoshida(order) * (0.5 * float(dt)) / float(substeps)
    return tuple(np.ascontiguousarray(a, dtype=np.float64) for a in (delta, kt, dof_kt, q, inv_q))


def default_dof(masses, batch_h, num_graphs, periodic):
    """[B] float64: 3 n_free - 3 for a periodic graph whose atoms all move (its total momentum is conserved), 3 n_free for a
    graph with an atom of infinite mass or an open one."""
    free = np.isfinite(host_f64(masses).reshape(-1))
    n_all = np.bincount(batch_h, minlength=num_graphs)
    n_free = np.bincount(batch_h, weights=free.astype(np.float64), minlength=num_graphs)
    return np.where((n_free == n_all) & bool(periodic), 3.0 * n_free - 3.0, 3.0 * n_free)


def conserved(snapshot):
    """E_pot + E_kin + E_nhc [rows,B] of a `DeviceNHC.fetch()` snapshot's log: the extended energy the scheme conserves."""
    log = snapshot.log
    return (log[..., 0] + log[..., 1]) + log[..., 3]


class DeviceNHC(DeviceMD):
    """See the module docstring.  Everything `DeviceMD` takes but `friction=` (refused: one thermostat), and `temperature`
    (K) and `tau` (fs; the thermostat's time constant, inf: off) -- scalars or [B]: replicas at different temperatures and
    time constants share one capture --, `chain` (M, 1..8 thermostats per graph), `order` (Suzuki-Yoshida weights: 1, 3 or
    5), `substeps` (>= 1) and `dof` (None: the module docstring's count, or [B]).

    ValueError, with the reason: `friction=`; `chain` outside 1..8; `order` not in {1, 3, 5}; `substeps < 1`; a temperature
    that is not positive and finite; `tau <= 0` (or NaN); a graph with `dof <= 0` (a thermostat needs a degree of freedom).

    `fetch()`: `DeviceMD`'s snapshot in the same ONE packed copy, `log` [rows,B,4] = (E_pot, E_kin behind the closing half
    step, edges found, E_nhc) per time step with E_nhc = sum_j Q_j v_xi_j^2 / 2 + dof kB T xi_1 + kB T sum_{j>=2} xi_j, and
    `xi`, `v_xi` [B,M], `nhc_scale` [B,2] (the last opening and closing factor), `temperature_now` [B] = 2 E_kin / (dof kB)
    of the velocities fetched.  `conserved(snapshot)` adds the log's three energies."""

    __slots__ = ("tau", "chain", "order", "substeps", "dof", "delta", "kt", "dof_kt", "q", "inv_q", "xi", "v_xi", "xi0",
                 "v_xi0", "scale", "_tables")
    LOG_WIDTH = 4

    def __init__(self, model, atomic_number, cell, pos, masses, dt, temperature=None, tau=100.0, chain=3, order=3, substeps=1,
                 dof=None, batch=None, num_graphs=None, **kw):
        if kw.get("friction") is not None:
            raise ValueError("DeviceNHC: friction= is Langevin's: one thermostat per run (a Nose-Hoover chain is deterministic)")
        kw.pop("friction", None)
        if int(chain) != chain or not 1 <= int(chain) <= MAX_CHAIN:
            raise ValueError("DeviceNHC: chain (thermostats per graph) must be an integer in 1..%d" % MAX_CHAIN)
        if order not in (1, 3, 5):
            raise ValueError("DeviceNHC: order (the number of Suzuki-Yoshida weights) is one of 1, 3, 5")
        if int(substeps) != substeps or int(substeps) < 1:
            raise ValueError("DeviceNHC: substeps must be an integer >= 1")
        if temperature is None or not np.all(np.isfinite(host_f64(temperature)) & (host_f64(temperature) > 0.0)):
            raise ValueError("DeviceNHC: the temperature (K) must be positive and finite")
        if not np.all(host_f64(tau) > 0.0):
            raise ValueError("DeviceNHC: tau (fs) must be > 0 (inf: the thermostat is off)")
        n = int(torch.as_tensor(atomic_number).numel())
        B = 1 if batch is None else int(num_graphs if num_graphs is not None else int(torch.as_tensor(batch)[-1]) + 1)
        batch_h = np.zeros(n, dtype=np.int64) if batch is None else np.asarray(torch.as_tensor(batch).cpu(), dtype=np.int64)
        if batch_h.shape != (n,) or host_f64(masses).size != n or (n and (batch_h.min() < 0 or batch_h.max() >= B)):
            raise ValueError("DeviceNHC: masses and batch are [N], batch in [0, num_graphs)")
        d = default_dof(masses, batch_h, B, cell is not None) if dof is None else per_graph(dof, B)
        if not np.all(d > 0.0):
            g = int(np.nonzero(~(d > 0.0))[0][0])
            raise ValueError("DeviceNHC: graph %d has dof = %g <= 0: a thermostat needs a degree of freedom to act on (3 n_free "
                             "- 3 where the total momentum is conserved; pass dof= to count otherwise)" % (g, d[g]))
        self.tau = tau                                    # as given (fs, a scalar or [B])
        self.chain, self.order, self.substeps = int(chain), int(order), int(substeps)       # M, weights, substeps
        self.dof = d                                      # [B] float64, on the host
        super().__init__(model, atomic_number, cell, pos, masses, dt, temperature=temperature, friction=None, batch=batch,
                         num_graphs=num_graphs, **kw)

    def _own_state(self, masses):
        """`DeviceMD`'s coefficients (NVE), then the chains': the tables of `chain_tables` and the state, zeros."""
        super()._own_state(masses)
        B, M, dev = self.num_graphs, self.chain, self.device
        tables = chain_tables(per_graph(self.temperature, B), per_graph(self.tau, B), self.dof, self.dt, M, self.order,
                              self.substeps)
        self.delta, self.kt, self.dof_kt, self.q, self.inv_q = (torch.from_numpy(a).to(dev) for a in tables)
        zeros = lambda: torch.zeros(B, M, dtype=torch.float64, device=dev)
        self.xi, self.v_xi = zeros(), zeros()             # the chains [B,M]; the advance's and the finish's graph kernels
        self.xi0, self.v_xi0 = zeros(), zeros()           # ... at the start of the step; the advance's graph kernel
        self.scale = torch.ones(B, 2, dtype=torch.float64, device=dev)    # the last opening / closing factor; the same two
        P = _lib.ptr
        self._tables = (M, self.order, self.substeps, P(self.delta), P(self.kt), P(self.dof_kt), P(self.q), P(self.inv_q),
                        P(self.xi), P(self.v_xi), P(self.xi0), P(self.v_xi0), P(self.scale))    # in the order of the C boundary

    def _advance(self, step):
        P = _lib.ptr
        flags, cell, inv = self._advance_cell(step)
        _lib.call("hermnet_nhc_advance", self.n, self.num_graphs, flags, self.dt, *self._advance_atoms(), P(self.batch), cell,
                  inv, P(self._pos_input(step)), P(self.state), P(self.graph_ptr), P(self.half_mass), *self._tables,
                  torch.cuda.current_stream(self.device).cuda_stream)

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        _lib.call("hermnet_nhc_finish", self.n, self.num_graphs, P(self.graph_ptr), P(self.batch), P(forces), P(energy),
                  P(total), int(step.capacity), *self._finish_atoms(step), *self._tables, *self._finish_tail())

    # ---- the packed fetch's own part ------------------------------------------------------------------------------------------
    def _fetch_extras(self):
        return [self.xi, self.v_xi, self.scale]

    def _read_extras(self, s, word, h):
        B, M = self.num_graphs, self.chain
        s.xi, s.v_xi = h[:B * M].reshape(B, M).copy(), h[B * M:2 * B * M].reshape(B, M).copy()
        s.nhc_scale = h[2 * B * M:2 * B * M + 2 * B].reshape(B, 2).copy()

    def _unpack(self, h, o, rows):
        s = super()._unpack(h, o, rows)
        ke = np.where(self._free, 0.5 * self._m, 0.0) * (s.velocities ** 2).sum(axis=1)
        s.temperature_now = 2.0 * np.bincount(self._batch_h, weights=ke, minlength=self.num_graphs) / (self.dof * KB)
        return s
