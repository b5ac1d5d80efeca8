"""Device-resident multiple-walker metadynamics: collective variables, a shared bias of Gaussian hills and its forces INSIDE
the replayed hipGraph.

Every other driver of the family samples the unbiased surface; the rare events these potentials are bought for (a vacancy
hop, a bond breaking, a change of coordination) sit behind barriers of many kT that `DeviceMD` never crosses in a run anyone
can afford, and a host-driven bias costs a `fetch()`, a CV code and an upload every step.  `DeviceMetaD` puts a stage of four
launches (csrc/metad_kernels.hip; the definition is csrc/metad_step.h) between the force backward and the unchanged
`hermnet_md_finish`, which integrates with the BIASED forces, so `run(n)` stays free of synchronisation across deposits:

    cvs = [Distance([0], [1]), Coordination(range(32), range(32), r0=2.8, r_cut=5.0)]
    md = DeviceMetaD(model, z, cells, pos, masses, dt=1.0, cvs=cvs, height=0.05, sigma=[0.1, 0.5], pace=50,
                     temperature=300.0, friction=0.01, bias_factor=10.0, batch=batch, num_graphs=4)
    md.run(1000)                # 1000 replays, 20 deposits of 4 hills; returns at once
    s = md.fetch()              # s.hill_count, s.hill_centres [K,D], s.hill_heights [K], s.bias_forces, s.cv_log [rows,B,D+2]
    f = free_energy(s, grid)    # numpy, on the host

The B graphs of the batch are B WALKERS of one system of n_rep = N / B atoms under ONE shared bias (B = 1: ordinary
metadynamics); CVs are written in atom indices of one copy.  The bias is V(s) = sum_k h_k prod_d exp(-(s_d - c_kd)^2 /
(2 sigma_d^2)).  With the state at step s the advance has moved the atoms to x(s+1): CVs, bias force, `cv_log` row and hill
belong to x(s+1).  Every `pace`-th committed step -- (s + 1) % pace == 0 -- each walker appends one hill at its own CV value,
in ascending graph order, of height `height`, or well-tempered `height exp(-V(s) / (kB (bias_factor - 1) T))` with V the bias
the step began with: all walkers of one deposit see the same list.  `f_prev`, `forces` of the snapshot, are biased forces.

Halt protocol, `resume()`, `maxwell_boltzmann`, `zero_momentum`, `observers=`: `DeviceMD`'s.  A void step appends no hill and
writes no row; the prime applies the bias and deposits nothing; a halted or parked replay does nothing.  A restart from
positions, velocities and `hills=` reproduces the uninterrupted run bit for bit where it does not directly follow a deposit
(its prime sees the whole list; the uninterrupted run's next half kick used forces made in front of that deposit).  Both CVs
use the minimum image by rounding the fractional difference, the nearest image below half the smallest cell height: a
`Coordination` refuses a larger `r_cut`, a `Distance` is meant for centres closer than that.

Out of scope: a variable cell or a barostat under bias, the bias contribution to the virial, grids in place of the hill list,
other CVs, independent biases per graph, atom shards."""
import math
import types

import numpy as np
import torch

from . import _lib
from ._resident import host_f64
from .md import KB, CopiesMD, same_copies, stack_atoms
from .observe import rdf_fits

MAX_CVS = 2                               # csrc/metad_step.h: the walker's row holds two CVs
MAX_POWER = 64                            # ... the largest p = nn / 2 the host twins accept
DISTANCE, COORDINATION = 1, 2             # ... MT_DISTANCE, MT_COORDINATION


def _group(name, group, n_rep):
    g = np.asarray(list(group) if not isinstance(group, np.ndarray) else group, dtype=np.int64).reshape(-1)
    if g.size == 0 or len(np.unique(g)) != g.size:
        raise ValueError("%s: a group is a non-empty list of distinct atom indices" % name)
    if g.min() < 0 or g.max() >= n_rep:
        raise ValueError("%s: atom index %d is outside one copy of the system (0 <= index < n_rep = %d): CVs are written in "
                         "the atom indices of ONE walker" % (name, int(g.min() if g.min() < 0 else g.max()), n_rep))
    return g


class Distance(object):
    """The length of the minimum-image vector between the weighted centres of two groups (atom indices of one copy).  The
    centres are those of the UNWRAPPED coordinates x + image @ cell, so a group that straddles the boundary is whole; the
    weights (None: equal) are normalised to sum 1.  The gradient at zero distance is zero."""

    def __init__(self, group_a, group_b, weights_a=None, weights_b=None):
        self.group_a, self.group_b, self.weights_a, self.weights_b = group_a, group_b, weights_a, weights_b

    def _tables(self, n_rep, fits):
        w = np.zeros((2, n_rep))
        for k, (group, weights) in enumerate(((self.group_a, self.weights_a), (self.group_b, self.weights_b))):
            g = _group("Distance", group, n_rep)
            u = np.ones(g.size) if weights is None else host_f64(weights).reshape(-1)
            if u.size != g.size or not np.all(np.isfinite(u)) or not (u.sum() > 0.0):
                raise ValueError("Distance: one finite weight per atom of the group, with a positive sum")
            w[k, g] = u / u.sum()
        return (DISTANCE, 0), np.zeros(8), np.zeros(n_rep, dtype=np.uint8), w


def switch_constants(r0, nn, r_cut):
    """cv_par of csrc/metad_step.h for the rational switch s(w) = 1 / (1 + w^p), w = r^2 / r0^2, p = nn / 2, shifted and
    stretched to reach 0 at r_cut: (1 / r0^2, r_cut^2, s_c, 1 / (1 - s_c), 2 / (r0^2 (1 - s_c))), with s_c = s(w_c) formed by
    the kernel's own operations."""
    inv_r0sq, rc2 = 1.0 / (float(r0) * float(r0)), float(r_cut) * float(r_cut)
    w, wp = rc2 * inv_r0sq, 1.0
    for _ in range(int(nn) // 2):
        wp = wp * w
    s_c = 1.0 / (1.0 + wp)
    inv_norm = 1.0 / (1.0 - s_c)
    return inv_r0sq, rc2, s_c, inv_norm, 2.0 * inv_r0sq * inv_norm


class Coordination(object):
    """sum_{i in A} sum_{j in B, j != i} s~(r_ij) over ordered pairs (A = B counts a pair twice: it is sum_i n_i);
    `mean=True` divides by |A|.  s(w) = 1 / (1 + w^p), w = r^2 / r0^2, p = nn / 2 -- the rational switch with mm = 2 nn,
    which has no singularity and needs no sqrt --, s~ = (s(w) - s(w_c)) / (1 - s(w_c)) below `r_cut` and 0 beyond.
    ValueError: an odd `nn` (the power p = nn / 2 is an integer: powers are multiplications), nn outside 2..128, r_cut <= r0
    or above half the smallest cell height (the minimum image by rounding holds only below it)."""

    def __init__(self, group_a, group_b, r0, nn=6, r_cut=None, mean=False):
        self.group_a, self.group_b, self.r0, self.nn, self.r_cut, self.mean = group_a, group_b, r0, nn, r_cut, bool(mean)

    def _tables(self, n_rep, fits):
        nn = self.nn
        if int(nn) != nn or int(nn) % 2 != 0 or not (2 <= int(nn) <= 2 * MAX_POWER):
            raise ValueError("Coordination: nn = %r -- nn must be even (the switch uses the integer power p = nn / 2, by "
                             "multiplications) and 2 <= nn <= %d" % (nn, 2 * MAX_POWER))
        if self.r_cut is None or not (float(self.r0) > 0.0) or not (float(self.r_cut) > float(self.r0)) \
                or not math.isfinite(float(self.r_cut)):
            raise ValueError("Coordination: r0 > 0 and a finite r_cut= above r0 are required (r0=%r, r_cut=%r)" % (self.r0, self.r_cut))
        ok = fits(float(self.r_cut))
        if not np.all(ok):
            raise ValueError("Coordination: r_cut = %g A is more than half the smallest cell height of graph %d (rounding the "
                             "fractional difference is the minimum image only below it)" % (float(self.r_cut), int(np.argmin(ok))))
        a, b = _group("Coordination", self.group_a, n_rep), _group("Coordination", self.group_b, n_rep)
        role = np.zeros(n_rep, dtype=np.uint8)
        role[a] |= 1
        role[b] |= 2
        par = np.zeros(8)
        par[:5] = switch_constants(self.r0, nn, self.r_cut)
        par[5] = 1.0 / a.size if self.mean else 1.0
        return (COORDINATION, int(nn) // 2), par, role, np.zeros((2, n_rep))


def cv_tables(cvs, n_rep, cell):
    """The host-made tables of the collective variables `cvs` for walkers of `n_rep` atoms in `cell` ([3,3] or [B,3,3]): a
    namespace of `kind` [D,2] int32, `par` [D,8] float64, `role` [D,n_rep] uint8 and `weight` [D,2,n_rep] float64
    (csrc/metad_step.h).  ValueError, naming the limit: no CV or more than 2, anything that is no `Distance` / `Coordination`,
    and what those refuse."""
    cvs = list(cvs) if isinstance(cvs, (list, tuple)) else [cvs]
    if not 1 <= len(cvs) <= MAX_CVS:
        raise ValueError("DeviceMetaD: %d collective variables -- 1 or 2 (at most %d)" % (len(cvs), MAX_CVS))
    if cell is None:
        raise ValueError("DeviceMetaD: cell=None -- the collective variables and the shared bias need a fixed periodic cell")
    c32 = torch.as_tensor(cell).detach().float().cpu().numpy().astype(np.float64).reshape(-1, 3, 3)
    inv = np.linalg.inv(c32)
    fits = lambda r: rdf_fits(r, inv)     # observe.RDF's own check of r_max
    rows = []
    for cv in cvs:
        if not isinstance(cv, (Distance, Coordination)):
            raise ValueError("DeviceMetaD: a collective variable is a Distance or a Coordination, not %r" % (cv,))
        rows.append(cv._tables(int(n_rep), fits))
    return types.SimpleNamespace(kind=np.ascontiguousarray([r[0] for r in rows], dtype=np.int32),
                                 par=np.ascontiguousarray([r[1] for r in rows], dtype=np.float64),
                                 role=np.ascontiguousarray([r[2] for r in rows], dtype=np.uint8),
                                 weight=np.ascontiguousarray([r[3] for r in rows], dtype=np.float64))


def bias_tables(num_cvs, height, sigma, pace, temperature, bias_factor, max_hills, hills):
    """The bias's host-made constants: a namespace of `sigma` [D], `sigma_par` [D,2] = (1 / (2 sigma^2), 1 / sigma^2),
    `height`, `inv_kt` = 1 / (kB (bias_factor - 1) T) (0.0: no tempering), `pace`, `max_hills`, `bias_factor`, and the
    preloaded list `centres` [K,D], `heights` [K].  ValueError, naming the limit, for what the kernels cannot honour."""
    D = int(num_cvs)
    sg = host_f64(sigma).reshape(-1)
    if sg.size != D or not np.all(np.isfinite(sg) & (sg > 0.0)):
        raise ValueError("DeviceMetaD: sigma= is one positive finite width per collective variable (%d)" % D)
    if not math.isfinite(float(height)) or float(height) < 0.0:
        raise ValueError("DeviceMetaD: height must be finite and >= 0")
    if int(pace) != pace or int(pace) < 1 or int(max_hills) != max_hills or int(max_hills) < 1:
        raise ValueError("DeviceMetaD: pace and max_hills are integers >= 1")
    t = host_f64(temperature).reshape(-1)
    if t.size != 1 or not (math.isfinite(t[0]) and t[0] > 0.0):
        raise ValueError("DeviceMetaD: temperature= is one positive finite number (K): the walkers share one bias")
    inv_kt = 0.0
    if bias_factor is not None:
        if not (math.isfinite(float(bias_factor)) and float(bias_factor) > 1.0):
            raise ValueError("DeviceMetaD: bias_factor must be finite and > 1 (None: no tempering)")
        inv_kt = 1.0 / (KB * (float(bias_factor) - 1.0) * float(t[0]))
    centres, heights = np.zeros((0, D)), np.zeros(0)
    if hills is not None:
        centres, heights = host_f64(hills[0]).reshape(-1, D).copy(), host_f64(hills[1]).reshape(-1).copy()
        if len(centres) != len(heights) or not (np.all(np.isfinite(centres)) and np.all(np.isfinite(heights))):
            raise ValueError("DeviceMetaD: hills=(centres [K,%d], heights [K]), finite" % D)
        if len(heights) > int(max_hills):
            raise ValueError("DeviceMetaD: hills= holds %d hills, more than max_hills = %d" % (len(heights), int(max_hills)))
    return types.SimpleNamespace(sigma=sg.copy(), sigma_par=np.ascontiguousarray(np.stack([1.0 / (2.0 * sg * sg), 1.0 / (sg * sg)], axis=1)),
                                 height=float(height), inv_kt=inv_kt, pace=int(pace), max_hills=int(max_hills),
                                 bias_factor=None if bias_factor is None else float(bias_factor), centres=centres, heights=heights)


def deposits_within(step, n, pace, walkers):
    """Hills that `n` more committed steps behind `step` completed ones append: `walkers` per multiple of `pace` in
    (step, step + n]."""
    return int(walkers) * ((int(step) + int(n)) // int(pace) - int(step) // int(pace))


def refuse_overflow(name, n, step, pending, pace, walkers, known, max_hills):
    """RuntimeError where `run(n)` could append beyond `max_hills`: `known` hills at the last fetch (at `step`), `pending`
    replays enqueued since."""
    due = known + deposits_within(step, pending + n, pace, walkers)
    if due > max_hills:
        raise RuntimeError("%s.run(%d) would deposit beyond the hill list (%d hills known, up to %d due, max_hills=%d): "
                           "construct with a larger max_hills= (hills= carries the list over)" % (name, n, known, due, max_hills))


class DeviceMetaD(CopiesMD):
    """See the module docstring.  model, atomic_number [N], cell [B,3,3] ([3,3] with `batch=None`: one walker), pos [N,3],
    masses [N], dt, `batch` [N] with `num_graphs` = B, `seed`, `velocities`, `capacity`, `log_steps`, `wrap`,
    `reference_compat`, `device`, `observers`: `DeviceMD`'s; the B graphs are the walkers.  `cvs`: a list of 1 or 2 `Distance`
    / `Coordination`.  `height` (eV), `sigma` [D] (the CVs' units), `pace` (steps between deposits), `temperature` (K, one
    number; the thermostat's with `friction=`, the tempering's with `bias_factor=`), `friction=None`: NVE, else Langevin;
    `bias_factor=None`: plain metadynamics, else well-tempered; `max_hills`: the list's room; `hills=(centres, heights)`: a
    preloaded list (a restart, or a fixed bias where `pace` exceeds the run).

    ValueError / RuntimeError, naming the limit: `cell=None`; a barostat's arguments (the cell is fixed); more than 2 CVs;
    what `Distance` / `Coordination` refuse; walkers that differ in atom count, atomic numbers, masses or cell; `hills=`
    beyond `max_hills`; and `run(n)` whose deposits -- B per committed multiple of `pace` -- could exceed `max_hills`.

    `fetch()`: `DeviceMD`'s snapshot (`forces`: the biased ones), and `hill_count`, `hill_centres` [K,D], `hill_heights` [K],
    `bias_forces` [N,3] float64 (of the last evaluation), `cv_log` [rows,B,D+2] = (s_1..s_D, V(s), height deposited this
    step or 0) per time step since the last fetch, `sigma` [D] and `bias_factor` (what `bias_on_grid` / `free_energy` read)."""

    __slots__ = ("cvs", "tables", "bias", "cv_kind", "cv_par", "cv_role", "cv_weight", "sigma_par", "cv_atom", "cv_walker",
                 "hill_count", "hill_centres", "hill_heights", "forces_b", "bias_forces", "cv_log", "_known", "_sent")

    def __init__(self, model, atomic_number, cell, pos, masses, dt, cvs, height, sigma, pace, temperature, friction=None,
                 bias_factor=None, max_hills=16384, hills=None, batch=None, num_graphs=None, seed=0, **kw):
        for word in ("pressure", "compressibility", "taup", "coupling", "mask", "max_strain"):
            if word in kw:
                raise ValueError("DeviceMetaD: %s= is a barostat's -- the cell is fixed under the bias (a variable cell is out of "
                                 "scope)" % word)
        if cell is None:
            raise ValueError("DeviceMetaD: cell=None -- the collective variables and the shared bias need a fixed periodic cell")
        z = torch.as_tensor(atomic_number).reshape(-1)
        if batch is None:
            B, self.n_rep = 1, int(z.numel())
        else:
            batch_h = np.asarray(torch.as_tensor(batch).cpu(), dtype=np.int64).reshape(-1)
            B = int(num_graphs if num_graphs is not None else batch_h[-1] + 1)
            self.n_rep = same_copies("DeviceMetaD", "walker", atomic_number, cell, masses, batch_h, B)
        self.cvs = list(cvs) if isinstance(cvs, (list, tuple)) else [cvs]     # as given
        self.tables = cv_tables(self.cvs, self.n_rep, cell)                   # on the host
        self.bias = bias_tables(len(self.cvs), height, sigma, pace, temperature, bias_factor, max_hills, hills)   # on the host
        super().__init__(model, atomic_number, cell, pos, masses, dt, temperature=float(host_f64(temperature).reshape(-1)[0]),
                         friction=friction, seed=seed, batch=batch, num_graphs=None if batch is None else B, **kw)

    def _own_state(self, masses):
        super()._own_state(masses)
        n, B, D, dev, tb, bs = self.n, self.num_graphs, len(self.cvs), self.device, self.tables, self.bias
        put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.cv_kind, self.cv_par, self.cv_role, self.cv_weight = put(tb.kind), put(tb.par), put(tb.role), put(tb.weight)
        self.sigma_par = put(bs.sigma_par)                                # [D,2] f64
        self.cv_atom = torch.zeros(D, n, 6, dtype=torch.float64, device=dev)          # scratch; the per-atom pass
        self.cv_walker = torch.zeros(B, 16, dtype=torch.float64, device=dev)          # scratch; the walkers' kernel
        K = len(bs.heights)
        self.hill_count = torch.tensor([K], dtype=torch.int64).to(dev)    # the deposit kernel
        self.hill_centres = torch.zeros(bs.max_hills, D, dtype=torch.float64, device=dev)     # the deposit kernel
        self.hill_heights = torch.zeros(bs.max_hills, dtype=torch.float64, device=dev)        # the deposit kernel
        if K:
            self.hill_centres[:K].copy_(torch.from_numpy(bs.centres))
            self.hill_heights[:K].copy_(torch.from_numpy(bs.heights))
        self.forces_b = torch.zeros(n, 3, dtype=torch.float32, device=dev)            # what the finish reads; the apply kernel
        self.bias_forces = torch.zeros(n, 3, dtype=torch.float64, device=dev)         # the apply kernel
        self.cv_log = torch.zeros(self.log_steps, B, D + 2, dtype=torch.float64, device=dev)      # the walkers' kernel
        self._known = K                   # `fetch`: the hills counted at its snapshot
        self._sent = (0, 0)               # `_fetch_extras`: (hills, rows) the packed copy carries

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        cell, B, bs = step.cell, self.num_graphs, self.bias
        if cell is None or cell.dtype != torch.float32 or not cell.is_contiguous() or cell.numel() != 9 * B:
            raise RuntimeError("DeviceMetaD: the step's cell must be a contiguous float32 [B,3,3]")
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.call("hermnet_metad_bias", self.n, B, len(self.cvs), P(self.graph_ptr), P(self.x), P(self.image), P(cell),
                  P(self._inverse_of(cell)), P(self.cv_kind), P(self.cv_par), P(self.cv_role), P(self.cv_weight),
                  P(self.sigma_par), bs.height, bs.inv_kt, bs.pace, bs.max_hills, P(forces), P(energy), P(total),
                  int(step.capacity), P(self.state), P(self.cv_atom), P(self.cv_walker), P(self.hill_count),
                  P(self.hill_centres), P(self.hill_heights), P(self.forces_b), P(self.bias_forces), P(self.cv_log),
                  self.log_steps, stream)
        _lib.call("hermnet_md_finish", self.n, B, P(self.graph_ptr), P(self.forces_b), P(energy), P(total), int(step.capacity),
                  *self._finish_atoms(step), *self._finish_tail())

    def run(self, n):
        """`DeviceMD.run`; also refuses an `n` whose deposits could exceed `max_hills`."""
        refuse_overflow(type(self).__name__, int(n), self._logged, self._pending, self.bias.pace, self.num_graphs, self._known,
                        self.bias.max_hills)
        super().run(n)

    def resume(self):
        """`DeviceMD.resume`, and the last accepted forces stay (as `DeviceNPT.resume` keeps them): they were biased by the
        list as it stood in front of the last step's own deposit, the recapture's prime sees the whole list -- the next
        step's first kick is the one an uninterrupted run makes.  (After a change of weights that one half kick still uses
        the old weights' forces.)"""
        f = self.f_prev.clone()
        super().resume()
        self.f_prev.copy_(f)

    # ---- the packed fetch's own part ------------------------------------------------------------------------------------------
    def _fetch_extras(self):
        rows = self._pending
        K = min(self.bias.max_hills, self._known + deposits_within(self._logged, rows, self.bias.pace, self.num_graphs))
        self._sent = (K, rows)
        idx = (torch.arange(rows, device=self.device) + self._logged) % self.log_steps
        return [self.hill_count, self.hill_centres[:K], self.hill_heights[:K], self.bias_forces, self.cv_log.index_select(0, idx)]

    def _read_extras(self, s, word, h):
        (K, rows), D, n, B = self._sent, len(self.cvs), self.n, self.num_graphs
        count = s.hill_count = int(h[0])
        assert 0 <= count <= K, (count, K)
        s.hill_centres = h[1:1 + K * D].reshape(K, D)[:count].copy()
        s.hill_heights = h[1 + K * D:1 + K * D + K][:count].copy()
        o = 1 + K * D + K
        s.bias_forces = h[o:o + 3 * n].reshape(n, 3).copy()
        done = max(0, min(rows, s.step - self._logged))
        s.cv_log = h[o + 3 * n:o + 3 * n + rows * B * (D + 2)].reshape(rows, B, D + 2)[:done].copy()
        s.sigma, s.bias_factor = self.bias.sigma.copy(), self.bias.bias_factor
        self._known = count

    # ---- ASE hand-off (duck-typed) ------------------------------------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, atoms, model, dt, cvs, height, sigma, pace, temperature, walkers=None, device="cuda:0", **kw):
        """`atoms`: one periodic structure, replicated into `walkers` graphs, or the list of the B walkers (then `walkers` is
        None or B) -- what `md.stack_atoms` takes."""
        if isinstance(atoms, (list, tuple)):
            members = list(atoms)
            if not members or (walkers is not None and int(walkers) != len(members)):
                raise ValueError("DeviceMetaD.from_atoms: a list of the B walkers (walkers=%r, %d given)" % (walkers, len(members)))
        else:
            if walkers is None or int(walkers) < 1:
                raise ValueError("DeviceMetaD.from_atoms: walkers >= 1")
            members = [atoms] * int(walkers)
        dev = torch.device(device)
        s = stack_atoms(members, "DeviceMetaD.from_atoms", "walkers", dev)
        return cls(model, s.z, s.cell, s.pos, s.masses, dt, cvs, height, sigma, pace, temperature, batch=s.batch,
                   num_graphs=len(members), velocities=s.velocities, device=dev, **kw)

    def to_atoms(self, walkers, snapshot=None):
        """Write positions (wrapped) and velocities (ASE units) of `snapshot` (default: a fetch()) into the list `walkers`,
        entry g taking walker g.  Returns the snapshot."""
        s = snapshot if snapshot is not None else self.fetch()
        if not isinstance(walkers, (list, tuple)) or len(walkers) != self.num_graphs:
            raise ValueError("DeviceMetaD.to_atoms: a list of %d walkers" % self.num_graphs)
        for g, atoms in enumerate(walkers):
            self._write_member(atoms, s, g)
        return s


# ---- host helpers (numpy only) ----------------------------------------------------------------------------------------------------
def bias_on_grid(snapshot, grid):
    """V [G] of the hill list of `snapshot` (`hill_centres` [K,D], `hill_heights` [K], `sigma` [D]) at the points `grid`
    [G,D] ([G] for one CV)."""
    sg = np.asarray(snapshot.sigma, dtype=np.float64).reshape(-1)
    pts = np.asarray(grid, dtype=np.float64).reshape(-1, sg.size)
    c, h = np.asarray(snapshot.hill_centres, dtype=np.float64).reshape(-1, sg.size), np.asarray(snapshot.hill_heights, dtype=np.float64)
    v = np.zeros(len(pts))
    for lo in range(0, len(c), 4096):     # (blocks of hills: the [G,K] table stays small)
        d = (pts[:, None, :] - c[None, lo:lo + 4096, :]) / sg
        v += np.exp(-0.5 * (d * d).sum(axis=2)) @ h[lo:lo + 4096]
    return v


def free_energy(snapshot, grid):
    """The free-energy estimate on `grid`, up to a constant: -gamma / (gamma - 1) V for a well-tempered run
    (`snapshot.bias_factor` = gamma), -V without tempering."""
    gamma = getattr(snapshot, "bias_factor", None)
    v = bias_on_grid(snapshot, grid)
    return -v if gamma is None else -(gamma / (gamma - 1.0)) * v
