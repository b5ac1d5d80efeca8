"""Device-resident NPT that samples the isothermal-isobaric ensemble: a Nose-Hoover (Martyna-Tobias-Klein) barostat with
Nose-Hoover chains on the particles and on the barostat, INSIDE the replayed hipGraph.

`DeviceNPT`'s Berendsen barostat relaxes a cell to a target pressure but its volume fluctuations are not the ensemble's, so
nothing read from V(t) -- compressibilities, thermal-expansion statistics -- is right.  `DeviceMTK` integrates the extended
system of Martyna, Tobias and Klein in the measure-preserving, time-reversible splitting of Tuckerman, Alejandre,
Lopez-Rendon, Jochim and Martyna (J. Phys. A 39, 5629 (2006); LAMMPS: `fix npt iso` / `aniso`):

    md = DeviceMTK(model, z, cell, pos, masses, dt=1.0, temperature=300.0, pressure=1.0 * GPA, tau=100.0, taup=1000.0)
    md.maxwell_boltzmann(300.0); md.zero_momentum()
    md.run(1000)
    s = md.fetch()                  # s.cell [B,3,3] f64, s.volume, s.v_cell [B,3], s.xi_baro ..., s.log [rows,B,7]
    h = conserved(s)                # E_pot + E_kin + E_nhc (both chains) + P0 V + W v_g^2 / 2: constant up to O(dt^2)

It is a `DeviceNHC` (the particles' chain is that driver's, unchanged) with, per graph, a barostat velocity `v_cell` [3] --
the diagonal of the cell's rate in Cartesian axes; "isotropic": one number three times; "axes": the entries outside `mask`
stay 0 -- of mass W = (dof + 3) kB T taup^2 (a third of that per axis under "axes"), and a second chain of the same length,
order and substeps on the barostat.  One time step, every half of length dt / 2:

    NHC_baro . NHC_particles . baro-kick | scaled kick . scaled drift . cell | [search, forces, virial in the NEW cell] |
    scaled kick | baro-kick . NHC_particles . NHC_baro

`hermnet_mtk_advance` / `hermnet_mtk_finish` (csrc/mtk_kernels.hip; the definition, operation by operation, is
csrc/mtk_step.h) are the capture's two hooks: two launches in front of the search -- the cell moves BEFORE the search reads
it -- and four behind the virial.  The float64 cell is the truth, the step's float32 cell its rounding, the wrap's inverse
that of the widened float32 cell, as under `DeviceNPT`.  The barostat's half kicks use the virial of the last accepted
evaluation (`w_prev`, kept the way the forces are), so there is one evaluation per step and `resume()` needs no exception:
the prime's forces and virial are exactly what the next step reads.

Limits that hold bit for bit: `taup=inf` never moves or writes the cell and is `DeviceNHC`; `tau=inf` switches both chains
off (NPH); both: `DeviceMD`'s NVE.

Void steps: a step whose barostat asks for more than `max_strain` (|v_cell| dt, per axis) or whose factors or virial are not
finite is VOID like one with an incomplete list -- the search never reads a cell that is not finite; atoms, cell, v_cell and
both chains return, the halt (code 256) is recorded, `refused` counts the graph.

Out of scope: open structures, the fully flexible cell (matrix exponentials), atom shards, HTNet, combination with the other
drivers."""
import numpy as np
import torch

from . import _lib
from ._resident import HN_MD_WRAP, host_f64, per_graph
from .md import GPA, HN_MD_BARO, KB, _det3  # noqa: F401  (GPA: for callers)
from .nhc import DeviceNHC

LOG_WIDTH = 7
COUPLINGS = ("isotropic", "axes")


def baro_tables(temperature, tau, taup, dof, pressure, coupling, mask, chain):
    """What the kernels read of the barostat, made once in float64 on the host: (par [B,5] = (w, 1 / w, 1 + 3 / dof, 1 / dof,
    P0), dof_kt_b [B], q_b [B,M], inv_q_b [B,M]); `temperature`, `tau`, `taup`, `dof`, `pressure` are [B], `mask` the bits of
    the coupled axes.  taup = inf: w = 1 / w = 0 and the barostat's chain is off; tau = inf: that chain is off."""
    kt = KB * np.asarray(temperature, dtype=np.float64)
    dof = np.asarray(dof, dtype=np.float64)
    tau, taup = np.asarray(tau, dtype=np.float64), np.asarray(taup, dtype=np.float64)
    moves = np.isfinite(taup)
    taup2 = np.where(moves, taup, 1.0) ** 2
    w = (dof + 3.0) * kt * taup2
    if coupling == "axes":
        w = w / 3.0
    w = np.where(moves, w, 0.0)
    with np.errstate(divide="ignore"):
        inv_w = np.where(moves, 1.0 / w, 0.0)
    par = np.stack([w, inv_w, 1.0 + 3.0 / dof, 1.0 / dof, np.asarray(pressure, dtype=np.float64)], axis=1)
    dof_b = 1.0 if coupling == "isotropic" else float(bin(mask).count("1"))
    dof_kt_b = dof_b * kt
    on = moves & np.isfinite(tau)
    q = np.repeat((kt * taup2)[:, None], chain, axis=1)
    q[:, 0] = dof_kt_b * taup2
    q = np.where(on[:, None], q, 0.0)
    with np.errstate(divide="ignore"):
        inv_q = np.where(on[:, None], 1.0 / q, 0.0)
    return tuple(np.ascontiguousarray(a, dtype=np.float64) for a in (par, dof_kt_b, q, inv_q))


def conserved(snapshot):
    """E_pot + E_kin + E_nhc (both chains) + (P0 V + W v_g^2 / 2) [rows,B] of a `DeviceMTK.fetch()` snapshot's log: the
    extended energy the scheme conserves."""
    log = snapshot.log
    return ((log[..., 0] + log[..., 1]) + log[..., 3]) + log[..., 6]


class DeviceMTK(DeviceNHC):
    """See the module docstring.  Everything `DeviceNHC` takes (`temperature`, `tau`, `chain`, `order`, `substeps`, `dof`),
    `cell` (required; float64 is kept) and `pressure` (the target, eV/A^3; `GPA` converts), `taup` (fs; inf: the barostat is
    off) -- scalars or [B]: replicas at different state points share one capture --, `coupling` ("isotropic" or "axes"),
    `mask` ("axes": the Cartesian axes that are coupled) and `max_strain` (the largest |v_cell| dt of one step, in (0, 0.1]).

    ValueError, with the reason: `DeviceNHC`'s refusals; `taup <= 0`; a pressure that is not finite; a `coupling` that is
    not offered; "axes" with an empty mask; `max_strain` outside (0, 0.1].  RuntimeError: `cell=None`.

    `fetch()`: `DeviceNHC`'s snapshot in the same ONE packed copy, and `cell` [B,3,3] float64, `volume` [B], `v_cell` [B,3],
    `xi_baro`, `v_xi_baro` [B,M], `nhc_scale_baro` [B,2], `mtk_factors` [B,12] (the last step's a, b, rx, rv), `refused` [B].
    `log` [rows,B,7] = (E_pot, E_kin behind the closing factor, edges found, E_nhc of both chains, pressure tr P / 3 at the end
    of the step, volume, E_baro = P0 V + W sum v_cell^2 / 2); `conserved(snapshot)` adds columns 0, 1, 3 and 6."""

    __slots__ = ("pressure", "taup", "coupling", "mask", "max_strain", "cell64", "par", "dof_kt_b", "q_b", "inv_q_b", "xi_b",
                 "v_xi_b", "scale_b", "v_cell", "w_prev", "factors", "backup", "flag", "refused", "e_code", "_cell_given")
    LOG_WIDTH = LOG_WIDTH

    def __init__(self, model, atomic_number, cell, pos, masses, dt, temperature=None, pressure=0.0, tau=100.0, taup=1000.0,
                 coupling="isotropic", mask=(1, 1, 1), chain=3, order=3, substeps=1, dof=None, max_strain=1e-2, batch=None,
                 num_graphs=None, **kw):
        if cell is None:
            raise RuntimeError("DeviceMTK: a barostat needs periodic cells (cell=None, open structures, have no volume)")
        if coupling not in COUPLINGS:
            raise ValueError("DeviceMTK: coupling is one of %s (the fully flexible cell is not offered)" % (COUPLINGS,))
        if len(tuple(mask)) != 3:
            raise ValueError("DeviceMTK: mask has three entries")
        bits = 7 if coupling == "isotropic" else sum(1 << k for k, on in enumerate(tuple(mask)) if on)
        if bits == 0:
            raise ValueError('DeviceMTK: coupling="axes" with an empty mask couples nothing (taup=inf switches a barostat off)')
        if not np.all(host_f64(taup) > 0.0):
            raise ValueError("DeviceMTK: taup (fs) must be > 0 (inf: the barostat is off)")
        if not np.all(np.isfinite(host_f64(pressure))):
            raise ValueError("DeviceMTK: the pressure (eV/A^3) must be finite")
        if not 0.0 < float(max_strain) <= 0.1:
            raise ValueError("DeviceMTK: max_strain must lie in (0, 0.1] (the sinhc polynomial of the kernels is exact there)")
        self.pressure, self.taup = pressure, taup         # as given
        self.coupling, self.mask = coupling, bits         # "isotropic" or "axes"; bit k = axis k is coupled
        self.max_strain = float(max_strain)               # the largest |v_cell| dt of a step that is not refused
        self._cell_given = cell                           # `_own_state` makes cell64 of it
        super().__init__(model, atomic_number, cell, pos, masses, dt, temperature=temperature, tau=tau, chain=chain,
                         order=order, substeps=substeps, dof=dof, batch=batch, num_graphs=num_graphs, **kw)

    def _own_state(self, masses):
        """`DeviceNHC`'s, then the barostat's: the tables of `baro_tables`, the cell in float64 with the inverse of its
        rounding, and the state, zeros."""
        super()._own_state(masses)
        B, M, dev = self.num_graphs, self.chain, self.device
        tables = baro_tables(per_graph(self.temperature, B), per_graph(self.tau, B), per_graph(self.taup, B), self.dof,
                             per_graph(self.pressure, B), self.coupling, self.mask, M)
        self.par, self.dof_kt_b, self.q_b, self.inv_q_b = (torch.from_numpy(a).to(dev) for a in tables)
        cell = host_f64(self._cell_given).reshape(B, 3, 3).copy()
        self._cell_given = None
        self.cell64 = torch.from_numpy(cell).to(dev)      # the cell [B,3,3] f64: the truth; the advance's graph kernel
        # of the f32 cell, made as `ResidentDriver._inverse_of` makes it: a graph whose cell never moves is DeviceNHC's by bits
        inv = np.linalg.inv(cell.astype(np.float32).astype(np.float64))
        self.inv_cell = torch.from_numpy(np.ascontiguousarray(inv)).to(dev)           # the advance's graph kernel
        f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
        self.xi_b, self.v_xi_b = f64(B, M), f64(B, M)     # the barostat's chain [B,M]; the two graph kernels
        self.scale_b = torch.ones(B, 2, dtype=torch.float64, device=dev)              # its last opening / closing factor
        self.v_cell = f64(B, 3)                           # the barostat's velocity; the two graph kernels
        self.w_prev = torch.zeros(B, 9, dtype=torch.float32, device=dev)              # the last ACCEPTED virial; finish
        self.factors = torch.ones(B, 12, dtype=torch.float64, device=dev)             # a, b, rx, rv of the step; advance
        self.backup = f64(B, 2 * M + 30)                  # barostat, its chain and the cell at the start of the step; advance
        self.flag = torch.zeros(B, dtype=torch.int64, device=dev)                     # the step's factors were refused; advance
        self.refused = torch.zeros(B, dtype=torch.int64, device=dev)                  # how often; finish
        self.e_code = torch.zeros(B, dtype=torch.float32, device=dev)                 # the commit kernel's energies; finish

    def _step_options(self, single):
        return dict(stress=True, variable_cell=True) if single else dict(stress=True)

    def _inverse_of(self, cell):
        return self.inv_cell              # device state: the advance rewrites it with the cell

    def _baro_args(self, step):
        """The barostat's twenty arguments, in the order of the C boundary; cell32 is the tensor the search reads."""
        cell, P = step.cell, _lib.ptr
        if cell is None or cell.dtype != torch.float32 or not cell.is_contiguous() or cell.numel() != 9 * self.num_graphs:
            raise RuntimeError("DeviceMTK: the step's cell must be a contiguous float32 [B,3,3]")
        return (HN_MD_BARO[self.coupling], self.mask, self.max_strain, P(self.par), P(self.dof_kt_b), P(self.q_b),
                P(self.inv_q_b), P(self.xi_b), P(self.v_xi_b), P(self.scale_b), P(self.v_cell), P(self.cell64), P(cell),
                P(self.inv_cell), P(self.w_prev), P(self.factors), P(self.backup), P(self.flag), P(self.refused),
                P(self.e_code))

    def _advance(self, step):
        P = _lib.ptr
        flags = (self.flags | HN_MD_WRAP) if self.wrap else (self.flags & ~HN_MD_WRAP)
        _lib.call("hermnet_mtk_advance", self.n, self.num_graphs, flags, self.dt, *self._advance_atoms(), P(self.batch),
                  P(self._pos_input(step)), P(self.state), P(self.graph_ptr), P(self.half_mass), *self._tables,
                  *self._baro_args(step), torch.cuda.current_stream(self.device).cuda_stream)

    def _finish(self, step, out):
        P = _lib.ptr
        energy, forces, total = self._step_outputs(out)
        virial = out[2]
        if virial.dtype != torch.float32 or not virial.is_contiguous() or virial.numel() != 9 * self.num_graphs:
            raise RuntimeError("DeviceMTK: the captured step must return a contiguous float32 virial [B,3,3]")
        _lib.call("hermnet_mtk_finish", self.n, self.num_graphs, P(self.graph_ptr), P(self.batch), P(forces), P(energy),
                  P(virial), P(total), int(step.capacity), self.dt, *self._finish_atoms(step), *self._tables,
                  *self._baro_args(step), *self._finish_tail())

    # ---- the packed fetch's own part ------------------------------------------------------------------------------------------
    def _fetch_extras(self):
        return super()._fetch_extras() + [self.cell64, self.v_cell, self.xi_b, self.v_xi_b, self.scale_b, self.factors,
                                          self.refused]

    def _read_extras(self, s, word, h):
        B, M = self.num_graphs, self.chain
        super()._read_extras(s, word, h)
        o = 2 * B * M + 2 * B

        def take(*shape):
            nonlocal o
            size = int(np.prod(shape))
            o += size
            return h[o - size:o].reshape(shape).copy()

        s.cell, s.v_cell = take(B, 3, 3), take(B, 3)
        s.xi_baro, s.v_xi_baro, s.nhc_scale_baro = take(B, M), take(B, M), take(B, 2)
        s.mtk_factors, s.refused = take(B, 12), take(B).astype(np.int64)
        s.volume = np.abs(_det3(s.cell))

    # ---- ASE hand-off ---------------------------------------------------------------------------------------------------------
    CELLS_FLOAT64 = True                  # `_own_state` makes cell64 of it

    def to_atoms(self, atoms, snapshot=None):
        """`DeviceMD.to_atoms`, and the cell (one structure) -- written first and without moving the atoms: the positions
        are already those of the moved cell."""
        s = snapshot if snapshot is not None else self.fetch()
        if self.num_graphs != 1:
            raise ValueError("DeviceMTK.to_atoms: one structure (a batch: take `cell` and `positions` of the snapshot)")
        if hasattr(atoms, "set_cell"):
            atoms.set_cell(s.cell[0].copy(), scale_atoms=False)
        else:
            atoms.cell = s.cell[0].copy()
        return super().to_atoms(atoms, s)
