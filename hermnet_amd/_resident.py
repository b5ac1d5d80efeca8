"""The device-resident drivers' common base (md.DeviceMD, relax.DeviceRelax): `ResidentDriver` owns everything that makes
a driver resident -- the float64 state on the device, the parked `state` words, the log ring, the graphed step captured
between the driver's two hooks, `run` / `fetch` / `resume` and the reaction to a fetched halt code.  A subclass adds its own
arrays, its two hooks (`_advance`, `_finish`: the launches of its kernels), what follows a capture (`_unpark`) and the extra
tensors of its packed `fetch()`.  The step protocol the kernels keep is stated in csrc/resident_step.h.  The MD drivers also
take observers (observe.py: frames, g(r), MSD): launched behind the finish, checked by `run`, carried by the same `fetch()`.

Also here, for `graph.GraphedMDStep.fetch` and `plugin/ase_interface` too: the one packed device-to-host copy with its one
synchronisation (`fetch_packed`), the reaction to a list's flags (`list_flags_seen`) and the once-per-model NaN warning
(`warn_nan_once`)."""
import types
import warnings

import numpy as np
import torch

from ._lib import HN_MD_LANGEVIN, HN_MD_WRAP  # noqa: F401  (md.py, relax.py: the advance flags)
from ._lib import HN_MD_HALT_NONFINITE as HALT_NONFINITE  # halt code: an energy that is not finite

HALT_CAPACITY = 4                         # ... list flag bit 2: more pairs than columns
PARKED = 1 << 20                          # host-side halt code while a capture is made: its replays must not move anything


def host_f64(a):
    """A tensor or array-like as a float64 array on the host."""
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)


def per_graph(a, num_graphs):
    """A scalar or [B] (tensor or array-like) as a float64 [B] array of its own."""
    t = host_f64(a)
    return np.broadcast_to(t.reshape(-1) if t.ndim else t, (num_graphs,)).copy()


def fetch_packed(packed, host, room=None):
    """`packed` (float64, on the device) through ONE copy and ONE synchronisation: (a numpy view of its values in the pinned
    buffer, the buffer to keep for the next call).  `host`: that buffer or None; `room`: the elements a new one gets (the
    largest this caller can fetch; default: this fetch's)."""
    if host is None or host.numel() < packed.numel():
        host = torch.empty(room if room is not None else packed.numel(), dtype=torch.float64).pin_memory()
    view = host[:packed.numel()]
    view.copy_(packed, non_blocking=True)
    torch.cuda.current_stream(packed.device).synchronize()
    return view.numpy(), host


def list_flags_seen(flags, device):
    """What a fetch does about the neighbour list's flags it read: a stash overflow enlarges the next search's stash."""
    if flags & 2:
        from .neighbor import _stash_overflowed
        _stash_overflowed(device)


def warn_nan_once(model, message, stacklevel):
    """`message` as a RuntimeWarning, once per model (`stacklevel`: as if the caller had called `warnings.warn`)."""
    if not model.__dict__.get("_warned_nan_repair"):
        model.__dict__["_warned_nan_repair"] = True
        warnings.warn(message, RuntimeWarning, stacklevel=stacklevel + 1)


class ResidentDriver(object):
    """See the module docstring.  Every field is written by `_start` (during construction) unless its line names another
    writer; the kernels' writes are those of one replay.  Undeclared fields raise.  A subclass provides `_own_state(**own)`
    (its arrays, from its own constructor arguments; n, num_graphs, _batch_h, x ... exist, the capture follows), the hooks
    `_advance(step)` in front of the search and `_finish(step, out)` behind the force backward, and `_unpark()` (what follows
    a capture: the halt words cleared, the state ready for `run`)."""

    __slots__ = ("device", "model", "z", "n", "num_graphs", "_batch_h", "batch", "graph_ptr", "x", "x0", "v", "image",
                 "image0", "f_prev", "state", "log", "log_steps", "wrap", "inv_cell", "_inv_of", "step", "_logged", "_pending",
                 "_host", "_observers")
    LOG_WIDTH = None                      # columns of a log row: the subclass's

    def _start(self, model, atomic_number, cell, pos, batch, num_graphs, capacity, log_steps, wrap, reference_compat, device,
               observers=None, **own):
        """The constructor: the common state, the subclass's (`_own_state(**own)`), the observers' (`observers`: the MD
        drivers'), then the capture between its hooks.  The state stays parked; the subclass unparks it."""
        from .graph import GraphedBatchMDStep, GraphedMDStep
        name = type(self).__name__
        dev = torch.device(device) if device is not None else (pos.device if torch.is_tensor(pos) else torch.device("cuda:0"))
        if dev.type != "cuda":
            raise RuntimeError("%s needs GPU tensors" % name)
        self.device = dev                 # the GPU everything lives on
        self.model = model                # the HVNet of the captured step; `_after_halt` drops its caches
        self.z = torch.as_tensor(atomic_number).long().to(dev)    # atomic numbers [N]
        n = self.n = int(self.z.numel())  # atoms
        self.num_graphs = 1 if batch is None else int(num_graphs if num_graphs is not None else int(torch.as_tensor(batch)[-1]) + 1)
        B = self.num_graphs               # structures in the batch
        batch_h = np.zeros(n, dtype=np.int64) if batch is None else np.asarray(torch.as_tensor(batch).cpu(), dtype=np.int64)
        if batch_h.shape != (n,) or np.any(np.diff(batch_h) < 0) or (n and (batch_h[0] < 0 or batch_h[-1] >= B)):
            raise ValueError("%s: batch must be [N], non-decreasing, in [0, num_graphs)" % name)
        self._batch_h = batch_h           # `batch` on the host (zeros for one structure)
        self.batch = None if batch is None else torch.from_numpy(batch_h).to(dev)     # [N] int64, None: one structure
        self.graph_ptr = torch.from_numpy(np.searchsorted(batch_h, np.arange(B + 1)).astype(np.int32)).to(dev)    # [B+1] int32
        self.x = torch.as_tensor(host_f64(pos)).reshape(n, 3).contiguous().to(dev)    # coordinates [N,3] f64; advance, void finish
        self.x0 = torch.zeros_like(self.x)                                            # x at the start of the step; advance
        self.v = torch.zeros(n, 3, dtype=torch.float64, device=dev)                   # velocities [N,3] f64; the kernels
        self.image = torch.zeros(n, 3, dtype=torch.int32, device=dev)                 # lattice vectors removed; advance, void finish
        self.image0 = torch.zeros_like(self.image)                                    # image at the start of the step; advance
        self.f_prev = torch.zeros(n, 3, dtype=torch.float32, device=dev)              # the last ACCEPTED forces; finish
        self.state = torch.tensor([0, PARKED, 0, 0], dtype=torch.int64).to(dev)       # finish's last kernel; `resume`, `_unpark`
        self.log_steps = int(log_steps)   # rows of the ring
        self.log = torch.zeros(self.log_steps, B, self.LOG_WIDTH, dtype=torch.float64, device=dev)    # finish: row step % log_steps
        self.wrap = bool(wrap)            # wrap coordinates into the cell where the step has one
        self.inv_cell = self._inv_of = None     # `_inverse_of`: the float64 inverse [B,3,3] and the cell tensor it was made of
        self._logged = self._pending = 0  # `fetch`: the step its last snapshot stood at; `run`, `fetch`: replays enqueued since
        self._host = None                 # `fetch`: the pinned buffer
        self._own_state(**own)
        self._observers = tuple(observers or ())    # observe.py's Frames / RDF / MSD behind the finish (md.DeviceMD: observers=)
        for ob in self._observers:
            ob._bind(self, cell)
        # the captured step: advance -> the graphed step's own _eager() -> finish (-> the observers, where there are any)
        cell_t = None if cell is None else torch.as_tensor(cell).detach().float().to(dev).contiguous()
        kw = dict(capacity=capacity, reference_compat=reference_compat,
                  hooks=(self._advance, self._finish_observed if self._observers else self._finish))
        kw.update(self._step_options(batch is None))
        if batch is None:
            if cell_t is None:
                raise RuntimeError("%s: one structure needs a periodic cell (open structures: batch=, cell=None)" % name)
            self.step = GraphedMDStep(model, self.z, cell_t.reshape(3, 3), self.x.float(), **kw)
        else:
            self.step = GraphedBatchMDStep(model, self.z, cell_t, self.x.float(), self.batch, B, **kw)

    def _finish_observed(self, step, out):
        """The capture's second hook where there are observers: the finish, then each observer's launches (they read the
        state the finish's commit kernel left)."""
        self._finish(step, out)
        for ob in self._observers:
            ob._launch(self, step)

    # ---- what the two hooks of the capture check and pass on ----------------------------------------------------------------
    def _pos_input(self, step):
        """The step's float32 coordinate input, checked."""
        if step.pos.dtype != torch.float32 or not step.pos.is_contiguous() or step.pos.numel() != 3 * self.n:
            raise RuntimeError("%s: the step's coordinate input must be a contiguous float32 [N,3]" % type(self).__name__)
        return step.pos

    def _step_outputs(self, out):
        """(energy [B] float32, forces [N,3] float32, total [2] int64) of the captured step, checked."""
        energy, forces, total = out[0], out[1], out[-2]
        if (energy.dtype != torch.float32 or not energy.is_contiguous() or energy.numel() != self.num_graphs
                or forces.dtype != torch.float32 or not forces.is_contiguous() or forces.numel() != 3 * self.n
                or total.dtype != torch.int64 or total.numel() != 2):
            raise RuntimeError("%s: unexpected outputs of the captured step" % type(self).__name__)
        return energy, forces, total

    def _cell_args(self, step):
        """(wrap?, cell pointer, inverse-cell pointer): the cell is the tensor the search reads; its inverse is made here."""
        cell = step.cell
        if cell is None or not self.wrap:
            return False, None, None
        if cell.dtype != torch.float32 or not cell.is_contiguous() or cell.numel() != 9 * self.num_graphs:
            raise RuntimeError("%s: the step's cell must be a contiguous float32 [B,3,3]" % type(self).__name__)
        return True, cell.data_ptr(), self._inverse_of(cell).data_ptr()

    def _inverse_of(self, cell):
        """The float64 inverse [B,3,3] of the step's cell tensor: made on the host, once per tensor.  A subclass whose
        kernels move the cell keeps `inv_cell` as device state of its own and answers with that."""
        if self._inv_of is not cell:
            inv = np.linalg.inv(cell.detach().double().cpu().numpy().reshape(-1, 3, 3))
            self.inv_cell, self._inv_of = torch.from_numpy(np.ascontiguousarray(inv)).to(self.device), cell
        return self.inv_cell

    def _step_options(self, single):
        """Further keyword arguments of the graphed step (`single`: one structure, a `GraphedMDStep`): none.  A subclass
        that needs the virial or a cell it can move asks for `stress=` / `variable_cell=` here."""
        return {}

    # ---- running --------------------------------------------------------------------------------------------------------------
    @property
    def capacity(self):
        return self.step.capacity

    def stale(self):
        return self.step.stale()

    def run(self, n):
        """Enqueue `n` replays (MD: time steps; relaxation: force evaluations) back to back and return at once: no
        synchronisation, no copy."""
        n, name = int(n), type(self).__name__
        if n < 0:
            raise ValueError("run(n): n >= 0")
        if self.step.stale():
            raise RuntimeError("%s: the model's weight copies were rebuilt after the capture -- resume() recaptures" % name)
        if self._pending + n > self.log_steps:
            raise RuntimeError("%s.run(%d) would overwrite log rows not fetched yet (%d pending, log_steps=%d): fetch() "
                               "first" % (name, n, self._pending, self.log_steps))
        for ob in self._observers:
            ob._check_run(self, n)
        replay = self.step.graph.replay
        for _ in range(n):
            replay()
        self._pending += n

    def resume(self):
        """After a halt (or a stale capture): a new capture -- with a larger capacity where the list had outgrown it --, halt
        cleared.  The state is that of the last completed step, so the run continues as if it had never stopped."""
        self.state[1].fill_(PARKED)               # the capture's warm-up runs and its first replay must not move anything
        self.step.recapture()
        self._unpark()

    def fetch(self):
        """Everything a caller wants on the host through ONE packed device-to-host copy and one synchronisation: `step`
        (replays completed), `halted`, `halt_code` (list flags in the low bits, 4 = more pairs than capacity, 256 = an energy
        that is not finite), `halt_step`, `positions` [N,3] float64 (wrapped), `images` [N,3] int32, `velocities` [N,3]
        float64, `forces` [N,3] float32 (the last accepted ones), `log` [rows,B,width] float64 of the replays completed since
        the last fetch, and the subclass's own fields (its class docstring)."""
        rows = self._pending
        extras = [t.double().reshape(-1) for t in self._fetch_extras()]
        o = 4 + sum(t.numel() for t in extras)
        packed, room = self._pack(extras, rows), o + 12 * self.n + self.log.numel()
        if not self._observers:
            h, self._host = fetch_packed(packed, self._host, room)
            return self._unpack(h, o, rows)
        # the observers' parts ride behind the driver's own in the same copy: their words, counts and the ring entries not
        # fetched yet
        own = packed.numel()
        packed = torch.cat([packed] + [t for ob in self._observers for t in ob._parts(self)])
        h, self._host = fetch_packed(packed, self._host, max(room, packed.numel()))
        s = self._unpack(h[:own], o, rows)
        s.observers = []
        for ob in self._observers:
            entry, used = ob._read(self, h[own:])
            s.observers.append(entry)
            own += used
        return s

    def _pack(self, extras, rows):
        """state | the subclass's extras | x | image | v | f_prev | the `rows` log rows not fetched yet, as one float64 array."""
        idx = (torch.arange(rows, device=self.device) + self._logged) % self.log_steps
        return torch.cat([self.state.double()] + extras +
                         [self.x.reshape(-1), self.image.double().reshape(-1), self.v.reshape(-1),
                          self.f_prev.double().reshape(-1), self.log.index_select(0, idx).reshape(-1)])

    def _unpack(self, h, o, rows):
        """The snapshot of the packed array `h` (the atoms' part starts at `o`); counts the fetch and reacts to a halt."""
        n = self.n
        step, code, halt_step = int(h[0]), int(h[1]), int(h[2])
        s = types.SimpleNamespace(step=step, halted=code != 0, halt_code=code, halt_step=halt_step if code else None)
        self._read_extras(s, int(h[3]), h[4:o])
        s.positions = h[o:o + 3 * n].reshape(n, 3).copy()
        s.images = h[o + 3 * n:o + 6 * n].astype(np.int32).reshape(n, 3)
        s.velocities = h[o + 6 * n:o + 9 * n].reshape(n, 3).copy()
        s.forces = h[o + 9 * n:o + 12 * n].astype(np.float32).reshape(n, 3)
        done = max(0, min(rows, step - self._logged))
        s.log = h[o + 12 * n:].reshape(rows, self.num_graphs, self.LOG_WIDTH)[:done].copy()
        self._logged, self._pending = step, 0
        self._after_halt(code, halt_step)
        return s

    def _after_halt(self, code, halt_step):
        """What `fetch()` does about a halt code it read: the list's flags as any fetch treats them; a non-finite energy
        drops the model's caches (with one warning per model)."""
        list_flags_seen(code, self.device)
        if code & HALT_NONFINITE:
            # the captured step holds the stale-cache guard's check-and-poison kernel: after a write through `.data` every
            # replay answers NaN.  The halt kept the NaN forces out of the driver's state; the caches are dropped here.
            warn_nan_once(self.model, "hermnet_amd: %s halted at step %d on an energy that is not finite (weights written "
                          "through `.data` behind the cached copies?); the caches were dropped -- call resume() to "
                          "recapture and continue from the last completed step." % (type(self).__name__, halt_step), 3)
            self.model.invalidate_caches()

    # ---- the packed fetch's own part of a subclass ------------------------------------------------------------------------------
    def _fetch_extras(self):
        """Its tensors that travel behind `state` in the packed fetch."""
        return []

    def _read_extras(self, s, word, h):
        """Its fields of the snapshot `s`, from the fourth state word and the slice `h` of its extras."""
