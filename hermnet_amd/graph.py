"""Whole-step hipGraph replay: energy + forces of a FIXED neighbour list as one graph launch.

A step is ~200 kernel launches; eager enqueueing costs 2.7 ms of host time for a 3.8 ms step at 10k atoms, and is the
limit for small systems (a 1024-molecule batch: ~7 ms eager for ~2.5 ms of GPU work).  Capturing relation build +
forward + force backward once and replaying it removes the host from the loop.

Scope: the graph bakes in every launch geometry, so it is valid while `edge_index` (hence E and the relation layout)
stays the same -- repeated evaluation on one list (benchmarks, line searches, finite differences, several MD steps on a
list that is rebuilt every k steps).  The reference rebuilds the list every step (`calculator.py:49`), and beyond-cutoff
edges still send the `rbf_proj` bias, so a calculator may only reuse a graph while its list is unchanged;
`GraphedStep.matches(data)` is the check.

What made replay work (ROCm 7.2, bisected with tools/graph_probe.py): captured `hipMemsetAsync` nodes do not survive
eager memsets issued between two replays (the second replay skips / mis-addresses the fill), so nothing on the step
path uses hipMemsetAsync / hipMemcpyAsync any more (csrc/relation_kernels.hip: zero / copy / scan kernels).
"""
import gc

import torch


def _energy_forces(model, data, pos, stress):
    """(energy, forces) of `data`, with `stress` (energy, forces, virial): ONE forward and ONE backward either way."""
    if stress:
        from .stress import energy_forces_virial
        return tuple(energy_forces_virial(model, data, pos))
    e = model(data)
    f = -torch.autograd.grad(e.sum(), pos)[0]
    return e.detach(), f


def _capture(step, warmup):
    """`warmup` eager runs of `step()` on a side stream (caches, weights, library workspaces), then one run captured:
    returns (graph, what the captured run returned: the static outputs)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    # No garbage collection inside the capture: a resident driver and its step refer to each other through the hooks, so a
    # dead driver's capture is freed by the collector alone, and destroying a CUDAGraph synchronises the device on ROCm --
    # inside a capture in progress that call is refused and the refusal, raised in a destructor, ends the process.  Dead
    # captures are collected here instead, and the collector stays out until this capture has ended.
    collecting = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            out = step()
    finally:
        if collecting:
            gc.enable()
    torch.cuda.synchronize()
    return graph, out


class GraphedStep(object):
    """energy, forces = step(pos) for a fixed graph topology.

    model: HVNet / HTNet in eval() with parameters that do not require grad; data: `Data` on the GPU with
    `edge_index` (and `cell` / `edge_shift`) already built.  Construction runs `warmup` eager steps on a side stream,
    then captures one step.  `__call__(pos=None)` copies `pos` into the static input (if given), replays, and returns
    the static output tensors (valid until the next call; clone them to keep them).
    `stress=True`: the capture contains the virial kernels (stress.energy_forces_virial: the same forward and the same ONE
    backward) and a call returns (energy, forces, virial [B,3,3]); energy and forces are bit for bit the plain step's."""

    def __init__(self, model, data, warmup=3, stress=False):
        if not data.pos.is_cuda:
            raise RuntimeError("GraphedStep needs GPU tensors")
        if model.training:
            raise RuntimeError("GraphedStep captures the eval() path")
        self.model, self.data, self.stress = model, data, bool(stress)
        self.virial = None
        self.pos = data.pos.detach().clone().requires_grad_(True)      # static input
        data.pos = self.pos
        if data.get("batch") is None:      # (a single graph, as the forward fills it in)
            data.batch = torch.zeros(self.pos.size(0), dtype=torch.long, device=self.pos.device)
        # the capture reads the atom set's arrays: held here for as long as the capture may be replayed
        self.atoms = data._hn_atoms = model.atom_set(data.atomic_number, data.batch)
        self.graph, out = _capture(self._eager, warmup)
        self.energy, self.forces = out[:2]
        if self.stress:
            self.virial = out[2]
        # the captured topology: the tensor OBJECTS (kept alive here, so their addresses cannot be handed to a rebuilt
        # list of the same size) and their versions (in-place edits)
        self._topo = self._topology(data)

    def _eager(self):
        return _energy_forces(self.model, self.data, self.pos, self.stress)

    @staticmethod
    def _topology(data):
        keep = [data.get(k) for k in ("edge_index", "edge_shift", "cell", "atomic_number", "batch")]
        return [(t, None if t is None else t._version) for t in keep]

    def matches(self, data):
        """True while `data` carries the neighbour list (edge_index, edge_shift, cell, atomic numbers, batch) this graph
        was captured for: the same tensor objects, not modified in place since."""
        now = self._topology(data)
        return all(a is b and va == vb for (a, va), (b, vb) in zip(self._topo, now))

    def __call__(self, pos=None):
        if pos is not None:
            with torch.no_grad():
                self.pos.copy_(pos)
        self.graph.replay()
        if self.stress:
            return self.energy, self.forces, self.virial
        return self.energy, self.forces


class GraphedMDStep(object):
    """energy, forces = step(pos) INCLUDING the neighbour search: cell list -> padded neighbour list -> relation build ->
    forward -> force backward as ONE hipGraph launch that stays valid across list rebuilds (the
    reference rebuilds its list on the host every step, `plugin/ase_interface/calculator.py:49`).

    What makes the launch geometry independent of the edge count: the list is padded to `capacity` columns with NULL
    edges that the relation build files behind every row (`neighbor.neighbor_search_padded`), and the search itself runs
    without a host read, library sort or memset.  model: HVNet in eval(), parameters not requiring grad; one periodic
    structure (atomic_number [N], cell [3,3], both on the GPU and unchanged for the life of the object -- unless
    `variable_cell`, below --; `pos` [N,3] gives the first coordinates).  `capacity` defaults to the first list's edge count + 4 %.

        step = GraphedMDStep(model, z, cell, pos0)
        e, f = step(pos)            # static outputs: valid until the next call
        ok, n_edges = step.check()  # a host read -- do it when e / f are copied to the host anyway; not ok: the list
                                    # outgrew the capacity (or left the cell by > 8 images): `step.recapture(pos)`

    `stress=True`: the capture contains the virial kernels; a call returns (energy, forces, virial [1,3,3]) and `fetch()`
    carries the nine virial values in its one packed copy (a fifth result).
    `variable_cell=True`: the cell is a static INPUT like the coordinates -- `step(pos, cell)` copies a new [3,3] cell into
    the device tensor that search, edge geometry and virial kernels read (`neighbor_search_padded(..., device_cell=True)`:
    the bin geometry is made on the device, no host copy of the cell is consulted), so one capture serves NPT dynamics and
    cell relaxation.  A degenerate cell (singular, or far smaller than the cutoff) cannot raise inside a replay: flag bit 3
    makes `check()` / `fetch()` report "not ok" (`last_flags & 8`), the step's numbers are to be discarded and the capture
    stays valid for the next sane cell."""

    def __init__(self, model, atomic_number, cell, pos, capacity=None, warmup=3, reference_compat=False, stress=False,
                 variable_cell=False, hooks=None):
        if not pos.is_cuda or cell is None:
            raise RuntimeError("GraphedMDStep needs GPU tensors and a periodic cell")
        self.variable_cell = bool(variable_cell)
        self.cell = cell.detach().float().reshape(3, 3).contiguous().clone() if self.variable_cell else cell   # static input
        self.batch = torch.zeros(atomic_number.numel(), dtype=torch.long, device=pos.device)
        self._start(model, atomic_number, pos, capacity, warmup, reference_compat, stress, hooks)

    def _start(self, model, atomic_number, pos, capacity, warmup, reference_compat, stress, hooks, **search):
        """The tail of both constructors, behind `self.cell / batch / variable_cell`: the refusals, the static inputs, the atom
        set the capture reads, the first capacity (from an exact search with `search`) and the capture."""
        from .neighbor import neighbor_search, padded_capacity
        if not pos.is_cuda:
            raise RuntimeError("%s needs GPU tensors" % type(self).__name__)
        if model.training:
            raise RuntimeError("%s captures the eval() path" % type(self).__name__)
        self.reference_compat = bool(reference_compat)      # edge conventions of the reference's own pipeline (neighbor.py)
        if self.cell is None and self.reference_compat:
            raise NotImplementedError("the reference pipeline's 32-neighbour cap needs the exact list (neighbor_search)")
        self.model, self.z, self._hooks, self._warmup = model, atomic_number, hooks, warmup
        self.stress, self.virial, self.last_flags = bool(stress), None, 0
        self.pos = pos.detach().clone().float().requires_grad_(True)      # static input
        # the capture reads the atom set's arrays: held here, handed to every `Data` of the step (`_eager`)
        self.atoms = model.atom_set(self.z, self.batch)
        if capacity is None:
            out = neighbor_search(self.pos.detach(), model.rc, self.cell, reference_compat=self.reference_compat, **search)
            capacity = padded_capacity(int((out if self.cell is None else out[0]).size(1)))
        self._capture(int(capacity))

    def _data(self):
        """(the step's `Data` on a freshly searched padded list, the list's `total`)."""
        from .data import Data
        from .neighbor import neighbor_search_padded
        ei, sh, total = neighbor_search_padded(self.pos.detach(), self.model.rc, self.cell, self.capacity,
                                               reference_compat=self.reference_compat, device_cell=self.variable_cell)
        return Data(pos=self.pos, atomic_number=self.z, batch=self.batch, cell=self.cell.reshape(1, 3, 3), edge_index=ei,
                    edge_shift=sh), total

    def _eager(self):
        """search + step: (energy, forces, total), with `stress` (energy, forces, virial, total), and behind them everything
        a caller copies to the host per step as ONE array (`fetch`): energies | (edges, flags) | forces (| virial)."""
        d, total = self._data()
        d._hn_edge_count, d._hn_atoms = total, self.atoms
        out = _energy_forces(self.model, d, self.pos, self.stress)
        parts = [out[0].double().reshape(-1), total.double(), out[1].double().reshape(-1)]
        parts += [w.double().reshape(-1) for w in out[2:]]
        return out + (total, torch.cat(parts))

    def _step(self):
        """What is captured: `_eager()`, or with `hooks=(before, behind)` (md.DeviceMD: the integrator's kernels)
        `before(self)`, `_eager()`, `behind(self, its results)` -- work enqueued in front of the search and behind the force
        backward becomes part of every replay."""
        if self._hooks is None:
            return self._eager()
        self._hooks[0](self)
        out = self._eager()
        self._hooks[1](self, out)
        return out

    def stale(self):
        """True once the model's derived weight copies were dropped after the capture (`load_state_dict`, `.to()`,
        `train()` / `eval()`, `invalidate_caches()`): the captured launches read the OLD copies -- capture again."""
        return self.model.__dict__.get("_cache_epoch", 0) != self._epoch

    def _capture(self, capacity):
        self.capacity = capacity
        self._epoch = self.model.__dict__.get("_cache_epoch", 0)
        self.graph, out = _capture(self._step, self._warmup)      # (warm-up: also the cell on the host, the row layout)
        self.energy, self.forces, self.total, self.packed = out[0], out[1], out[-2], out[-1]
        if self.stress:
            self.virial = out[2]
        self._host = None

    def __call__(self, pos=None, cell=None):
        """`pos` [N,3]: a device tensor, or a float32 host tensor (uploaded straight into the captured input); `cell` [3,3]
        likewise (`variable_cell=True` only)."""
        if cell is not None and not self.variable_cell:
            raise RuntimeError("GraphedMDStep: the cell is baked into this capture (construct it with variable_cell=True)")
        with torch.no_grad():
            if pos is not None:
                self.pos.copy_(pos)
            if cell is not None:
                self.cell.copy_(cell.reshape(self.cell.shape))
        self.graph.replay()
        if self.stress:
            return self.energy, self.forces, self.virial
        return self.energy, self.forces

    def fetch(self):
        """The last call's results on the host through ONE device-to-host copy and one synchronisation (separate reads of
        the energy, the forces and the list's counters cost a round trip each -- as much as the whole replay of a small
        cell): (energy [graphs] float32 array, forces [N,3] float32 array, list complete?, edges found), with `stress` also
        the virial [graphs,3,3] float32 array as a fifth result.  `last_flags` keeps the list's flags."""
        import numpy as np
        from ._resident import fetch_packed, list_flags_seen
        h, self._host = fetch_packed(self.packed, self._host)
        ng = self.energy.numel()
        n_edges, flags = int(h[ng]), int(h[ng + 1])
        self.last_flags = flags
        list_flags_seen(flags, self.packed.device)       # (a stash overflow: the repeat gets a larger stash slot per atom)
        if self.stress:
            nf = self.forces.numel()
            return (h[:ng].astype(np.float32), h[ng + 2:ng + 2 + nf].astype(np.float32).reshape(-1, 3), flags == 0, n_edges,
                    h[ng + 2 + nf:].astype(np.float32).reshape(-1, 3, 3))
        return h[:ng].astype(np.float32), h[ng + 2:].astype(np.float32).reshape(-1, 3), flags == 0, n_edges

    def check(self):
        """(list complete?, edges found) of the last call: one host read."""
        from .neighbor import padded_list_ok
        ok, n_edges = padded_list_ok(self.total)
        self.last_flags = 0 if ok else int(self.total[1])
        return ok, n_edges

    def recapture(self, pos=None, capacity=None, cell=None):
        """A new graph for a larger capacity (default: from the last edge count); returns the step's results."""
        from .neighbor import padded_capacity
        with torch.no_grad():
            if pos is not None:
                self.pos.copy_(pos)
            if cell is not None and self.variable_cell:
                self.cell.copy_(cell.reshape(self.cell.shape))
        if capacity is None:
            capacity = padded_capacity(max(int(self.total[0]), self.capacity))
        self._capture(int(capacity))
        return self.__call__()


class GraphedBatchMDStep(GraphedMDStep):
    """`GraphedMDStep` for a batch of structures (path-integral beads, replicas, displaced supercells): the batched
    neighbour search (`neighbor.neighbor_search_padded(..., batch=, num_graphs=)`), the relation build, the forward and the
    force backward of ALL of them as ONE hipGraph launch.  atomic_number [N], batch [N] int64 non-decreasing, `num_graphs`
    = B and cell [B,3,3], or None for a batch of open structures (molecules), all on the GPU.

        step = GraphedBatchMDStep(model, z, cells, pos0, batch, B)
        e, f = step(pos)            # energy [B], forces [N,3]: static outputs, valid until the next call
        e, f = step(pos, cells)     # periodic batches: the cells are static INPUTS like the coordinates

    The search reads cells, atom ranges and bounding boxes on the device, so nothing inside the capture reads the host and
    one capture serves NVT and NPT replicas; `stress=True` adds virial [B,3,3].  `fetch()` (its packed copy carries the B
    energies), `check()`, `recapture()` and `stale()` are the single form's.  Flag bit 3 (`last_flags & 8`) marks a
    degenerate cell of one replica -- that replica listed no pair, discard the step --, bit 4 a `batch` that decreases."""

    def __init__(self, model, atomic_number, cell, pos, batch, num_graphs, capacity=None, warmup=3, reference_compat=False,
                 stress=False, hooks=None):
        self.num_graphs, self.variable_cell = int(num_graphs), cell is not None
        self.batch = batch.detach().long().contiguous()
        self.cell = None if cell is None else cell.detach().float().reshape(self.num_graphs, 3, 3).contiguous().clone()
        self._start(model, atomic_number, pos, capacity, warmup, reference_compat, stress, hooks,
                    batch=self.batch, num_graphs=self.num_graphs)

    def _data(self):
        from .data import Data
        from .neighbor import neighbor_search_padded
        ei, sh, total = neighbor_search_padded(self.pos.detach(), self.model.rc, self.cell, self.capacity,
                                               reference_compat=self.reference_compat, batch=self.batch,
                                               num_graphs=self.num_graphs)
        d = Data(pos=self.pos, atomic_number=self.z, batch=self.batch, edge_index=ei)
        if self.cell is not None:
            d.cell, d.edge_shift = self.cell, sh
        return d, total
