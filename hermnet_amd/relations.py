"""Relation-ordered graph: the build's replacement for `in_subgraph`
(`HermNet/utils.py:11-24`, called per relation per layer at `hermnet.py:52-54`).

Instead of N_t O(E) scans per relation per layer, edges are sorted ONCE per
neighbour list: atoms are renumbered by (relation of their element, id) and the
edge list is kept in two orders,
  CSR  (row(target), edge id)                      -> forward segmented sums,
  CSC  (relation(target), row(source), CSR pos)    -> backward segmented sums,
plus (torch build only) the out-adjacency by source row.  All index arrays are
int32 device tensors.  One small D2H copy per atom set (atoms per relation,
number of graphs) tells the host where each relation's rows start.

What follows from (atomic_number, batch, z_list) alone is an `AtomSet`: that
host read, the `RowArrays` of every row layout, the read-out order and the
small constants the native kernels read.  Its owners keep it alive -- every
graph built from it, every captured step that replays its addresses --;
`AtomSet.of` finds the set of tensors passed again (8 most recent).

Every piece is stated once and the four builds (HVNet / HTNet, torch / native)
are assembled from them: `_classify` (relation of every atom),
`RelationalGraph._layout` (where the relations' rows start), `_source_rows`
(rows of the atoms), `_order_edges` (CSR + CSC, one key-width rule),
`_active_relations`, the set's `graph_order` / `triadic_src_ranges`; the
native builds share the set's `new_rows` / `keep_rows` and `_native_edges`
(output arrays + `RelationsOut`).  The torch builds define the result bit for
bit.  Other modules keep values derived from the immutable graph through
`RelationalGraph.derived`.
"""
import ctypes

import torch

from . import _lib, switches
from .ops import _stream

_ATOM_SETS = []      # AtomSet.of: the lookup index, most recent first, at most 8 sets; dropping one frees nothing an owner reads


def _classify(atomic_number, z_list):
    """The torch restatement of `hermnet_relation_counts`: (relation of every atom [NA] -- the first matching element, T
    for "not in elems" (hermnet.py:53 finds none) --, atoms per relation + unknown [T+1]), both on the atoms' device; the
    host reads the counts once per atom set (`AtomSet`)."""
    dev, NA, T = atomic_number.device, int(atomic_number.numel()), len(z_list)
    eq = atomic_number.long()[:, None] == torch.tensor(list(z_list), dtype=torch.long, device=dev)[None, :]
    rel = torch.where(eq.any(1), eq.int().argmax(1), torch.full((NA,), T, dtype=torch.long, device=dev))
    counts = torch.zeros(T + 1, dtype=torch.long, device=dev).index_add_(0, rel, torch.ones_like(rel))
    return rel, counts


class RowArrays(object):
    """The row arrays of ONE row layout of an atom set (`AtomSet.rows`), which a native build's kernel fills on the first
    build and reads (`rows_ready`) on every later one."""

    __slots__ = ("type_rowptr", "node_order", "row_of_node", "z_rows", "row_real", "node_order64", "row_of_node64",
                 "z_rows64", "batch32")

    def __init__(self, starts, num_atoms, n_rows, dev):
        e32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
        self.type_rowptr = torch.tensor(list(starts), dtype=torch.int32, device=dev)  # here (one upload); build kernels, graph
        self.node_order = e32(num_atoms)        # the first build's kernel; later builds' kernels
        self.row_of_node = e32(num_atoms)       # the first build's kernel; later builds' kernels
        self.z_rows = e32(n_rows)               # the first build's kernel; later builds' kernels
        self.row_real = torch.empty(n_rows, dtype=torch.float32, device=dev)    # the first build's kernel; graph.row_real
        self.node_order64 = self.row_of_node64 = self.z_rows64 = None   # `finish`; the graphs' node_order / row_of_node / z_rows
        self.batch32 = None                     # `finish`; graph.batch32

    def finish(self, batch):
        """After the kernel: int64 copies for the host code's gathers (embedding, index_select) and `batch32`."""
        self.z_rows64, self.row_of_node64, self.node_order64 = self.z_rows.long(), self.row_of_node.long(), self.node_order.long()
        self.batch32 = None if batch is None else batch.to(torch.int32).contiguous()


class AtomSet(object):
    """Everything that follows from (atomic_number, batch, z_list) alone: the atom counts of the one host sync and the
    device arrays the builds make once and then READ -- a captured step bakes in their addresses.  Nothing in a set is
    ever cleared or evicted; it lives as long as its owners: every `RelationalGraph` built from it (`graph.atoms`), every
    object that replays a capture (graph.py: `step.atoms`, handed to each `Data` as `_hn_atoms`), and the lookup index
    `AtomSet.of` while the set is among its 8 most recent.  Undeclared fields raise."""

    __slots__ = ("atomic_number", "z_version", "batch", "batch_version", "z_list", "device", "zl", "z64", "counts_host",
                 "num_graphs", "rows", "graph_perm", "graph_lengths", "active", "src_ranges", "triadic_counts")

    def __init__(self, atomic_number, batch, z_list):
        dev, NA, T = atomic_number.device, int(atomic_number.numel()), len(z_list)
        # the key (written here, read by `matches`): the caller's tensor OBJECTS, kept alive here -- an address alone could be
        # reused by a different tensor of the same size -- with their versions (in-place edits), and the model's elements
        self.atomic_number, self.z_version = atomic_number, atomic_number._version
        self.batch, self.batch_version = batch, None if batch is None else batch._version
        self.z_list = tuple(z_list)
        self.device = dev
        self.zl = torch.tensor(list(z_list), dtype=torch.int32, device=dev)     # here; the native builds' kernels
        self.z64 = atomic_number.to(torch.int64, copy=True).contiguous()        # here (the set's own copy); the native builds' kernels
        if atomic_number.is_cuda and switches.native_relations:
            counts = torch.empty(T + 1, dtype=torch.int32, device=dev)
            _lib.call("hermnet_relation_counts", _lib.ptr(self.z64), NA, _lib.ptr(self.zl), T, _lib.ptr(counts), _stream())
        else:
            counts = _classify(self.z64, z_list)[1]
        nb = batch.long().max().reshape(1) + 1 if (batch is not None and NA > 0) else torch.ones(1, dtype=torch.long, device=dev)
        host = torch.cat([counts.long(), nb]).cpu().tolist()      # the ONE host sync of an atom set
        self.counts_host = host[:T + 1]         # here; all four builds: atoms per relation + unknown [T+1]
        self.num_graphs = int(host[-1])         # here; all four builds
        self.rows = {}                          # `keep_rows`: layout key -> RowArrays; the native builds
        self.graph_perm = self.graph_lengths = None     # `graph_order`; all four builds (the graphs' read-out order)
        self.active = {}                        # `active_flags`: pattern -> uint8 [n_rel]; the native builds' kernels
        self.src_ranges = None                  # `triadic_src_ranges`; both HTNet builds (graph.src_ranges)
        self.triadic_counts = None              # `_build_triadic_native`: int32 [T] atoms per element; its kernel

    def matches(self, atomic_number, batch, z_list):
        return (self.atomic_number is atomic_number and self.z_version == atomic_number._version and self.batch is batch
                and self.batch_version == (None if batch is None else batch._version) and self.z_list == tuple(z_list))

    @staticmethod
    def of(atomic_number, batch, z_list, given=None):
        """The set of these atoms: `given` (an owner's, e.g. `data._hn_atoms`; one made for other tensors raises), else the
        one the index holds for the same tensor objects, unmodified, and the same elements, else a new one (the host sync;
        atom types and batch assignment do not change along an MD trajectory)."""
        if given is not None:
            if not given.matches(atomic_number, batch, z_list):
                raise ValueError("this AtomSet was made for other atomic_number / batch tensors (or they were modified in "
                                 "place since) or for other elements")
            return given
        for s in _ATOM_SETS:
            if s.matches(atomic_number, batch, z_list):
                return s
        s = AtomSet(atomic_number, batch, z_list)
        _ATOM_SETS.insert(0, s)
        del _ATOM_SETS[8:]
        return s

    def new_rows(self, key, starts, n_rows):
        """-> (the RowArrays of layout `key`, filled already?); new ones are for the kernel to fill, then `keep_rows`."""
        rows = self.rows.get(key)
        if rows is not None:
            return rows, True
        return RowArrays(starts, int(self.atomic_number.numel()), n_rows, self.device), False

    def keep_rows(self, g, key, rows):
        """After the kernel: the layout's arrays are kept (once) and go on the graph."""
        if key not in self.rows:
            rows.finish(self.batch)
            self.rows[key] = rows
        g.type_rowptr, g.row_real, g.batch32 = rows.type_rowptr, rows.row_real, rows.batch32
        g.z_rows, g.row_of_node, g.node_order = rows.z_rows64, rows.row_of_node64, rows.node_order64

    def graph_order(self):
        """Deterministic per-graph read-out: (atoms grouped by graph, stable; segment lengths), or (None, None) for one graph."""
        if self.batch is None or self.num_graphs <= 1:
            return None, None
        if self.graph_perm is None:
            b64 = self.batch.long()
            self.graph_lengths = torch.zeros(self.num_graphs, dtype=torch.long, device=self.device).index_add_(
                0, b64, torch.ones_like(b64))
            self.graph_perm = torch.argsort(b64, stable=True)
        return self.graph_perm, self.graph_lengths

    def active_flags(self, flags):
        """uint8 device flags of a relation pattern (a tuple of bools), uploaded once: a pageable H2D copy per step would
        also break hipGraph capture of the step."""
        t = self.active.get(flags)
        if t is None:
            t = self.active[flags] = torch.tensor(list(flags), dtype=torch.uint8, device=self.device)
        return t

    def triadic_src_ranges(self):
        """HTNet [T P, 4]: relation (c; p, q) gathers sources of elements p and q only (the x_proj chain skips the other
        rows): rows [p B, p B + N_p) and, for q != p, [q B, q B + N_q); B = the largest element's atom count."""
        if self.src_ranges is None:
            T, cnt = len(self.z_list), self.counts_host
            B = max(cnt[:T]) if T > 0 else 0
            per_pair = [v for p in range(T) for q in range(p, T)
                        for v in (p * B, p * B + cnt[p], (q * B if q != p else 0), (q * B + cnt[q] if q != p else 0))]
            self.src_ranges = torch.tensor(per_pair * T, dtype=torch.int32, device=self.device).view(T * T * (T + 1) // 2, 4)
        return self.src_ranges


def _source_rows(rel, counts, starts, n_rows, z):
    """Rows of the atoms: sorted by (relation, id), relation t from row `starts[t]` on, unknown elements from `starts[T]`
    (`RelationalGraph._layout`).  -> (node_order [NA], row_of_node [NA], z_rows [n_rows], row_real [n_rows] 1 / 0,
    local [NA] index of every atom within its relation).  HTNet's source rows are HVNet's uniform layout."""
    dev, NA, T = rel.device, int(rel.numel()), len(starts) - 1
    node_order = torch.sort(rel.to(torch.int32), stable=True).indices
    first_sorted = torch.zeros(T + 1, dtype=torch.long, device=dev)
    first_sorted[1:] = torch.cumsum(counts[:T], 0)          # position of each relation in the sorted list
    rel_sorted = rel[node_order]
    local_sorted = torch.arange(NA, device=dev) - first_sorted[rel_sorted]
    row_of_node, local = torch.empty_like(node_order), torch.empty_like(node_order)
    row_of_node[node_order] = local_sorted + torch.tensor(starts, dtype=torch.long, device=dev)[rel_sorted]
    local[node_order] = local_sorted
    z_rows = torch.zeros(n_rows, dtype=torch.long, device=dev)
    z_rows[row_of_node] = z
    row_real = torch.zeros(n_rows, dtype=torch.float32, device=dev)
    row_real[row_of_node] = 1.0
    return node_order, row_of_node, z_rows, row_real, local


def _group(keys, n_keys, n_groups=None, wide=None):
    """Stable sort of integer keys < n_keys -> (sorted keys, permutation, row pointer [n_groups + 1] of the keys
    < n_groups (default: all); by searchsorted, which does not sync the host as bincount does).  The one key-width rule:
    int32 keys (half the radix passes) whenever the largest key fits; `wide` forces either width (tests)."""
    wide = n_keys > 2 ** 31 if wide is None else wide
    s, perm = torch.sort(keys.to(torch.long if wide else torch.int32), stable=True)
    s = s.long()
    return s, perm, torch.searchsorted(s, torch.arange((n_keys if n_groups is None else n_groups) + 1, device=keys.device))


def _order_edges(target_row, source_row, rel_of_target, n_target_rows, n_source_rows, n_rel, wide=None):
    """The two edge orders: CSR = (target row, edge id), CSC = (relation of the target, source row, CSR position); edges
    of relation n_rel (unknown-element targets) sort behind the CSC row pointer.  All int32 but the CSR permutation.
    -> (csr_perm, csr_src, csr_rowptr [n_target_rows + 1], csc_pos, csc_tgt, csc_rowptr [n_rel n_source_rows + 1])"""
    i32 = torch.int32
    tgt_sorted, csr_perm, csr_rowptr = _group(target_row, n_target_rows, wide=wide)
    csr_src = source_row[csr_perm]
    _, csc_pos, csc_rowptr = _group(rel_of_target[csr_perm] * n_source_rows + csr_src, (n_rel + 1) * n_source_rows,
                                    n_rel * n_source_rows, wide)
    return csr_perm, csr_src.to(i32), csr_rowptr.to(i32), csc_pos.to(i32), tgt_sorted[csc_pos].to(i32), csc_rowptr.to(i32)


def _active_relations(rel_active, atoms, edges_per_relation=None):
    """Which relations run.  Torch form (`edges_per_relation` given): bool [n_rel], by default "it receives an edge".
    Native form: uint8 device flags or None (the kernel decides by the edges).  `rel_active` (list, or device tensor:
    slab plans, no host read): the caller knows better, e.g. a shard whose relation has edges on other ranks only."""
    native, dev = edges_per_relation is None, atoms.device
    if rel_active is None:
        return None if native else edges_per_relation > 0
    if torch.is_tensor(rel_active):
        return rel_active.to(device=dev, dtype=torch.uint8 if native else torch.bool).contiguous()
    flags = tuple(bool(a) for a in rel_active)
    return atoms.active_flags(flags) if native else torch.tensor(flags, dtype=torch.bool, device=dev)


def _native_edges(g, rows, n_target_rows, n_csc_rows, E, edge_shift, dev):
    """Allocate the edge arrays of a native build on `g` (no out-adjacency: the position gradient reads the out-edges
    from the CSC order, ops.EdgeGeometry).  -> (`_lib.RelationsOut` over them and `rows`, the contiguous input shifts)"""
    P = _lib.ptr
    e32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    g.row_active = torch.empty(n_target_rows, dtype=torch.float32, device=dev)
    g.csr_rowptr, g.csr_src, g.csr_perm, g.src_id, g.tgt_id = e32(n_target_rows + 1), e32(E), e32(E), e32(E), e32(E)
    g.csc_rowptr, g.csc_tgt, g.csc_pos = e32(n_csc_rows + 1), e32(E), e32(E)
    g.out_rowptr = g.out_edges = None
    shift = None if edge_shift is None else edge_shift.float().contiguous()
    g.shift = None if shift is None else torch.empty(E, 3, dtype=torch.float32, device=dev)
    out = _lib.RelationsOut(P(rows.node_order), P(rows.row_of_node), P(rows.z_rows), P(rows.row_real),
                            P(g.row_active), P(g.csr_rowptr), P(g.csr_src), P(g.csr_perm), P(g.src_id), P(g.tgt_id),
                            P(g.shift), P(g.csc_rowptr), P(g.csc_tgt), P(g.csc_pos), None, None)
    return out, shift


class RelationalGraph(object):
    """Rows = atoms in relation order.  With `uniform` layout every relation owns a block of
    `block` = max_t N_t rows (short relations are padded with inert rows), so the per-relation node
    GEMMs of a layer are ONE batched GEMM over a [T, block, .] view; atoms of unknown element follow
    after the T blocks.  Without it (very unbalanced compositions) blocks are tight and the host
    loops over relations."""

    _DERIVED = ("_rowptr_c",        # nodeops._rowptr_host: type_rowptr_host as a ctypes int array
                "_upd_tile",        # nodeops.update_tile_rows: tile rows of the update kernels for this row layout, keyed on H
                "_row_keys",        # trainops._row_keys: gather / segmented-sum keys of the differentiable path
                "_edge_atoms64",    # trainops._edge_atoms: (source, target) atom of every edge as int64
                "_edge_sum_keys",   # trainops._edge_sum_keys: row keys of the adjoint of EdgeDiff
                "_row_graph")       # hermnet._GraphSpread: graph index and 0 / 1 mask of every row, keyed on the row count
    __slots__ = ("N", "E", "T", "num_atoms", "uniform", "block", "node_order", "row_of_node", "z_rows",
                 "type_rowptr", "type_rowptr_host", "csr_rowptr", "csr_src", "csr_perm", "csc_rowptr", "csc_tgt",
                 "csc_pos", "out_rowptr", "out_edges", "src_id", "tgt_id", "shift", "row_active", "row_real",
                 "batch32", "num_graphs", "graph_perm", "graph_lengths", "device", "_cstruct", "_rel_bounds",
                 "edge_table", "fwd_taps", "num_src", "res_row", "triadic_pairs", "src_real", "src_ranges",
                 "_all_known", "atoms") + _DERIVED

    def __init__(self):
        self._cstruct = None
        self._rel_bounds = None
        self.atoms = None          # the AtomSet this graph was built from (every build): owns what the native build kernels read
        self._all_known = False    # every atom has an element of the model (host knowledge from the atom counts): Ek == E
        self.edge_table = None     # [E+1,32] per-edge radial records of the current step, CSC order (set by HVNet.forward)
        self.fwd_taps = None       # [E,16] per-edge tap records of the current step, CSR order (set with edge_table), or None
        self.num_src = 0           # separate source-row space (HTNet): rows of xh / vec; 0 = same rows as the targets
        self.res_row = None        # [N] int32 source row feeding the residual of each target row, or None
        self.triadic_pairs = 0     # HTNet: pair relations per centre element (target rows = T_elem * pairs * block)
        self.src_real = None       # HTNet: [num_src] 1 for source rows that hold an atom
        self.src_ranges = None     # HTNet: [T,4] int32, the two source-row ranges a relation gathers from (nodeops.node_pre_fwd)
        for slot in self._DERIVED:
            setattr(self, slot, None)

    def derived(self, name, make, key=None):
        """A value that follows from this (immutable) graph alone, made on first use and kept in the declared slot
        `_<name>`; one made under another `key` is made again."""
        slot = "_" + name
        hit = getattr(self, slot)
        if hit is None or hit[0] != key:
            hit = (key, make())
            setattr(self, slot, hit)
        return hit[1]

    def rel_edge_bounds(self):
        """CSR edge ranges of the relations: edges of relation t are [b[t], b[t+1]) (rows are relation-ordered and
        CSR is row-ordered); edges to unknown-element targets follow after b[T].  One host sync per graph; used by
        the differentiable device-op path only."""
        if self._rel_bounds is None:
            self._rel_bounds = self.csr_rowptr[self.type_rowptr.long()].tolist()
        return self._rel_bounds

    def rel_edge_total(self):
        """Number of edges whose target has a known element (= rel_edge_bounds()[T]) WITHOUT a host read where the host
        already knows it: with no atom of an unknown element every edge counts (the train() path sizes its arrays by it; a
        read-back here was the last device sync of the training step after the relation build)."""
        if self._all_known:
            return self.E
        return self.rel_edge_bounds()[self.T]

    def rel_edge_bounds_dev(self):
        """`rel_edge_bounds` as a device tensor [T + 1] (no host read, no upload)."""
        return self.csr_rowptr[self.type_rowptr.long()]

    @staticmethod
    def build(atomic_number, edge_index, z_list, edge_shift=None, batch=None, rel_active=None, uniform=None, atoms=None):
        """atomic_number [N] int, edge_index [2,E] int (row 0 = source, row 1 = target,
        `hermnet.py:135`), z_list: atomic numbers of the model's elements in module order.
        `uniform`: None = automatic (padding overhead <= 15 %), True/False = forced.

        GPU tensors take the device-side build (`csrc/relation_kernels.hip`); host tensors (tests,
        planning) take the PyTorch restatement below, which defines the expected result bit for bit.
        (`switches.native_relations = False`: the restatement for GPU tensors too -- tests.)
        `atoms`: the caller's `AtomSet` of these tensors (an owner of a capture); default `AtomSet.of`."""
        atoms = AtomSet.of(atomic_number, batch, z_list, atoms)
        if atomic_number.is_cuda and switches.native_relations:
            return RelationalGraph._build_native(atoms, edge_index, edge_shift, rel_active, uniform)
        return RelationalGraph._build_torch(atomic_number, edge_index, z_list, edge_shift, batch, rel_active, uniform, atoms)

    @staticmethod
    def _layout(cnt_host, T, uniform):
        known = sum(cnt_host[:T])
        block = max(cnt_host[:T]) if T > 0 else 0
        if uniform is None:
            uniform = T > 1 and T * block <= 1.15 * known + 64
        uniform = bool(uniform) or T == 1
        if uniform:
            starts = [t * block for t in range(T)] + [T * block]
        else:
            starts, block = [0], 0
            for t in range(T):
                starts.append(starts[-1] + cnt_host[t])
        return uniform, block, starts, starts[T] + cnt_host[T]

    @staticmethod
    def _build_native(atoms, edge_index, edge_shift, rel_active, uniform):
        lib, P = _lib.load(), _lib.ptr
        g = RelationalGraph()
        dev, cnt_host = atoms.device, atoms.counts_host
        NA, E, T = int(atoms.z64.numel()), int(edge_index.size(1)), len(atoms.z_list)
        g.num_atoms, g.E, g.T, g.device, g.atoms, g.num_graphs = NA, E, T, dev, atoms, atoms.num_graphs
        ei = edge_index.long().contiguous()
        g.uniform, g.block, starts, N = RelationalGraph._layout(cnt_host, T, uniform)
        g.N, g.type_rowptr_host = N, starts[:T + 1]
        g._all_known = int(cnt_host[T]) == 0
        key = (g.uniform, N)
        rows, rows_ready = atoms.new_rows(key, starts[:T + 1], N)
        out, shift = _native_edges(g, rows, N, T * N, E, edge_shift, dev)
        act = _active_relations(rel_active, atoms)
        wbytes = lib.hermnet_build_relations_workspace(NA, N, E, T)
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        _lib.call("hermnet_build_relations", P(atoms.z64), P(ei), P(shift), NA, E, P(atoms.zl), T, P(rows.type_rowptr), N, P(act),
                  ctypes.byref(out), 1 if rows_ready else 0, P(work), wbytes, _stream())
        atoms.keep_rows(g, key, rows)
        g.graph_perm, g.graph_lengths = atoms.graph_order()
        return g

    @staticmethod
    def _build_torch(atomic_number, edge_index, z_list, edge_shift=None, batch=None, rel_active=None, uniform=None, atoms=None):
        g = RelationalGraph()
        g.atoms = atoms = AtomSet.of(atomic_number, batch, z_list, atoms)
        dev, i32 = atomic_number.device, torch.int32
        NA, E, T = int(atomic_number.numel()), int(edge_index.size(1)), len(z_list)
        g.num_atoms, g.E, g.T, g.device = NA, E, T, dev
        z = atomic_number.long()
        rel, counts = _classify(z, z_list)
        cnt_host, g.num_graphs = atoms.counts_host, atoms.num_graphs
        g.uniform, g.block, starts, N = RelationalGraph._layout(cnt_host, T, uniform)
        g.N, g.type_rowptr_host = N, starts[:T + 1]             # rows (>= atoms when padded)
        g.type_rowptr = torch.tensor(starts[:T + 1], dtype=i32, device=dev)
        g.node_order, g.row_of_node, g.z_rows, g.row_real, _ = _source_rows(rel, counts, starts, N, z)

        src, tgt = edge_index[0].long(), edge_index[1].long()
        g.csr_perm, g.csr_src, g.csr_rowptr, g.csc_pos, g.csc_tgt, g.csc_rowptr = _order_edges(
            g.row_of_node[tgt], g.row_of_node[src], rel[tgt], N, N, T)
        # out-adjacency by source row (tests read it; the device build leaves it off: ops.EdgeGeometry reads the CSC order)
        _, out_edges, out_rowptr = _group(g.csr_src, N)
        g.out_rowptr, g.out_edges = out_rowptr.to(i32), out_edges.to(i32)
        g.src_id, g.tgt_id = src[g.csr_perm].to(i32), tgt[g.csr_perm].to(i32)
        g.shift = None if edge_shift is None else edge_shift[g.csr_perm].float().contiguous()

        # hermnet.py:56-57: a relation without edges is skipped -> its rows stay zero; rows of
        # unknown-type atoms (hermnet.py:51) and padding rows are zero as well.
        tn = torch.arange(T + 1, device=dev) * N
        act = _active_relations(rel_active, atoms, g.csc_rowptr[tn[1:]] - g.csc_rowptr[tn[:-1]])
        act = torch.cat([act, torch.zeros(1, dtype=torch.bool, device=dev)])
        g.row_active = torch.zeros(N, dtype=torch.float32, device=dev)
        g.row_active[g.row_of_node] = act[rel].float()          # a row runs iff it holds an atom whose relation runs
        g.batch32 = None if batch is None else batch.to(i32).contiguous()
        g.graph_perm, g.graph_lengths = atoms.graph_order()
        return g

    @staticmethod
    def _build_triadic_native(atoms, edge_index, edge_shift, rel_active=None):
        """`build_triadic` through `hermnet_build_triadic` (csrc/relation_kernels.hip); None when an atom is of an
        element outside `z_list` (the torch build handles those)."""
        lib, P = _lib.load(), _lib.ptr
        dev, cnt_host = atoms.device, atoms.counts_host
        NA, E0, T = int(atoms.z64.numel()), int(edge_index.size(1)), len(atoms.z_list)
        if cnt_host[T] != 0:
            return None
        Pn = T * (T + 1) // 2
        TR, B = T * Pn, max(cnt_host[:T])
        Ns, Nt, E = T * B, TR * B, T * E0
        if TR * Ns + Nt + 8 >= 2 ** 31 or E >= 2 ** 31:
            return None
        g = RelationalGraph()
        g.num_atoms, g.T, g.device, g.uniform, g.block, g.num_graphs = NA, TR, dev, True, B, atoms.num_graphs
        g.N, g.num_src, g.triadic_pairs, g.E, g.atoms = Nt, Ns, Pn, E, atoms
        g.type_rowptr_host = [r * B for r in range(TR + 1)]
        key = ("triadic", B)
        rows, rows_ready = atoms.new_rows(key, g.type_rowptr_host, Ns)
        ei = edge_index.long().contiguous()
        out, shift = _native_edges(g, rows, Nt, TR * Ns, E, edge_shift, dev)
        tgt_real = torch.empty(Nt, dtype=torch.float32, device=dev)
        g.res_row = torch.empty(Nt, dtype=torch.int32, device=dev)
        if atoms.triadic_counts is None:
            atoms.triadic_counts = torch.tensor(cnt_host[:T], dtype=torch.int32, device=dev)
        wbytes = lib.hermnet_build_triadic_workspace(NA, E0, T, B)
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        act = _active_relations(rel_active, atoms)
        _lib.call("hermnet_build_triadic", P(atoms.z64), P(ei), P(shift), NA, E0, P(atoms.zl), T, B, P(atoms.triadic_counts),
                  P(act), ctypes.byref(out), P(tgt_real), P(g.res_row), 1 if rows_ready else 0, P(work), wbytes, _stream())
        atoms.keep_rows(g, key, rows)
        g.src_real = g.row_real                                    # the energy read-out masks SOURCE rows
        g.src_ranges = atoms.triadic_src_ranges()
        g.graph_perm, g.graph_lengths = atoms.graph_order()
        return g

    @staticmethod
    def build_triadic(atomic_number, edge_index, z_list, edge_shift=None, batch=None, rel_active=None, atoms=None):
        """HTNet's relation-ordered graph (DESIGN.md "HTNet"): relation rho = (centre element c, unordered pair
        {p, q} of neighbour elements), T * T(T+1)/2 of them.

        Two row spaces.  SOURCE rows: the atoms ordered by (element, id), every element padded to `block` rows (the
        HVNet order); unknown elements behind.  TARGET rows: one block of `block` rows per relation, block (c, k)
        holding the atoms of element c in the same order -- an atom is a target once per pair relation of its
        element ("virtual" rows; `res_row` maps them back to the atom's source row).  A directed edge j -> i appears
        once for every pair that contains element(j), i.e. T times: CSR by target row, CSC by (relation, SOURCE row),
        which is exactly the layout the message kernels consume with `num_src` / `res_row` set.

        `rel_active` [T P] (list or device tensor): overrides "a relation runs iff it receives an edge here" (atom shards).

        GPU tensors whose atoms are all of listed elements take the device-side build (`hermnet_build_triadic`, the
        HVNet build's counting sort over the expanded list); everything else the torch-op build below, which defines
        the result (tests/test_htnet.py compares the two)."""
        atoms = AtomSet.of(atomic_number, batch, z_list, atoms)
        if (atomic_number.is_cuda and switches.native_relations and len(z_list) > 0
                and atomic_number.numel() > 0):
            g = RelationalGraph._build_triadic_native(atoms, edge_index, edge_shift, rel_active)
            if g is not None:
                return g
        g = RelationalGraph()
        g.atoms = atoms
        dev, i32 = atomic_number.device, torch.int32
        NA, T = int(atomic_number.numel()), len(z_list)
        pairs = [(p, q) for p in range(T) for q in range(p, T)]
        P = len(pairs)
        TR = T * P
        z = atomic_number.long()
        rel, counts = _classify(z, z_list)
        cnt_host, g.num_graphs = atoms.counts_host, atoms.num_graphs
        _, B, starts, Ns = RelationalGraph._layout(cnt_host, T, True)
        Nt = TR * B
        g.num_atoms, g.T, g.device, g.uniform, g.block = NA, TR, dev, True, B
        g.N, g.num_src, g.triadic_pairs = Nt, Ns, P
        g.type_rowptr_host = [r * B for r in range(TR + 1)]
        g.type_rowptr = torch.tensor(g.type_rowptr_host, dtype=i32, device=dev)
        g.node_order, g.row_of_node, g.z_rows, g.src_real, local = _source_rows(rel, counts, starts, Ns, z)
        g.row_real = g.src_real                                   # energy read-out masks SOURCE rows

        # expanded edge list: edge (j -> i) once per pair containing element(j)
        pair_of = torch.full((T + 1, T), -1, dtype=torch.long, device=dev)      # element -> its T pair indices
        for e_ in range(T):
            ks = [k for k, (p, q) in enumerate(pairs) if e_ in (p, q)]
            pair_of[e_] = torch.tensor(ks, dtype=torch.long, device=dev)
        src, tgt = edge_index[0].long(), edge_index[1].long()
        tj, ti = rel[src], rel[tgt]
        eid = torch.nonzero((tj < T) & (ti < T)).reshape(-1)
        eid_x = eid.repeat_interleave(T)                           # expanded: (edge id major, pair minor)
        rel_x = ti[eid_x] * P + pair_of[tj[eid]].reshape(-1)
        vt_x = rel_x * B + local[tgt[eid_x]]                       # virtual target row
        g.E = int(eid_x.numel())
        csr_perm, g.csr_src, g.csr_rowptr, g.csc_pos, g.csc_tgt, g.csc_rowptr = _order_edges(
            vt_x, g.row_of_node[src[eid_x]], rel_x, Nt, Ns, TR)
        g.csr_perm = eid_x[csr_perm]
        g.out_rowptr = g.out_edges = None
        g.src_id, g.tgt_id = src[g.csr_perm].to(i32), tgt[g.csr_perm].to(i32)
        g.shift = None if edge_shift is None else edge_shift[g.csr_perm].float().contiguous()
        # target rows: real = the atom exists; active = its relation has at least one edge (hermnet.py:56-57)
        rows = torch.arange(Nt, device=dev)
        r_rel, r_loc = rows // max(B, 1), rows % max(B, 1)
        r_el = r_rel // P
        row_real = (r_loc < counts[:T][r_el.clamp(max=max(T - 1, 0))]).float() if Nt > 0 else torch.zeros(0, device=dev)
        tn = torch.arange(TR + 1, device=dev) * B
        act = _active_relations(rel_active, atoms, g.csr_rowptr[tn[1:]] - g.csr_rowptr[tn[:-1]])
        g.row_active = act[r_rel].float() * row_real if Nt > 0 else row_real
        g.res_row = (r_el * B + r_loc).to(i32)
        g.src_ranges = atoms.triadic_src_ranges()
        g.batch32 = None if batch is None else batch.to(i32).contiguous()
        g.graph_perm, g.graph_lengths = atoms.graph_order()
        return g

    def as_struct(self):
        if self._cstruct is None:      # the graph is immutable: build the ctypes view once, not per launch
            self._cstruct = _lib.Graph(self.N, self.E, self.T, self.type_rowptr.data_ptr(), self.csr_rowptr.data_ptr(),
                                       self.csr_src.data_ptr(), self.csc_rowptr.data_ptr(), self.csc_tgt.data_ptr(),
                                       self.csc_pos.data_ptr(), self.num_src, _lib.ptr(self.res_row))
        return self._cstruct
