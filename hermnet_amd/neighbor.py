"""Host-side cutoff neighbour search (input producer of the hot path).

Replaces `HermNet/data.py:14-24` (`neighbor_search`), which delegates to
`ase.neighborlist.primitive_neighbor_list('ijS', ...)` for periodic cells and to
`torch_cluster.radius_graph` otherwise -- neither package exists on the MI355X
image, so the build owns this step.

Conventions:
  * pair (i, j, S) is listed iff |pos[j] - pos[i] + S @ cell| < rc  (strict),
    (i, i, 0) is never listed, self-images (i, i, S != 0) are;
  * output order is canonical: lexicographic in (i, j, Sx, Sy, Sz);
  * indices are int64 (what the reference hands to the model), shifts int.

`neighbor_search` wraps the raw list in the reference's calling convention:
`edge_index = [i; j]` and an `edge_shift` such that the model-side formula
(`HermNet/hermnet.py:135-139`: pos[ei0] - pos[ei1] + edge_shift @ cell) yields
the true minimum-image vector, i.e. edge_shift = -S.  `reference_compat=True`
reproduces `data.py:19-24` literally (edge_shift = +S, the sign quirk described
in SURVEY.md section 0) for pipeline-level parity tests.
"""
import numpy as np
import os

import torch

from . import switches


def _expand_ranges(start, end):
    """Concatenate aranges [start_k, end_k) -> (flat_index, owner_k)."""
    cnt = (end - start).astype(np.int64)
    total = int(cnt.sum())
    if total == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    owner = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    first = np.cumsum(cnt) - cnt
    flat = np.arange(total, dtype=np.int64) - np.repeat(first, cnt) + np.repeat(start.astype(np.int64), cnt)
    return flat, owner


def neighbor_list(pos, rc, cell=None, pbc=(True, True, True), chunk=200000):
    """Cell-list neighbour search in float64.  Returns (i, j, S) canonical-sorted.

    pos [N,3]; cell [3,3] (rows are lattice vectors) or None for an open system.
    """
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    rc = float(rc)
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros((0, 3), np.int64)

    if cell is None:
        pts, owner, img = pos, np.arange(n, dtype=np.int64), np.zeros((n, 3), np.int64)
        wrap = np.zeros((n, 3), np.int64)
        real = pos
    else:
        cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
        pbc = np.asarray(pbc, dtype=bool).reshape(3)
        inv = np.linalg.inv(cell)
        frac = pos @ inv
        wrap = np.where(pbc, np.floor(frac), 0.0)
        fw = frac - wrap
        wrap = wrap.astype(np.int64)
        real = fw @ cell
        # plane spacings decide how many periodic images reach into the cutoff sphere
        heights = 1.0 / np.linalg.norm(inv, axis=0)
        nimg = np.where(pbc, np.ceil(rc / heights).astype(np.int64), 0)
        margin = rc / heights
        pts_l, owner_l, img_l = [], [], []
        ar = np.arange(n, dtype=np.int64)
        for sx in range(-nimg[0], nimg[0] + 1):
            for sy in range(-nimg[1], nimg[1] + 1):
                for sz in range(-nimg[2], nimg[2] + 1):
                    s = np.array([sx, sy, sz], dtype=np.float64)
                    f = fw + s
                    keep = np.all((f >= -margin - 1e-9) & (f <= 1.0 + margin + 1e-9) | ~pbc, axis=1)
                    if not keep.any():
                        continue
                    pts_l.append(f[keep] @ cell)
                    owner_l.append(ar[keep])
                    img_l.append(np.broadcast_to(np.array([sx, sy, sz], np.int64), (int(keep.sum()), 3)))
        pts = np.concatenate(pts_l)
        owner = np.concatenate(owner_l)
        img = np.concatenate(img_l)

    # uniform Cartesian bins of edge >= rc over the bounding box of all points
    lo = pts.min(axis=0) - 1e-6
    nb = np.maximum(((pts.max(axis=0) - lo) / rc).astype(np.int64) + 1, 1)
    pb = np.minimum(((pts - lo) / rc).astype(np.int64), nb - 1)
    pid = (pb[:, 0] * nb[1] + pb[:, 1]) * nb[2] + pb[:, 2]
    order = np.argsort(pid, kind="stable")
    pid_s = pid[order]
    rb = np.minimum(((real - lo) / rc).astype(np.int64), nb - 1)

    out_i, out_j, out_s = [], [], []
    rc2 = rc * rc
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        ids = np.arange(c0, c1, dtype=np.int64)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                bx = rb[c0:c1, 0] + dx
                by = rb[c0:c1, 1] + dy
                ok = (bx >= 0) & (bx < nb[0]) & (by >= 0) & (by < nb[1])
                if not ok.any():
                    continue
                # the three z-neighbour bins are contiguous in the sorted id space
                z0 = np.maximum(rb[c0:c1, 2] - 1, 0)
                z1 = np.minimum(rb[c0:c1, 2] + 1, nb[2] - 1)
                base = (bx * nb[1] + by) * nb[2]
                st = np.searchsorted(pid_s, base + z0, side="left")
                en = np.searchsorted(pid_s, base + z1, side="right")
                st = np.where(ok, st, 0)
                en = np.where(ok, en, 0)
                flat, own = _expand_ranges(st, en)
                if flat.size == 0:
                    continue
                cand = order[flat]
                ii = ids[own]
                d = pts[cand] - real[ii]
                d2 = np.einsum("ij,ij->i", d, d)
                sel = d2 < rc2
                jj = owner[cand]
                ss = img[cand]
                sel &= ~((jj == ii) & np.all(ss == 0, axis=1))
                out_i.append(ii[sel])
                out_j.append(jj[sel])
                out_s.append(ss[sel])
    if not out_i:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros((0, 3), np.int64)
    i = np.concatenate(out_i)
    j = np.concatenate(out_j)
    s = np.concatenate(out_s)
    # shifts were found for wrapped coordinates; express them for the caller's positions
    s = s - wrap[j] + wrap[i]
    key = np.lexsort((s[:, 2], s[:, 1], s[:, 0], j, i))
    return i[key], j[key], s[key]


_CELL_HOST = []        # [(cell tensor, version, 9 doubles)]: the cell of an MD run is the same tensor step after step


def _cell_on_host(cell):
    """The 3x3 cell as host doubles; read back once per tensor object and version (the read is a host sync)."""
    for ent in _CELL_HOST:
        if ent[0] is cell and ent[1] == cell._version:
            return ent[2]
    vals = cell.detach().double().cpu().reshape(-1, 3, 3)[0].contiguous().reshape(-1).tolist()
    _CELL_HOST.insert(0, (cell, cell._version, vals))
    del _CELL_HOST[4:]
    return vals


_STASH = {}       # device -> keys per atom of the search's stash slot (csrc/neighbor_kernels.hip)
_STASH_DEFAULT = 96       # fcc at rc = 5 A: 43 pairs per atom; 8 bytes per key and atom of workspace


def _stash_overflowed(dev):
    """An atom had more pairs than its slot (flag bit 1): the following searches get the largest slot."""
    _STASH[str(dev)] = 160


def _batch_args(pos, cell, batch, num_graphs):
    """(float32 pos, int64 batch, float32 [B,9] cells or None, B) of a batched search; `num_graphs` defaults to the number
    of cells or, for open structures, to one host read of `batch[-1]`."""
    if batch is None:
        raise ValueError("num_graphs without batch")
    p32 = pos.detach().float().contiguous()
    b64 = batch.detach().long().contiguous()
    if b64.dim() != 1 or b64.numel() != p32.size(0) or b64.device != p32.device:
        raise ValueError("batch must be [N] on the device of pos")
    cells = None
    if cell is not None:
        cells = cell.detach().float().reshape(-1, 9).contiguous()
        if cells.device != p32.device:
            raise ValueError("cell must be on the device of pos")
    if num_graphs is None:
        if cells is not None:
            num_graphs = cells.size(0)
        else:
            num_graphs = int(b64[-1]) + 1 if b64.numel() else 1
    B = int(num_graphs)
    if B <= 0 or (cells is not None and cells.size(0) != B):
        raise ValueError("a batched search takes cell = None or one [3,3] cell per graph ([num_graphs,3,3])")
    return p32, b64, cells, B


def _batch_flags_error(flags):
    if flags & 16:
        raise ValueError("batched neighbour search: `batch` must be non-decreasing with values in [0, num_graphs)")
    if flags & 8:
        raise RuntimeError("batched neighbour search: a cell of the batch is singular or far smaller than the cutoff")


def _device_search(pos, rc, cell, reference_compat, target_mask=None, device_cell=False, batch=None, num_graphs=None,
                   capacity=None):
    """The device cell list (`csrc/neighbor_kernels.hip`) in every form: one structure with its cell on the host or
    (`device_cell`) in device memory, or a batch (`batch` / `num_graphs`).  All of them prepare their arguments, size the
    workspace from the stash hint of the device and run their counting pass; then
      * `capacity` None: the exact list after ONE host read of (E, flags) -- what `neighbor_search` returns, or None where
        the host path has to answer (flag bit 0: an image shift beyond +-8 cells);
      * otherwise the padded list without a host read: (edge_index, edge_shift, total), see `neighbor_search_padded`."""
    import ctypes
    from . import _lib
    lib = _lib.load()
    P = _lib.ptr
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    batched, padded, periodic = batch is not None or num_graphs is not None, capacity is not None, cell is not None
    if batched:
        p32, b64, cells, B = _batch_args(pos, cell, batch, num_graphs)
    else:
        p32 = pos.detach().float().contiguous()
    dev, N = p32.device, int(p32.size(0))
    hint = _STASH.get(str(dev), _STASH_DEFAULT)       # keys per atom of the stash slot: the workspace's size decides it
    mask = None
    if batched:
        if N == 0:
            if padded:
                raise ValueError("a padded batched search needs at least one atom")
            ei = torch.empty(2, 0, dtype=torch.long, device=dev)
            return (ei, torch.empty(0, 3, dtype=torch.float32, device=dev)) if periodic else ei
        ws_bytes = lib.hermnet_neighbor_batch_workspace(N, B, hint)
        if ws_bytes == 0:
            raise RuntimeError("batched neighbour search: %d atoms in %d graphs are beyond the search's index range" % (N, B))
        count, head = "hermnet_neighbor_batch_count", (P(p32), N, P(b64), B, P(cells), float(rc))
    else:
        ws_bytes = lib.hermnet_neighbor_workspace_for(N, hint)
        if device_cell:
            if cell is None or not cell.is_cuda or cell.dtype != torch.float32 or cell.numel() != 9 or not cell.is_contiguous():
                raise ValueError("device_cell=True needs a contiguous float32 [3,3] cell on the GPU")
            if N == 0:
                raise ValueError("device_cell=True needs at least one atom")
            count, head = "hermnet_neighbor_count_devcell", (P(p32), N, P(cell), float(rc))
        else:
            dbl3 = ctypes.c_double * 3
            cell_h, lo_h, hi_h = None, dbl3(0, 0, 0), dbl3(1, 1, 1)
            if periodic:
                cell_h, lo_h, hi_h = (ctypes.c_double * 9)(*_cell_on_host(cell)), None, None
            elif N > 0:       # (an open structure's bounding box is a host read of its own: periodic cells are the MD case)
                mm = torch.stack([p32.min(0).values, p32.max(0).values]).double().cpu().tolist()
                lo_h, hi_h = dbl3(*mm[0]), dbl3(*mm[1])
            count, head = "hermnet_neighbor_count", (P(p32), N, cell_h, lo_h, hi_h, float(rc))
        if target_mask is not None:
            mask = (target_mask if target_mask.dtype == torch.uint8 else target_mask.to(torch.uint8)).contiguous()
            if mask.numel() != N or mask.device != dev:
                raise ValueError("target_mask must be [N] on the device of pos")
    work = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    total = torch.empty(2, dtype=torch.long, device=dev) if padded else torch.zeros(2, dtype=torch.long, device=dev)
    masks = () if batched else (P(mask),)             # (target masks are not part of the batched entry points)
    _lib.call(count, *head, P(work), ws_bytes, *masks, P(total), stream)
    source_first = 0 if periodic else 1
    sign = 1.0 if reference_compat else -1.0
    if padded:
        cap = int(capacity)
        edge_index = torch.empty(2, cap, dtype=torch.long, device=dev)
        shift = torch.empty(cap, 3, dtype=torch.float32, device=dev) if periodic else None
        if switches.debug_poison():
            # (tests: a column the search leaves unwritten would send the relation build far out of bounds)
            edge_index.fill_(0x3f3f3f3f3f3f3f3f)
            if shift is not None:
                shift.fill_(float("nan"))
        fill, shape = ("hermnet_neighbor_batch_fill_padded", (N, B)) if batched else ("hermnet_neighbor_fill_padded", (N,))
        _lib.call(fill, *shape, P(work), ws_bytes, cap, sign, source_first, P(edge_index), P(shift), P(total), stream)
        return edge_index, shift, total
    E, flags = total.tolist()                                # the one host read of the search
    if batched:
        _batch_flags_error(flags)
    if flags & 2:
        _stash_overflowed(dev)                               # (this search finishes in its two-pass form)
    if flags & 1:                                            # an image shift beyond +-8 cells: the host path handles it
        return None
    edge_index = torch.empty(2, E, dtype=torch.long, device=dev)
    shift = torch.empty(E, 3, dtype=torch.float32, device=dev) if periodic else None
    if E > 0:
        stash_ok = 0 if (flags & 2) else 1
        keys = None if stash_ok else torch.empty(E, dtype=torch.long, device=dev)
        fill, shape = ("hermnet_neighbor_batch_fill", (N, B)) if batched else ("hermnet_neighbor_fill", head)
        _lib.call(fill, *shape, P(work), ws_bytes, E, sign, source_first, stash_ok, P(keys), *masks, P(edge_index), P(shift),
                  stream)
    return (edge_index, shift) if periodic else edge_index


def _lists_as_tensors(i, j, s, periodic, reference_compat, dev):
    """(i, j, S) of the numpy list in `neighbor_search`'s calling conventions: periodic [i; j] with edge_shift = -S (+S with
    `reference_compat`); open [j; i], radius_graph's: row 0 = source (neighbour), row 1 = target (centre)."""
    if not periodic:
        return torch.from_numpy(np.vstack([j, i])).long().to(dev)
    sign = 1.0 if reference_compat else -1.0
    return torch.from_numpy(np.vstack([i, j])).long().to(dev), torch.from_numpy(sign * s.astype(np.float32)).float().to(dev)


def _neighbor_search_host_batched(pos, rc, cell, batch, num_graphs, reference_compat):
    """The batched search on the host: `neighbor_list` per structure, the atom offsets added."""
    p = pos.detach().cpu().numpy()
    b = batch.detach().cpu().numpy().astype(np.int64)
    cells = None if cell is None else cell.detach().cpu().numpy().reshape(-1, 3, 3)
    if num_graphs is None:
        num_graphs = cells.shape[0] if cells is not None else (int(b[-1]) + 1 if b.size else 1)
    B = int(num_graphs)
    if b.shape != (p.shape[0],) or B <= 0 or (cells is not None and cells.shape[0] != B):
        raise ValueError("a batched search takes batch [N] and cell = None or one [3,3] cell per graph ([num_graphs,3,3])")
    if b.size and (np.any(np.diff(b) < 0) or b[0] < 0 or b[-1] >= B):
        raise ValueError("batched neighbour search: `batch` must be non-decreasing with values in [0, num_graphs)")
    ptr = np.searchsorted(b, np.arange(B + 1))
    ii, jj, ss = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros((0, 3), np.int64)]
    for g in range(B):
        i, j, s = neighbor_list(p[ptr[g]:ptr[g + 1]], rc, None if cells is None else cells[g])
        ii.append(i + ptr[g]), jj.append(j + ptr[g]), ss.append(s)
    return _lists_as_tensors(np.concatenate(ii), np.concatenate(jj), np.concatenate(ss), cells is not None, reference_compat,
                             pos.device)


def neighbor_search_padded(pos, rc, cell, capacity, reference_compat=False, target_mask=None, device_cell=False, batch=None,
                           num_graphs=None):
    """The device cell list WITHOUT its host read: `capacity` columns are provided up front, the pairs
    found fill the first E of them and the rest become NULL edges (-1, -1; shift 0), which the relation build files behind
    every row -- the model runs on the padded list unchanged, with a launch geometry that does not depend on E.

    Returns (edge_index [2, capacity] int64, edge_shift [capacity, 3] float32 or None, total [2] int64 ON THE DEVICE):
    total[0] = E, total[1] = flags (include/hermnet_hip.h); read them when the step's results are copied to the host anyway.  The list is
    complete iff `padded_list_ok(total)`; otherwise (more pairs than columns, an atom with more pairs than its stash slot,
    coordinates many cells away from the cell) repeat with `neighbor_search` and a larger capacity.  GPU tensors only;
    open systems need `reference_compat=False` (the 32-neighbour cap is a host-side filter).
    `target_mask` [N] bool / uint8 (atom shards): list only the pairs whose target atom (row 1) is flagged.
    `device_cell=True` (periodic cells): the cell is read from DEVICE memory by the search itself -- no host copy of it is
    consulted (`_cell_on_host`), so a captured search follows a `cell` tensor that is rewritten between replays
    (graph.GraphedMDStep, `variable_cell`).  `cell` must then be a contiguous float32 [3,3] (or [1,3,3]) GPU tensor; for the
    same values the list is bit for bit the host-cell form's.  A degenerate cell (singular, or far smaller than the
    cutoff), which the host-cell form refuses with an error, raises flag bit 3 of total[1] instead.
    `batch` [N] int64, non-decreasing (with `num_graphs`; without it one host read finds it for open structures): a batch
    of structures searched in one pass, `cell` = None or [num_graphs,3,3].  Cells, atom ranges and bounding boxes are all
    read on the device (the cells as with `device_cell=True`), so the call is capturable for periodic and open batches
    alike; the list is the structures' lists concatenated with their atom offsets.  Flag bit 3 then marks a degenerate cell
    of one structure (which lists no pair; the others are complete), bit 4 a `batch` that decreases (no pair at all)."""
    if not pos.is_cuda:
        raise RuntimeError("neighbor_search_padded runs on the device list only")
    if cell is None and reference_compat:
        raise NotImplementedError("the reference pipeline's 32-neighbour cap needs the exact list (neighbor_search)")
    if (batch is not None or num_graphs is not None) and target_mask is not None:
        raise NotImplementedError("target_mask is not part of the batched search")
    return _device_search(pos, rc, cell, reference_compat, target_mask, device_cell, batch, num_graphs, int(capacity))


def padded_list_ok(total):
    """(complete?, E) of a padded list from its `total` tensor -- a host read: do it behind the step."""
    E, flags = total.tolist()
    if flags & 2:
        _stash_overflowed(total.device)           # an atom had more pairs than its stash slot: the repeat gets a larger one
    return flags == 0, int(E)


def padded_capacity(num_edges, margin=0.04, granule=4096):
    """A column count for the next steps' lists: the last count plus a margin, rounded up (a stable launch geometry)."""
    want = int(num_edges * (1.0 + margin)) + 64
    return (want + granule - 1) // granule * granule


def _cap_neighbors(edge_index, cap):
    """Keep at most `cap` in-edges per target (row 1), the ones with the lowest source index: the list is sorted
    by (target, source), so an edge's rank inside its target's run is its position minus the run's start."""
    E = edge_index.size(1)
    if E == 0:
        return edge_index
    tgt = edge_index[1]
    pos = torch.arange(E, device=tgt.device)
    first = torch.ones(E, dtype=torch.bool, device=tgt.device)
    first[1:] = tgt[1:] != tgt[:-1]
    start = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), 0).values
    return edge_index[:, (pos - start) < cap]


def neighbor_search(pos, rc, cell=None, reference_compat=False, target_mask=None, batch=None, num_graphs=None):
    """Drop-in for `HermNet/data.py:14-24`.

    pos: float Tensor [N,3]; cell: Tensor [3,3] or [1,3,3] or None.
    Returns `edge_index` (open system) or `(edge_index, edge_shift)` (periodic),
    int64 [2,E] / float32 [E,3], exactly the reference's return shapes.  GPU tensors are searched
    on the GPU and the result stays there; host tensors take the numpy cell list below.

    `reference_compat=True` reproduces the reference pipeline's edge conventions instead of the true
    minimum-image ones: periodic `edge_shift = +S` (`data.py:19-24`, see the module docstring) and, for open
    systems, `radius_graph`'s default cap of 32 neighbours per atom (`data.py:16`; torch_cluster keeps an
    implementation-defined subset -- its GPU kernel the 32 lowest source indices, which is what is kept here).

    `target_mask` [N] bool (no reference counterpart; `sharding.py`): keep only the edges whose target atom
    (`edge_index[1]`) is flagged, same order -- the list of an atom shard, without building the rest.

    `batch` [N] int64, non-decreasing (no reference counterpart): the structures of a batch, each searched on its own in
    one pass -- `cell` is then None (all open) or [num_graphs,3,3], and no pair crosses structures even where their
    coordinates overlap.  The result is the structures' lists concatenated, atom offsets added.  `num_graphs` defaults to
    the number of cells or, for open structures, to a host read of `batch[-1]`.
    """
    if cell is None and reference_compat:
        return _cap_neighbors(neighbor_search(pos, rc, None, False, target_mask, batch, num_graphs), 32)
    batched = batch is not None or num_graphs is not None
    if batched and target_mask is not None:
        raise NotImplementedError("target_mask is not part of the batched search")
    if batched and batch is None:
        raise ValueError("num_graphs without batch")
    if pos.is_cuda:
        out = _device_search(pos, rc, cell, reference_compat, target_mask, batch=batch, num_graphs=num_graphs)
        if out is not None:
            return out
    if batched:
        return _neighbor_search_host_batched(pos, rc, cell, batch, num_graphs, reference_compat)
    p = pos.detach().cpu().numpy()
    i, j, s = neighbor_list(p, rc, None if cell is None else cell.detach().cpu().numpy().reshape(-1, 3, 3)[0])
    if target_mask is not None:       # the target atom (row 1): i of an open list ([j; i]), j of a periodic one ([i; j])
        sel = target_mask.detach().cpu().numpy().astype(bool)[i if cell is None else j]
        i, j, s = i[sel], j[sel], s[sel]
    return _lists_as_tensors(i, j, s, cell is not None, reference_compat, pos.device)
