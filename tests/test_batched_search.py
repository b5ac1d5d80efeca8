"""The neighbour search of a BATCH of structures (hermnet_neighbor_batch_*, neighbor.neighbor_search(batch=...) /
neighbor_search_padded(batch=...), data.transform(per_graph=True)) and the replayed MD step of a batch
(graph.GraphedBatchMDStep).

The yardstick of every list is the project's float64 host list, `neighbor.neighbor_list`, run per structure and
concatenated with the atom offsets; indices and shifts are compared with `torch.equal` (no tolerance).  Each test first
asserts on the CPU that no candidate pair of its inputs lies within 1e-6 A of the cutoff (the "well-separated" precondition
of that bit-exactness): the host list for rc - 1e-6 and for rc + 1e-6 is the same list."""
import numpy as np
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import _lib, neighbor, synth
from hermnet_amd.neighbor import neighbor_list

RC = 5.0
BOUND = 1e-5            # the project's written bound on a structure of a batch against the same structure alone


# ---------------------------------------------------------------------------------------------------------------- inputs
def _ptr(batch, B):
    return np.searchsorted(np.asarray(batch), np.arange(B + 1))


def _join(structs, graph_ids=None):
    """[(pos float64 [n,3], cell [3,3] or None)] -> (pos float32 [N,3], batch int64 [N], cells float32 [B,3,3] or None)."""
    ids = list(range(len(structs))) if graph_ids is None else graph_ids
    pos = np.concatenate([s[0] for s in structs]).astype(np.float32)
    batch = np.concatenate([np.full(len(s[0]), g, dtype=np.int64) for s, g in zip(structs, ids)])
    cells = None if structs[0][1] is None else np.stack([s[1] for s in structs]).astype(np.float32)
    return pos, batch, cells


def _host_lists(pos, batch, cells, B, rc=RC):
    """The yardstick: (i, j, S) of `neighbor_list` per structure, atom offsets added, plus the well-separated check."""
    ptr = _ptr(batch, B)
    out = [[], [], []]
    for g in range(B):
        p, c = pos[ptr[g]:ptr[g + 1]], None if cells is None else cells[g]
        i, j, s = neighbor_list(p, rc, c)
        lo, hi = neighbor_list(p, rc - 1e-6, c), neighbor_list(p, rc + 1e-6, c)
        assert len(lo[0]) == len(i) == len(hi[0]), "a pair of structure %d lies within 1e-6 A of the cutoff" % g
        for k, v in enumerate((i + ptr[g], j + ptr[g], s)):
            out[k].append(v)
    return [np.concatenate(v) for v in out]


def _as_tensors(i, j, s, periodic):
    """The calling convention of `neighbor_search`: periodic [i; j] with edge_shift = -S, open [j; i]."""
    if periodic:
        return torch.from_numpy(np.vstack([i, j])).long(), torch.from_numpy(-s.astype(np.float32))
    return torch.from_numpy(np.vstack([j, i])).long(), None


def _fcc(reps, a=3.6, sigma=0.05, seed=0, shear=None, unwrap=None):
    pos, cell = synth._lattice(synth._FCC, a, reps)
    rs = np.random.RandomState(seed)
    pos = pos + rs.normal(scale=sigma, size=pos.shape)
    if shear is not None:
        m = np.eye(3) + np.asarray(shear)
        pos, cell = pos @ m, cell @ m
    if unwrap is not None:                     # whole lattice vectors added per atom: the same structure, unwrapped
        pos = pos + rs.randint(-unwrap, unwrap + 1, size=pos.shape).astype(np.float64) @ cell
    return pos, cell


def _periodic_four():
    """fcc cell of 3.6 A (smaller than the cutoff: reach 2, self-images) | 2x2x2 (one bin per axis) | sheared 3x3x3 |
    4x4x6 with coordinates unwrapped by up to +-2 cells."""
    return [_fcc((1, 1, 1), seed=11), _fcc((2, 2, 2), seed=12),
            _fcc((3, 3, 3), seed=13, shear=[[0, 0.08, 0], [0, 0, -0.05], [0.06, 0, 0]]),
            _fcc((4, 4, 6), seed=14, unwrap=2)]


def _ball(n, radius, seed, min_sep=0.9):
    rs = np.random.RandomState(seed)
    pts = []
    while len(pts) < n:
        p = rs.uniform(-radius, radius, size=3)
        if np.dot(p, p) <= radius * radius and (not pts or np.min(np.linalg.norm(np.asarray(pts) - p, axis=1)) >= min_sep):
            pts.append(p)
    pts = np.asarray(pts)
    return pts - pts.mean(0)                   # centred on the origin: the molecules of a batch overlap in space


def _open_molecules():
    """1, 2, 9 and 30 atoms in graphs 0, 1, 3, 4 of five: graph 2 is empty.  The 30-atom ball is wider than the cutoff."""
    return [(_ball(n, r, seed), None) for n, r, seed in ((1, 1.0, 21), (2, 1.5, 22), (9, 3.0, 23), (30, 4.5, 24))], [0, 1, 3, 4]


def _brute_force(pos, rc, cell):
    """O(N^2 images): every (i, j, S) with |pos_j - pos_i + S cell| < rc, canonical order."""
    pos = np.asarray(pos, dtype=np.float64)
    n, out = len(pos), []
    r = range(-3, 4) if cell is not None else (0,)
    c = np.zeros((3, 3)) if cell is None else np.asarray(cell, dtype=np.float64)
    for i in range(n):
        for j in range(n):
            for sx in r:
                for sy in r:
                    for sz in r:
                        if i == j and sx == sy == sz == 0:
                            continue
                        d = pos[j] - pos[i] + np.array([sx, sy, sz], dtype=np.float64) @ c
                        if d @ d < rc * rc:
                            out.append((i, j, sx, sy, sz))
    return np.asarray(sorted(out), dtype=np.int64).reshape(-1, 5)


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_host_batched_search_equals_the_per_structure_lists_and_a_brute_force():
    per = [_fcc((1, 1, 1), seed=11), _fcc((2, 2, 2), seed=12), _fcc((2, 2, 3), seed=15, shear=[[0, 0.05, 0], [0, 0, 0], [0, 0, 0]])]
    pos, batch, cells = _join(per)
    i, j, s = _host_lists(pos, batch, cells, 3)
    want_ei, want_sh = _as_tensors(i, j, s, True)
    ei, sh = hn.neighbor_search(torch.from_numpy(pos), RC, torch.from_numpy(cells), batch=torch.from_numpy(batch))
    assert torch.equal(ei, want_ei) and torch.equal(sh, want_sh) and ei.dtype == torch.long and sh.dtype == torch.float32
    ei2, sh2 = hn.neighbor_search(torch.from_numpy(pos), RC, torch.from_numpy(cells), reference_compat=True,
                                  batch=torch.from_numpy(batch), num_graphs=3)
    assert torch.equal(ei2, want_ei) and torch.equal(sh2, -want_sh)              # the reference's +S
    # the smallest structure against the brute force (3.6 A cell: images up to |S| = 2 are inside the cutoff)
    bf = _brute_force(pos[:4], RC, cells[0])
    n0 = int((batch[i] == 0).sum())
    assert n0 == len(bf) and np.array_equal(np.column_stack([i[:n0], j[:n0], s[:n0]]), bf)

    mols, ids = _open_molecules()
    pos, batch, _ = _join(mols[:3], ids[:3])                                      # graphs 0, 1, 3 of four: graph 2 is empty
    i, j, s = _host_lists(pos, batch, None, 4)
    want_ei, _ = _as_tensors(i, j, s, False)
    ei = hn.neighbor_search(torch.from_numpy(pos), RC, None, batch=torch.from_numpy(batch))
    assert torch.equal(ei, want_ei)
    assert torch.equal(hn.neighbor_search(torch.from_numpy(pos), RC, batch=torch.from_numpy(batch), num_graphs=4), want_ei)
    assert bool((torch.from_numpy(batch)[ei[0]] == torch.from_numpy(batch)[ei[1]]).all())      # no pair crosses graphs
    bf = _brute_force(pos[3:], RC, None)                                          # the 9-atom molecule
    sel = batch[i] == 3
    assert np.array_equal(np.column_stack([i[sel] - 3, j[sel] - 3]), bf[:, :2]) and not s.any()
    # ... whereas the unbatched search of the same coordinates pairs atoms of different molecules
    assert hn.neighbor_search(torch.from_numpy(pos), RC).size(1) > ei.size(1)

    with pytest.raises(NotImplementedError):
        hn.neighbor_search(torch.from_numpy(pos), RC, batch=torch.from_numpy(batch), target_mask=torch.ones(len(pos), dtype=torch.bool))
    with pytest.raises(ValueError):
        hn.neighbor_search(torch.from_numpy(pos), RC, batch=torch.from_numpy(batch[::-1].copy()))      # decreasing


def test_transform_default_is_unchanged_and_per_graph_searches_every_graph_with_its_own_cell():
    per = [_fcc((2, 2, 2), seed=12), _fcc((2, 2, 3), seed=15)]
    pos, batch, cells = _join(per)
    mk = lambda: hn.Data(pos=torch.from_numpy(pos), cell=torch.from_numpy(cells), batch=torch.from_numpy(batch),
                         atomic_number=torch.full((len(pos),), 13))
    d = hn.transform(mk(), RC)
    i, j, s = neighbor_list(pos, RC, cells[0])              # what it did before: ONE search, pairs across graphs, first cell
    want_ei, want_sh = _as_tensors(i, j, s, True)
    assert torch.equal(d.edge_index, want_ei) and torch.equal(d.edge_shift, want_sh)
    assert bool((d.batch[d.edge_index[0]] != d.batch[d.edge_index[1]]).any())
    dp = hn.transform(mk(), RC, per_graph=True)
    i, j, s = _host_lists(pos, batch, cells, 2)
    want_ei, want_sh = _as_tensors(i, j, s, True)
    assert torch.equal(dp.edge_index, want_ei) and torch.equal(dp.edge_shift, want_sh)
    # open systems, and a Data without `batch` (per_graph has nothing to split)
    mols, _ = _open_molecules()
    pos, batch, _ = _join(mols[1:3])
    do = hn.transform(hn.Data(pos=torch.from_numpy(pos), batch=torch.from_numpy(batch)), RC)
    i, j, _ = neighbor_list(pos, RC, None)
    assert torch.equal(do.edge_index, torch.from_numpy(np.vstack([j, i])))
    dq = hn.transform(hn.Data(pos=torch.from_numpy(pos), batch=torch.from_numpy(batch)), RC, per_graph=True)
    i, j, s = _host_lists(pos, batch, None, 2)
    assert torch.equal(dq.edge_index, _as_tensors(i, j, s, False)[0]) and dq.get("edge_shift") is None
    dn = hn.transform(hn.Data(pos=torch.from_numpy(pos)), RC, per_graph=True)
    assert torch.equal(dn.edge_index, do.edge_index) and torch.equal(dn.batch, torch.zeros(len(pos), dtype=torch.long))


def test_argument_checks_of_the_batched_search_need_no_gpu():
    lib = _lib.load()
    buf = np.zeros(256, dtype=np.float32)
    p = buf.ctypes.data
    ws = lib.hermnet_neighbor_batch_workspace(8, 3, 96)
    small = lib.hermnet_neighbor_batch_workspace(8, 3, 8)

    def count(n=8, b=3, pos=p, batch=p, cells=p, rc=RC, work=p, wbytes=ws, total=p):
        return lib.hermnet_neighbor_batch_count(pos, n, batch, b, cells, rc, work, wbytes, total, None)

    def fill(n=8, b=3, work=p, wbytes=ws, e=4, stash_ok=1, keys=None, ei=p):
        return lib.hermnet_neighbor_batch_fill(n, b, work, wbytes, e, -1.0, 0, stash_ok, keys, ei, p, None)

    def padded(n=8, b=3, work=p, wbytes=ws, cap=16, ei=p, total=p):
        return lib.hermnet_neighbor_batch_fill_padded(n, b, work, wbytes, cap, -1.0, 0, ei, p, total, None)

    assert count(b=0) == 1 and count(b=-1) == 1 and count(n=-1) == 1 and count(rc=0.0) == 1 and count(rc=float("nan")) == 1
    assert count(pos=None) == 1 and count(batch=None) == 1 and count(work=None) == 1 and count(total=None) == 1
    assert count(wbytes=small - 1) == 1 and count(b=4, wbytes=small) == 1           # a workspace too small for B
    assert count(n=2 ** 31 - 1, b=1, wbytes=2 ** 62) == 1                           # N * N * 17^3 beyond 64 bits
    assert count(n=70_000_000, b=1, wbytes=2 ** 62) == 1
    assert fill(n=0) == 1 and fill(b=0) == 1 and fill(e=-1) == 1 and fill(e=2 ** 31) == 1
    assert fill(work=None) == 1 and fill(ei=None) == 1 and fill(stash_ok=0, keys=None) == 1 and fill(wbytes=small - 1) == 1
    assert fill(e=0) == 0                                                            # nothing to write: done
    assert padded(n=0) == 1 and padded(b=0) == 1 and padded(cap=0) == 1 and padded(cap=2 ** 31) == 1
    assert padded(work=None) == 1 and padded(ei=None) == 1 and padded(total=None) == 1 and padded(wbytes=small - 1) == 1


def test_batched_workspace_query_grows_with_the_number_of_graphs():
    lib = _lib.load()
    q = lib.hermnet_neighbor_batch_workspace
    sizes = [q(1000, b, 96) for b in (1, 2, 16, 1024)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[0] >= lib.hermnet_neighbor_workspace_for(1000, 96)                 # the single search's arrays and more
    assert q(1000, 16, 8) < q(1000, 16, 96) < q(1000, 16, 160) == q(1000, 16, 1000)  # the stash slot: 8 .. 160 keys
    assert q(0, 5, 96) > 0                                                           # no atom: still a flags block
    assert q(1000, 0, 96) == 0 and q(-1, 1, 96) == 0 and q(2 ** 31 - 1, 1, 96) == 0  # shapes the search refuses


# ------------------------------------------------------------------------------------------------------------------- GPU
def _dev():
    return torch.device("cuda:0")


def _to(dev, pos, batch, cells):
    return (torch.from_numpy(pos).to(dev), torch.from_numpy(batch).to(dev), None if cells is None else torch.from_numpy(cells).to(dev))


@pytest.mark.gpu
def test_periodic_batch_equals_the_host_lists_and_four_single_device_searches():
    dev = _dev()
    per = _periodic_four()
    pos, batch, cells = _join(per)
    i, j, s = _host_lists(pos, batch, cells, 4)
    want_ei, want_sh = _as_tensors(i, j, s, True)
    assert np.abs(s).max() >= 4                           # (unwrapped coordinates: shifts of several cells are listed)
    assert (i[batch[i] == 0] == j[batch[i] == 0]).any()   # (self-images in the cell smaller than the cutoff)
    p, b, c = _to(dev, pos, batch, cells)
    ei, sh = hn.neighbor_search(p, RC, c, batch=b)                     # ONE call
    assert torch.equal(ei.cpu(), want_ei) and torch.equal(sh.cpu(), want_sh)
    ptr = _ptr(batch, 4)
    singles = [hn.neighbor_search(p[ptr[g]:ptr[g + 1]], RC, c[g]) for g in range(4)]
    assert torch.equal(ei, torch.cat([e + int(ptr[g]) for g, (e, _) in enumerate(singles)], 1))
    assert torch.equal(sh, torch.cat([x for _, x in singles]))
    ei2, sh2 = hn.neighbor_search(p, RC, c, reference_compat=True, batch=b, num_graphs=4)
    assert torch.equal(ei2, ei) and torch.equal(sh2, -sh)
    d = hn.transform(hn.Data(pos=p, cell=c, batch=b), RC, per_graph=True)
    assert torch.equal(d.edge_index, ei) and torch.equal(d.edge_shift, sh)


@pytest.mark.gpu
def test_open_batch_with_an_empty_graph_lists_no_pair_across_graphs():
    dev = _dev()
    mols, ids = _open_molecules()
    pos, batch, _ = _join(mols, ids)
    i, j, s = _host_lists(pos, batch, None, 5)
    want_ei, _ = _as_tensors(i, j, s, False)
    p, b, _ = _to(dev, pos, batch, None)
    ei = hn.neighbor_search(p, RC, None, batch=b)                      # (num_graphs from batch[-1])
    assert torch.equal(ei.cpu(), want_ei)
    assert bool((b[ei[0]] == b[ei[1]]).all())
    assert hn.neighbor_search(p, RC).size(1) > ei.size(1)             # the molecules do overlap in space
    assert torch.equal(hn.neighbor_search(p, RC, batch=b, num_graphs=7), ei)      # trailing empty graphs
    capped = hn.neighbor_search(p, RC, None, reference_compat=True, batch=b)     # the 32-neighbour cap, exact list only
    assert torch.equal(capped, neighbor._cap_neighbors(ei, 32))


@pytest.mark.gpu
def test_open_batch_equals_three_single_device_searches_coarsened_grid_included():
    """The batch's geometry is the single search's for open structures too: a 20-atom ball, a single atom, and two atoms
    60 A apart with nothing between them (10 x 6 x 2 bins of the cutoff's width against the 8 * 2 + 64 that two atoms are
    allowed: their grid is coarsened) give the concatenation of the three single device searches, atom offsets added."""
    dev = _dev()
    far = np.array([[-30.0, -17.0, -9.5], [22.0, 13.0, 4.5]])
    assert 60.0 < np.linalg.norm(far[1] - far[0]) and np.prod(np.floor((far[1] - far[0]) / RC)) > 8 * 2 + 64
    per = [(_ball(20, 4.0, 61), None), (_ball(1, 1.0, 62), None), (far, None)]
    pos, batch, _ = _join(per)
    i, j, s = _host_lists(pos, batch, None, 3)
    p, b, _ = _to(dev, pos, batch, None)
    ei = hn.neighbor_search(p, RC, None, batch=b, num_graphs=3)       # ONE call
    ptr = _ptr(batch, 3)
    singles = [hn.neighbor_search(p[ptr[g]:ptr[g + 1]], RC) for g in range(3)]
    assert singles[1].size(1) == 0 and singles[2].size(1) == 0 and singles[0].size(1) > 0
    assert torch.equal(ei, torch.cat([e + int(ptr[g]) for g, e in enumerate(singles)], 1))
    assert torch.equal(ei.cpu(), _as_tensors(i, j, s, False)[0])


@pytest.mark.gpu
def test_an_atom_with_more_pairs_than_its_stash_slot_takes_the_two_pass_fill(monkeypatch):
    dev = _dev()
    monkeypatch.setattr(neighbor, "_STASH", {})           # the default slot of 96 keys per atom
    per = [(_ball(120, 2.45, 31, min_sep=0.5), None), (_ball(5, 1.5, 32), None)]
    pos, batch, _ = _join(per)
    i, j, s = _host_lists(pos, batch, None, 2)
    assert np.bincount(i).max() > neighbor._STASH_DEFAULT
    p, b, _ = _to(dev, pos, batch, None)
    ei = hn.neighbor_search(p, RC, None, batch=b, num_graphs=2)
    assert neighbor._STASH.get(str(dev)) == 160           # flag bit 1 was met: this call finished in its two-pass form
    assert torch.equal(ei.cpu(), _as_tensors(i, j, s, False)[0])
    _, _, total = neighbor.neighbor_search_padded(p, RC, None, len(i) + 64, batch=b, num_graphs=2)
    assert total.tolist() == [len(i), 0]                  # (the larger slot holds them: the padded form is complete)


@pytest.mark.gpu
def test_padded_batched_search_and_its_flags(monkeypatch):
    dev = _dev()
    monkeypatch.setenv("HERMNET_DEBUG_POISON", "1")       # columns the search leaves unwritten would show
    per = _periodic_four()[:3]
    pos, batch, cells = _join(per)
    i, j, s = _host_lists(pos, batch, cells, 3)
    want_ei, want_sh = _as_tensors(i, j, s, True)
    E = len(i)
    p, b, c = _to(dev, pos, batch, cells)
    exact = hn.neighbor_search(p, RC, c, batch=b)
    cap = E + 333
    ei, sh, total = neighbor.neighbor_search_padded(p, RC, c, cap, batch=b, num_graphs=3)
    assert total.tolist() == [E, 0] and neighbor.padded_list_ok(total) == (True, E)
    assert torch.equal(ei[:, :E], exact[0]) and torch.equal(sh[:E], exact[1]) and torch.equal(ei[:, :E].cpu(), want_ei)
    assert bool((ei[:, E:] == -1).all()) and bool((sh[E:] == 0).all())           # NULL edges behind
    # fewer columns than pairs: flag bit 2, the columns that exist hold the list's first pairs
    ei, sh, total = neighbor.neighbor_search_padded(p, RC, c, E - 100, batch=b, num_graphs=3)
    assert total.tolist() == [E, 4]
    assert torch.equal(ei, exact[0][:, :E - 100]) and torch.equal(sh, exact[1][:E - 100])
    # a batch vector that decreases: flag bit 4, no pair at all
    b_bad = b.clone()
    b_bad[40] = 0
    ei, sh, total = neighbor.neighbor_search_padded(p, RC, c, cap, batch=b_bad, num_graphs=3)
    assert total.tolist() == [0, 16] and bool((ei == -1).all()) and bool((sh == 0).all())
    with pytest.raises(ValueError):
        hn.neighbor_search(p, RC, c, batch=b_bad, num_graphs=3)
    ei, sh, total = neighbor.neighbor_search_padded(p, RC, c, cap, batch=b + 1, num_graphs=3)      # a graph id beyond B
    assert total.tolist() == [0, 16] and bool((ei == -1).all())
    # one singular cell: flag bit 3, that structure lists nothing, the others' lists are what they were
    c_bad = c.clone()
    c_bad[1, 2] = c_bad[1, 1]
    ei, sh, total = neighbor.neighbor_search_padded(p, RC, c_bad, cap, batch=b, num_graphs=3)
    keep = torch.from_numpy(batch[i] != 1)
    n_keep = int(keep.sum())
    assert total.tolist() == [n_keep, 8]
    assert torch.equal(ei[:, :n_keep].cpu(), want_ei[:, keep]) and torch.equal(sh[:n_keep].cpu(), want_sh[keep])
    assert bool((ei[:, n_keep:] == -1).all()) and bool((sh[n_keep:] == 0).all())
    with pytest.raises(RuntimeError):
        hn.neighbor_search(p, RC, c_bad, batch=b)
    # open structures: the padded form needs no host read of a bounding box either
    mols, ids = _open_molecules()
    pos, batch, _ = _join(mols, ids)
    i, j, s = _host_lists(pos, batch, None, 5)
    p, b, _ = _to(dev, pos, batch, None)
    ei, sh, total = neighbor.neighbor_search_padded(p, RC, None, len(i) + 7, batch=b, num_graphs=5)
    assert sh is None and total.tolist() == [len(i), 0]
    assert torch.equal(ei[:, :len(i)].cpu(), _as_tensors(i, j, s, False)[0]) and bool((ei[:, len(i):] == -1).all())


def _model(dev, elems=("Al", "Ni", "Cu")):
    kw = dict(rc=RC, num_layers=3, hidden_channels=128, num_rbf=64)
    model = hn.HVNet(list(elems), **kw).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 8))
    model = model.to(dev)
    for p_ in model.parameters():
        p_.requires_grad_(False)
    return model


def _replicas():
    """Three replicas of the 32-atom cell (different jitters) and one 108-atom cell; species of the alloy."""
    per = [_fcc((2, 2, 2), seed=41), _fcc((2, 2, 2), seed=42), _fcc((2, 2, 2), seed=43), _fcc((3, 3, 3), seed=44)]
    rs = np.random.RandomState(45)
    z = np.asarray((13, 28, 29), dtype=np.int64)[rs.randint(0, 3, size=sum(len(s[0]) for s in per))]
    return per, z


def _walk(per, steps):
    """The structures moved (+-0.1 A per atom) and strained (a few percent, another strain per structure) step by step."""
    rs = np.random.RandomState(46)
    for _ in range(steps):
        out = []
        for pos, cell in per:
            eps = rs.uniform(-0.03, 0.03, size=(3, 3))
            m = np.eye(3) + 0.5 * (eps + eps.T)
            out.append(((pos + rs.uniform(-0.1, 0.1, size=pos.shape)) @ m, cell @ m))
        yield out


@pytest.mark.gpu
@pytest.mark.parametrize("stress", [False, True])
def test_batched_md_step_replays_periodic_replicas_as_one_graph(stress):
    from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep
    dev = _dev()
    per, z = _replicas()
    pos, batch, cells = _join(per)
    ptr = _ptr(batch, 4)
    p, b, c = _to(dev, pos, batch, cells)
    z_t = torch.from_numpy(z).to(dev)
    model = _model(dev)
    n_first = int(hn.neighbor_search(p, RC, c, batch=b)[0].size(1))
    step = GraphedBatchMDStep(model, z_t, c, p, b, 4, capacity=int(1.3 * n_first), stress=stress)
    captured = step.graph
    counts = set()
    for it, cur in enumerate(_walk(per, 4)):
        pos, _, cells = _join(cur)
        i, j, s = _host_lists(pos, batch, cells, 4)
        p, _, c = _to(dev, pos, batch, cells)
        out = [t.clone() for t in step(p, c)]
        host = step.fetch()
        ei, sh = hn.neighbor_search(p, RC, c, batch=b, num_graphs=4)
        assert torch.equal(ei.cpu(), _as_tensors(i, j, s, True)[0])
        d = hn.Data(pos=p.clone(), atomic_number=z_t, batch=b, cell=c, edge_index=ei, edge_shift=sh)
        ref = hn.energy_forces_stress(model, d)                       # eager, on the exact batched list
        torch.zeros(1 << 16, device=dev).sum()
        assert host[2] and host[3] == len(i) == int(ei.size(1)), (it, host[3], len(i))
        assert out[0].shape == (4,) and torch.equal(out[0], ref["energy"]) and torch.equal(out[1], ref["forces"]), it
        assert np.array_equal(host[0], ref["energy"].cpu().numpy()) and np.array_equal(host[1], ref["forces"].cpu().numpy())
        assert len(out) == (3 if stress else 2) and len(host) == (5 if stress else 4)
        if stress:
            assert out[2].shape == (4, 3, 3) and torch.equal(out[2], ref["virial"]), it
            assert np.array_equal(host[4], ref["virial"].cpu().numpy())
        counts.add(host[3])
    assert len(counts) > 1 and step.graph is captured and step.check() == (True, host[3]) and not step.stale()
    # every structure of the last step against the same structure alone
    for g in range(4):
        sl = slice(int(ptr[g]), int(ptr[g + 1]))
        if stress:
            e1, s1 = hn.neighbor_search(p[sl], RC, c[g])
            alone = hn.energy_forces_stress(model, hn.Data(pos=p[sl].clone(), atomic_number=z_t[sl], cell=c[g:g + 1],
                                                           batch=torch.zeros(sl.stop - sl.start, dtype=torch.long, device=dev),
                                                           edge_index=e1, edge_shift=s1))
            w1 = alone["virial"][0]
            assert float((out[2][g] - w1).abs().max()) <= BOUND * float(w1.abs().max()), g
            e_alone, f_alone = alone["energy"], alone["forces"]
        else:
            e_alone, f_alone = [t.clone() for t in GraphedMDStep(model, z_t[sl], c[g], p[sl])()]
        assert float((out[0][g] - e_alone[0]).abs()) <= BOUND * float(e_alone[0].abs()), g
        assert float((out[1][sl] - f_alone).abs().max()) <= BOUND * float(f_alone.abs().max()), g


@pytest.mark.gpu
def test_batched_md_step_replays_open_molecules_without_a_host_read():
    from hermnet_amd.graph import GraphedBatchMDStep
    dev = _dev()
    mols = [(_ball(n, r, seed), None) for n, r, seed in ((9, 3.0, 51), (14, 3.2, 52), (30, 4.5, 53), (22, 4.0, 54))]
    pos, batch, _ = _join(mols)
    z = np.asarray((1, 6, 8), dtype=np.int64)[np.random.RandomState(55).randint(0, 3, size=len(pos))]
    p, b, _ = _to(dev, pos, batch, None)
    z_t = torch.from_numpy(z).to(dev)
    model = _model(dev, ("H", "C", "O"))
    n_first = int(hn.neighbor_search(p, RC, batch=b, num_graphs=4).size(1))
    step = GraphedBatchMDStep(model, z_t, None, p, b, 4, capacity=int(1.3 * n_first))
    with pytest.raises(RuntimeError):
        step(p, torch.eye(3, device=dev).repeat(4, 1, 1))             # open structures have no cell to replace
    rs = np.random.RandomState(56)
    counts = set()
    for it in range(4):
        scale = 1.0 + 0.04 * it                                       # the molecules swell: pairs leave the cutoff
        cur = [((m[0] + rs.uniform(-0.05, 0.05, size=m[0].shape)) * scale, None) for m in mols]
        pos, _, _ = _join(cur)
        i, j, s = _host_lists(pos, batch, None, 4)
        p, _, _ = _to(dev, pos, batch, None)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                       # any host synchronisation inside the step raises
        try:
            e, f = step(p)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        he, hf, ok, n = step.fetch()                                  # the ONE synchronisation: the packed copy
        ei = hn.neighbor_search(p, RC, batch=b, num_graphs=4)
        assert ok and n == len(i) and torch.equal(ei.cpu(), _as_tensors(i, j, s, False)[0]), it
        d = hn.Data(pos=p.clone().requires_grad_(True), atomic_number=z_t, batch=b, edge_index=ei)
        e0 = model(d)
        f0 = -torch.autograd.grad(e0.sum(), d.pos)[0]
        assert torch.equal(e, e0.detach()) and torch.equal(f, f0), it
        assert np.array_equal(he, e0.detach().cpu().numpy()) and np.array_equal(hf, f0.cpu().numpy())
        counts.add(n)
    assert len(counts) > 1
