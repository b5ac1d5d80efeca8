"""Device-side relation build (csrc/relation_kernels.hip) against a torch restatement of "stable sort by key":
every array the build produces -- the row order, the CSR arrays, the CSC arrays, the out-adjacency and all
row pointers -- compared with `torch.equal`, on lists that exercise every path of the counting sort:

  * a grouped list from the device search          (wave-aggregated claims: a few keys per wave)
  * the same list with its edges permuted          (ungrouped: one claim per distinct key per wave)
  * a padded list with thousands of NULL edges     (all of them on one counter)
  * unknown elements and out-of-range endpoints    (filed in the extra key range / as NULL edges)
  * groups of 0, 1, 15, 16, 17, 32, 33, 64, 65 and > 128 members, as CSR rows and as CSC groups, with both
    wave assignments of the rank sort              (the packing boundaries)
  * the 1024-molecule batch

The build is called through the C ABI with the optional out-adjacency switched on, which the Python wrapper leaves off."""
import ctypes

import numpy as np
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import _lib, synth
from hermnet_amd.relations import RelationalGraph

pytestmark = pytest.mark.gpu

ZL = [13, 28, 29]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _layout(z, zl, uniform):
    zl_t = torch.tensor(zl, dtype=torch.long, device=z.device)
    eq = z[:, None] == zl_t[None, :]
    T = len(zl)
    rel = torch.where(eq.any(1), eq.int().argmax(1), torch.full_like(z, T))
    cnt = torch.bincount(rel, minlength=T + 1).cpu().tolist()
    _, _, starts, N = RelationalGraph._layout(cnt, T, uniform)
    return rel, cnt, starts, N


def native_orders(z, ei, shift, zl, uniform=None):
    """`hermnet_build_relations` with every output, the out-adjacency included."""
    from hermnet_amd.ops import _stream
    lib, P = _lib.load(), _lib.ptr
    dev = z.device
    NA, E, T = int(z.numel()), int(ei.size(1)), len(zl)
    _, _, starts, N = _layout(z, zl, uniform)
    i32 = torch.int32
    e32 = lambda n: torch.full((n,), -7, dtype=i32, device=dev)
    o = dict(node_order=e32(NA), row_of_node=e32(NA), z_rows=e32(N), row_real=torch.empty(N, device=dev),
             row_active=torch.empty(N, device=dev), csr_rowptr=e32(N + 1), csr_src=e32(E), csr_perm=e32(E), src_id=e32(E),
             tgt_id=e32(E), shift=None if shift is None else torch.full((E, 3), 7.0, device=dev),
             csc_rowptr=e32(T * N + 1), csc_tgt=e32(E), csc_pos=e32(E), out_rowptr=e32(N + 1), out_edges=e32(E))
    out = _lib.RelationsOut(P(o["node_order"]), P(o["row_of_node"]), P(o["z_rows"]), P(o["row_real"]), P(o["row_active"]),
                            P(o["csr_rowptr"]), P(o["csr_src"]), P(o["csr_perm"]), P(o["src_id"]), P(o["tgt_id"]), P(o["shift"]),
                            P(o["csc_rowptr"]), P(o["csc_tgt"]), P(o["csc_pos"]), P(o["out_rowptr"]), P(o["out_edges"]))
    zl_d = torch.tensor(zl, dtype=i32, device=dev)
    rs_d = torch.tensor(starts[:T + 1], dtype=i32, device=dev)
    wbytes = lib.hermnet_build_relations_workspace(NA, N, E, T)
    work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    ei_c, sh_c = ei.long().contiguous(), None if shift is None else shift.float().contiguous()
    _lib.check(lib.hermnet_build_relations(P(z), P(ei_c), P(sh_c), NA, E, P(zl_d), T, P(rs_d), N, None, ctypes.byref(out), 0,
                                           P(work), wbytes, _stream()), "hermnet_build_relations")
    torch.cuda.synchronize()
    o["N"], o["starts"] = N, starts
    return o


def expected_orders(z, ei, shift, zl, uniform=None):
    """The same orders as stable sorts (torch)."""
    dev = z.device
    NA, E, T = int(z.numel()), int(ei.size(1)), len(zl)
    rel, cnt, starts, N = _layout(z, zl, uniform)
    x = {"N": N}
    x["node_order"] = torch.sort(rel, stable=True).indices
    first = torch.tensor([0] + np.cumsum(cnt[:T]).tolist(), device=dev)
    starts_d = torch.tensor(starts[:T + 1], device=dev)
    rel_s = rel[x["node_order"]]
    row_of_node = torch.empty(NA, dtype=torch.long, device=dev)
    row_of_node[x["node_order"]] = torch.arange(NA, device=dev) - first[rel_s] + starts_d[rel_s]
    x["row_of_node"] = row_of_node
    x["z_rows"] = torch.zeros(N, dtype=torch.long, device=dev)
    x["z_rows"][row_of_node] = z
    x["row_real"] = torch.zeros(N, device=dev)
    x["row_real"][row_of_node] = 1.0
    rel_row = torch.full((N,), T, dtype=torch.long, device=dev)
    for t in range(T):
        rel_row[starts[t]:starts[t + 1]] = t

    src, tgt = ei[0].long(), ei[1].long()
    real = (src >= 0) & (src < NA) & (tgt >= 0) & (tgt < NA)          # anything else is filed as a NULL edge
    R = int(real.sum())
    rs = row_of_node[src.clamp(0, NA - 1)]
    rt = torch.where(real, row_of_node[tgt.clamp(0, NA - 1)], torch.full_like(tgt, N))
    rt_s, perm = torch.sort(rt, stable=True)
    x["R"] = R
    x["csr_perm"] = perm[:R]
    x["csr_rowptr"] = torch.searchsorted(rt_s, torch.arange(N + 1, device=dev))
    zeros = torch.zeros(E - R, dtype=torch.long, device=dev)
    x["csr_src"] = torch.cat([rs[perm[:R]], zeros])                    # NULL edges: atom 0 onto itself, no shift
    x["src_id"] = torch.cat([src[perm[:R]], zeros])
    x["tgt_id"] = torch.cat([tgt[perm[:R]], zeros])
    if shift is not None:
        x["shift"] = torch.cat([shift[perm[:R]].float(), torch.zeros(E - R, 3, device=dev)])
    key2 = rel_row[rt_s[:R]] * N + x["csr_src"][:R]
    key2_s, csc_pos = torch.sort(key2, stable=True)
    x["csc_rowptr"] = torch.searchsorted(key2_s, torch.arange(T * N + 1, device=dev))
    K = int(x["csc_rowptr"][-1])                                        # edges with a known-relation target
    x["K"] = K
    x["csc_pos"] = csc_pos[:K]
    x["csc_tgt"] = rt_s[csc_pos[:K]]
    src_s, out_edges = torch.sort(x["csr_src"], stable=True)
    x["out_rowptr"] = torch.searchsorted(src_s, torch.arange(N + 1, device=dev))
    x["out_edges"] = out_edges
    tn = torch.arange(T + 1, device=dev) * N
    act = torch.cat([(x["csc_rowptr"][tn[1:]] - x["csc_rowptr"][tn[:-1]]) > 0, torch.zeros(1, dtype=torch.bool, device=dev)])
    x["row_active"] = act[rel_row].float() * x["row_real"]
    return x


def check(z, ei, shift, zl=ZL, uniform=None):
    nat, ref = native_orders(z, ei, shift, zl, uniform), expected_orders(z, ei, shift, zl, uniform)
    assert nat["N"] == ref["N"]
    names = ["node_order", "row_of_node", "z_rows", "row_real", "row_active", "csr_rowptr", "csr_perm", "csr_src", "src_id",
             "tgt_id", "csc_rowptr", "csc_pos", "csc_tgt", "out_rowptr", "out_edges"] + ([] if shift is None else ["shift"])
    for f in names:
        b = ref[f]
        a = nat[f][:b.size(0)]            # (csr_perm behind the real edges, csc_* behind the known targets: undefined)
        assert torch.equal(a if a.dtype == torch.float32 else a.long(), b), f
    return nat, ref


def _cell(reps=(6, 6, 6), unknown=False):
    dev = _dev()
    pos, cell, z = synth.fcc_alloy_atoms(reps=reps)
    if unknown:
        z = z.copy()
        z[::7] = 79
    pos_t = torch.from_numpy(pos.astype(np.float32)).to(dev)
    cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
    return pos_t, cell_t, torch.from_numpy(z).to(dev)


@pytest.mark.parametrize("uniform", [None, False])
def test_grouped_list_from_the_device_search(uniform):
    pos, cell, z = _cell()
    ei, sh = hn.neighbor_search(pos, 5.0, cell)
    assert ei.size(1) > 30000
    nat, ref = check(z, ei, sh, uniform=uniform)
    assert ref["R"] == ei.size(1) == ref["K"]


def test_the_same_list_with_its_edges_permuted():
    pos, cell, z = _cell()
    ei, sh = hn.neighbor_search(pos, 5.0, cell)
    p = torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(3)).to(ei.device)
    check(z, ei[:, p].contiguous(), sh[p].contiguous())


@pytest.mark.parametrize("extra", [5000, 0])
def test_padded_list_with_thousands_of_null_edges(extra):
    from hermnet_amd.neighbor import neighbor_search_padded
    pos, cell, z = _cell()
    E = int(hn.neighbor_search(pos, 5.0, cell)[0].size(1))
    eip, shp, _ = neighbor_search_padded(pos, 5.0, cell, E + extra)
    nat, ref = check(z, eip, shp)
    assert ref["R"] == E and int(nat["csr_rowptr"][-1]) == E


def test_unknown_element_and_out_of_range_endpoints():
    pos, cell, z = _cell(unknown=True)
    ei, sh = hn.neighbor_search(pos, 5.0, cell)
    ei = ei.clone()
    NA, E = z.numel(), ei.size(1)
    g = torch.Generator().manual_seed(5)
    bad = torch.randperm(E, generator=g)[:400].to(ei.device)
    ei[0, bad[:100]] = NA + 3               # source behind the atoms
    ei[1, bad[100:200]] = NA                # target behind the atoms
    ei[0, bad[200:300]] = -5                # negative source
    ei[1, bad[300:400]] = -1                # a NULL target in the middle of the list
    nat, ref = check(z, ei, sh)
    assert ref["R"] == E - 400 and ref["K"] < ref["R"]          # edges onto the unknown element are in no CSC segment


SIZES = [0, 1, 15, 16, 17, 32, 33, 64, 65, 130, 200]


def _sized_list(idle_atoms, seed):
    """Every atom of the first block receives SIZES[...] edges from distinct sources; quads of neighbouring rows mix the
    sizes.  `idle_atoms` atoms without edges: 67 (210 atoms) leaves the mean group size above the rank sort's switch of
    wave assignment (16 members), thousands pull it under."""
    rs = np.random.RandomState(seed)
    sizes = np.concatenate([rs.permutation(SIZES) for _ in range(11)] + [np.repeat(SIZES, 2)])
    NA = len(sizes) + idle_atoms
    src, tgt = [], []
    for t, n in enumerate(sizes):
        src.append((t + 1 + np.arange(n)) % 210)            # distinct sources of one target
        tgt.append(np.full(n, t))
    src, tgt = np.concatenate(src), np.concatenate(tgt)
    p = rs.permutation(len(src))
    return NA, torch.from_numpy(np.vstack([src[p], tgt[p]])).long()


@pytest.mark.parametrize("idle_atoms", [67, 6000])
@pytest.mark.parametrize("transposed", [False, True])
def test_group_sizes_at_the_packing_boundaries(idle_atoms, transposed):
    dev = _dev()
    NA, ei = _sized_list(idle_atoms, seed=11)
    if transposed:                         # the sizes as (relation, source) groups of the CSC order: one element only
        ei = ei.flip(0).contiguous()
        z, zl = torch.full((NA,), 13, dtype=torch.long), [13]
    else:
        z, zl = torch.from_numpy(np.random.RandomState(2).choice([13, 28], size=NA)), [13, 28]
    nat, ref = check(z.to(dev), ei.to(dev), None, zl=zl, uniform=False)
    groups = (len(zl) + 1) * NA if transposed else NA
    assert (ei.size(1) > 16 * groups) == (idle_atoms < 100)
    rp = ref["csc_rowptr"] if transposed else ref["csr_rowptr"]
    assert set(SIZES) <= set((rp[1:] - rp[:-1]).cpu().tolist())


def test_the_1024_molecule_batch():
    d = synth.molecule_batch(num_graphs=1024).to(_dev())
    check(d.atomic_number, d.edge_index, None, zl=[1, 6, 8])
