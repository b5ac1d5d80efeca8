"""Neighbour lists and edge geometry on hostile cells, against a brute force that shares nothing with either cell list.

Every model-level comparison of the suite hands ONE list to both sides, so a missing or duplicated pair passes them all; the
list's own ground truth is what this file adds.  The cases: strongly skewed, left-handed and unreduced cells, a cell whose
plane spacing asks for reach 8 (the largest the kernels accept), a periodic grid sparse enough to be coarsened, atoms on cell
faces, coincident atoms, pairs exactly on the cutoff, positions many cells outside the cell (image shifts up to 7, and
beyond 8: flag bit 0), open structures of zero extent and of 10^4 A, and a single atom.

`_brute` is the reference: float64 on the float32-rounded inputs (the numbers the device widens), a dense distance matrix per
periodic image, strict `<`, (i, i, 0) excluded, lexsorted by (i, j, Sx, Sy, Sz).  It works on the caller's positions and
never wraps them.  The host list, the device list and the brute force form a distance differently and may disagree in its
last ulps, so every case must satisfy the BAND CONDITION: no pair with 0 < |d - rc| <= 1e-7 rc.  That is a condition on the
inputs (the seeds below are chosen for it; the CPU tests show a bad seed before anything runs on a GPU), not a tolerance on
the result: with it, every list comparison here is exact.

`single` (one atom, diag(6, 6, 6), rc 5) lists no pair, periodic or open -- the nearest self-image is 6 A away -- so
`single_tight` (one atom, diag(4, 4.5, 6): four self-images inside the cutoff) stands beside it for what consumes self-image
edges."""
import functools
import itertools

import numpy as np
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import neighbor
from hermnet_amd.neighbor import neighbor_list

BATCH_RC = 5.0        # the one cutoff of the periodic batch (the batched search takes one)
OPEN_RC = 3.0


def _f64(a):
    """float32-rounded values as float64: exactly the numbers the device widens."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _heights(cell):
    return 1.0 / np.linalg.norm(np.linalg.inv(cell), axis=0)


def _nimg(pos, cell, rc):
    """Images per axis the brute force has to look at: ceil(rc / h_k) + the largest wrap difference of the case + 1."""
    if cell is None:
        return None
    w = np.floor(pos @ np.linalg.inv(cell))
    return tuple(int(v) for v in np.ceil(rc / _heights(cell)) + (w.max(0) - w.min(0)) + 1)


def _brute(pos, cell, rc, nimg):
    """(i, j, S, band): every (i, j, S) with |pos[j] + S @ cell - pos[i]| < rc except (i, i, 0), lexsorted, and the number
    of pairs with 0 < |d - rc| <= 1e-7 rc.  `nimg` [3]: S runs over range(-nimg_k, nimg_k + 1) per axis (None: open)."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    if cell is None:
        shifts = np.zeros((1, 3), dtype=np.int64)
        vecs = np.zeros((1, 3))
    else:
        shifts = np.array(list(itertools.product(*[range(-m, m + 1) for m in nimg])), dtype=np.int64)
        vecs = shifts.astype(np.float64) @ np.asarray(cell, dtype=np.float64)
    I, J, S, band = [], [], [], 0
    step = max(1, 3000000 // max(1, n * n))
    for c0 in range(0, len(shifts), step):
        sv = vecs[c0:c0 + step]
        dm = np.linalg.norm(pos[None, None, :, :] + sv[:, None, None, :] - pos[None, :, None, :], axis=-1)     # [m, i, j]
        band += int(np.count_nonzero((np.abs(dm - rc) <= 1e-7 * rc) & (dm != rc)))
        m, ii, jj = np.nonzero(dm < rc)
        ss = shifts[c0 + m]
        keep = ~((ii == jj) & ~ss.any(axis=1))
        I.append(ii[keep]), J.append(jj[keep]), S.append(ss[keep])
    I, J, S = np.concatenate(I), np.concatenate(J), np.concatenate(S)
    k = np.lexsort((S[:, 2], S[:, 1], S[:, 0], J, I))
    return I[k].astype(np.int64), J[k].astype(np.int64), S[k], band


# ---- the cases: name -> (seed, builder(rs) -> (pos, cell or None, rc)); everything is rounded to float32 ------------------
_C30, _S30 = np.cos(np.pi / 6), np.sin(np.pi / 6)
_ORTHO = np.diag([8.0, 8.5, 9.0])


def _in_cell(rs, n, cell):
    return rs.uniform(0, 1, size=(n, 3)) @ cell


def _skew30(rs):
    cell = np.array([[10.0, 0, 0], [10 * _C30, 10 * _S30, 0], [3.0, 2.0, 9.0]])
    return _in_cell(rs, 40, cell), cell, 4.0


def _left_handed(rs):
    cell = np.array([[0, 9.5, 0], [9.0, 0, 0], [1.0, -1.0, 10.0]])
    return _in_cell(rs, 40, cell), cell, 4.0


def _unimodular(rs):
    cell = np.array([[1, 2, 0], [0, 1, 0], [1, 0, 1]], dtype=np.float64) @ np.diag([9.0, 9.5, 10.0])
    return _in_cell(rs, 40, cell), cell, 4.0


def _needle(rs):
    cell = np.diag([3.0, 3.2, 40.0])
    return _in_cell(rs, 30, cell), cell, 5.0


def _reach8(rs):
    cell = np.array([[0.7, 0, 0], [0.1, 9.0, 0], [0, 0.3, 9.0]])
    return _in_cell(rs, 3, cell), cell, 5.0


def _sparse(rs):
    # one pair across the x face, one pair inside; 20^3 bins of the cutoff's width against the 8 N + 64 = 96 of four atoms
    pos = np.array([[0.5, 30.0, 30.0], [59.0, 30.5, 30.0], [20.0, 20.0, 20.0], [21.5, 20.5, 19.0]])
    return pos + rs.uniform(-0.05, 0.05, size=pos.shape), np.diag([60.0, 60.0, 60.0]), 3.0


def _lattice_on_cutoff(rs):
    pos = np.array([[0, 0, 0], [8, 0, 0], [4, 4, 8], [4, 4, 8], [3, 4, 0], [0, 8, 16], [-0.0, 3, 12], [4, 0, 3], [7, 4, 4],
                    [1, 1, 1]], dtype=np.float64)
    return pos, np.diag([8.0, 8.0, 16.0]), 5.0


def _unwrapped3(rs):
    return _in_cell(rs, 30, _ORTHO) + rs.randint(-3, 4, size=(30, 3)) @ _ORTHO, _ORTHO, 3.5


def _unwrapped6(rs):
    return _in_cell(rs, 30, _ORTHO) + rs.randint(-6, 7, size=(30, 3)) @ _ORTHO, _ORTHO, 3.5


def _open_line(rs):
    pos = np.zeros((25, 3))
    pos[:, 0] = rs.uniform(0.0, 30.0, size=25)
    return pos, None, 3.0


def _open_far(rs):
    a, b = rs.uniform(0, 4, size=(10, 3)), rs.uniform(0, 4, size=(10, 3)) + np.array([1.0e4, 0, 0])
    twin = np.array([[5000.0, 1.5, 2.5]])
    return np.concatenate([a, twin, b, twin]), None, 3.0


_BUILDERS = {
    "skew30": (11, _skew30), "left_handed": (12, _left_handed), "unimodular": (13, _unimodular), "needle": (14, _needle),
    "reach8": (15, _reach8), "sparse": (16, _sparse), "lattice_on_cutoff": (17, _lattice_on_cutoff),
    "unwrapped3": (18, _unwrapped3), "unwrapped6": (19, _unwrapped6), "open_line": (20, _open_line),
    "open_far": (21, _open_far),
    "single": (22, lambda rs: (_in_cell(rs, 1, np.diag([6.0, 6.0, 6.0])), np.diag([6.0, 6.0, 6.0]), 5.0)),
    "single_open": (22, lambda rs: (_in_cell(rs, 1, np.diag([6.0, 6.0, 6.0])), None, 5.0)),
    "single_tight": (23, lambda rs: (_in_cell(rs, 1, np.diag([4.0, 4.5, 6.0])), np.diag([4.0, 4.5, 6.0]), 5.0)),
}
PERIODIC = ["skew30", "left_handed", "unimodular", "needle", "reach8", "sparse", "lattice_on_cutoff", "unwrapped3",
            "unwrapped6", "single", "single_tight"]
OPEN = ["open_line", "open_far", "single_open"]
ALL = PERIODIC + OPEN
BATCHED = [c for c in PERIODIC if c != "unwrapped6"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(pos, cell or None, rc) of a case, float32 values as float64."""
    seed, build = _BUILDERS[name]
    pos, cell, rc = build(np.random.RandomState(seed))
    return _f64(pos), None if cell is None else _f64(cell), rc


@functools.lru_cache(maxsize=None)
def _ref_at(name, rc):
    pos, cell, _ = _case(name)
    return _brute(pos, cell, rc, _nimg(pos, cell, rc))


def _ref(name, rc=None):
    """The brute-force list of a case (at its own cutoff, or at `rc`), computed once: (i, j, S, band)."""
    return _ref_at(name, _case(name)[2] if rc is None else float(rc))


def _as_tensors(i, j, s, periodic):
    """`neighbor_search`'s conventions: periodic [i; j] with edge_shift = -S, open [j; i]."""
    if not periodic:
        return torch.from_numpy(np.vstack([j, i])), None
    return torch.from_numpy(np.vstack([i, j])), torch.from_numpy(-s.astype(np.float32))


# ---- re-basing: the same lattice in another basis --------------------------------------------------------------------------
_REBASE_M = {
    "shear": np.array([[1, 1, 0], [0, 1, 0], [0, 0, 1]]),
    "shear_cubed": np.array([[1, 3, 0], [0, 1, 0], [0, 0, 1]]),
    "unimodular": np.array([[1, 2, 0], [0, 1, 0], [1, 0, 1]]),
    "row_swap": np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]]),
}
REBASE_RC = 4.0


@functools.lru_cache(maxsize=None)
def _rebase_base():
    """A cell whose entries are multiples of 1/8 A and 40 positions rounded to 1/1024 A: M @ cell is exact in float32 for the
    integer matrices above, and so is every image vector S @ (M @ cell) = (S @ M) @ cell and every difference of positions."""
    rs = np.random.RandomState(31)
    cell = np.array([[9.0, 0, 0], [1.5, 9.5, 0], [0.75, -1.25, 10.0]])
    pos = np.round(_in_cell(rs, 40, cell) * 1024.0) / 1024.0
    assert np.array_equal(_f64(cell), cell) and np.array_equal(_f64(pos), pos)
    assert np.array_equal(np.linalg.matrix_power(_REBASE_M["shear"], 3), _REBASE_M["shear_cubed"])
    return pos, cell


@functools.lru_cache(maxsize=None)
def _rebase_ref(which):
    pos, cell = _rebase_base()
    c = cell if which == "base" else _REBASE_M[which].astype(np.float64) @ cell
    assert np.array_equal(_f64(c), c)
    return (pos, c) + _brute(pos, c, REBASE_RC, _nimg(pos, c, REBASE_RC))


def _to_base(i, j, s, which):
    """A list found in the re-based cell M @ cell, expressed in the base cell: same (i, j), S_base = S @ M, sorted again."""
    sb = s @ _REBASE_M[which]
    k = np.lexsort((sb[:, 2], sb[:, 1], sb[:, 0], j, i))
    return i[k], j[k], sb[k]


# =================================================================================================================== CPU
@pytest.mark.parametrize("name", ALL)
def test_host_list_equals_the_brute_force_and_the_band_is_empty(name):
    pos, cell, rc = _case(name)
    I, J, S, band = _ref(name)
    assert band == 0, "%d pairs within 1e-7 rc of the cutoff: choose another seed" % band
    i, j, s = neighbor_list(pos, rc, cell)
    assert np.array_equal(i, I) and np.array_equal(j, J) and np.array_equal(s, S)
    assert not ((I == J) & ~S.any(axis=1)).any()
    if cell is not None and len(I):       # what the list promises the model: |pos[j] - pos[i] + S cell| < rc
        assert np.linalg.norm(pos[J] - pos[I] + S @ cell, axis=1).max() < rc
    if name in BATCHED and rc != BATCH_RC:      # the periodic batch runs every structure at one cutoff
        I, J, S, band = _ref(name, BATCH_RC)
        assert band == 0, "%d pairs within 1e-7 rc of the batch's cutoff: choose another seed" % band
        i, j, s = neighbor_list(pos, BATCH_RC, cell)
        assert np.array_equal(i, I) and np.array_equal(j, J) and np.array_equal(s, S)
    if name in BATCHED:                   # (the padded batch is asked for flags 0: no atom beyond the default stash slot)
        assert len(I) == 0 or np.bincount(_ref(name, BATCH_RC)[0]).max() <= neighbor._STASH_DEFAULT


def test_the_cases_are_what_their_names_say():
    """What each case is for, stated on the brute-force lists and an independent inverse (numpy's)."""
    h = lambda n: _heights(_case(n)[1])
    smax = lambda n: int(np.abs(_ref(n)[2]).max())
    c = _case("skew30")[1]
    assert h("skew30")[0] < 0.5 * np.linalg.norm(c[0])                             # plane spacing << vector length
    assert np.linalg.det(_case("left_handed")[1]) < 0
    assert smax("unimodular") == 2
    assert np.ceil(5.0 / h("needle")).tolist() == [2, 2, 1]
    I, J, S, _ = _ref("needle")
    assert ((I == J).sum() > 0) and 30 <= len(I) / 30 <= 60                        # self-images; tens of pairs per atom
    assert np.ceil(5.0 / h("reach8")).tolist() == [8, 1, 1] and smax("reach8") == 7
    I, J, S, _ = _ref("sparse")
    assert sorted(zip(I.tolist(), J.tolist(), map(tuple, S.tolist()))) == [(0, 1, (-1, 0, 0)), (1, 0, (1, 0, 0)),
                                                                           (2, 3, (0, 0, 0)), (3, 2, (0, 0, 0))]
    assert 3 <= smax("unwrapped3") <= 7 and smax("unwrapped6") > 8
    I, J, S, _ = _ref("open_far")
    assert (10, 21) in set(zip(I.tolist(), J.tolist())) and (21, 10) in set(zip(I.tolist(), J.tolist()))
    assert len(_ref("single")[0]) == 0 and len(_ref("single_open")[0]) == 0
    I, J, S, _ = _ref("single_tight")
    assert sorted(map(tuple, S.tolist())) == [(-1, 0, 0), (0, -1, 0), (0, 1, 0), (1, 0, 0)]
    p = _case("open_line")[0]
    assert not p[:, 1:].any() and len(_ref("open_line")[0]) > 0


def test_lattice_on_cutoff_is_exact():
    """Integer coordinates and power-of-two cell edges: every fractional coordinate, product and d^2 is exact, so the list is
    known without a band: coincident atoms (distinct ones and periodic copies) once each way at d = 0, a pair at exactly rc
    not listed, no (i, i, 0), atoms at fractional coordinate exactly 0 or 1 found once."""
    pos, cell, rc = _case("lattice_on_cutoff")
    I, J, S, band = _ref("lattice_on_cutoff")
    d = np.linalg.norm(pos[J] - pos[I] + S @ cell, axis=1)
    trip = list(zip(I.tolist(), J.tolist(), map(tuple, S.tolist())))
    assert len(set(trip)) == len(trip)
    # coincident: atoms 2 and 3; the origin (0), (8, 0, 0) (1) and (0, 8, 16) (5) are periodic copies of one point
    zero = sorted(t for t, dd in zip(trip, d) if dd == 0.0)
    assert zero == sorted([(2, 3, (0, 0, 0)), (3, 2, (0, 0, 0)), (0, 1, (-1, 0, 0)), (1, 0, (1, 0, 0)), (0, 5, (0, -1, -1)),
                           (5, 0, (0, 1, 1)), (1, 5, (1, -1, -1)), (5, 1, (-1, 1, 1))])
    # exactly on the cutoff: (3, 4, 0), (4, 0, 3) and (0, 3, 12) = (0, 3, -4) + c are 5 A from the origin -- never listed
    pairs = set((a, b) for a, b, _ in trip)
    for a in (0, 1, 5):
        for b in (4, 7, 6):
            assert (a, b) not in pairs and (b, a) not in pairs
    assert (d < rc).all() and d[d > 0].min() >= 1.0
    i, j, s = neighbor_list(pos, rc, cell)
    assert np.array_equal(i, I) and np.array_equal(j, J) and np.array_equal(s, S)


@pytest.mark.parametrize("which", sorted(_REBASE_M))
def test_rebasing_is_exact_on_the_host(which):
    """The lists of one lattice in two bases map one to one: same (i, j), S_base = S_rebased @ M -- for the brute force
    (whose image vectors are exact here) and for `neighbor_list`."""
    pos, cell, I, J, S, band = _rebase_ref("base")
    _, cm, Im, Jm, Sm, band_m = _rebase_ref(which)
    assert band == 0 and band_m == 0 and len(I) > 0
    assert abs(round(np.linalg.det(_REBASE_M[which]))) == 1
    got = _to_base(Im, Jm, Sm, which)
    assert np.array_equal(got[0], I) and np.array_equal(got[1], J) and np.array_equal(got[2], S)
    i, j, s = neighbor_list(pos, REBASE_RC, cm)
    assert np.array_equal(i, Im) and np.array_equal(j, Jm) and np.array_equal(s, Sm)
    got = _to_base(i, j, s, which)
    assert np.array_equal(got[0], I) and np.array_equal(got[1], J) and np.array_equal(got[2], S)


@functools.lru_cache(maxsize=None)
def _virial_batch():
    """`needle`, `reach8`, the single atoms and two needle-like cells of 257 and 255 atoms as one batch at rc 3: (pos, cells,
    batch, edge_index, edge_shift, pairs in the band)."""
    rc = 3.0
    rs = np.random.RandomState(41)
    parts = [(_case(nm)[0], _case(nm)[1]) for nm in ("needle", "reach8", "single", "single_tight")]
    for n_big, cz in ((257, 64.0), (255, 63.5)):
        cell = np.diag([6.0, 6.5, cz])
        parts.append((_f64(_in_cell(rs, n_big, cell)), cell))
    pos, cells, batch, ii, jj, ss, off, bands = [], [], [], [], [], [], 0, 0
    for g, (p_, c_) in enumerate(parts):
        I, J, S, band = _brute(p_, c_, rc, _nimg(p_, c_, rc))
        bands += band
        pos.append(p_), cells.append(c_), batch.append(np.full(len(p_), g, dtype=np.int64))
        ii.append(I + off), jj.append(J + off), ss.append(S)
        off += len(p_)
    assert off == 30 + 3 + 1 + 1 + 257 + 255
    ei, sh = _as_tensors(np.concatenate(ii), np.concatenate(jj), np.concatenate(ss), True)
    return (torch.from_numpy(np.concatenate(pos).astype(np.float32)), torch.from_numpy(np.stack(cells).astype(np.float32)),
            torch.from_numpy(np.concatenate(batch)), ei, sh, bands)


@functools.lru_cache(maxsize=None)
def _coincident():
    """Twelve atoms in the cell of `skew30`, the first two (an Al and a Ni) on one point: (pos, cell, rc, i, j, S, band)."""
    rs = np.random.RandomState(51)
    cell = _case("skew30")[1]
    pos = _f64(_in_cell(rs, 12, cell))
    pos[1] = pos[0]
    return (pos, cell, 4.0) + _brute(pos, cell, 4.0, _nimg(pos, cell, 4.0))


def test_the_structures_of_the_consumer_tests_have_an_empty_band_too():
    assert _virial_batch()[5] == 0
    pos, cell, rc, I, J, S, band = _coincident()
    assert band == 0 and (0, 1, (0, 0, 0)) in set(zip(I.tolist(), J.tolist(), map(tuple, S.tolist())))
    i, j, s = neighbor_list(pos, rc, cell)
    assert np.array_equal(i, I) and np.array_equal(j, J) and np.array_equal(s, S)


def test_search_geometry_of_the_hostile_cells():
    """The search's one geometry routine (`nbr_make_geom`, through its host probe) on these cells, against what a grid must
    satisfy rather than a restatement of its text: bins at least rc wide, `reach` bins cover the cutoff sphere, the bin
    count inside the workspace's 8 N + 64; reach 8 is accepted; the periodic grid of `sparse` is coarsened."""
    import ctypes
    from hermnet_amd import _lib
    lib = _lib.load()
    for name in PERIODIC:
        pos, cell, rc = _case(name)
        n = len(pos)
        geom, grid = np.zeros(22), np.zeros(7, dtype=np.int32)
        assert lib.hermnet_host_neighbor_geometry((ctypes.c_double * 9)(*cell.reshape(-1)), None, None, rc, n, geom.ctypes.data,
                                                  grid.ctypes.data) == 0, name
        nb, reach, hk = grid[:3].astype(np.int64), grid[3:6].astype(np.int64), _heights(cell)
        assert grid[6] == 1 and (nb >= 1).all() and nb.prod() <= 8 * n + 64, name
        assert ((hk / nb >= rc * (1 - 1e-12)) | (nb == 1)).all(), name
        assert (reach * (hk / nb) >= rc * (1 - 1e-9)).all() and (reach <= 8).all(), name
        assert np.allclose(geom[9:18].reshape(3, 3), np.linalg.inv(cell), rtol=1e-12, atol=1e-15), name
        if name == "reach8":
            assert reach.tolist() == [8, 1, 1] and nb.tolist() == [1, 1, 1]
        if name == "sparse":
            assert nb.tolist() == [3, 5, 5] and reach.tolist() == [1, 1, 1]
    pos, _, rc = _case("open_far")
    geom, grid = np.zeros(22), np.zeros(7, dtype=np.int32)
    lo, hi = pos.min(0), pos.max(0)
    assert lib.hermnet_host_neighbor_geometry(None, (ctypes.c_double * 3)(*lo), (ctypes.c_double * 3)(*hi), rc, len(pos),
                                              geom.ctypes.data, grid.ctypes.data) == 0
    nb = grid[:3].astype(np.int64)
    assert nb.tolist() == [128, 1, 1] and nb.prod() <= 8 * len(pos) + 64              # 3333 -> clamp 1024 -> coarsened
    assert (1.0 / geom[[9, 13, 17]] >= rc).all()                                      # bin widths


# =================================================================================================================== GPU
def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _gpu_inputs(name, dev):
    pos, cell, rc = _case(name)
    p = torch.from_numpy(pos.astype(np.float32)).to(dev)
    c = None if cell is None else torch.from_numpy(cell.astype(np.float32)).to(dev)
    return p, c, rc


def _want(name, rc=None):
    I, J, S, band = _ref(name, rc)
    assert band == 0
    return _as_tensors(I, J, S, _case(name)[1] is not None)


def _assert_list(got, want, periodic, what):
    if periodic:
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), what
    else:
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want[0]), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_device_search_equals_the_brute_force(name):
    """`neighbor_search` on GPU tensors (cell on the host).  `unwrapped6` raises flag bit 0 on the device and is answered from
    the host list: the result is the brute force's all the same."""
    dev = _dev()
    p, c, rc = _gpu_inputs(name, dev)
    got = hn.neighbor_search(p, rc, c)
    _assert_list(got, _want(name), c is not None, name)
    if name == "unwrapped6":
        assert neighbor._device_search(p, rc, c, False) is None


@pytest.mark.gpu
@pytest.mark.parametrize("name", PERIODIC)
def test_padded_device_cell_search_equals_the_brute_force(name, monkeypatch):
    """The captured steps' form: the cell read from device memory, the list padded to a capacity with NULL edges."""
    dev = _dev()
    monkeypatch.setenv("HERMNET_DEBUG_POISON", "1")          # columns the search leaves unwritten would show
    monkeypatch.setattr(neighbor, "_STASH", {})
    p, c, rc = _gpu_inputs(name, dev)
    I, J, S, band = _ref(name)
    want_ei, want_sh = _want(name)
    E, N = len(I), p.size(0)
    cap = neighbor.padded_capacity(E)
    ei, sh, total = neighbor.neighbor_search_padded(p, rc, c, cap, device_cell=True)
    assert ei.shape == (2, cap) and sh.shape == (cap, 3)
    ei, sh = ei.cpu(), sh.cpu()
    if name != "unwrapped6":
        assert total.tolist() == [E, 0] and neighbor.padded_list_ok(total) == (True, E)
        assert torch.equal(ei[:, :E], want_ei) and torch.equal(sh[:E], want_sh)
        assert bool((ei[:, E:] == -1).all()) and bool((sh[E:] == 0).all())
        return
    # image shifts beyond +-8: flag bit 0; every column is a NULL edge or a pair AND shift the brute force also has
    found, flags = total.tolist()
    ok, _ = neighbor.padded_list_ok(total)
    assert not ok and (flags & 1) and found == E
    assert int(ei.min()) >= -1 and int(ei.max()) < N
    null = ei[0] < 0
    assert bool((ei[1][null] == -1).all()) and bool((sh[null] == 0).all()) and bool((ei[1][~null] >= 0).all())
    have = set(zip(I.tolist(), J.tolist(), map(tuple, S.tolist())))
    real = torch.cat([ei.t()[~null], -sh[~null].long()], 1).tolist()
    assert 0 < len(real) < E and len(set(map(tuple, real))) == len(real)
    assert all((r[0], r[1], (r[2], r[3], r[4])) in have for r in real)
    # ... and exactly the brute force's pairs whose shift has a code: |S| <= 8 on every axis
    assert len(real) == int((np.abs(S).max(axis=1) <= 8).sum())


def _join(names, rc, with_empty=None):
    """One batch of the cases `names`: (pos, batch, cells or None, B, the brute-force lists concatenated with atom offsets)."""
    pos, batch, cells, ii, jj, ss, off, g = [], [], [], [], [], [], 0, 0
    for name in names:
        if name is None:                 # an empty structure
            g += 1
            continue
        p, c, _ = _case(name)
        I, J, S, band = _ref(name, rc)
        assert band == 0
        pos.append(p), batch.append(np.full(len(p), g, dtype=np.int64)), cells.append(c)
        ii.append(I + off), jj.append(J + off), ss.append(S)
        off += len(p)
        g += 1
    periodic = cells[0] is not None
    want = _as_tensors(np.concatenate(ii), np.concatenate(jj), np.concatenate(ss), periodic)
    cells = torch.from_numpy(np.stack(cells).astype(np.float32)) if periodic else None
    return torch.from_numpy(np.concatenate(pos).astype(np.float32)), torch.from_numpy(np.concatenate(batch)), cells, g, want


@pytest.mark.gpu
def test_batched_search_equals_the_brute_force_lists_concatenated(monkeypatch):
    """All periodic cases but `unwrapped6` as ONE batch, all open cases with an empty structure in the middle as another.
    Each structure's grid is bounded by its own 8 N_b + 64 bins and filed behind the others', so `sparse` and the single
    atoms coarsen and bin differently inside a batch than alone.  The exact and the padded form."""
    dev = _dev()
    monkeypatch.setenv("HERMNET_DEBUG_POISON", "1")
    monkeypatch.setattr(neighbor, "_STASH", {})
    for names, rc in ((BATCHED, BATCH_RC), (["open_line", None, "open_far", "single_open"], OPEN_RC)):
        pos, batch, cells, B, want = _join(names, rc)
        periodic = cells is not None
        p, b, c = pos.to(dev), batch.to(dev), None if cells is None else cells.to(dev)
        got = hn.neighbor_search(p, rc, c, batch=b, num_graphs=B)
        _assert_list(got, want, periodic, names)
        E = want[0].size(1)
        cap = neighbor.padded_capacity(E)
        ei, sh, total = neighbor.neighbor_search_padded(p, rc, c, cap, batch=b, num_graphs=B)
        assert total.tolist() == [E, 0]
        assert torch.equal(ei[:, :E].cpu(), want[0]) and bool((ei[:, E:] == -1).all())
        if periodic:
            assert torch.equal(sh[:E].cpu(), want[1]) and bool((sh[E:] == 0).all())
        else:
            assert sh is None


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["skew30", "needle", "open_far"])
def test_target_mask_gives_the_brute_force_list_filtered_by_its_target_row(name):
    dev = _dev()
    p, c, rc = _gpu_inputs(name, dev)
    want = _want(name)
    mask = torch.zeros(p.size(0), dtype=torch.bool)
    mask[::2] = True
    keep = mask[want[0][1]]
    assert 0 < int(keep.sum()) < keep.numel()
    got = hn.neighbor_search(p, rc, c, target_mask=mask.to(dev))
    _assert_list(got, (want[0][:, keep], None if want[1] is None else want[1][keep]), c is not None, name)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(_REBASE_M))
def test_rebasing_is_exact_on_the_device(which, monkeypatch):
    """The device lists of one lattice in two bases map one to one (S_base = S_rebased @ M), with the cell on the host and
    with the cell in device memory; each equals the brute force of its own cell."""
    dev = _dev()
    monkeypatch.setenv("HERMNET_DEBUG_POISON", "1")
    pos, cell, I, J, S, band = _rebase_ref("base")
    _, cm, Im, Jm, Sm, band_m = _rebase_ref(which)
    assert band == 0 and band_m == 0
    p = torch.from_numpy(pos.astype(np.float32)).to(dev)
    for c_np, (wi, wj, ws), M in ((cell, (I, J, S), None), (cm, (Im, Jm, Sm), which)):
        c = torch.from_numpy(c_np.astype(np.float32)).to(dev)
        want = _as_tensors(wi, wj, ws, True)
        E = len(wi)
        ei, sh = hn.neighbor_search(p, REBASE_RC, c)
        _assert_list((ei, sh), want, True, "host cell")
        eip, shp, total = neighbor.neighbor_search_padded(p, REBASE_RC, c, neighbor.padded_capacity(E), device_cell=True)
        assert total.tolist() == [E, 0]
        _assert_list((eip[:, :E], shp[:E]), want, True, "device cell")
        assert bool((eip[:, E:] == -1).all())
        if M is not None:
            for e_, s_ in ((ei, sh), (eip[:, :E], shp[:E])):
                e_, s_ = e_.cpu().numpy(), -s_.cpu().numpy().astype(np.int64)
                got = _to_base(e_[0], e_[1], s_, M)
                assert np.array_equal(got[0], I) and np.array_equal(got[1], J) and np.array_equal(got[2], S)


# ---- what consumes the list ------------------------------------------------------------------------------------------------
_Z3 = [13, 28, 29]
GEOMETRY_CASES = ["skew30", "left_handed", "unimodular", "needle", "reach8", "unwrapped3", "lattice_on_cutoff"]


def _graphs(name, dev, rc=None, z=None):
    """(pos, cell [1,3,3], CPU graph from the PyTorch restatement of the relation build, the device build's graph (CSC walk
    of the position gradient) and the restatement's on the device (out-adjacency walk)) on the brute-force list."""
    from hermnet_amd.relations import RelationalGraph
    pos, cell, _ = _case(name)
    ei, sh = _want(name, rc)
    n = len(pos)
    z = torch.tensor([_Z3[k % 3] for k in range(n)]) if z is None else z
    batch = torch.zeros(n, dtype=torch.long)
    p, c = torch.from_numpy(pos.astype(np.float32)), torch.from_numpy(cell.astype(np.float32)).reshape(1, 3, 3)
    cpu = RelationalGraph._build_torch(z, ei, _Z3, sh, batch)
    nat = RelationalGraph.build(z.to(dev), ei.to(dev), _Z3, sh.to(dev), batch.to(dev))
    out = RelationalGraph._build_torch(z.to(dev), ei.to(dev), _Z3, sh.to(dev), batch.to(dev))
    for g in (nat, out):
        assert torch.equal(g.src_id.cpu(), cpu.src_id) and torch.equal(g.tgt_id.cpu(), cpu.tgt_id)
        assert torch.equal(g.shift.cpu(), cpu.shift)
    assert nat.out_rowptr is None and out.out_rowptr is not None
    return p, c, cpu, nat, out


def _edge_vectors64(p, c, g):
    """D_e in float64 on the float32 inputs, CSR order of graph `g` (a CPU graph)."""
    j, i = g.src_id.long(), g.tgt_id.long()
    return p.double()[j] - p.double()[i] + g.shift.double() @ c.double()[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GEOMETRY_CASES)
def test_edge_geometry_forward_per_edge(name):
    """`EdgeGeometry` forward against `ref_ops.geometry_ref` in float64, judged PER EDGE: large shifts and unwrapped
    positions cancel in float32, so an edge passes within the suite's usual bound (1e-6 on rhat absolute and on d relative)
    or within 8 x the error a plain float32 torch evaluation of the same formula makes on that edge
    (`test_node_chain_kernels_on_adversarial_operands` set this rule).  Coincident atoms reach the clamp: d = 1e-6, rhat = 0."""
    import ref_ops
    from hermnet_amd.ops import EdgeGeometry
    dev = _dev()
    p, c, cpu, nat, _ = _graphs(name, dev)
    edge = EdgeGeometry.apply(p.to(dev), c.to(dev), nat).cpu()
    r64 = ref_ops.geometry_ref(p.double(), cpu, c.double())
    r32 = ref_ops.geometry_ref(p, cpu, c)
    assert bool(torch.isfinite(edge).all())
    err_r = (edge[:, :3].double() - r64[:, :3]).abs().max(dim=1).values
    base_r = (r32[:, :3].double() - r64[:, :3]).abs().max(dim=1).values
    err_d = (edge[:, 3].double() - r64[:, 3]).abs() / r64[:, 3]
    base_d = (r32[:, 3].double() - r64[:, 3]).abs() / r64[:, 3]
    bound_r, bound_d = torch.clamp(8.0 * base_r, min=1e-6), torch.clamp(8.0 * base_d, min=1e-6)
    print("edge geometry %s: E = %d, worst err / bound: rhat %.3f, d %.3f; worst err: rhat %.2e, d %.2e (plain fp32: %.2e, %.2e)"
          % (name, edge.size(0), float((err_r / bound_r).max()), float((err_d / bound_d).max()), float(err_r.max()),
             float(err_d.max()), float(base_r.max()), float(base_d.max())))
    assert bool((err_r <= bound_r).all()) and bool((err_d <= bound_d).all())
    if name == "lattice_on_cutoff":
        zero = _edge_vectors64(p, c, cpu).norm(dim=1) == 0
        assert int(zero.sum()) == 8
        assert bool((edge[zero, 3] == torch.tensor(1.0e-6, dtype=torch.float32)).all()) and not bool(edge[zero, :3].any())
        assert float(edge[~zero, 3].min()) >= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", GEOMETRY_CASES)
def test_edge_geometry_backward_on_both_walks(name):
    """gpos against the float64 index_add restatement, for the CSC walk (device-built graph) and the out-adjacency walk."""
    from hermnet_amd.ops import EdgeGeometry
    from helpers import rel_err
    dev = _dev()
    p, c, cpu, nat, out = _graphs(name, dev)
    gD = torch.randn(cpu.E, 4, generator=torch.Generator().manual_seed(5))
    ref = torch.zeros(len(p), 3, dtype=torch.float64).index_add_(0, cpu.src_id.long(), gD[:, :3].double())
    ref.index_add_(0, cpu.tgt_id.long(), -gD[:, :3].double())
    for g in (nat, out):
        pos = p.to(dev).requires_grad_(True)
        edge = EdgeGeometry.apply(pos, c.to(dev), g)
        (gp,) = torch.autograd.grad(edge, pos, gD.to(dev))
        assert rel_err(gp.cpu().double(), ref) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["single", "single_tight", "reach8"])
def test_self_image_edges_contribute_exactly_nothing_to_gpos(name):
    """An edge between an atom and its own periodic image is in the out- and in the in-segment of one row with the same
    gradient: +g - g.  With one element (rows = atoms) such an edge has the same rank in both segments -- the pairs (a, j)
    in front of it mirror the pairs (j, a) -- so with at most 64 edges per row one lane adds and subtracts it, and the row
    is bit for bit the row computed with that edge's gradient removed.  (With several elements, or more than 64 edges per
    row, the two land in different partial sums and cancel to rounding only: the 1e-5 of the test above.)"""
    from hermnet_amd.ops import EdgeGeometry
    dev = _dev()
    n = len(_case(name)[0])
    p, c, cpu, nat, out = _graphs(name, dev, z=torch.full((n,), 13))
    self_edge = cpu.src_id == cpu.tgt_id
    if name != "single":
        assert int(self_edge.sum()) > 0 and int(torch.bincount(cpu.tgt_id.long()).max()) <= 64
    gD = torch.randn(cpu.E, 4, generator=torch.Generator().manual_seed(6))
    gD0 = gD.clone()
    gD0[self_edge] = 0.0
    for g in (nat, out):
        rows = []
        for grad in (gD, gD0):
            pos = p.to(dev).requires_grad_(True)
            edge = EdgeGeometry.apply(pos, c.to(dev), g)
            rows.append(torch.autograd.grad(edge, pos, grad.to(dev))[0].cpu())
        assert torch.equal(rows[0], rows[1])
        if name != "reach8":                           # a single atom: nothing but self-images
            assert not bool(rows[0].any())


def _virial64(p, c, g, gD, n):
    """W_i = -1/2 sum_{e touching i} D_e (x) g_e in float64; a self-image edge is added at both of its ends: fully to i."""
    outer = -0.5 * _edge_vectors64(p, c, g)[:, :, None] * gD[:, None, :3].double()
    w = torch.zeros(n, 3, 3, dtype=torch.float64).index_add_(0, g.src_id.long(), outer)
    return w.index_add_(0, g.tgt_id.long(), outer)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["needle", "reach8", "single", "single_tight"])
def test_per_atom_virial_with_self_image_edges(name):
    """`hermnet_edge_geometry_bwd_virial` (through `EdgeGeometry` with an `AtomSink`) on cells small enough to have edges
    between an atom and its own images, both walks: W_i against float64 at the per-atom virial comparison's 1e-5
    (`tests/test_atom_properties.py`), gpos bit for bit the plain backward's."""
    from hermnet_amd.ops import EdgeGeometry, AtomSink
    from helpers import rel_err
    dev = _dev()
    p, c, cpu, nat, out = _graphs(name, dev)
    n = len(p)
    gD = torch.randn(cpu.E, 4, generator=torch.Generator().manual_seed(7))
    want = _virial64(p, c, cpu, gD, n)
    if name != "single":
        assert int((cpu.src_id == cpu.tgt_id).sum()) > 0 and float(want.abs().max()) > 0
    for g in (nat, out):
        got = []
        for sink in (None, AtomSink(virials=True, graph_virial=True)):
            pos = p.to(dev).requires_grad_(True)
            edge = EdgeGeometry.apply(pos, c.to(dev), g, sink)
            got.append(torch.autograd.grad(edge, pos, gD.to(dev))[0])
        assert torch.equal(got[0], got[1])
        w = sink.virials.cpu().double()
        assert w.shape == (n, 3, 3) and sink.graph_virial.shape == (1, 3, 3)
        if name == "single":
            assert not bool(w.any()) and not bool(sink.graph_virial.any())
        else:
            assert rel_err(w, want) <= 1e-5


@pytest.mark.gpu
def test_graph_virial_sum_rule_across_chunk_boundaries():
    """sum_i W_i = -sum_e D_e (x) g_e per graph through `hermnet_graph_virial`, on a batch of `needle`, `reach8`, the single
    atoms and two needle-like cells of 257 and 255 atoms (rc 3): the chunk boundaries of 256 rows fall inside a graph (rows
    35 .. 291) and at the ragged ends of the next.  Bound: 1e-5 of the largest per-graph sum of |W_i| (the total
    itself may cancel; `_vtol` of tests/test_atom_properties.py)."""
    from hermnet_amd.ops import EdgeGeometry, AtomSink
    from hermnet_amd.relations import RelationalGraph
    dev = _dev()
    p, c, b, ei, sh, band = _virial_batch()
    assert band == 0
    off = p.size(0)
    z = torch.tensor([_Z3[k % 3] for k in range(off)])
    B = c.size(0)
    cpu = RelationalGraph._build_torch(z, ei, _Z3, sh, b)
    j, i = cpu.src_id.long(), cpu.tgt_id.long()
    D = p.double()[j] - p.double()[i] + torch.einsum("ni,nij->nj", cpu.shift.double(), c.double()[b[j]])
    gD = torch.randn(cpu.E, 4, generator=torch.Generator().manual_seed(8))
    outer = D[:, :, None] * gD[:, None, :3].double()
    want = torch.zeros(B, 3, 3, dtype=torch.float64).index_add_(0, b[j], -outer)
    scale = torch.zeros(B, 3, 3, dtype=torch.float64).index_add_(0, b[j], outer.abs())
    for build in (RelationalGraph.build, RelationalGraph._build_torch):
        g = build(z.to(dev), ei.to(dev), _Z3, sh.to(dev), b.to(dev))
        assert torch.equal(g.src_id.cpu(), cpu.src_id)
        sink = AtomSink(virials=True, graph_virial=True)
        posd = p.to(dev).requires_grad_(True)
        edge = EdgeGeometry.apply(posd, c.to(dev), g, sink)
        torch.autograd.grad(edge, posd, gD.to(dev))
        got = sink.graph_virial.cpu().double()
        assert got.shape == (B, 3, 3)
        err = (got - want).abs().amax(dim=(1, 2))
        print("graph virial sum rule: err / scale per graph", (err / scale.amax(dim=(1, 2)).clamp(min=1e-30)).tolist())
        assert bool((err <= 1e-5 * scale.amax(dim=(1, 2))).all())
        assert not bool(got[2].any())                                               # the atom without an edge
        per_atom = torch.zeros(B, 3, 3, dtype=torch.float64).index_add_(0, b, sink.virials.cpu().double())
        assert bool(((per_atom - want).abs().amax(dim=(1, 2)) <= 1e-5 * scale.amax(dim=(1, 2))).all())


def _model_case(name):
    if name.startswith("rebase_"):
        pos, cell = _rebase_ref(name[7:])[:2]
        return pos, cell, REBASE_RC, _rebase_ref(name[7:])[2:]
    pos, cell, rc = _case(name)
    return pos, cell, rc, _ref(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["skew30", "left_handed", "needle", "unwrapped3"] + ["rebase_" + k for k in sorted(_REBASE_M)])
def test_model_energy_and_forces_on_the_device_list_vs_the_oracle(name):
    """HVNet (2 layers, H = 64, 20 radial functions; Al / Ni / Cu round-robin) on the list the DEVICE search gives (equal to
    the brute force), energy and forces against the float64 oracle on the same input at the project's 1e-5."""
    from test_gpu_parity import _oracle_vs_hip
    dev = _dev()
    pos, cell, rc, (I, J, S, band) = _model_case(name)
    assert band == 0
    p, c = torch.from_numpy(pos.astype(np.float32)), torch.from_numpy(cell.astype(np.float32))
    ei, sh = hn.neighbor_search(p.to(dev), rc, c.to(dev))
    _assert_list((ei, sh), _as_tensors(I, J, S, True), True, name)
    n = len(pos)
    data = hn.Data(pos=p, atomic_number=torch.tensor([_Z3[k % 3] for k in range(n)]), batch=torch.zeros(n, dtype=torch.long),
                   cell=c.reshape(1, 3, 3), edge_index=ei.cpu(), edge_shift=sh.cpu())
    e, f = _oracle_vs_hip(data, ["Al", "Ni", "Cu"], dict(rc=rc, num_layers=2, hidden_channels=64, num_rbf=20), 9)
    assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(f).all())


@pytest.mark.gpu
def test_model_with_a_coincident_pair_follows_the_reference_clamp():
    """An Al and a Ni atom on one point: d is replaced by the constant 1e-6 and rhat = D / 1e-6 is still differentiated
    through D (the reference's semantics, which the oracle carries).  Finite outputs, energy and forces within 1e-5."""
    from test_gpu_parity import _oracle_vs_hip
    dev = _dev()
    pos, cell, rc, I, J, S, band = _coincident()
    assert band == 0
    p, c = torch.from_numpy(pos.astype(np.float32)), torch.from_numpy(cell.astype(np.float32))
    ei, sh = hn.neighbor_search(p.to(dev), rc, c.to(dev))
    _assert_list((ei, sh), _as_tensors(I, J, S, True), True, "coincident")
    data = hn.Data(pos=p, atomic_number=torch.tensor([_Z3[k % 3] for k in range(12)]), batch=torch.zeros(12, dtype=torch.long),
                   cell=c.reshape(1, 3, 3), edge_index=ei.cpu(), edge_shift=sh.cpu())
    e, f = _oracle_vs_hip(data, ["Al", "Ni", "Cu"], dict(rc=rc, num_layers=2, hidden_channels=64, num_rbf=20), 9)
    assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(f).all())
