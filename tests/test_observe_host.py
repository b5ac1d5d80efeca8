"""CPU: the MD observers (hermnet_amd/csrc/observe_step.h) through the library's host twins hermnet_host_observe_frames /
_msd / _rdf -- against their numpy transcription (tests/observe_reference.py) as equal integers and equal bits, the pair
histogram against a brute-force search over lattice images, its normalisation on an ideal gas, and the sampling protocol."""
import itertools

import numpy as np
import pytest

from hermnet_amd import synth
from hermnet_amd.observe import msd_of, rdf_fits, rdf_g
from md_reference import bits
from observe_reference import HostFrames, HostMSD, HostRDF, NumpyFrames, NumpyMSD, NumpyRDF, state_words

SKEWED = np.array([[9.0, 0.0, 0.0], [7.5, 8.0, 0.0], [-6.0, 5.0, 7.0]])


def _inverse(cell):
    """The float64 inverse of the float32 cell, as DeviceMD makes it."""
    return np.linalg.inv(np.asarray(cell, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3))


def _same_rdf(a, b):
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.samples, b.samples) and np.array_equal(a.skipped, b.skipped)
    assert np.array_equal(bits(a.volume_sum), bits(b.volume_sum)) and np.array_equal(a.obs, b.obs)


def test_triclinic_histogram_equals_numpy_and_a_brute_force_search_over_images():
    """150 atoms of three species in a strongly skewed cell, r_max just under half the smallest height, 40 bins: host twin =
    numpy transcription = the minimum over the 9^3 images -4..4 of every pair, as integers per species pair and bin."""
    rs = np.random.RandomState(5)
    n, bins = 150, 40
    x = rs.uniform(0.0, 1.0, (n, 3)) @ SKEWED
    z = np.array([13, 28, 29])[rs.randint(0, 3, n)]
    inv = _inverse(SKEWED)
    heights = 1.0 / np.sqrt((inv[0] ** 2).sum(axis=0))
    r_max = 0.999 * 0.5 * heights.min()
    assert rdf_fits(r_max, inv).all() and not rdf_fits(1.002 * 0.5 * heights.min(), inv).any()
    pair = [cls(z, [0, n], r_max, bins) for cls in (HostRDF, NumpyRDF)]
    for p in pair:
        p.offer(state_words(0), x, SKEWED, inv)
    _same_rdf(*pair)
    host = pair[0]
    # brute force: the shortest of the 729 images of every pair
    shifts = np.array(list(itertools.product(range(-4, 5), repeat=3)), dtype=np.float64) @ SKEWED
    i, j = np.triu_indices(n, 1)
    d = (x[i] - x[j])[:, None, :] + shifts[None, :, :]
    r2 = (d * d).sum(axis=2).min(axis=1)
    b = np.searchsorted(host.edge2, r2, side="right") - 1
    keep = b < bins
    brute = np.zeros_like(host.counts)
    za, zb = host.species[i][keep], host.species[j][keep]
    np.add.at(brute[0], (host.pair_index(np.minimum(za, zb), np.maximum(za, zb)), b[keep]), 1)
    assert np.array_equal(host.counts, brute)
    assert host.counts.sum() == keep.sum() > 500 and (host.counts.sum(axis=2) > 0).all()
    assert host.samples.tolist() == [1] and host.skipped.tolist() == [0]
    assert abs(host.volume_sum[0] - 9.0 * 8.0 * 7.0) < 1e-9


def _batch(rs, sizes, box):
    x = np.concatenate([rs.uniform(0.0, box, (k, 3)) for k in sizes])
    z = np.array([13, 28, 29])[rs.randint(0, 3, sum(sizes))]
    return x, z, np.concatenate([[0], np.cumsum(sizes)])


def test_batches_count_every_graph_as_that_graph_alone_and_open_pairs_exactly():
    """Graphs of 32, 48 and 300 atoms (the last spans two tiles: two diagonal tile pairs and an off-diagonal one): each
    graph's counts equal that graph run alone and numpy's.  An open batch with r_max above every diameter: the counts of a
    species pair sum to exactly N_a N_b, or N_a (N_a - 1) / 2 for a = b."""
    rs = np.random.RandomState(11)
    sizes, box = [32, 48, 300], 12.0
    x, z, ptr = _batch(rs, sizes, box)
    cell = np.stack([np.diag([box, box, box + g]) for g in range(3)])
    inv = _inverse(cell)
    pair = [cls(z, ptr, 5.0, 25) for cls in (HostRDF, NumpyRDF)]
    for p in pair:
        p.offer(state_words(0), x, cell, inv)
    _same_rdf(*pair)
    assert len(pair[0].work) == 1 + 1 + 3
    for g in range(3):
        mine = slice(ptr[g], ptr[g + 1])
        alone = HostRDF(z[mine], [0, sizes[g]], 5.0, 25)
        assert len(alone.kinds) == 3                      # (every graph holds all three species: the histograms line up)
        alone.offer(state_words(0), x[mine], cell[g], inv[g])
        assert np.array_equal(alone.counts[0], pair[0].counts[g]) and alone.counts.sum() > 0
    # open structures: every pair is counted exactly once
    opened = [cls(z, ptr, 2.0 * box * np.sqrt(3.0), 7, periodic=False) for cls in (HostRDF, NumpyRDF)]
    for p in opened:
        p.offer(state_words(0), x)
    _same_rdf(*opened)
    assert np.array_equal(opened[0].counts.sum(axis=2), opened[0].n_pairs)
    assert opened[0].n_pairs.sum(axis=1).tolist() == [k * (k - 1) // 2 for k in sizes]
    assert not opened[0].volume_sum.any()


def test_perfect_fcc_has_twelve_nearest_neighbours():
    """sigma = 0: the bin that holds a / sqrt(2) holds exactly 6 N pairs over all species pairs (edges off the shells)."""
    a = 4.0
    x, cell, z = synth.fcc_alloy_atoms(reps=(3, 3, 3), a=a, sigma=0.0)
    n, bins = len(z), 9
    host = HostRDF(z, [0, n], 0.9 * a, bins)             # edges at multiples of 0.1 a: 0.7071 a sits inside bin 7
    host.offer(state_words(0), x, cell, _inverse(cell))
    per_bin = host.counts[0].sum(axis=0)
    assert per_bin.tolist() == [0] * 7 + [6 * n, 0]
    ref = NumpyRDF(z, [0, n], 0.9 * a, bins)
    ref.offer(state_words(0), x, cell, _inverse(cell))
    _same_rdf(host, ref)


def test_ideal_gas_normalises_to_one():
    """4096 uniform points in a cube of 24 A, r_max 10 A, 20 bins: every bin of g within 4 Poisson standard deviations of 1."""
    rs = np.random.RandomState(7)
    n, box, r_max, bins = 4096, 24.0, 10.0, 20
    x = rs.uniform(0.0, box, (n, 3))
    cell = np.diag([box] * 3)
    host = HostRDF(np.full(n, 14), [0, n], r_max, bins)
    host.offer(state_words(0), x, cell, _inverse(cell))
    g = rdf_g(host.counts, host.samples, host.volume_sum, host.n_pairs, r_max, bins)
    assert g.shape == (1, 1, bins)
    expected = host.n_pairs[0, 0] * (4.0 * np.pi / 3.0) * np.diff(host.edges ** 3) / box ** 3
    dev = np.abs(g[0, 0] - 1.0) * np.sqrt(expected)
    print("ideal gas: largest deviation %.2f Poisson standard deviations" % dev.max())
    assert np.all(dev <= 4.0), dev


def _observers(z, ptr, stride, r_max=3.0):
    n, B = len(z), len(ptr) - 1
    return (HostFrames(n, B, stride, 64, velocities=True, images=True), HostMSD(z, ptr, stride, 64), HostRDF(z, ptr, r_max, 12, stride))


def _fingerprint(obs):
    f, m, r = obs
    return [a.copy() for a in (f.obs, f.steps, f.positions, f.velocities, f.images, f.cells, m.obs, m.steps, m.sums, m.x_origin,
                               m.image_origin, r.obs, r.counts, r.samples, r.skipped, r.volume_sum)]


def _offer(obs, state, x, v, image, cell, inv):
    f, m, r = obs
    f.offer(state, x, v, image, cell)
    m.offer(state, x, image, cell)
    r.offer(state, x, cell, inv)


def _unchanged(before, obs):
    return all(np.array_equal(a, b) for a, b in zip(before, _fingerprint(obs)))


@pytest.mark.parametrize("stride", [1, 3, 7])
def test_protocol_samples_the_multiples_of_the_stride_once_and_nothing_under_a_halt(stride):
    rs = np.random.RandomState(stride)
    x, z, ptr = _batch(rs, [20, 30], 8.0)
    n = len(z)
    cell = np.stack([np.diag([8.0] * 3)] * 2)
    inv = _inverse(cell)
    obs = _observers(z, ptr, stride)
    taken = []
    for step in range(0, 23):
        xs, v, image = x + 0.01 * step, rs.normal(size=(n, 3)), rs.randint(-2, 3, (n, 3)).astype(np.int32)
        # a replay with a halt code set (a void step's, a parked capture's) changes nothing
        before = _fingerprint(obs)
        for code in (4, 256, 1 << 20):
            _offer(obs, state_words(step, code), xs, v, image, cell, inv)
        assert _unchanged(before, obs)
        _offer(obs, state_words(step), xs, v, image, cell, inv)
        if step % stride == 0:
            taken.append(step)
            assert not _unchanged(before, obs)
        else:
            assert _unchanged(before, obs)
        # the same step offered again (the prime behind a resume) samples nothing
        before = _fingerprint(obs)
        _offer(obs, state_words(step), xs + 1.0, v, image, cell, inv)
        assert _unchanged(before, obs)
    assert taken == list(range(0, 23, stride))
    f, m, r = obs
    for o in (f, m, r):
        assert o.obs.tolist() == [taken[-1], len(taken), 0, 0]
    assert f.steps[:len(taken)].tolist() == taken == m.steps[:len(taken)].tolist()
    assert r.samples.tolist() == [len(taken)] * 2 and not r.skipped.any()


def test_a_graph_whose_cell_shrank_below_twice_r_max_is_skipped_not_miscounted():
    rs = np.random.RandomState(2)
    x, z, ptr = _batch(rs, [40, 40], 7.0)
    wide, tight = np.stack([np.diag([8.0] * 3)] * 2), np.stack([np.diag([8.0] * 3), np.diag([8.0, 5.9, 8.0])])
    pair = [cls(z, ptr, 3.0, 12) for cls in (HostRDF, NumpyRDF)]
    for p in pair:
        p.offer(state_words(0), x, wide, _inverse(wide))
    first = pair[0].counts.copy()
    for p in pair:
        p.offer(state_words(1), x, tight, _inverse(tight))
    _same_rdf(*pair)
    host = pair[0]
    assert host.samples.tolist() == [2, 1] and host.skipped.tolist() == [0, 1] and host.obs.tolist() == [1, 2, 0, 0]
    assert np.array_equal(host.counts[1], first[1]) and np.array_equal(host.counts[0], 2 * first[0])
    assert host.volume_sum.tolist() == [1024.0, 512.0]


def test_frames_and_msd_twins_equal_numpy_bit_for_bit():
    """A skewed cell and a cubic one, three species, atoms wandering over several cells, rings that wrap (5 slots, 9
    samples): every array of the host twins equals the numpy transcription's, float64 by their bits."""
    rs = np.random.RandomState(9)
    sizes = [70, 300]
    cell = np.stack([SKEWED, np.diag([8.0, 9.0, 10.0])])
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    n = int(ptr[-1])
    z = np.array([13, 28, 29])[rs.randint(0, 3, n)]
    x = rs.uniform(0.0, 8.0, (n, 3))
    image = np.zeros((n, 3), dtype=np.int32)
    frames = [cls(n, 2, 2, 5, velocities=True, images=True) for cls in (HostFrames, NumpyFrames)]
    msds = [cls(z, ptr, 2, 5) for cls in (HostMSD, NumpyMSD)]
    for step in range(18):
        x = x + rs.normal(scale=0.3, size=(n, 3))
        image = image + rs.randint(-1, 2, (n, 3)).astype(np.int32)
        v = rs.normal(size=(n, 3))
        c = (cell * (1.0 + 0.001 * step)).astype(np.float32)
        for f in frames:
            f.offer(state_words(step), x, v, image, c)
        for m in msds:
            m.offer(state_words(step), x, image, c)
    h, r = frames
    assert h.obs.tolist() == r.obs.tolist() == [16, 9, 0, 0]
    for k in ("steps", "positions", "velocities", "images", "cells"):
        assert np.array_equal(getattr(h, k), getattr(r, k)), k
    assert sorted(h.steps.tolist()) == [8, 10, 12, 14, 16]
    h, r = msds
    assert h.obs.tolist() == r.obs.tolist() == [16, 9, 0, 0] and np.array_equal(h.steps, r.steps)
    assert np.array_equal(bits(h.sums), bits(r.sums)) and np.array_equal(bits(h.x_origin), bits(r.x_origin))
    assert np.array_equal(h.image_origin, r.image_origin) and np.abs(h.sums).min() > 0


def test_msd_of_a_rigid_shift_across_wraps_is_exact():
    """Every atom shifted by t = (0.5, 0.25, -0.5) A per step in a cubic 8 A cell and wrapped as the driver wraps: after k
    steps sum |d|^2 / n = k^2 |t|^2 and sum d / n = k t exactly (every number is binary-exact), over several wraps."""
    rs = np.random.RandomState(4)
    n, box, t = 96, 8.0, np.array([0.5, 0.25, -0.5])
    z = np.array([13, 29])[rs.randint(0, 2, n)]
    x0 = rs.randint(0, 8 * 64, (n, 3)) / 64.0
    cell = np.diag([box] * 3)
    pair = [cls(z, [0, n], 1, 64) for cls in (HostMSD, NumpyMSD)]
    for step in range(40):
        u = x0 + step * t
        image = np.floor(u / box).astype(np.int32)
        for m in pair:
            m.offer(state_words(step), u - image * box, image, cell)
    host, ref = pair
    assert np.array_equal(bits(host.sums), bits(ref.sums))
    k = np.arange(40, dtype=np.float64)
    msd, corrected = msd_of(host.sums[:40], np.bincount(host.species)[None])
    assert np.array_equal(msd[:, 0, :], np.repeat((k * k * (t @ t))[:, None], 2, axis=1))
    assert not corrected.any()
    assert np.abs(np.floor((x0 + 39 * t) / box)).max() >= 2          # the path really left the cell, both ways


def test_refusals_of_the_constructors_and_the_entry_points():
    """What cannot be counted is refused, by the observers' constructors and by the library: a stride, ring or bin count
    below 1, more bins than the kernel's edges (1024) or histogram cells than its LDS budget (8192), a missing pointer."""
    import types
    import torch
    from hermnet_amd import _lib
    from hermnet_amd.observe import MSD, RDF, Frames
    for make in (lambda: Frames(stride=0), lambda: Frames(frames=0), lambda: MSD(rows=0), lambda: MSD(stride=1.5),
                 lambda: RDF(r_max=0.0, bins=10), lambda: RDF(r_max=3.0, bins=0), lambda: RDF(r_max=3.0, bins=1025)):
        with pytest.raises(ValueError):
            make()
    four_species = types.SimpleNamespace(z=torch.tensor([1, 6, 7, 8] * 4), num_graphs=1, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="10 species pairs x 900 bins = 9000 histogram cells -- at most 8192"):
        RDF(r_max=3.0, bins=900)._bind(four_species, None)
    with pytest.raises(ValueError, match="DeviceREMD alone"):
        RDF(r_max=3.0, bins=10, by_rung=True)._bind(four_species, None)
    # the library's own checks (they need no GPU: nothing is launched)
    lib = _lib.load()
    z = np.array([13, 28, 29, 8] * 3)
    host = HostRDF(z, [0, 12], 3.0, 10)
    x = np.zeros((12, 3))
    from observe_reference import _p
    common = lambda bins, edge2: (12, 1, 4, bins, 1, 1, 9.0, _p(host.ptr), _p(host.species), _p(x), None, None, None, edge2,
                                  _p(host.work), 1, _p(state_words(0)), _p(host.obs), _p(host.counts), _p(host.samples),
                                  _p(host.skipped), _p(host.volume_sum))
    assert lib.hermnet_host_observe_rdf(*common(10, _p(host.edge2))) == _lib.HN_OK
    assert lib.hermnet_host_observe_rdf(*common(10, None)) == _lib.HN_ERR_BAD_ARG
    assert lib.hermnet_host_observe_rdf(*common(900, _p(host.edge2))) == _lib.HN_ERR_BAD_ARG          # 10 pairs x 900 bins
    assert lib.hermnet_observe_rdf(*(common(1025, _p(host.edge2)) + (None,))) == _lib.HN_ERR_BAD_ARG
    bad_work = np.array([[1, 0, 0]], dtype=np.int32)
    args = list(common(10, _p(host.edge2)))
    args[14] = _p(bad_work)
    assert lib.hermnet_host_observe_rdf(*args) == _lib.HN_ERR_BAD_ARG
    assert lib.hermnet_observe_frames(4, 1, 0, 8, None, None, None, None, None, None, None, None, None, None, None, None) == _lib.HN_ERR_BAD_ARG
    assert lib.hermnet_observe_msd(4, 1, 0, 1, 8, None, None, None, None, None, None, None, None, None, None, None, None) == _lib.HN_ERR_BAD_ARG
