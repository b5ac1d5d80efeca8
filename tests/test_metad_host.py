"""CPU: the metadynamics stage of csrc/metad_step.h through its host twins (hermnet_host_metad_bias / _cv / _exp) -- the
library's own exp against its numpy transcription and math.exp; the collective variables and the bias force against brute
force over 5^3 images and central differences on a skewed triclinic cell; the twins against `metad_reference.NumpyMetaD` bit
for bit; the protocol (void step, prime, zero height, restart from `hills=`); the free energy of an analytic double well;
the refusals of hermnet_amd/metad.py.  No GPU."""
import math
import types

import numpy as np
import pytest

from hermnet_amd import metad
from hermnet_amd.metad import Coordination, Distance, bias_on_grid, free_energy
from md_reference import AMU, KB, HostMD, bits
from metad_reference import HostMetaD, NumpyMetaD, bound_step, host_cv, host_exp, np_exp
from test_hostile_cells import _skew30
from test_md_host import TRICLINIC, _well


# ---- mt_exp ---------------------------------------------------------------------------------------------------------------------
def test_exp_twin_equals_its_transcription_and_math_exp():
    """10^4 arguments in [-750, 0], end points included (and the saturation's edge): host twin and numpy transcription
    bit-equal; relative error against math.exp <= 1e-14 where the result is normal (a few roundings of Horner at 1.1e-16 each,
    the reduction's rounding, truncation < 5e-18)."""
    a = np.concatenate([np.linspace(-750.0, 0.0, 9000), np.random.RandomState(0).uniform(-750.0, 0.0, 995),
                        [-745.0, np.nextafter(-745.0, -1000.0), -0.0, -1e-300, -math.log(2.0) / 2]])
    assert len(a) == 10 ** 4 and a[0] == -750.0 and a[8999] == 0.0
    got, want = host_exp(a), np_exp(a)
    assert np.array_equal(bits(got), bits(want))
    assert got[0] == 0.0 and got[8999] == 1.0 and got[9996] == 0.0 and got[9995] > 0.0
    exact = np.array([math.exp(v) for v in a])
    normal = exact >= 2.2250738585072014e-308
    assert normal.sum() > 9000
    assert np.max(np.abs(got[normal] - exact[normal]) / exact[normal]) <= 1e-14
    assert np.all(np.diff(got[:9000]) >= 0.0) and np.all(got <= 1.0)


# ---- CVs and bias against brute force and finite differences ---------------------------------------------------------------------
R0, NN, R_CUT = 1.6, 6, 2.4
_CACHE = {}


def _skew():
    """The skew30 cell of tests/test_hostile_cells.py (heights 5.0, 4.88, 9.0) with its 40 atoms; atoms 0 and 1 are moved so
    that the group {0, 1} straddles the boundary: atom 1 sits at fractional 0.03 with image (1, 0, 0), next to atom 0 at 0.98;
    atoms 5 and 9 likewise, two cells further down."""
    if "skew" not in _CACHE:
        pos, cell, _ = _skew30(np.random.RandomState(11))
        cell = cell.astype(np.float32).astype(np.float64)
        image = np.zeros((40, 3), dtype=np.int32)
        pos[0] = np.array([0.98, 0.40, 0.50]) @ cell
        pos[1] = np.array([0.03, 0.45, 0.52]) @ cell
        image[1] = (1, 0, 0)
        pos[5] = np.array([0.05, 0.47, 0.44]) @ cell
        pos[9] = np.array([0.95, 0.38, 0.56]) @ cell
        image[5], image[9] = (-1, 0, 0), (-2, 0, 0)
        image[7] = (-2, 1, 0)
        _CACHE["skew"] = (pos, image, cell)
    return _CACHE["skew"]


def _images5(cell):
    n = np.array([(a, b, c) for a in range(-2, 3) for b in range(-2, 3) for c in range(-2, 3)], dtype=np.float64)
    return n @ cell


def _switch64(r):
    s = lambda q: 1.0 / (1.0 + np.power(q / R0, NN))
    return np.where(r < R_CUT, (s(r) - s(R_CUT)) / (1.0 - s(R_CUT)), 0.0)


def _coordination_brute(pos, cell, a, b):
    shifts, total = _images5(cell), 0.0
    for i in a:
        for j in b:
            r = np.linalg.norm(pos[i] - pos[j] + shifts, axis=1)
            if i == j:
                r = r[r > 0.0]
            total += _switch64(r).sum()
    return total


@pytest.mark.parametrize("groups", ["a_is_b", "a_not_b", "overlap"])
def test_coordination_equals_the_brute_force_over_125_images(groups):
    pos, image, cell = _skew()
    a, b = {"a_is_b": (range(40), range(40)), "a_not_b": (range(0, 15), range(15, 40)), "overlap": (range(0, 25), range(10, 40))}[groups]
    a, b = list(a), list(b)
    for mean in (False, True):
        values, _ = host_cv([Coordination(a, b, R0, nn=NN, r_cut=R_CUT, mean=mean)], 1, pos, image, cell)
        want = _coordination_brute(pos, cell, a, b) / (len(a) if mean else 1)
        assert want > 1.0 / (len(a) if mean else 1)
        assert abs(values[0, 0] - want) <= 1e-12 * want, (values[0, 0], want)
    if groups == "a_is_b":                                   # the order is fixed: A = B counts every pair twice
        half = sum(_switch64(np.linalg.norm(pos[i] - pos[j] + _images5(cell), axis=1)).sum() for i in range(40) for j in range(i))
        assert abs(values[0, 0] * 40 - 2.0 * half) <= 1e-12 * 2.0 * half


def test_distance_keeps_a_group_whole_across_the_boundary():
    """Group a = {0, 1} straddles the boundary (one image apart), group b = {5, 9} straddles it two cells further down: the
    centres are those of the unwrapped coordinates, their difference goes through the minimum image."""
    pos, image, cell = _skew()
    w = np.array([1.0, 3.0])
    cv = Distance([0, 1], [5, 9], weights_a=w)
    values, _ = host_cv([cv], 1, pos, image, cell)
    u = pos + image @ cell
    centre_a, centre_b = (w[:, None] * u[[0, 1]]).sum(axis=0) / w.sum(), u[[5, 9]].mean(axis=0)
    assert np.abs((centre_a - centre_b) @ np.linalg.inv(cell)).max() > 1.9          # two cells apart
    want = np.linalg.norm(centre_a - centre_b + _images5(cell), axis=1).min()
    assert 0.1 < want < 2.4 and abs(values[0, 0] - want) <= 1e-12 * want, (values[0, 0], want)
    broken, _ = host_cv([cv], 1, pos, np.zeros_like(image), cell)
    assert abs(broken[0, 0] - want) > 0.1                    # without the images the groups are torn: the test has teeth
    same, grads = host_cv([Distance([3], [3])], 1, pos, image, cell)
    assert same[0, 0] == 0.0 and not grads.any()             # the gradient at zero distance is zero


def _cvs_skew():
    return [Distance([0, 1], [5, 9], weights_a=[1.0, 3.0]), Coordination(range(0, 25), range(10, 40), R0, nn=NN, r_cut=R_CUT)]


def _hills_skew(values):
    rs = np.random.RandomState(5)
    centres = values[0] + rs.normal(scale=[0.3, 1.5], size=(50, 2))
    return centres, rs.uniform(0.01, 0.05, 50)


SIGMA_SKEW = [0.4, 2.0]


def _twin_bias(pos, image, cell, hills):
    """(s [D], V, bias forces [N,3]) of the host twin at `pos`: a prime of hermnet_host_metad_bias over the preloaded hills."""
    host = HostMetaD(1, pos, np.zeros_like(pos), np.full(len(pos), 20.0), 1.0, cell, _cvs_skew(), 0.02, SIGMA_SKEW, 10, 300.0,
                     hills=hills, wrap=False)
    host.image[:] = image
    host.state[3] = 1
    host.finish(np.zeros((len(pos), 3), dtype=np.float32))
    return host.cv_walker[0, :2].copy(), float(host.cv_walker[0, 2]), host.bias_forces.copy(), host


def test_gradients_and_bias_force_equal_central_differences_of_the_twin():
    """h = 1e-5 A: truncation ~ h^2 f''' ~ 1e-10, round-off / h ~ 1e-16 x 10 / 1e-5 = 1e-10; tolerance 1e-6 of the largest
    component.  The bias forces sum to zero to 1e-12 (pairs are visited from both ends; a distance's weights cancel)."""
    pos, image, cell = _skew()
    values, grads = host_cv(_cvs_skew(), 1, pos, image, cell)
    hills = _hills_skew(values)
    s0, v0, f_bias, host = _twin_bias(pos, image, cell, hills)
    assert np.array_equal(bits(s0), bits(values[0])) and v0 > 1e-3
    h = 1e-5
    fd_s, fd_v = np.zeros((2, 40, 3)), np.zeros((40, 3))
    for i in range(40):
        for k in range(3):
            up, down = pos.copy(), pos.copy()
            up[i, k] += h
            down[i, k] -= h
            sp, vp, _, _ = _twin_bias(up, image, cell, hills)
            sm, vm, _, _ = _twin_bias(down, image, cell, hills)
            fd_s[:, i, k], fd_v[i, k] = (sp - sm) / (2 * h), (vp - vm) / (2 * h)
    for d in range(2):
        assert np.abs(grads[d]).max() > 0.1
        assert np.abs(grads[d] - fd_s[d]).max() <= 1e-6 * np.abs(fd_s[d]).max(), d
    assert np.abs(f_bias).max() > 1e-3
    assert np.abs(f_bias + fd_v).max() <= 1e-6 * np.abs(fd_v).max()
    assert np.abs(f_bias.sum(axis=0)).max() <= 1e-12
    # what the stage hands the finish: (float)((double)f - (-f_bias)), with f = 0 here
    assert np.array_equal(host.forces_b, f_bias.astype(np.float32))
    # the numpy V of the same list (library exp within 1e-14 of numpy's)
    centres, heights = hills
    assert abs(bias_on_grid(types.SimpleNamespace(hill_centres=centres, hill_heights=heights, sigma=SIGMA_SKEW), [s0])[0] - v0) <= 1e-12


# ---- bit for bit against the numpy transcription -----------------------------------------------------------------------------------
def _walkers(B, n_rep, cell, seed):
    rs = np.random.RandomState(seed)
    x = rs.uniform(0.25, 0.75, (B * n_rep, 3)) @ cell
    x[::7] += np.array([1, -1, 0]) @ cell                    # some atoms start a cell outside: wrap and images
    v = rs.normal(scale=0.01, size=(B * n_rep, 3))
    return x, v, np.tile(rs.uniform(10.0, 60.0, n_rep), B)


def _same(host, ref, what):
    for name in ("x", "v", "bias_forces", "cv_log", "hill_centres", "hill_heights"):
        assert np.array_equal(bits(getattr(host, name)), bits(getattr(ref, name))), (what, name)
    assert np.array_equal(host.image, ref.image) and np.array_equal(host.forces_b, ref.forces_b), what
    assert host.hill_count[0] == ref.hill_count[0] and host.state.tolist() == ref.state.tolist(), what


@pytest.mark.parametrize("n_rep,steps", [(20, 200), (257, 3)], ids=["3x20", "3x257"])
def test_host_twin_equals_the_numpy_transcription_bit_for_bit(n_rep, steps):
    """3 walkers, D = 2, pace 5 (pace 2 for the short run), well-tempered, Langevin, harmonic-well forces: positions,
    velocities, images, hills, cv_log and bias forces equal after EVERY step.  257 atoms per walker with a coordination over
    all of them cross a tile boundary with a one-atom tile."""
    B, cell = 3, TRICLINIC.astype(np.float32).astype(np.float64)
    x, v, m = _walkers(B, n_rep, cell, seed=n_rep)
    group = range(n_rep) if n_rep > 100 else range(2, n_rep)
    cvs = [Distance([0, 1], [2, 3, 4]), Coordination(group, group, 3.0, nn=8, r_cut=4.4, mean=n_rep > 100)]
    pace = 5 if steps > 10 else 2
    kw = dict(friction=0.02, bias_factor=8.0, seed=99, log_steps=16, max_hills=256)
    args = (B, x, v, m, 0.5, cell, cvs, 0.05, [0.2, 1.0], pace, 400.0)
    host, ref = HostMetaD(*args, **kw), NumpyMetaD(*args, **kw)
    centre = np.array([0.5, 0.5, 0.5]) @ cell
    for o in (host, ref):                                    # the prime: biased forces of the start, no hill, no row
        o.state[3] = 1
        o.finish(_well(o.advance().copy(), centre), energy=np.zeros(B))
    _same(host, ref, "prime")
    assert host.hill_count[0] == 0 and np.all(host.cv_log == -7.0) and host.state.tolist() == [0, 0, 0, 0]
    for step in range(steps):
        p_host, p_ref = host.advance().copy(), ref.advance().copy()
        assert np.array_equal(p_host.view(np.uint32), p_ref.view(np.uint32)), step
        f = _well(p_host, centre)
        host.finish(f, energy=np.full(B, -1.5), total=(100 + step, 0))
        ref.finish(f, energy=np.full(B, -1.5), total=(100 + step, 0))
        _same(host, ref, step)
        assert host.hill_count[0] == B * ((step + 1) // pace)
    centres, heights = host.hills()
    assert len(heights) == B * (steps // pace) and np.all(heights > 0.0) and np.all(heights <= 0.05)
    assert heights[-1] < 0.05 or steps < 10                  # tempering acted: later hills are lower
    assert np.abs(host.bias_forces).max() > 1e-4 and np.abs(host.image).max() >= 1
    rows = host.cv_log[[s % 16 for s in range(steps - min(steps, 16), steps)]]
    assert np.all(rows[:, :, 2] >= 0.0) and np.all((rows[:, :, 3] > 0.0) == ((np.arange(steps - len(rows), steps) + 1) % pace == 0)[:, None])


# ---- protocol ------------------------------------------------------------------------------------------------------------------------
def _small(**kw):
    B, cell = 2, TRICLINIC.astype(np.float32).astype(np.float64)
    x, v, m = _walkers(B, 12, cell, seed=4)
    cvs = [Distance([0, 1], [2, 3, 4]), Coordination(range(12), range(12), 3.0, nn=6, r_cut=4.4)]
    args = dict(friction=0.02, bias_factor=6.0, seed=5, log_steps=32, max_hills=64)
    args.update(kw)
    height = args.pop("height", 0.05)
    return HostMetaD(B, x, v, m, 0.5, cell, cvs, height, [0.2, 1.0], 5, 350.0, **args), np.array([0.5, 0.5, 0.5]) @ cell


def _prime(host, centre):
    host.state[1:3] = 0
    host.state[3] = 1
    host.finish(_well(host.advance().copy(), centre), energy=np.zeros(host.B))


def _steps(host, centre, n):
    for _ in range(n):
        host.finish(_well(host.advance().copy(), centre), energy=np.zeros(host.B), total=(50, 0), capacity=60)


def _everything(host):
    return (bits(host.x).tobytes(), bits(host.v).tobytes(), host.image.tobytes(), host.f_prev.tobytes(), host.hill_count[0],
            bits(host.hill_centres).tobytes(), bits(host.hill_heights).tobytes(), bits(host.cv_log).tobytes(), host.state.tolist())


@pytest.mark.parametrize("why", ["capacity", "nan"])
def test_void_step_deposits_nothing_and_the_run_goes_on_as_if_it_had_not_happened(why):
    base, centre = _small()
    _prime(base, centre)
    _steps(base, centre, 12)
    host, _ = _small()
    _prime(host, centre)
    _steps(host, centre, 4)
    before = _everything(host)
    f = _well(host.advance().copy(), centre)                 # step 4 is a deposit step: (4 + 1) % 5 == 0
    energy = np.array([0.0, np.nan]) if why == "nan" else np.zeros(2)
    host.finish(f, energy=energy, total=(61 if why == "capacity" else 50, 0), capacity=60)
    assert host.state.tolist() == [4, 4 if why == "capacity" else 256, 4, 0]
    assert np.array_equal(host.forces_b, f)                  # passed through untouched
    assert _everything(host)[:8] == before[:8]               # no hill, no row, the atoms back where the step began
    _steps(host, centre, 2)                                  # halted: nothing moves
    assert _everything(host)[:8] == before[:8]
    saved = host.f_prev.copy()                               # (DeviceMetaD.resume keeps the last accepted forces)
    _prime(host, centre)
    assert np.array_equal(host.f_prev, saved) and host.hill_count[0] == 0
    _steps(host, centre, 8)
    assert _everything(host) == _everything(base) and host.hill_count[0] == 4


def test_prime_applies_the_bias_and_deposits_nothing():
    probe, centre = _small()
    _prime(probe, centre)
    hills = (probe.cv_walker[:, :2] + np.array([0.1, -0.5]), np.array([0.3, 0.2]))     # hills beside the walkers' own CVs
    host, centre = _small(hills=hills)
    host.state[0] = 4                                        # a prime on what would be a deposit step
    log = host.cv_log.copy()
    host.state[3] = 1
    f = _well(host.advance().copy(), centre)
    host.finish(f, energy=np.zeros(2))
    assert host.state.tolist() == [4, 0, 0, 0] and host.hill_count[0] == 2 and np.array_equal(host.cv_log, log)
    assert np.abs(host.bias_forces).max() > 1e-6
    assert np.array_equal(host.forces_b, (f.astype(np.float64) + host.bias_forces).astype(np.float32))
    assert np.array_equal(host.f_prev, host.forces_b) and not np.array_equal(host.forces_b, f)


def test_zero_height_returns_the_input_forces_bit_for_bit():
    host, centre = _small(height=0.0, hills=(np.array([[3.0, 20.0]]), np.array([0.0])))
    _prime(host, centre)
    for step in range(11):
        f = _well(host.advance().copy(), centre)
        f[step % 24] = (-0.0, 0.0, np.float32(1e-30))
        host.finish(f, energy=np.zeros(2))
        assert np.array_equal(host.forces_b.view(np.uint32), f.view(np.uint32)), step
        assert not host.bias_forces.any()
    assert host.hill_count[0] == 1 + 2 * 2 and not host.hill_heights.any()


def test_restart_from_hills_equals_the_uninterrupted_run():
    """Stopped after 12 steps (not directly behind a deposit: the prime of a restart sees the whole list, the half kick of an
    uninterrupted run used forces made in front of the step's own deposit) and restarted from positions, velocities, images
    and `hills=`: bit-equal to 20 uninterrupted steps."""
    base, centre = _small()
    _prime(base, centre)
    _steps(base, centre, 12)
    again, _ = _small(hills=base.hills())
    again.x[:], again.v[:], again.image[:], again.state[0] = base.x, base.v, base.image, 12
    _prime(again, centre)
    assert np.array_equal(again.f_prev, base.f_prev) and again.hill_count[0] == base.hill_count[0] == 4
    _steps(base, centre, 8)
    _steps(again, centre, 8)
    assert _everything(again)[:7] == _everything(base)[:7] and again.state.tolist() == base.state.tolist()
    assert np.array_equal(bits(again.cv_log[12:20]), bits(base.cv_log[12:20])) and base.hill_count[0] == 8


# ---- physics: the free energy of a double well in the distance of two atoms ----------------------------------------------------------
T_WELL, BARRIER_KT, R_MID, HALF_WIDTH = 300.0, 10.0, 3.0, 0.5
WELL_STEPS, WELL_SEEDS = 200000, (1, 2, 3, 4)
WELL_GRID = np.linspace(2.45, 3.55, 12)


def _double_well(r):
    """(U, dU/dr) of U(r) = E_b ((r - r_m)^2 / w^2 - 1)^2."""
    q = (r - R_MID) / HALF_WIDTH
    return BARRIER_KT * KB * T_WELL * (q * q - 1.0) ** 2, BARRIER_KT * KB * T_WELL * 4.0 * (q * q - 1.0) * q / HALF_WIDTH


def _exact_free_energy(r):
    return _double_well(r)[0] - 2.0 * KB * T_WELL * np.log(r)


def _well_run(seed, walkers, steps, biased=True):
    """`walkers` pairs of atoms in a 20 A box each, started in the inner well, `steps` steps of the host twins: (the free
    energy on WELL_GRID or None, the largest distance seen).  The forces are those of the double well on the distance of each
    pair, from the float32 coordinates, rounded to float32: what a model hands the integrator."""
    box = 20.0
    rs = np.random.RandomState(seed)
    x = np.zeros((2 * walkers, 3))
    x[0::2] = rs.uniform(8.0, 12.0, (walkers, 3))
    x[1::2] = x[0::2] + np.array([R_MID - HALF_WIDTH, 0.0, 0.0])
    m = np.full(2 * walkers, 40.0)
    v = rs.normal(size=x.shape) * np.sqrt(KB * T_WELL / (m * AMU))[:, None]
    cell = np.diag([box] * 3)
    if biased:
        host = HostMetaD(walkers, x, v, m, 2.0, cell, [Distance([0], [1])], 0.25 * KB * T_WELL, [0.05], 100, T_WELL,
                         friction=0.2, bias_factor=8.0, seed=seed, log_steps=8, max_hills=steps // 100 * walkers + walkers)
    else:
        host = HostMD(x, v, m, 2.0, cell=np.tile(cell, (walkers, 1, 1)), batch=np.repeat(np.arange(walkers), 2), friction=0.2,
                      temperature=T_WELL, seed=seed, log_steps=8, num_graphs=walkers)
    seen = [0.0]

    def forces(pos32, out):
        p = pos32.tolist()
        for w in range(walkers):
            a, b = p[2 * w], p[2 * w + 1]
            d = [a[k] - b[k] - box * round((a[k] - b[k]) / box) for k in range(3)]
            r = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            c = -_double_well(r)[1] / r
            out[2 * w] = (c * d[0], c * d[1], c * d[2])
            out[2 * w + 1] = (-c * d[0], -c * d[1], -c * d[2])
            if r > seen[0]:
                seen[0] = r

    step = bound_step(host, forces, biased)
    host.state[3] = 1                                        # the prime: the forces of the start
    step()
    assert host.state.tolist() == [0, 0, 0, 0]
    for _ in range(steps):
        step()
    assert host.state.tolist() == [steps, 0, 0, 0]
    return (free_energy(host.snapshot(), WELL_GRID) if biased else None), seen[0]


@pytest.mark.parametrize("walkers", [1, 4])
def test_free_energy_of_a_double_well(walkers):
    """Two atoms (40 amu, dt 2 fs, Langevin 0.2 / fs at 300 K) with U(r) = 10 kB T ((r - 3)^2 / 0.25 - 1)^2 in their distance;
    well-tempered (bias factor 8, hills of kB T / 4 every 100 steps, sigma 0.05 A), 2 x 10^5 steps with one walker and
    5 x 10^4 with four.  `free_energy` on 12 grid points from 2.45 to 3.55 A (both wells and the barrier) against
    U(r) - 2 kB T ln r, each curve shifted by its mean over the grid: every grid point of the mean over 4 seeds lies within
    5 standard errors of the exact curve.  The unbiased twin with the same seeds and length never leaves the inner well
    (r < 3 A throughout): the barrier is crossed by the bias alone.
    Observed with these seeds: one walker, largest |mean - exact| 0.0050 eV (0.19 kB T), standard errors 0.0019 .. 0.0047 eV,
    worst deviation 1.29 standard errors; four walkers, 0.0054 eV (0.21 kB T), 0.0017 .. 0.0043 eV, 3.04 standard errors."""
    steps = WELL_STEPS // walkers
    curves = []
    for seed in WELL_SEEDS:
        _, r_max = _well_run(seed, walkers, steps, biased=False)
        assert r_max < R_MID, (seed, r_max)                  # a condition on the inputs, not a tolerance
        f, r_seen = _well_run(seed, walkers, steps)
        assert r_seen > R_MID + HALF_WIDTH                   # the biased run reached the outer well
        curves.append(f - f.mean())
    curves = np.array(curves)
    exact = _exact_free_energy(WELL_GRID)
    exact = exact - exact.mean()
    mean, err = curves.mean(axis=0), curves.std(axis=0, ddof=1) / math.sqrt(len(curves))
    deviation = np.abs(mean - exact)
    print("walkers %d: max |mean - exact| = %.4f eV (%.2f kT), standard errors %.4f .. %.4f eV, worst ratio %.2f"
          % (walkers, deviation.max(), deviation.max() / (KB * T_WELL), err.min(), err.max(), (deviation / err).max()))
    assert np.all(deviation <= 5.0 * err), (deviation / err)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_limit():
    cell = TRICLINIC                                          # heights above 9 A
    ok = Coordination(range(10), range(10), 3.0, nn=6, r_cut=4.4)
    metad.cv_tables([ok, Distance([0], [1])], 10, cell)
    with pytest.raises(ValueError, match="nn must be even"):
        metad.cv_tables([Coordination(range(10), range(10), 3.0, nn=7, r_cut=4.4)], 10, cell)
    with pytest.raises(ValueError, match="half the smallest cell height"):
        metad.cv_tables([Coordination(range(10), range(10), 3.0, nn=6, r_cut=4.8)], 10, cell)
    with pytest.raises(ValueError, match="at most 2"):
        metad.cv_tables([ok, ok, ok], 10, cell)
    with pytest.raises(ValueError, match="outside one copy.*n_rep = 10"):
        metad.cv_tables([Distance([0], [10])], 10, cell)
    with pytest.raises(ValueError, match="outside one copy"):
        metad.cv_tables([Coordination([-1, 2], range(10), 3.0, r_cut=4.4)], 10, cell)
    with pytest.raises(ValueError, match="cell=None"):
        metad.cv_tables([ok], 10, None)
    with pytest.raises(ValueError, match="more than max_hills = 4"):
        metad.bias_tables(1, 0.1, [0.1], 5, 300.0, None, 4, (np.zeros((5, 1)), np.zeros(5)))
    with pytest.raises(ValueError, match="sigma"):
        metad.bias_tables(2, 0.1, [0.1], 5, 300.0, None, 4, None)
    # run(n): B hills per committed multiple of pace
    assert metad.deposits_within(0, 9, 5, 3) == 3 and metad.deposits_within(4, 1, 5, 3) == 3 and metad.deposits_within(5, 4, 5, 3) == 0
    metad.refuse_overflow("DeviceMetaD", 10, 0, 0, 5, 3, 10, 16)
    with pytest.raises(RuntimeError, match=r"run\(15\) would deposit beyond the hill list .*max_hills=16"):
        metad.refuse_overflow("DeviceMetaD", 15, 0, 0, 5, 3, 10, 16)
    with pytest.raises(RuntimeError, match="max_hills=16"):
        metad.refuse_overflow("DeviceMetaD", 10, 10, 5, 5, 3, 10, 16)    # 5 pending replays count too
    # the constructor refuses in front of anything that needs a GPU
    z, pos, m = np.full(10, 13), np.zeros((10, 3)), np.full(10, 27.0)
    with pytest.raises(ValueError, match="cell=None"):
        metad.DeviceMetaD(None, z, None, pos, m, 1.0, [ok], 0.1, [0.1], 5, 300.0)
    with pytest.raises(ValueError, match="the cell is fixed"):
        metad.DeviceMetaD(None, z, cell, pos, m, 1.0, [ok], 0.1, [0.1], 5, 300.0, pressure=0.0)
    with pytest.raises(ValueError, match="at most 2"):
        metad.DeviceMetaD(None, z, cell, pos, m, 1.0, [ok, ok, ok], 0.1, [0.1, 0.1, 0.1], 5, 300.0)
    with pytest.raises(ValueError, match="walker 1 differs from walker 0 in atom count"):
        metad.DeviceMetaD(None, z, np.tile(cell, (2, 1, 1)), pos, m, 1.0, [ok], 0.1, [0.1], 5, 300.0,
                          batch=np.repeat([0, 1], [6, 4]), num_graphs=2)
