"""CPU: the device-resident integrator (hermnet_amd/csrc/md_kernels.hip, md_step.h) through its host twins -- the noise
generator against Philox known answers, the step against a numpy float64 transcription bit for bit, the thermostat against
the temperature it is set to, and the halt protocol.  No GPU: hermnet_host_md_advance / _finish / _noise run the text the
kernels run."""
import numpy as np
import pytest

from md_reference import AMU, KB, NONFINITE, HostMD, NumpyMD, bits, host_noise, noise_words, philox4x32_10

TRICLINIC = np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]])
CUBIC = np.diag([10.0, 11.0, 12.0])


def test_philox_known_answers_and_counter_layout():
    """The pure-Python Philox4x32-10 reproduces the Random123 known-answer vectors, and the library's raw words equal it
    for the documented counter layout (atom, step low, step high, stream) and key (seed low, seed high) -- whatever `n` and
    whatever the order of the calls."""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join("%08x" % w for w in philox4x32_10(ctr, key)) == want
    cases = [(0, 0), (1, 0), (0x123456789abcdef0, 7), (5, (3 << 32) + 11), (2 ** 64 - 1, 2 ** 40)]
    first = {}
    for seed, step in cases:
        words, _ = host_noise(seed, step, 67)
        first[(seed, step)] = words
        for atom in (0, 1, 63, 64, 66):
            assert words[atom].tolist() == noise_words(seed, step, atom), (seed, step, atom)
    for seed, step in reversed(cases):                  # another order of calls, other sizes: the same words
        for n in (1, 5, 200):
            words, gauss = host_noise(seed, step, n)
            m = min(n, 67)
            assert np.array_equal(words[:m], first[(seed, step)][:m])
            assert np.array_equal(bits(gauss[:m]), bits(host_noise(seed, step, 67)[1][:m]))
    assert not np.array_equal(first[(0, 0)], first[(1, 0)])


def test_gaussian_moments():
    """3 * 2^18 samples: mean, variance and the correlations between an atom's three components, each within 5 standard
    errors (mean: 1/sqrt(n); variance: sqrt(2/n); a correlation of unit-variance pairs over n/3 atoms: sqrt(3/n))."""
    atoms = 1 << 18
    _, g = host_noise(2024, 3, atoms)
    n = g.size
    assert np.all(np.isfinite(g))
    assert abs(g.mean()) < 5.0 / np.sqrt(n), g.mean()
    assert abs(g.var() - 1.0) < 5.0 * np.sqrt(2.0 / n), g.var()
    for a, b in ((0, 1), (0, 2), (1, 2)):
        c = float(np.mean(g[:, a] * g[:, b]))
        assert abs(c) < 5.0 / np.sqrt(atoms), (a, b, c)
    for k in range(3):                                   # ... and every component on its own
        assert abs(g[:, k].mean()) < 5.0 / np.sqrt(atoms) and abs(g[:, k].var() - 1.0) < 5.0 * np.sqrt(2.0 / atoms)


def _system(n, cell, seed, outside=True, infinite=True):
    rs = np.random.RandomState(seed)
    x = rs.uniform(0, 1, (n, 3)) @ cell
    if outside:
        x[::3] += np.array([3, -3, 3]) @ cell              # atoms that start three cells outside
    v = rs.normal(scale=0.02, size=(n, 3))
    m = rs.uniform(10.0, 60.0, n)
    if infinite and n > 1:
        m[n // 2], v[n // 2] = np.inf, 0.0
    return x, v, m


def _well(pos32, centre):
    """A fixed harmonic well, evaluated in numpy float64 and rounded to float32 (what a model hands the integrator)."""
    return (-0.8 * (pos32.astype(np.float64) - centre)).astype(np.float32)


def _same_state(host, ref):
    assert np.array_equal(bits(host.x), bits(ref.x))
    assert np.array_equal(bits(host.v), bits(ref.v))
    assert np.array_equal(host.image, ref.image)


@pytest.mark.parametrize("friction", [None, 0.02], ids=["nve", "baoab"])
@pytest.mark.parametrize("n,cell", [(1, CUBIC), (63, TRICLINIC), (64, TRICLINIC), (65, CUBIC), (257, TRICLINIC)])
def test_host_twin_equals_the_numpy_transcription_bit_for_bit(n, cell, friction):
    """50 steps of hermnet_host_md_advance / _finish against velocity Verlet (friction None) or BAOAB (noise from
    hermnet_host_md_noise) written out in numpy float64: x, v and image bit-equal after every step, pos32 the rounding of x, the
    logged kinetic energy within N 2^-52 relative of the numpy sum (the summation order may differ)."""
    x, v, m = _system(n, cell, seed=n)
    kw = dict(cell=cell, friction=friction, temperature=None if friction is None else 500.0, seed=77)
    host, ref = HostMD(x, v, m, 0.5, **kw), NumpyMD(x, v, m, 0.5, **kw)
    centre = np.array([0.5, 0.5, 0.5]) @ cell
    f = _well(host.pos32, centre)
    host.f_prev[:] = f
    ref.f = f.copy()
    x_start = x.copy()
    for step in range(50):
        p_host, p_ref = host.advance().copy(), ref.advance()
        assert np.array_equal(p_host.view(np.uint32), p_ref.view(np.uint32)), step
        host.finish(_well(p_host, centre), energy=[-3.25], total=(1000 + step, 0))
        ref.finish(_well(p_ref, centre))
        _same_state(host, ref)
        assert host.state.tolist() == [step + 1, 0, 0, 0]
        e_pot, e_kin, edges = host.log[step % host.log_steps, 0]
        want = float(np.sum(ref.ke))
        assert e_pot == -3.25 and edges == 1000 + step
        assert abs(e_kin - want) <= n * 2.0 ** -52 * abs(want), (e_kin, want)
    assert np.array_equal(host.f_prev, ref.f)
    # the first step wrapped the atoms that began three cells outside; image keeps the unwrapped path
    if n > 1:
        assert np.abs(host.image).max() >= 3
        s = host.x @ np.linalg.inv(cell.astype(np.float32).astype(np.float64))
        assert s.min() > -1e-9 and s.max() < 1 + 1e-9
    free = np.isfinite(m)
    if not free.all():          # infinite mass: kick = sigma = 0 -- the atom never moves (it is only wrapped)
        i = int(np.where(~free)[0][0])
        unwrapped = host.x[i] + host.image[i] @ cell.astype(np.float32).astype(np.float64)
        assert np.allclose(unwrapped, x_start[i], rtol=0, atol=1e-9) and not host.v[i].any()


def test_step_without_wrap_leaves_images_alone():
    x, v, m = _system(20, CUBIC, seed=3)
    host, ref = HostMD(x, v, m, 1.0), NumpyMD(x, v, m, 1.0)
    for _ in range(5):
        f = _well(host.advance(), 5.0)
        ref.advance()
        host.finish(f)
        ref.finish(f)
    _same_state(host, ref)
    assert not host.image.any() and np.abs(host.x).max() > 30.0


def _temperature(v, m):
    return (m[:, None] * AMU * v * v).sum() / (3 * len(v)) / KB


def test_free_particle_thermostat_reaches_its_temperature():
    """f = 0, N = 4096, friction dt = 0.1, 300 steps from v = 0: <m v^2> / kB within 5 standard errors (sqrt(2 / 12288)
    relative) of T -- BAOAB's O-step is exact for free particles, and after 300 steps the memory of v = 0 is e^-60."""
    n, T = 4096, 300.0
    rs = np.random.RandomState(0)
    m = rs.uniform(5.0, 100.0, n)
    host = HostMD(rs.uniform(0, 10, (n, 3)), np.zeros((n, 3)), m, 2.0, friction=0.05, temperature=T, seed=12345, log_steps=8)
    zero = np.zeros((n, 3), dtype=np.float32)
    for _ in range(300):
        host.advance()
        host.finish(zero)
    got = _temperature(host.v, m)
    assert abs(got / T - 1.0) < 5.0 * np.sqrt(2.0 / (3 * n)), got
    # the log's kinetic energy says the same
    assert abs(host.log[299 % 8, 0, 1] / (1.5 * n * KB) / T - 1.0) < 5.0 * np.sqrt(2.0 / (3 * n))


def test_two_graph_batch_gets_each_graph_its_own_temperature():
    n = 4096
    batch = np.repeat([0, 1], n)
    rs = np.random.RandomState(1)
    m = rs.uniform(5.0, 100.0, 2 * n)
    host = HostMD(rs.uniform(0, 10, (2 * n, 3)), np.zeros((2 * n, 3)), m, 2.0, batch=batch, friction=0.05,
                  temperature=[100.0, 900.0], seed=99, log_steps=4)
    zero = np.zeros((2 * n, 3), dtype=np.float32)
    for _ in range(300):
        host.advance()
        host.finish(zero, energy=[0.0, 0.0])
    for g, T in ((0, 100.0), (1, 900.0)):
        sel = batch == g
        got = _temperature(host.v[sel], m[sel])
        assert abs(got / T - 1.0) < 5.0 * np.sqrt(2.0 / (3 * n)), (g, got)
        assert abs(host.log[299 % 4, g, 1] / (1.5 * n * KB) / T - 1.0) < 5.0 * np.sqrt(2.0 / (3 * n))


@pytest.mark.parametrize("why", ["flags", "count", "nan", "inf"])
def test_halt_restores_the_last_completed_step(why):
    """A list flag, more pairs than columns or an energy that is not finite at step k: x, v, image return bit-exactly to the
    end of step k-1, code and step are recorded, no log row is written, and further steps change nothing."""
    n, k = 65, 6
    x, v, m = _system(n, TRICLINIC, seed=5, outside=False)
    batch = np.repeat([0, 1], [30, 35])
    kw = dict(cell=np.stack([TRICLINIC, TRICLINIC]), batch=batch, friction=0.02, temperature=[300.0, 600.0], seed=4, log_steps=16)
    host = HostMD(x, v, m, 0.5, **kw)
    centre = np.array([0.5, 0.5, 0.5]) @ TRICLINIC
    good = dict(energy=[-1.0, -2.0], total=(500, 0), capacity=512)
    for _ in range(k):
        host.finish(_well(host.advance(), centre), **good)
    keep = [a.copy() for a in (host.x, host.v, host.image, host.f_prev, host.log)]
    bad = {"flags": dict(good, total=(500, 2)), "count": dict(good, total=(513, 0)),
           "nan": dict(good, energy=[-1.0, np.nan]), "inf": dict(good, energy=[np.inf, -2.0])}[why]
    code = {"flags": 2, "count": 4, "nan": NONFINITE, "inf": NONFINITE}[why]
    moved = host.advance().copy()
    assert not np.array_equal(bits(host.x), bits(keep[0]))
    host.finish(np.full((n, 3), np.nan, dtype=np.float32) if why in ("nan", "inf") else _well(moved, centre), **bad)
    for _ in range(3):                                   # further steps, good or bad, change nothing
        assert host.state.tolist() == [k, code, k, 0]
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8))
                   for a, b in zip((host.x, host.v, host.image, host.f_prev, host.log), keep))
        assert np.array_equal(host.pos32, keep[0].astype(np.float32))
        host.finish(_well(host.advance(), centre), **good)
    assert np.all(host.log[k:] == -7.0) and np.all(host.log[:k, :, 0] == [-1.0, -2.0])
    # cleared by the caller and primed, the run goes on -- as an uninterrupted one does (the noise is a function of the step)
    twin = HostMD(x, v, m, 0.5, **kw)
    for _ in range(k + 2):
        twin.finish(_well(twin.advance(), centre), **good)
    host.state[1:3] = 0
    host.state[3] = 1
    host.finish(_well(host.advance(), centre), **good)
    assert host.state.tolist() == [k, 0, 0, 0]
    for _ in range(2):
        host.finish(_well(host.advance(), centre), **good)
    assert np.array_equal(bits(host.x), bits(twin.x)) and np.array_equal(bits(host.v), bits(twin.v))
    assert np.array_equal(host.image, twin.image) and np.array_equal(bits(host.log[:k + 2]), bits(twin.log[:k + 2]))


def test_prime_mode_changes_neither_step_nor_velocities():
    x, v, m = _system(40, CUBIC, seed=9)
    host = HostMD(x, v, m, 1.0, cell=CUBIC)
    host.state[3] = 1
    p = host.advance().copy()
    assert np.array_equal(p, x.astype(np.float32))                   # (not even wrapped: the coordinates as they are)
    f = _well(p, 5.0)
    host.finish(f, energy=[1.5], total=(10, 0))
    assert host.state.tolist() == [0, 0, 0, 0] and np.array_equal(host.f_prev, f)
    assert np.array_equal(bits(host.x), bits(x)) and np.array_equal(bits(host.v), bits(v)) and not host.image.any()
    assert np.all(host.log == -7.0)
    # a prime evaluation that fails halts (nothing to restore) and leaves f_prev alone
    host.state[3] = 1
    host.advance()
    host.finish(np.zeros_like(f), energy=[np.nan], total=(10, 0))
    assert host.state.tolist() == [0, NONFINITE, 0, 0] and np.array_equal(host.f_prev, f)


def _sequential(terms):
    """hermnet_host_md_finish's kinetic-energy sum: one accumulator from 0.0, atoms in ascending order."""
    s = 0.0
    for t in terms:
        s = s + float(t)
    return s


@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
@pytest.mark.parametrize("n", [0, 1, 256, 257, 513])
def test_one_graph_on_both_sides_of_the_lane_boundary(n, wrap):
    """No atom, one, a full row of 256 lanes, one over, two rows and one: four BAOAB steps bit-equal to the numpy
    transcription, the log row's kinetic energy bit-equal to the host twin's own (sequential) order."""
    x, v, m = _system(n, TRICLINIC, seed=100 + n)
    kw = dict(cell=TRICLINIC if wrap else None, friction=0.02, temperature=400.0, seed=5, num_graphs=1)
    host, ref = HostMD(x, v, m, 0.5, log_steps=3, **kw), NumpyMD(x, v, m, 0.5, **kw)
    centre = np.array([0.5, 0.5, 0.5]) @ TRICLINIC
    for step in range(4):
        p_host, p_ref = host.advance().copy(), ref.advance()
        assert np.array_equal(p_host.view(np.uint32), p_ref.view(np.uint32))
        host.finish(_well(p_host, centre), energy=[0.5 * step], total=(7 * step, 0))
        ref.finish(_well(p_ref, centre))
        _same_state(host, ref)
        assert host.state.tolist() == [step + 1, 0, 0, 0]
        assert bits(host.log[step % 3, 0]).tolist() == bits([0.5 * step, _sequential(ref.ke), 7.0 * step]).tolist()
    assert bool(host.image.any()) == (wrap and n > 0)


_HOSTILE = dict(sizes=(130, 0, 70), temperature=[300.0, 500.0, 700.0])


def _hostile_batch(broken, friction=0.02):
    """Three graphs, the middle one empty, a triclinic and an orthogonal cell; `broken`: the first and the last `batch` entry
    out of range on either side (the library clamps them to the graphs they belong to: the numpy twin keeps the sound batch)."""
    n = sum(_HOSTILE["sizes"])
    x, v, m = _system(n, CUBIC, seed=21)
    batch = np.repeat([0, 1, 2], _HOSTILE["sizes"])
    kw = dict(cell=np.stack([TRICLINIC, CUBIC, CUBIC]), batch=batch, friction=friction,
              temperature=None if friction is None else _HOSTILE["temperature"], seed=8, num_graphs=3)
    host, ref = HostMD(x, v, m, 0.5, log_steps=8, **kw), NumpyMD(x, v, m, 0.5, **kw)
    if broken:
        host.batch[0], host.batch[-1] = -7, 99
    return host, ref, np.array([5.0, 5.5, 6.0])


@pytest.mark.parametrize("friction", [None, 0.02], ids=["nve", "baoab"])
@pytest.mark.parametrize("broken", [False, True], ids=["sound", "broken"])
def test_batch_with_an_empty_graph_and_a_batch_out_of_range(broken, friction):
    host, ref, centre = _hostile_batch(broken, friction)
    ptr = host.graph_ptr
    assert ptr.tolist() == [0, 130, 130, 200]
    for step in range(4):
        p_host, p_ref = host.advance().copy(), ref.advance()
        assert np.array_equal(p_host.view(np.uint32), p_ref.view(np.uint32))
        host.finish(_well(p_host, centre), energy=[-1.0, -2.0, -3.0], total=(40 + step, 0))
        ref.finish(_well(p_ref, centre))
        _same_state(host, ref)
        want = [[-1.0 - g, _sequential(ref.ke[ptr[g]:ptr[g + 1]]), 40.0 + step] for g in range(3)]
        assert np.array_equal(bits(host.log[step]), bits(want))
    assert host.state.tolist() == [4, 0, 0, 0] and np.all(host.log[4:] == -7.0) and host.image.any()


@pytest.mark.parametrize("why", ["flags", "count", "nan", "inf"])
def test_void_step_in_the_hostile_batch(why):
    """Each halt cause on its own, at step 3 of the batch above with its broken `batch`: x, v, image, f_prev and the log
    bit-equal to the end of step 2, pos32 the rounding of x, state = (3, code, 3, 0), and a second call changes nothing."""
    host, _, centre = _hostile_batch(True)
    good = dict(energy=[-1.0, -2.0, -3.0], total=(500, 0), capacity=512)
    for _ in range(3):
        host.finish(_well(host.advance(), centre), **good)
    names = ("x", "v", "image", "f_prev", "log", "ke_atom")
    keep = [getattr(host, k).copy() for k in names]
    bad, code = {"flags": (dict(good, total=(500, 16)), 16), "count": (dict(good, total=(513, 0)), 4),
                 "nan": (dict(good, energy=[-1.0, np.nan, -3.0]), NONFINITE),
                 "inf": (dict(good, energy=[-1.0, -2.0, -np.inf]), NONFINITE)}[why]
    moved = host.advance().copy()
    assert not np.array_equal(bits(host.x), bits(keep[0]))
    host.finish(_well(moved, centre), **bad)
    for again in range(2):
        assert host.state.tolist() == [3, code, 3, 0]
        assert all(np.array_equal(getattr(host, k).view(np.uint8), b.view(np.uint8)) for k, b in zip(names, keep))
        assert np.array_equal(host.pos32, keep[0].astype(np.float32))
        host.finish(_well(host.advance(), centre), **good)


@pytest.mark.parametrize("code", [0, 4], ids=["clean", "halting"])
def test_prime_in_the_hostile_batch(code):
    """Mode 1 with and without a halt code: nothing moves and no row is written; a clean prime takes the forces and clears
    the mode, a failing one records the halt (at the step it stands at) and leaves f_prev alone."""
    host, _, centre = _hostile_batch(True)
    host.finish(_well(host.advance(), centre), energy=[0.0, 0.0, 0.0])
    names = ("x", "v", "image", "log", "ke_atom")
    keep = [getattr(host, k).copy() for k in names]
    f_before = host.f_prev.copy()
    host.state[3] = 1
    p = host.advance().copy()
    assert np.array_equal(p, keep[0].astype(np.float32))
    f = _well(p, centre) + np.float32(1.0)
    host.finish(f, energy=[0.0, 0.0, 0.0], total=(11 if code else 10, 0), capacity=10)
    assert host.state.tolist() == [1, code, 1 if code else 0, 0]
    assert all(np.array_equal(getattr(host, k).view(np.uint8), b.view(np.uint8)) for k, b in zip(names, keep))
    assert np.array_equal(host.f_prev, f_before if code else f)


def test_argument_checks_of_the_md_entry_points_need_no_gpu():
    host = HostMD(*_system(4, CUBIC, seed=1), 1.0, cell=CUBIC)
    lib, P = host.lib, lambda a: a.ctypes.data
    assert lib.hermnet_md_noise(0, 0, -1, None, None, None) == 1 and lib.hermnet_md_noise(0, 0, 0, P(host.x), None, None) == 0
    assert lib.hermnet_host_md_noise(0, 0, 3, None, None) == 1
    assert lib.hermnet_md_advance(0, 1, 0, 1.0, 0, *([None] * 16)) == 0               # no atoms: done
    assert lib.hermnet_md_advance(4, 1, 0, 1.0, 0, *([None] * 16)) == 1               # atoms but no state
    assert lib.hermnet_md_advance(0, 1, 4, 1.0, 0, *([None] * 16)) == 1               # unknown flag
    assert lib.hermnet_md_advance(0, 0, 0, 1.0, 0, *([None] * 16)) == 1               # no graph
    assert lib.hermnet_md_finish(4, 1, *([None] * 4), 16, *([None] * 12), 8, None, None) == 1
