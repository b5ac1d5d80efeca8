"""CPU: the ring-polymer step (hermnet_amd/csrc/pimd_step.h) through the library's host twins hermnet_host_pimd_advance /
_finish -- against its numpy transcription bit for bit, its noise against a pure-Python Philox, one bead against DeviceMD's
host twins bit for bit, and its physics: the free ring polymer's conserved energy and the quantum harmonic oscillator's
finite-P energies."""
import math

import numpy as np
import pytest

from hermnet_amd.pimd import HBAR, ring_matrix, ring_tables
from md_reference import AMU, KB, HostMD, bits, host_noise, noise_words
from pimd_reference import FIELDS, HostPIMD, NumpyPIMD

TRICLINIC = np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]])
CASES = [(1, 5), (2, 3), (3, 1), (4, 257), (6, 63), (32, 9), (128, 2)]      # (P, n_rep): odd P, P = 2, ragged tiles, the cap
DT, T = 0.5, 300.0


def _same(a, b, what, fields=FIELDS):
    for k in fields:
        p, q = getattr(a, k), getattr(b, k)
        if p.dtype == np.float64:
            assert np.array_equal(bits(p), bits(q)), (what, k)
        else:
            assert np.array_equal(p, q), (what, k)


def _ring(P, n_rep, seed, cell=None, inf_atom=None, spread=0.05):
    """A ring polymer's start: beads within `spread` of the atom's place (inside `cell`, or a 6 A box), velocities, masses."""
    rs = np.random.RandomState(seed)
    base = rs.uniform(0.0, 1.0, (n_rep, 3)) @ (cell if cell is not None else np.diag([6.0, 6.0, 6.0]))
    x = (base[None] + rs.normal(scale=spread, size=(P, n_rep, 3))).reshape(-1, 3)
    v = rs.normal(scale=0.02, size=(P * n_rep, 3))
    m_rep = rs.uniform(1.0, 40.0, n_rep)
    if inf_atom is not None:
        m_rep[inf_atom] = np.inf
    m = np.tile(m_rep, P)
    v[~np.isfinite(m)] = 0.0
    return x, v, m, rs


def _pair(P, n_rep, thermostat, seed=3, cell=None, inf_atom=None, tau0=100.0, **kw):
    x, v, m, rs = _ring(P, n_rep, seed, cell, inf_atom)
    args = dict(tau0=tau0, thermostat=thermostat, seed=(5 << 32) + 9, log_steps=4, cell=cell)
    args.update(kw)
    pair = [cls(P, x, v, m, DT, T, **args) for cls in (HostPIMD, NumpyPIMD)]
    f0 = rs.normal(size=(P * n_rep, 3)).astype(np.float32)
    for p in pair:
        p.f_prev[:] = f0
    return pair[0], pair[1], rs


@pytest.mark.parametrize("P", sorted(set(p for p, _ in CASES)))
def test_the_normal_mode_matrix_is_orthogonal(P):
    c = ring_matrix(P)
    assert np.abs(c.T @ c - np.eye(P)).max() <= 1e-13 and np.abs(c @ c.T - np.eye(P)).max() <= 1e-13
    # it diagonalises the ring's spring matrix with the eigenvalues (omega_k / omega_P)^2 = 4 sin^2(k pi / P)
    a = 2.0 * np.eye(P) - np.roll(np.eye(P), 1, axis=0) - np.roll(np.eye(P), -1, axis=0)
    lam = 4.0 * np.sin(np.arange(P) * math.pi / P) ** 2
    assert np.abs(c.T @ a @ c - np.diag(lam)).max() <= 1e-12
    tb = ring_tables(P, DT, T, np.array([AMU]))
    assert np.allclose(tb.omega, tb.omega_p * np.sqrt(lam), rtol=1e-14, atol=0) and tb.omega_p == P * KB * T / HBAR


@pytest.mark.parametrize("thermostat", [False, True], ids=["rpmd", "pile"])
@pytest.mark.parametrize("P,n_rep", CASES)
def test_host_twins_equal_the_numpy_transcription_bit_for_bit(P, n_rep, thermostat):
    """Six steps in a triclinic cell, one atom of infinite mass where there are two or more: every array -- x, v, image, the
    backups, f_prev, pos32, the centroid scratch, the log ring, state -- bit-equal after every advance and every finish.  With
    the thermostat both take the Gaussians of the library's host form."""
    host, ref, rs = _pair(P, n_rep, thermostat, seed=P, cell=TRICLINIC, inf_atom=1 if n_rep > 1 else None)
    n = P * n_rep
    for step in range(6):
        assert np.array_equal(host.advance().view(np.uint32), ref.advance().view(np.uint32)), step
        _same(host.snapshot(), ref.snapshot(), ("advance", step))
        f, e = rs.normal(size=(n, 3)).astype(np.float32), rs.normal(size=P).astype(np.float32)
        host.finish(f, e, total=(100 + step, 0))
        ref.finish(f, e, total=(100 + step, 0))
        _same(host.snapshot(), ref.snapshot(), ("finish", step))
        assert host.state.tolist() == [step + 1, 0, 0, 0]
        images = host.image.reshape(P, n_rep, 3)
        assert np.all(images == images[0])                      # beads of one atom never get different images
    assert np.all(host.log[[0, 1]][:, :, 2] == [[104], [105]]) and np.all(np.isfinite(host.log))
    if n_rep > 1:
        held = host.x.reshape(P, n_rep, 3)[:, 1]
        assert np.array_equal(held.reshape(-1, 3), host.x0.reshape(P, n_rep, 3)[:, 1].reshape(-1, 3))
        assert not host.v.reshape(P, n_rep, 3)[:, 1].any()


def _python_gaussians(seed, step, n):
    """md_gaussians on the pure-Python Philox words of the indices 0..n-1."""
    out = np.zeros((n, 3))
    u = lambda hi, lo: float(((hi >> 5) << 26) | (lo >> 6))
    s = 1.0 / 9007199254740992.0
    for i in range(n):
        w = noise_words(seed, step, i)
        ra, ta = math.sqrt(-2.0 * math.log((u(w[0], w[1]) + 1.0) * s)), 2.0 * math.pi * (u(w[2], w[3]) * s)
        rb, tb = math.sqrt(-2.0 * math.log((u(w[4], w[5]) + 1.0) * s)), 2.0 * math.pi * (u(w[6], w[7]) * s)
        out[i] = (ra * math.cos(ta), ra * math.sin(ta), rb * math.cos(tb))
    return out


def test_the_noise_of_mode_k_and_atom_a_is_philox_of_k_n_rep_plus_a():
    """Raw words bit for bit against the pure-Python Philox at the index k n_rep + a; the twin's thermostatted step equals
    the transcription fed with Gaussians made in pure Python from those words, within 1e-12 of the state's scale (the last
    digits of two log / cos implementations); noise shifted by one index, or of another step, does not."""
    P, n_rep, seed = 6, 7, (5 << 32) + 9
    x, v, m, rs = _ring(P, n_rep, 11)
    for step in (0, 3, (1 << 32) + 2):
        words, gauss = host_noise(seed, step, P * n_rep)
        for k, a in ((0, 0), (1, 0), (5, 6), (3, 2)):
            assert words[k * n_rep + a].tolist() == noise_words(seed, step, k * n_rep + a)
        assert np.abs(gauss - _python_gaussians(seed, step, P * n_rep)).max() <= 1e-12
    host = HostPIMD(P, x, v, m, DT, T, seed=seed)
    host.state[0] = 3
    host.advance()
    for shift, same in ((0, True), (1, False)):
        ref = NumpyPIMD(P, x, v, m, DT, T, seed=seed, gaussians=lambda s: np.roll(_python_gaussians(seed, s, P * n_rep), shift, 0))
        ref.state[0] = 3
        ref.advance()
        close = (np.abs(ref.x - host.x).max() <= 1e-12 * np.abs(host.x).max()
                 and np.abs(ref.v - host.v).max() <= 1e-12 * np.abs(host.v).max())
        assert close == same, shift


def test_a_centroid_that_crosses_a_face_takes_every_bead_with_it():
    """A triclinic cell; atom 0's centroid sits 1e-3 inside the face s_0 = 1 and moves out this step, while some of its
    beads are still inside: every bead loses the same lattice vector, images are equal, the wrapped centroid is inside."""
    P, n_rep = 4, 3
    host, ref, _ = _pair(P, n_rep, False, cell=TRICLINIC)
    cell = TRICLINIC.astype(np.float32).astype(np.float64)
    for p in (host, ref):
        X, V = p.x.reshape(P, n_rep, 3), p.v.reshape(P, n_rep, 3)
        X[:, 0] = np.array([0.999, 0.4, 0.6]) @ cell + np.array([[0.05, 0, 0], [-0.05, 0, 0], [0.02, 0, 0], [-0.02, 0, 0]])
        V[:, 0] = np.array([0.05, 0.0, 0.0])
        p.f_prev[:] = 0.0
    before = host.x.reshape(P, n_rep, 3)[:, 0].copy()
    host.advance()
    ref.advance()
    _same(host.snapshot(), ref.snapshot(), "face")
    img = host.image.reshape(P, n_rep, 3)
    assert np.all(img[:, 0] == [1, 0, 0]) and not img[:, 1:].any()
    s_beads = (before + DT * 0.05 * np.array([1.0, 0, 0])) @ np.linalg.inv(cell)
    assert s_beads[:, 0].min() < 1.0 < s_beads[:, 0].max()            # some beads had crossed, some had not
    s_c = host.centroid[0] @ np.linalg.inv(cell)
    assert 0.0 <= s_c[0] < 0.01 and np.allclose(host.x.reshape(P, n_rep, 3)[:, 0].mean(axis=0), host.centroid[0], atol=1e-12)


@pytest.mark.parametrize("what", ["capacity", "nonfinite", "prime", "halted"])
def test_a_step_that_is_not_committed(what):
    """A void step (more pairs than capacity; a NaN energy) restores x, v and image of every bead and writes no row; a prime
    moves nothing, takes the forces and clears the mode; a set halt code changes nothing at all."""
    P, n_rep = 6, 63
    host, ref, rs = _pair(P, n_rep, True, cell=TRICLINIC, inf_atom=2)
    n = P * n_rep
    for _ in range(2):
        f, e = rs.normal(size=(n, 3)).astype(np.float32), rs.normal(size=P).astype(np.float32)
        for p in (host, ref):
            p.advance()
            p.finish(f, e)
    if what == "prime":
        host.state[3] = ref.state[3] = 1
    if what == "halted":
        host.state[1:3] = ref.state[1:3] = (2, 1)
    before = host.snapshot()
    f, e = rs.normal(size=(n, 3)).astype(np.float32), rs.normal(size=P).astype(np.float32)
    total, capacity = (500, 0), 1000
    if what == "capacity":
        total = (1001, 0)
    if what == "nonfinite":
        e[P - 1] = np.nan
    for p in (host, ref):
        p.advance()
    if what in ("capacity", "nonfinite"):
        assert not np.array_equal(host.x, before.x)                   # the step had moved the beads ...
    for p in (host, ref):
        p.finish(f, e, total=total, capacity=capacity)
    after = host.snapshot()
    _same(after, ref.snapshot(), what, [k for k in FIELDS if k not in ("x0", "v0", "image0") or what != "halted"])
    for k in ("x", "v", "image", "log"):                              # ... and is back where it began, with no row
        assert np.array_equal(getattr(before, k), getattr(after, k)), k
    assert np.array_equal(after.pos32, after.x.astype(np.float32))
    want = {"capacity": [2, 4, 2, 0], "nonfinite": [2, 256, 2, 0], "prime": [2, 0, 0, 0], "halted": [2, 2, 1, 0]}[what]
    assert after.state.tolist() == want
    assert np.array_equal(after.f_prev, f if what == "prime" else before.f_prev)


def test_entry_points_refuse_what_they_cannot_run():
    x, v, m, _ = _ring(2, 3, 0)
    host = HostPIMD(2, x, v, m, DT, T)
    host.B = 129                                                      # more than 128 beads
    host.advance(expect=1)
    host.B, host.n = 2, 5                                             # atoms that the beads do not divide
    host.advance(expect=1)
    host.n = 6
    host.graph_ptr[1] = 2                                             # beads of unequal ranges
    host.finish(np.zeros((6, 3), dtype=np.float32), expect=1)


def test_a_free_ring_polymer_conserves_its_energy_and_its_centroid_moves_uniformly():
    """Zero forces, no thermostat, P = 6, dt = 5 fs, 2,000 steps: `ring_energy` constant to 1e-11 relative (each step is an
    exact rotation of every mode: only rounding accumulates), the centroid on a straight line.  A wrong C, omega_k, sw or
    ws fails this at once."""
    P, n_rep, steps, dt = 6, 5, 2000, 5.0
    x, v, m, _ = _ring(P, n_rep, 21)
    host = HostPIMD(P, x, v, m, dt, T, thermostat=False, log_steps=steps)
    zero = np.zeros((P * n_rep, 3), dtype=np.float32)
    c0, vc = host.x.reshape(P, n_rep, 3).mean(axis=0), host.v.reshape(P, n_rep, 3).mean(axis=0)
    worst = 0.0
    for step in range(steps):
        host.advance()
        host.finish(zero)
        worst = max(worst, np.abs(host.centroid - (c0 + (step + 1) * dt * vc)).max())
    ring = host.estimators()[3]
    drift = np.abs(ring / ring[0] - 1.0).max()
    print("free ring polymer: relative drift of ring_energy %.2e, centroid off its line by %.2e A" % (drift, worst))
    assert ring[0] > 0.0 and drift <= 1e-11
    assert worst <= 1e-10
    spring = host.log[:, :, 3].sum(axis=1)
    assert spring.std() > 0.05 * spring.mean()                        # the springs really exchange energy with the beads


@pytest.mark.parametrize("thermostat", [True, False], ids=["langevin", "nve"])
def test_one_bead_is_device_md(thermostat):
    """P = 1 against hermnet_host_md_advance / _finish, bit for bit in x, v and image over 50 steps in a triclinic cell with
    atoms that start cells outside: Langevin with friction = 1 / tau0, and NVE with the thermostat off."""
    n, tau0 = 65, 40.0
    rs = np.random.RandomState(4)
    x = rs.uniform(-1.5, 2.5, (n, 3)) @ TRICLINIC
    v, m = rs.normal(scale=0.02, size=(n, 3)), rs.uniform(1.0, 60.0, n)
    m[7], v[7], x[7] = np.inf, 0.0, np.array([0.3, 0.4, 0.5]) @ TRICLINIC     # (held, and inside: DeviceMD would wrap it,
    kw = dict(friction=1.0 / tau0, temperature=T) if thermostat else {}       #  a ring leaves a held atom where it was given)
    md = HostMD(x, v, m, DT, cell=TRICLINIC, seed=77, **kw)
    ring = HostPIMD(1, x, v, m, DT, T, tau0=tau0, thermostat=thermostat, seed=77, cell=TRICLINIC)
    f = (-0.8 * (x - np.array([0.5, 0.5, 0.5]) @ TRICLINIC)).astype(np.float32)
    md.f_prev[:], ring.f_prev[:] = f, f
    for step in range(50):
        pa, pb = md.advance(), ring.advance()
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), step
        f = (-0.8 * (pa.astype(np.float64) - np.array([0.5, 0.5, 0.5]) @ TRICLINIC)).astype(np.float32)
        md.finish(f)
        ring.finish(f)
        assert np.array_equal(bits(md.x), bits(ring.x)) and np.array_equal(bits(md.v), bits(ring.v)), step
        assert np.array_equal(md.image, ring.image)
    assert np.abs(ring.image).max() >= 1 and np.all(ring.log[:50 % ring.log_steps, 0, 3] == 0.0)


# ---- the quantum harmonic oscillator: host twins only ---------------------------------------------------------------------------
N_WELL, M_WELL, STEPS, BLOCK = 8, 1.008, 40000, 1000
OMEGA = 4.0 * KB * T / HBAR                       # hbar omega = 4 kB T: the ground state dominates
K_WELL = M_WELL * AMU * OMEGA * OMEGA
CLASSICAL = 1.5 * N_WELL * KB * T
_WELL = {}


def _theory(P):
    """(3N/2) kB T sum_k omega^2 / (omega_k^2 + omega^2): the finite-P value of <V> and of both kinetic estimators."""
    wk = 2.0 * (P * KB * T / HBAR) * np.sin(np.arange(P) * math.pi / P)
    return CLASSICAL * float(np.sum(OMEGA ** 2 / (wk ** 2 + OMEGA ** 2)))


def _forces(host, P):
    """V = k/2 sum |x|^2 per bead: (forces, energies), rounded to float32 as a model hands them over."""
    e = (0.5 * K_WELL * (host.x * host.x).reshape(P, -1).sum(axis=1)).astype(np.float32)
    return (-K_WELL * host.x).astype(np.float32), e


def _well(P, steps=STEPS, tau0=20.0, thermostat=True, start=None):
    """`steps` steps of 8 hydrogen atoms x P beads in the well, open, dt = 0.5 fs, through the host twins; cached."""
    key = (P, steps, tau0, thermostat, start is not None)
    if key not in _WELL:
        rs = np.random.RandomState(17)
        n = P * N_WELL
        if start is None:
            x = rs.normal(size=(n, 3)) * math.sqrt(KB * T / K_WELL)
            v = rs.normal(size=(n, 3)) * math.sqrt(KB * P * T / (M_WELL * AMU))
        else:
            x, v = start
        host = HostPIMD(P, x, v, np.full(n, M_WELL), 0.5, T, tau0=tau0, thermostat=thermostat, seed=2024, log_steps=steps)
        host.f_prev[:] = _forces(host, P)[0]
        for _ in range(steps):
            host.advance()
            f, e = _forces(host, P)
            host.finish(f, e)
        assert host.state.tolist() == [steps, 0, 0, 0]
        _WELL[key] = (host.estimators(), host.x.copy(), host.v.copy())
    return _WELL[key]


def _blocked(series):
    blocks = series.reshape(-1, BLOCK).mean(axis=1)
    return series.mean(), blocks.std(ddof=1) / math.sqrt(len(blocks))


@pytest.mark.parametrize("P,theory", [(8, 0.62533), (4, 0.57908)])
def test_well_estimators_equal_the_finite_bead_theory(P, theory):
    """40,000 steps, PILE-L with tau0 = 20 fs: the means of `potential`, `kinetic_primitive` and `kinetic_virial` equal
    (3N/2) kB T sum_k omega^2 / (omega_k^2 + omega^2) within 5 standard errors from blocks of 1,000 steps, and -- whatever the
    error bars -- within a fifth of the gap to the classical value (3N/2) kB T = 0.31022 eV (0.063 eV at P = 8): a run cannot
    pass by being noisy.  A numpy prototype gave 0.6283 +- 0.0030, 0.6256 +- 0.0032 and 0.6245 +- 0.0009 at P = 8."""
    assert abs(_theory(P) - theory) < 5e-6 and abs(CLASSICAL - 0.31022) < 5e-6
    pot, prim, vir, _ = _well(P)[0]
    for name, series in (("potential", pot), ("kinetic_primitive", prim), ("kinetic_virial", vir)):
        mean, se = _blocked(series)
        print("P = %d %s: %.5f +- %.5f, theory %.5f, classical %.5f" % (P, name, mean, se, _theory(P), CLASSICAL))
        assert abs(mean - _theory(P)) <= 5.0 * se, (name, mean, se)
        assert abs(mean - _theory(P)) <= 0.2 * (_theory(P) - CLASSICAL), (name, mean)


def test_well_rpmd_conserves_the_ring_energy_as_well_as_velocity_verlet_conserves_its_own():
    """TRPMD (tau0 = None) runs from the sampled ensemble and keeps its temperature; RPMD started from its end: the drift of
    `ring_energy` over 4,000 steps, relative to its mean, is below twice that of hermnet_host_md_advance / _finish (NVE) on
    the same well, dt and atoms (one bead of that ensemble)."""
    P, steps = 8, 4000
    _, x, v = _well(P)
    est, x, v = _well(P, steps=steps, tau0=None, start=(x, v))
    assert abs(est[0].mean() - _theory(P)) <= 0.2 * (_theory(P) - CLASSICAL)
    ring = _well(P, steps=steps, thermostat=False, start=(x, v))[0][3]
    rpmd = np.abs(ring - ring[0]).max() / abs(ring.mean())
    md = HostMD(x[:N_WELL], v[:N_WELL], np.full(N_WELL, M_WELL), 0.5, log_steps=steps)
    md.f_prev[:] = (-K_WELL * md.x).astype(np.float32)
    for _ in range(steps):
        md.advance()
        md.finish((-K_WELL * md.x).astype(np.float32), [np.float32(0.5 * K_WELL * (md.x * md.x).sum())])
    total = md.log[:, 0, 0] + md.log[:, 0, 1]
    nve = np.abs(total - total[0]).max() / abs(total.mean())
    print("drift over %d steps: RPMD ring_energy %.3e, velocity Verlet %.3e (relative)" % (steps, rpmd, nve))
    assert rpmd <= 2.0 * nve
