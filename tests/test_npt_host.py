"""CPU: the barostat of the device-resident integrator (hermnet_amd/csrc/npt_step.h) through the library's host twin
hermnet_host_md_finish_npt -- against the numpy float64 transcription bit for bit, the steps that must not scale (void, prime,
parked), the two safety conditions, compressibility 0 against hermnet_host_md_finish, and the argument checks.  No GPU: the
host twin runs the text the device kernels run (tests/test_npt_device.py compares the two on the same inputs)."""
import numpy as np
import pytest

from hermnet_amd import _lib
from md_reference import HostMD, bits
from npt_reference import HostNPT, NumpyNPT

SIZES = [1, 5, 257, 300]        # below a lane count; one past 256: the strided lane sum and the fold both act; unequal ranges
CELLS = np.array([[[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]],
                  [[8.0, 0.0, 0.0], [1.5, 9.0, 0.0], [0.5, -2.0, 10.0]],
                  [[12.1, 1.4, 0.2], [-0.8, 10.7, 1.9], [2.2, 0.6, 13.3]],
                  [[10.0, 2.0, 1.0], [0.3, 12.5, -1.1], [-2.4, 0.9, 11.8]]])
PRESSURES = [0.0, 0.004, -0.003, 0.01]
DT = 0.5


def synthetic(seed=5):
    """A batch of four graphs in triclinic cells, some atoms cells away (the wrap acts), one atom held."""
    rs = np.random.RandomState(seed)
    batch = np.repeat(np.arange(4), SIZES)
    n = len(batch)
    x = np.einsum("nk,nkj->nj", rs.uniform(-1.5, 2.5, (n, 3)), CELLS[batch])
    m = rs.uniform(10.0, 60.0, n)
    m[40] = np.inf
    v = rs.normal(scale=0.003, size=(n, 3))
    v[40] = 0.0
    return dict(x=x, v=v, m=m, batch=batch, n=n)


def evaluation(rs, n, B=4, scale=40.0):
    """Synthetic float32 forces [n,3], virial [B,9] (not symmetric: sym() acts) and energies [B]."""
    return (rs.normal(size=(n, 3)).astype(np.float32), (scale * rs.normal(size=(B, 9))).astype(np.float32),
            rs.normal(size=B).astype(np.float32))


def make(cls, s, coupling="isotropic", friction=None, compressibility=0.1, pressure=PRESSURES, **kw):
    lang = {} if friction is None else dict(friction=friction, temperature=[300.0, 600.0, 900.0, 450.0], seed=(3 << 32) + 9)
    return cls(s["x"], s["v"], s["m"], DT, CELLS, pressure, compressibility, DT, coupling=coupling, mask=(1, 0, 1),
               batch=s["batch"], num_graphs=4, **lang, **kw)


@pytest.mark.parametrize("coupling,friction", [("isotropic", None), ("axes", 0.02), ("full", None)])
def test_host_twin_equals_the_numpy_transcription_bit_for_bit(coupling, friction):
    """Five steps on synthetic forces and virials: x, v, images, cell64, cell32, inv, mu and the log row of the host twin
    against numpy, bit for bit, per graph pressures, all three couplings ("axes" with mask (1,0,1), under Langevin)."""
    s = synthetic()
    host, ref = make(HostNPT, s, coupling, friction), make(NumpyNPT, s, coupling, friction)
    rs = np.random.RandomState(17)
    start = host.cell64.copy()
    for k in range(5):
        f, w, e = evaluation(rs, s["n"])
        p_host, p_ref = host.advance(), ref.advance()
        assert np.array_equal(p_host, p_ref)
        host.finish(f, w, energy=e, total=(1000 + k, 0))
        ref.finish(f, w, energy=e, edges=1000 + k)
        assert host.state.tolist() == [k + 1, 0, 0, 0]
        assert np.array_equal(bits(host.x), bits(ref.x)) and np.array_equal(bits(host.v), bits(ref.v))
        assert np.array_equal(host.image, ref.image) and np.array_equal(host.pos32, ref.x.astype(np.float32))
        assert np.array_equal(bits(host.cell64), bits(ref.cell64)) and np.array_equal(host.cell, ref.cell32)
        assert np.array_equal(bits(host.inv), bits(ref.inv64)) and np.array_equal(bits(host.mu), bits(ref.mu))
        assert np.array_equal(bits(host.log[k]), bits(ref.log[k]))
        assert np.all(host.log[k][:, 2] == 1000 + k) and np.all(host.log[k][:, 4] > 0)
        # inv is the inverse of the widened float32 cell
        prod = np.einsum("gij,gjk->gik", host.cell.astype(np.float64).reshape(4, 3, 3), host.inv.reshape(4, 3, 3))
        assert np.abs(prod - np.eye(3)).max() < 1e-13
    assert not host.clamped.any() and not ref.clamped.any()
    assert np.abs(host.image).max() >= 1                                              # the wrap acted
    assert np.all(np.abs(host.cell64 - start).reshape(4, -1).max(axis=1) > 1e-4)        # every graph's cell moved
    mu = host.mu.reshape(4, 3, 3)
    if coupling == "axes":
        assert np.all(mu[:, 1, 1] == 1.0) and np.all(mu[:, 0, 0] != 1.0) and np.all(mu[:, 2, 2] != 1.0)
    if coupling != "full":
        assert not mu[:, ~np.eye(3, dtype=bool)].any()
    else:
        assert np.all(mu[:, ~np.eye(3, dtype=bool)] != 0.0) and np.array_equal(mu, mu.transpose(0, 2, 1))
    if coupling == "isotropic":
        assert np.all(mu[:, 0, 0] == mu[:, 1, 1]) and np.all(mu[:, 0, 0] == mu[:, 2, 2])
        assert len(set(mu[:, 0, 0].tolist())) == 4                                    # its own pressure per graph


def _cell_state(h):
    return bits(h.cell64).tobytes(), h.cell.tobytes(), bits(h.inv).tobytes(), bits(h.mu).tobytes(), h.clamped.tobytes()


@pytest.mark.parametrize("why,total,nan_energy,code", [("capacity", (5001, 0), False, 4), ("list flag", (10, 2), False, 2),
                                                       ("energy", (10, 0), True, 256)])
def test_a_void_step_does_not_scale(why, total, nan_energy, code):
    """A step that does not commit leaves cell64, cell32 and inv bit-unchanged and restores x, v and the images."""
    s = synthetic()
    host = make(HostNPT, s, "full")
    rs = np.random.RandomState(2)
    f, w, e = evaluation(rs, s["n"])
    host.advance()
    host.finish(f, w, energy=e, total=(10, 0), capacity=5000)                        # one committed step
    assert host.state.tolist() == [1, 0, 0, 0]
    before = (bits(host.x).tobytes(), bits(host.v).tobytes(), host.image.tobytes(), host.f_prev.tobytes()) + _cell_state(host)
    log = host.log.copy()
    f, w, e = evaluation(rs, s["n"])
    if nan_energy:
        e[2] = np.nan
    host.advance()
    assert bits(host.x).tobytes() != before[0]
    host.finish(f, w, energy=e, total=total, capacity=5000)
    assert host.state.tolist() == [1, code, 1, 0], why
    after = (bits(host.x).tobytes(), bits(host.v).tobytes(), host.image.tobytes(), host.f_prev.tobytes()) + _cell_state(host)
    assert after == before and np.array_equal(bits(host.log), bits(log))
    assert np.array_equal(host.pos32, host.x.astype(np.float32))
    host.advance()                                                                    # halted: nothing moves any more
    host.finish(f, w, energy=np.zeros(4, dtype=np.float32), total=(10, 0), capacity=5000)
    after = (bits(host.x).tobytes(), bits(host.v).tobytes(), host.image.tobytes(), host.f_prev.tobytes()) + _cell_state(host)
    assert after == before and host.state.tolist() == [1, code, 1, 0]


def test_prime_and_parked_replays_do_not_scale():
    """Mode 1 takes the forces and nothing else; a parked state (the capture's warm-ups) leaves everything as it is."""
    s = synthetic()
    host = make(HostNPT, s, "isotropic")
    f, w, e = evaluation(np.random.RandomState(4), s["n"])
    x, v, cells, log = host.x.copy(), host.v.copy(), _cell_state(host), host.log.copy()
    host.state[3] = 1
    host.advance()
    host.finish(f, w, energy=e, total=(10, 0))
    assert host.state.tolist() == [0, 0, 0, 0] and np.array_equal(host.f_prev, f)
    assert np.array_equal(bits(host.x), bits(x)) and np.array_equal(bits(host.v), bits(v)) and _cell_state(host) == cells
    assert np.array_equal(bits(host.log), bits(log))
    host.state[1] = 1 << 20
    f2 = (2.0 * f).astype(np.float32)
    host.advance()
    host.finish(f2, w, energy=e, total=(10, 0))
    assert host.state.tolist() == [0, 1 << 20, 0, 0] and np.array_equal(host.f_prev, f)
    assert np.array_equal(bits(host.x), bits(x)) and np.array_equal(bits(host.v), bits(v)) and _cell_state(host) == cells
    assert np.array_equal(bits(host.log), bits(log))


def _one_graph(coupling, compressibility=3.0, max_strain=1e-2):
    """One graph of 5 atoms at rest, c = 1 (taup = dt, compressibility 3), target pressure 0."""
    rs = np.random.RandomState(8)
    x = rs.uniform(0.1, 0.9, (5, 3)) @ CELLS[0]
    return HostNPT(x, np.zeros((5, 3)), np.full(5, 30.0), DT, CELLS[:1], 0.0, compressibility, DT, coupling=coupling,
                   max_strain=max_strain)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_the_clamp_moves_the_cell_by_exactly_max_strain(sign):
    """A virial that asks for a 10 % change: every diagonal entry of mu is exactly 1 -+ max_strain, the cell and the
    coordinates are scaled by exactly that, and the event is counted."""
    host = _one_graph("isotropic")
    vol = abs(np.linalg.det(CELLS[0]))
    w = (np.eye(3) * (-sign * 0.1 * vol)).reshape(1, 9).astype(np.float32)             # P = -+0.1: c (P0 - P) = +-0.1
    host.advance()                                                                    # (at rest, f_prev 0: nothing moves)
    x, cell = host.x.copy(), host.cell64.copy()
    host.finish(np.zeros((5, 3), dtype=np.float32), w)
    s = 1.0 - sign * 1e-2
    assert host.state.tolist() == [1, 0, 0, 0] and host.clamped.tolist() == [1]
    assert np.array_equal(bits(host.mu), bits(np.diag([s, s, s]).reshape(1, 9)))
    assert np.array_equal(bits(host.cell64), bits(cell * s)) and np.array_equal(bits(host.x), bits(x * s))
    assert np.array_equal(host.cell, (cell * s).astype(np.float32))
    assert abs(host.log[0, 0, 3] + sign * 0.1) < 1e-6 and abs(host.log[0, 0, 4] / vol - 1) < 1e-12


@pytest.mark.parametrize("coupling", ["isotropic", "axes", "full"])
def test_a_nan_virial_with_a_finite_energy_gives_the_identity(coupling):
    host = _one_graph(coupling)
    w = np.zeros((1, 9), dtype=np.float32)
    w[0, 5] = np.nan
    host.advance()
    x, cells = host.x.copy(), _cell_state(host)
    host.finish(np.zeros((5, 3), dtype=np.float32), w, energy=np.array([-1.0], dtype=np.float32))
    assert host.state.tolist() == [1, 0, 0, 0] and host.clamped.tolist() == [1]
    assert np.array_equal(bits(host.mu), bits(np.eye(3).reshape(1, 9)))
    assert np.array_equal(bits(host.x), bits(x)) and _cell_state(host)[:3] == cells[:3]


@pytest.mark.parametrize("coupling", ["isotropic", "axes", "full"])
@pytest.mark.parametrize("friction", [None, 0.02], ids=["nve", "langevin"])
def test_zero_compressibility_equals_md_finish(coupling, friction):
    """compressibility 0: x, v and images bit-equal to hermnet_host_md_advance / _finish on the same inputs."""
    s = synthetic()
    npt = make(HostNPT, s, coupling, friction, compressibility=0.0)
    lang = {} if friction is None else dict(friction=friction, temperature=[300.0, 600.0, 900.0, 450.0], seed=(3 << 32) + 9)
    md = HostMD(s["x"], s["v"], s["m"], DT, cell=CELLS, batch=s["batch"], num_graphs=4, **lang)
    md.inv = npt.inv.copy()                                                          # the same inputs: one inverse
    rs = np.random.RandomState(23)
    cells = _cell_state(npt)[:3]
    for k in range(4):
        f, w, e = evaluation(rs, s["n"])
        assert np.array_equal(npt.advance(), md.advance())
        npt.finish(f, w, energy=e, total=(77, 0))
        md.finish(f, energy=e, total=(77, 0))
        assert np.array_equal(bits(npt.x), bits(md.x)) and np.array_equal(bits(npt.v), bits(md.v))
        assert np.array_equal(npt.image, md.image) and np.array_equal(npt.f_prev, md.f_prev)
        assert npt.state.tolist() == md.state.tolist() == [k + 1, 0, 0, 0]
        assert _cell_state(npt)[:3] == cells
        assert np.array_equal(npt.log[k][:, [0, 2]], md.log[k][:, [0, 2]])
        assert np.all(np.abs(npt.log[k][:, 1] - md.log[k][:, 1]) <= s["n"] * 2.0 ** -52 * np.abs(md.log[k][:, 1]))
    assert np.abs(npt.image).max() >= 1 and not npt.clamped.any()


def test_argument_checks_need_no_gpu():
    """HN_ERR_BAD_ARG (1) from both entry points: null pointers, an unknown coupling, max_strain <= 0, log_steps < 1."""
    lib = _lib.load()
    assert {"hermnet_md_finish_npt", "hermnet_host_md_finish_npt"} <= set(_lib.SIGNATURES)
    host = _one_graph("isotropic")
    f, e = np.zeros((5, 3), dtype=np.float32), np.zeros(1, dtype=np.float32)
    w, tot = np.zeros((1, 9), dtype=np.float32), np.zeros(2, dtype=np.int64)
    from md_reference import _p

    def call(fn, tail, coupling=0, mask=7, max_strain=1e-2, log_steps=64, drop=()):
        h = host
        ptrs = dict(graph_ptr=h.graph_ptr, batch=h.batch, f=f, e=e, w=w, tot=tot, p0=h.p0, c=h.c, x=h.x, v=h.v, x0=h.x0, v0=h.v0,
                    image=h.image, image0=h.image0, f_prev=h.f_prev, kick=h.kick, half_mass=h.half_mass, pos32=h.pos32,
                    ke_atom=h.ke_atom, cell64=h.cell64, cell32=h.cell, inv=h.inv, mu=h.mu, clamped=h.clamped, log=h.log,
                    state=h.state)
        q = {k: (None if k in drop else _p(a)) for k, a in ptrs.items()}
        return fn(5, 1, q["graph_ptr"], q["batch"], q["f"], q["e"], q["w"], q["tot"], 100, coupling, mask, max_strain, q["p0"],
                  q["c"], q["x"], q["v"], q["x0"], q["v0"], q["image"], q["image0"], q["f_prev"], q["kick"], q["half_mass"],
                  q["pos32"], q["ke_atom"], q["cell64"], q["cell32"], q["inv"], q["mu"], q["clamped"], q["log"], log_steps,
                  q["state"], *tail)

    host.state[1] = 1 << 20                                                          # parked: a served call changes nothing
    assert call(lib.hermnet_host_md_finish_npt, ()) == 0
    # (the device entry point is only called with arguments it refuses: nothing is launched)
    for fn, tail in ((lib.hermnet_host_md_finish_npt, ()), (lib.hermnet_md_finish_npt, (None,))):
        for name in ("w", "p0", "c", "cell64", "cell32", "inv", "mu", "clamped", "state", "log", "e", "tot", "graph_ptr", "x"):
            assert call(fn, tail, drop=(name,)) == 1, name
        assert call(fn, tail, coupling=3) == 1 and call(fn, tail, coupling=-1) == 1
        assert call(fn, tail, max_strain=0.0) == 1 and call(fn, tail, max_strain=-1e-2) == 1
        assert call(fn, tail, max_strain=float("nan")) == 1
        assert call(fn, tail, log_steps=0) == 1 and call(fn, tail, mask=8) == 1
