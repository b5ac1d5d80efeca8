"""CPU: the finish skeleton the four MD drivers share (hermnet_amd/csrc/md_finish.h: md_host_finish), through each driver's
host twin -- hermnet_host_md_finish, _md_finish_npt, _remd_finish and _pimd_finish -- on 2 graphs x 3 atoms, the smallest
shape all four accept (REMD: 2 replicas or more; PIMD: beads of equal size).  What is each driver's own (barostat, exchange,
ring) has its own tests; here: a halted state changes nothing, a prime takes the forces alone, a void step goes back to where
it began and records its halt, a committed step is counted and writes one log row per graph."""
import numpy as np
import pytest

from md_reference import HostMD, bits
from npt_reference import HostNPT
from pimd_reference import HostPIMD
from remd_reference import HostREMD

B, N_REP, LOG_STEPS, DT = 2, 3, 4, 0.5
N = B * N_REP
CELL = np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]])
DRIVERS = ["md", "npt", "remd", "pimd"]


def _host(driver, rs):
    """The driver's host twin on 2 graphs x 3 atoms in one triclinic cell, and its finish as f(forces, energy, total,
    capacity)."""
    m = np.tile(rs.uniform(10.0, 60.0, N_REP), B)
    x, v = rs.uniform(0.0, 1.0, (N, 3)) @ CELL, rs.normal(scale=0.02, size=(N, 3))
    batch, cells = np.repeat(np.arange(B), N_REP), np.tile(CELL, (B, 1, 1))
    if driver == "md":
        h = HostMD(x, v, m, DT, cell=cells, batch=batch, friction=0.02, temperature=300.0, seed=7, log_steps=LOG_STEPS)
    elif driver == "npt":
        h = HostNPT(x, v, m, DT, cells, 0.01, 0.5, 100.0, coupling="full", log_steps=LOG_STEPS, batch=batch, seed=7)
    elif driver == "remd":
        h = HostREMD(x, v, m, DT, [300.0, 330.0], 0.02, 1, seed=7, log_steps=LOG_STEPS, cell=cells)
    else:
        h = HostPIMD(B, x, v, m, DT, 300.0, seed=7, log_steps=LOG_STEPS, cell=CELL)
    h.f_prev[:] = rs.normal(size=(N, 3)).astype(np.float32)
    if driver != "npt":
        return h, h.finish
    virial = rs.normal(size=(B, 9)).astype(np.float32)
    return h, lambda f, e, **kw: h.finish(f, virial, e, **kw)


def _arrays(h):
    return {k: a.copy() for k, a in vars(h).items() if isinstance(a, np.ndarray)}


def _evaluation(rs):
    return rs.normal(size=(N, 3)).astype(np.float32), rs.normal(size=B).astype(np.float32)


def _started(driver):
    """The twin behind one committed step (step = 1, every array in use), its finish and the generator."""
    rs = np.random.RandomState(DRIVERS.index(driver))
    h, finish = _host(driver, rs)
    f, e = _evaluation(rs)
    h.advance()
    finish(f, e, total=(500, 0), capacity=1000)
    assert h.state.tolist() == [1, 0, 0, 0]
    return h, finish, rs


@pytest.mark.parametrize("driver", DRIVERS)
def test_a_halted_state_changes_no_byte(driver):
    h, finish, rs = _started(driver)
    h.state[1:3] = (4, 1)
    before = _arrays(h)
    f, e = _evaluation(rs)
    h.advance()
    finish(f, e, total=(500, 0), capacity=1000)
    after = _arrays(h)
    assert sorted(after) == sorted(before)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k


@pytest.mark.parametrize("driver", DRIVERS)
def test_a_prime_takes_the_forces_and_clears_its_mode(driver):
    h, finish, rs = _started(driver)
    h.state[3] = 1
    before = _arrays(h)
    f, e = _evaluation(rs)
    h.advance()
    finish(f, e, total=(500, 0), capacity=1000)
    assert np.array_equal(h.f_prev, f)
    assert h.state.tolist() == [1, 0, 0, 0]                           # the mode is cleared, the step is not counted
    for k in ("x", "v", "image", "log"):
        assert before[k].tobytes() == getattr(h, k).tobytes(), k


@pytest.mark.parametrize("what", ["capacity", "nonfinite"])
@pytest.mark.parametrize("driver", DRIVERS)
def test_a_void_step_goes_back_to_where_it_began(driver, what):
    h, finish, rs = _started(driver)
    before = _arrays(h)
    f, e = _evaluation(rs)
    total = (1001, 0) if what == "capacity" else (500, 0)
    if what == "nonfinite":
        e[B - 1] = np.nan
    h.advance()
    assert not np.array_equal(h.x, before["x"])                       # the step had moved the atoms ...
    finish(f, e, total=total, capacity=1000)
    for k in ("x", "v", "image"):                                     # ... and they are back, from the step's own backup
        assert np.array_equal(before[k], getattr(h, k + "0")), k
        assert getattr(h, k).tobytes() == getattr(h, k + "0").tobytes(), k
    assert np.array_equal(h.pos32, h.x0.astype(np.float32))
    assert h.state.tolist() == [1, 4 if what == "capacity" else 256, 1, 0]
    assert before["log"].tobytes() == h.log.tobytes()
    assert np.array_equal(h.f_prev, before["f_prev"])


@pytest.mark.parametrize("driver", DRIVERS)
def test_a_committed_step_is_counted_and_writes_one_row_per_graph(driver):
    h, finish, rs = _started(driver)
    before = _arrays(h)
    f, e = _evaluation(rs)
    h.advance()
    finish(f, e, total=(500, 0), capacity=1000)
    assert h.state.tolist() == [2, 0, 0, 0]
    assert np.array_equal(h.f_prev, f)
    changed = np.any(bits(h.log) != bits(before["log"]), axis=2)     # [rows, B]
    want = np.zeros((LOG_STEPS, B), dtype=bool)
    want[1 % LOG_STEPS] = True                                        # the row of step 1, for every graph
    assert np.array_equal(changed, want)
    assert np.array_equal(h.log[1, :, 0], e.astype(np.float64)) and np.all(h.log[1, :, 2] == 500.0)
