"""CPU: the Nose-Hoover chain step (hermnet_amd/csrc/nhc_step.h) through the library's host twins hermnet_host_nhc_advance /
_finish -- against the numpy transcription bit for bit, against the NVE twins with the thermostat off, the conserved extended
energy and its order in dt, the canonical distribution of the kinetic energy, a void step, the refusals."""
import math
import types

import numpy as np
import pytest

from hermnet_amd import _lib
from hermnet_amd.nhc import DeviceNHC, chain_tables, conserved, default_dof, suzuki_yoshida
from md_reference import KB, HostMD, _p, bits
from nhc_reference import HostNHC, NumpyNHC, Wells, run_wells, tables, weights
from remd_reference import canonical_sum

FIELDS = ("x", "v", "image", "f_prev", "pos32", "xi", "v_xi", "scale", "log", "state")


def _same(a, b, what):
    for k in FIELDS:
        p, q = getattr(a, k), getattr(b, k)
        if p.dtype == np.float64:
            assert np.array_equal(bits(p), bits(q)), (what, k)
        else:
            assert np.array_equal(p, q), (what, k)


def _potential(n, batch, B):
    """A synthetic float32 potential: E_g = sum_i a_i (sin x_i + sin y_i + sin z_i) over graph g, f_i = -a_i cos(.)."""
    a = (0.05 + 0.01 * (np.arange(n) % 7)).astype(np.float32)

    def evaluate(pos32):
        per_atom = a * np.sin(pos32).sum(axis=1, dtype=np.float32)
        e = np.array([per_atom[batch == g].sum(dtype=np.float32) for g in range(B)], dtype=np.float32)
        return (-a[:, None] * np.cos(pos32)).astype(np.float32), e
    return evaluate


def _unequal_batch():
    """Graphs of 1, 7 and 300 atoms (the last crosses the 256-lane tile of the canonical sum) in triclinic and orthogonal
    cells, an atom of infinite mass in the graph of 7; per-graph temperatures, time constants and degrees of freedom."""
    rs = np.random.RandomState(3)
    counts = [1, 7, 300]
    batch = np.repeat(np.arange(3), counts)
    n = len(batch)
    m = rs.uniform(12.0, 60.0, n)
    m[4] = np.inf
    cell = np.stack([np.diag([8.0, 9.0, 10.0]), np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]]),
                     np.diag([22.0, 21.0, 20.5])])
    x = np.einsum("nk,nkj->nj", rs.uniform(-0.5, 1.5, (n, 3)), cell[batch])
    v = rs.normal(scale=0.003, size=(n, 3))
    v[4] = 0.0
    return dict(x=x, v=v, m=m, batch=batch, cell=cell, temperature=[300.0, 500.0, 800.0], tau=[20.0, 50.0, 35.0],
                dof=[3.0, 18.0, 897.0])


@pytest.mark.parametrize("chain,order,substeps", [(1, 1, 1), (3, 3, 2), (8, 5, 1)])
def test_host_twin_equals_the_numpy_transcription_bit_for_bit(chain, order, substeps):
    """200 steps behind the prime of the unequal batch, energies and forces from the synthetic potential at the float32
    coordinates each advance hands out: state, x, image, v, f_prev, pos32, the chains, both factors and the log are bit-equal
    after every replay.  The chains are active (factors that differ from 1, thermostat velocities of both signs)."""
    s = _unequal_batch()
    kw = dict(chain=chain, order=order, substeps=substeps, cell=s["cell"], batch=s["batch"], log_steps=16, num_graphs=3)
    host, ref = (cls(s["x"], s["v"], s["m"], 0.5, s["temperature"], s["tau"], s["dof"], **kw) for cls in (HostNHC, NumpyNHC))
    evaluate = _potential(len(s["x"]), s["batch"], 3)
    for p in (host, ref):
        p.state[3] = 1
    low = high = 0
    for replay in range(201):
        pos_h, pos_r = host.advance(), ref.advance()
        assert np.array_equal(pos_h, pos_r), replay
        f, e = evaluate(pos_r)
        host.finish(f, e, total=(100 + replay, 0))
        ref.finish(f, e, total=(100 + replay, 0))
        _same(host.snapshot(), ref.snapshot(), replay)
        low, high = low + int((host.scale < 1.0).sum()), high + int((host.scale > 1.0).sum())
    assert host.state.tolist() == [200, 0, 0, 0]
    assert low >= 50 and high >= 50, (low, high)
    assert (host.v_xi != 0.0).all() and (host.xi != 0.0).all() and not host.v[4].any()
    assert (host.xi0 != -7.0).all() and host.log[(200 - 1) % 16, :, 2].tolist() == [300.0] * 3


def test_tables_of_the_driver_equal_the_reference():
    """`chain_tables`, `suzuki_yoshida` and `default_dof` of hermnet_amd/nhc.py against the reference's plain loops, bit for
    bit; the weights of an order add up to 1; tau = inf gives q = 1 / q = 0."""
    t, tau, dof = np.array([300.0, 650.0, 12.5]), np.array([100.0, np.inf, 7.25]), np.array([21.0, 3.0, 594.0])
    for chain, order, substeps in ((1, 1, 1), (3, 3, 2), (8, 5, 3)):
        got, want = chain_tables(t, tau, dof, 0.7, chain, order, substeps), tables(t, tau, dof, 0.7, chain, order, substeps)
        for a, b in zip(got, want):
            assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(bits(a), bits(b))
        assert np.array_equal(suzuki_yoshida(order), np.array(weights(order))) and abs(sum(weights(order)) - 1.0) < 1e-15
        assert not got[3][1].any() and not got[4][1].any() and got[3][0, 0] == (21.0 * (KB * 300.0)) * (100.0 * 100.0)
    m = np.array([1.0, 2.0, np.inf, 4.0, 5.0, 6.0, 7.0])
    batch = np.array([0, 0, 0, 1, 1, 1, 1])
    assert default_dof(m, batch, 2, True).tolist() == [6.0, 9.0] and default_dof(m, batch, 2, False).tolist() == [6.0, 12.0]


def test_tau_inf_is_the_nve_twin_bit_for_bit():
    """The unequal batch with every thermostat off against hermnet_host_md_advance / _finish (NVE) over 100 steps: x, v,
    image, f_prev, pos32 and the log's columns 0 and 2 are bit-equal after every step, xi = v_xi = 0 and both factors are 1.0
    throughout.  Column 1: hermnet_host_md_finish adds a graph's kinetic energies sequentially (frozen with ABI v13) where the
    device -- and this driver's twin -- take the canonical order, so that column equals the canonical sum of the NVE twin's
    own per-atom kinetic energies bit for bit, and the NVE twin's log itself for the graph of one atom."""
    s = _unequal_batch()
    nhc = HostNHC(s["x"], s["v"], s["m"], 0.5, s["temperature"], np.inf, s["dof"], chain=3, order=3, substeps=2, cell=s["cell"],
                  batch=s["batch"], log_steps=16, num_graphs=3)
    nve = HostMD(s["x"], s["v"], s["m"], 0.5, cell=s["cell"], batch=s["batch"], log_steps=16, num_graphs=3)
    evaluate = _potential(len(s["x"]), s["batch"], 3)
    for p in (nhc, nve):
        p.state[3] = 1
    for replay in range(101):
        pos = nhc.advance()
        assert np.array_equal(pos, nve.advance()), replay
        f, e = evaluate(pos)
        nhc.finish(f, e, total=(7 * replay, 0))
        nve.finish(f, e, total=(7 * replay, 0))
        for k in ("x", "v"):
            assert np.array_equal(bits(getattr(nhc, k)), bits(getattr(nve, k))), (replay, k)
        for k in ("image", "f_prev", "pos32", "state"):
            assert np.array_equal(getattr(nhc, k), getattr(nve, k)), (replay, k)
        assert not nhc.xi.any() and not nhc.v_xi.any() and (nhc.scale == 1.0).all()
        if replay:
            row, old = nhc.log[(replay - 1) % 16], nve.log[(replay - 1) % 16]
            assert np.array_equal(bits(row[:, [0, 2]]), bits(old[:, [0, 2]])) and not row[:, 3].any()
            want = [canonical_sum(nve.ke_atom[nve.graph_ptr[g]:nve.graph_ptr[g + 1]]) for g in range(3)]
            assert np.array_equal(bits(row[:, 1]), bits(np.array(want))) and bits(row[0, 1]) == bits(old[0, 1])
            assert np.allclose(row[:, 1], old[:, 1], rtol=1e-13, atol=0.0)
    assert nhc.state.tolist() == [100, 0, 0, 0] and nhc.image.any()


def _deviation(wells, x, v, dt, tau, time=4000.0):
    """max |E - E_0| of the extended energy over `time` fs of the host twins in the wells."""
    steps = int(round(time / dt))
    host = HostNHC(x, v, wells.masses, dt, 300.0, tau, 3.0 * wells.n, log_steps=steps)
    e = conserved(types.SimpleNamespace(log=run_wells(host, wells, steps)[:, None, :]))[:, 0]
    return float(np.abs(e - e[0]).max())


def test_the_extended_energy_is_conserved_to_second_order():
    """16 atoms of unequal masses in anisotropic quartic wells with harmonic springs between ring neighbours
    (nhc_reference.Wells), 300 K, tau = 50 fs, M = 3, order 3, 4000 fs from Maxwell-Boltzmann velocities.  The yardstick is the
    same twins with the thermostat off (tau = inf) on the same system, start and dt: max |E - E_0| of E_pot + E_kin.  The
    chain adds splitting-error terms of the same order and nothing larger, so `conserved()` must stay within 3 x that figure;
    and halving dt must cut its deviation by a factor between 3 and 5 (second order: 4 asymptotically).

    Seen (HostNHC; NumpyNHC is bit-identical, the first test):
        dt    NVE yardstick   NHC deviation   ratio
        4.0   1.381e-2 eV     1.264e-2 eV     0.91
        2.0   3.324e-3        3.033e-3        0.91     / dt 4.0: 4.17
        1.0   8.262e-4        7.569e-4        0.92     / dt 2.0: 4.01
        0.5   2.064e-4        1.886e-4        0.91     / dt 1.0: 4.01
    so dt = 2.0 and 1.0 fs (asserted) are inside the asymptotic regime; the float32 energy's rounding (3e-8 eV) is far below."""
    wells = Wells()
    x, v = wells.start(300.0, 1)
    seen = {}
    for dt in (2.0, 1.0):
        yardstick, nhc = _deviation(wells, x, v, dt, np.inf), _deviation(wells, x, v, dt, 50.0)
        print("dt %.1f: NVE max|E - E0| = %.4e eV, NHC max|E' - E'0| = %.4e eV, ratio %.3f" % (dt, yardstick, nhc, nhc / yardstick))
        assert nhc <= 3.0 * yardstick, (dt, nhc, yardstick)
        seen[dt] = nhc
    factor = seen[2.0] / seen[1.0]
    print("halving dt: factor %.3f" % factor)
    assert 3.0 <= factor <= 5.0, factor


def test_the_kinetic_energy_is_canonically_distributed():
    """The wells at 300 K, tau = 50 fs, M = 3, order 3, dt = 2 fs, dof = 48: 42,000 steps per seed (initial velocities), the
    first 2,000 dropped, 20 blocks of 2,000.  On each of 4 seeds <E_kin> = dof kB T / 2 and Var(E_kin) / <E_kin>^2 = 2 / dof
    within 5 blocked standard errors.

    Seen (HostNHC = NumpyNHC bit for bit), in standard errors: mean -0.46, +0.65, +0.02, -0.56; variance -0.76, +1.15, +0.14,
    +0.35.  (With ISOTROPIC wells the variance came out +3 to +6 standard errors wide: see nhc_reference.Wells.)"""
    wells = Wells()
    temperature, dof, steps, drop, blocks = 300.0, 48.0, 42000, 2000, 20
    for seed in range(4):
        x, v = wells.start(temperature, 100 + seed)
        host = HostNHC(x, v, wells.masses, 2.0, temperature, 50.0, dof, log_steps=steps)
        ke = run_wells(host, wells, steps)[drop:, 1].reshape(blocks, -1)
        mean, want = ke.mean(), 0.5 * dof * KB * temperature
        mean_err = ke.mean(axis=1).std(ddof=1) / math.sqrt(blocks)
        rel = ((ke - mean) ** 2).mean(axis=1) / mean ** 2
        var, var_err = rel.mean(), rel.std(ddof=1) / math.sqrt(blocks)
        print("seed %d: <E_kin> = %.5f +- %.5f eV (want %.5f: %+.2f sigma); Var/<>^2 = %.5f +- %.5f (want %.5f: %+.2f sigma)"
              % (seed, mean, mean_err, want, (mean - want) / mean_err, var, var_err, 2.0 / dof, (var - 2.0 / dof) / var_err))
        assert abs(mean - want) <= 5.0 * mean_err, (seed, mean, mean_err, want)
        assert abs(var - 2.0 / dof) <= 5.0 * var_err, (seed, var, var_err, 2.0 / dof)


def test_a_step_fed_a_nan_energy_is_void_and_the_chain_returns_with_the_atoms():
    """x, v, image, pos32, xi and v_xi are those of the step's start bit for bit, f_prev and the log are untouched, `state`
    records the halt with the non-finite bit, and later calls change nothing; after the halt is cleared and the prime, the
    run equals one that never saw the NaN."""
    s = _unequal_batch()
    make = lambda: HostNHC(s["x"], s["v"], s["m"], 0.5, s["temperature"], s["tau"], s["dof"], cell=s["cell"], batch=s["batch"],
                           log_steps=16, num_graphs=3)
    host, twin = make(), make()
    evaluate = _potential(len(s["x"]), s["batch"], 3)
    for p in (host, twin):
        p.state[3] = 1
        for replay in range(6):
            f, e = evaluate(p.advance())
            p.finish(f, e)
    before = host.snapshot()
    moved = host.advance().copy()
    assert not np.array_equal(host.xi, before.xi) and not np.array_equal(host.v, before.v)
    assert np.array_equal(bits(host.xi0), bits(before.xi)) and np.array_equal(bits(host.v0), bits(before.v))
    f, e = evaluate(moved)
    bad = e.copy()
    bad[1] = np.nan
    host.finish(f, bad)
    after = host.snapshot()
    assert after.state.tolist() == [5, 256, 5, 0]
    for k in ("x", "v", "image", "f_prev", "pos32", "xi", "v_xi", "log"):
        assert getattr(after, k).tobytes() == getattr(before, k).tobytes(), k
    host.finish(f, e)                                     # halted: nothing
    assert np.array_equal(host.advance(), before.pos32)
    halted = host.snapshot()
    for k in FIELDS:
        assert getattr(halted, k).tobytes() == getattr(after, k).tobytes(), k
    host.state[1:3] = 0                                   # resume: the halt cleared, the prime, then the same step
    host.state[3] = 1
    f0, e0 = evaluate(host.advance())
    host.finish(f0, e0)
    assert host.xi.tobytes() == before.xi.tobytes() and host.v_xi.tobytes() == before.v_xi.tobytes()
    for p in (host, twin):
        for replay in range(3):
            f, e = evaluate(p.advance())
            p.finish(f, e)
    _same(host.snapshot(), twin.snapshot(), "resumed")
    assert host.state.tolist() == [8, 0, 0, 0]


def test_refusals_name_their_reason_without_a_gpu():
    z, x = np.full(5, 14), np.arange(15, dtype=np.float64).reshape(5, 3)
    make = lambda **kw: DeviceNHC(None, z, np.eye(3) * 20.0, x, np.full(5, 28.0), 1.0, **dict(dict(temperature=300.0), **kw))
    with pytest.raises(ValueError, match="friction= is Langevin's"):
        make(friction=0.01)
    for bad in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="chain .* in 1..8"):
            make(chain=bad)
    for bad in (0, 2, 4, 7):
        with pytest.raises(ValueError, match="order .* one of 1, 3, 5"):
            make(order=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="substeps"):
            make(substeps=bad)
    for bad in (None, 0.0, -5.0, np.inf, np.nan, [300.0, 0.0]):
        with pytest.raises(ValueError, match="temperature .* positive and finite"):
            make(temperature=bad)
    for bad in (0.0, -1.0, np.nan, [50.0, -50.0]):
        with pytest.raises(ValueError, match="tau .* > 0"):
            make(tau=bad)
    with pytest.raises(ValueError, match="graph 0 has dof = 0 <= 0: a thermostat needs a degree of freedom"):
        DeviceNHC(None, z[:1], np.eye(3) * 20.0, x[:1], np.full(1, 28.0), 1.0, temperature=300.0)
    with pytest.raises(ValueError, match="graph 1 has dof = -3 <= 0"):
        make(batch=np.array([0, 0, 0, 1, 1]), num_graphs=2, dof=[6.0, -3.0])
    with pytest.raises(ValueError, match="graph 1 has dof = 0 <= 0"):        # both atoms of graph 1 are fixed
        DeviceNHC(None, z, None, x, np.array([28.0, 28.0, 28.0, np.inf, np.inf]), 1.0, temperature=300.0,
                  batch=np.array([0, 0, 0, 1, 1]), num_graphs=2)


def test_malformed_calls_are_refused_by_the_argument_checks():
    """HN_ERR_BAD_ARG from the host twins for what the header lists; the device entry points refuse the same before
    anything is launched, so with no GPU."""
    bad_arg = _lib.HN_ERR_BAD_ARG
    x = np.arange(15, dtype=np.float64).reshape(5, 3)
    zero_f = np.zeros((5, 3), dtype=np.float32)

    def fresh():
        return HostNHC(x, np.zeros((5, 3)), np.full(5, 28.0), 1.0, 300.0, 50.0, 15.0)

    host = fresh()
    host.advance()
    host.finish(zero_f)
    assert host.state.tolist() == [1, 0, 0, 0]
    for name, value in (("chain", 0), ("chain", 9), ("order", 2), ("order", 7), ("substeps", 0), ("flags", 1)):
        host = fresh()
        setattr(host, name, value)
        host.advance(expect=bad_arg)
        if name != "flags":
            host.finish(zero_f, expect=bad_arg)
    for name in ("delta", "kt", "dof_kt", "q", "inv_q", "xi", "v_xi", "xi0", "v_xi0", "scale"):
        host = fresh()
        setattr(host, name, None)
        host.advance(expect=bad_arg)
        host.finish(zero_f, expect=bad_arg)
        assert host.state.tolist() == [0, 0, 0, 0] and np.array_equal(host.x, x)
    for name in ("half_mass", "graph_ptr"):
        host = fresh()
        setattr(host, name, None)
        host.advance(expect=bad_arg)
    lib, h = _lib.load(), fresh()
    h.chain = 9
    rc = lib.hermnet_nhc_advance(5, 1, 0, 1.0, _p(h.x), _p(h.v), _p(h.x0), _p(h.v0), _p(h.image), _p(h.image0), _p(h.f_prev),
                                 _p(h.kick), None, None, None, _p(h.pos32), _p(h.state), _p(h.graph_ptr), _p(h.half_mass),
                                 *h._chains(), None)
    assert rc == bad_arg
    e, tot = np.zeros(1, dtype=np.float32), np.zeros(2, dtype=np.int64)
    rc = lib.hermnet_nhc_finish(5, 1, _p(h.graph_ptr), None, _p(zero_f), _p(e), _p(tot), 100, *h._finish_atoms(), *h._chains(),
                                _p(h.log), 64, _p(h.state), None)
    assert rc == bad_arg
