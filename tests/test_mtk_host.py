"""CPU: the MTK barostat step (hermnet_amd/csrc/mtk_step.h) through the library's host twins hermnet_host_mtk_advance /
_finish -- against the numpy transcription bit for bit, against the chain twins with the barostat off and the NVE twins with
everything off, the conserved extended energy and its order in dt, time reversal, the isothermal-isobaric averages, the void
steps, the refusals."""
import math

import numpy as np
import pytest

from hermnet_amd import _lib
from hermnet_amd import mtk as mtk_module
from hermnet_amd.mtk import DeviceMTK
from md_reference import KB, HostMD, _p, bits
from mtk_reference import AXES, ISOTROPIC, STATE_FIELDS, HostMTK, NumpyMTK, Pairs, baro_tables, conserved_log, run_pairs
from nhc_reference import HostNHC
from remd_reference import canonical_sum

CONFIGS = [(1, 1, 1), (3, 3, 2), (8, 5, 1)]
COUPLINGS = [("isotropic", (1, 1, 1)), ("axes", (1, 0, 1))]


def _same(a, b, what, fields=STATE_FIELDS):
    for k in fields:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)


def _unequal_batch():
    """Graphs of 1, 7 and 300 atoms (the last crosses the 256-lane tile of the canonical sums) in triclinic cells, an atom of
    infinite mass in the graph of 7; per-graph temperatures, pressures, time constants and degrees of freedom."""
    rs = np.random.RandomState(3)
    counts = [1, 7, 300]
    batch = np.repeat(np.arange(3), counts)
    n = len(batch)
    m = rs.uniform(12.0, 60.0, n)
    m[4] = np.inf
    cell = np.stack([np.array([[8.0, 0.3, 0.0], [-0.4, 9.0, 0.2], [0.1, 0.5, 10.0]]),
                     np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]]),
                     np.array([[22.0, 0.0, 1.0], [0.5, 21.0, 0.0], [0.0, -2.0, 20.5]])])
    x = np.einsum("nk,nkj->nj", rs.uniform(-0.5, 1.5, (n, 3)), cell[batch])
    v = rs.normal(scale=0.003, size=(n, 3))
    v[4] = 0.0
    volume = np.abs(np.linalg.det(cell))
    return dict(x=x, v=v, m=m, batch=batch, cell=cell, temperature=[300.0, 500.0, 800.0], tau=[20.0, 50.0, 35.0],
                taup=[60.0, 90.0, 120.0], dof=[3.0, 18.0, 897.0], volume=volume,
                pressure=(np.array([0.4, 2.0, 60.0]) / (3.0 * volume)).tolist())


def _potential(n, batch, B, scale=(0.4, 2.0, 60.0)):
    """A synthetic float32 evaluation: E_g = sum_i a_i (sin x_i + sin y_i + sin z_i) over graph g, f_i = -a_i cos(.), and a
    virial W_g = scale_g (I / 3 + a small asymmetric part that follows the coordinates): tr W_g = scale_g (1 + ...) balances
    the target pressures of `_unequal_batch` near the starting volumes, so the cells oscillate instead of running away."""
    a = (0.05 + 0.01 * (np.arange(n) % 7)).astype(np.float32)
    shape = np.array([[1.0, 0.3, -0.2], [0.1, 0.8, 0.4], [-0.3, 0.2, 1.2]])

    def evaluate(pos32):
        per_atom = a * np.sin(pos32).sum(axis=1, dtype=np.float32)
        e = np.array([per_atom[batch == g].sum(dtype=np.float32) for g in range(B)], dtype=np.float32)
        w = np.stack([scale[g] * (np.eye(3) / 3.0 + 0.05 * shape * np.cos(pos32[batch == g].astype(np.float64)).mean())
                      for g in range(B)])
        return (-a[:, None] * np.cos(pos32)).astype(np.float32), e, w.astype(np.float32).reshape(B, 9)
    return evaluate


def _drivers(s, classes, dt=0.5, **kw):
    kw = dict(dict(cell=s["cell"], pressure=s["pressure"], taup=s["taup"], batch=s["batch"], log_steps=16, num_graphs=3,
                   max_strain=0.05), **kw)
    tau = kw.pop("tau", s["tau"])
    return [cls(s["x"], s["v"], s["m"], dt, s["temperature"], tau, s["dof"], **kw) for cls in classes]


@pytest.mark.parametrize("coupling,mask", COUPLINGS)
@pytest.mark.parametrize("chain,order,substeps", CONFIGS)
def test_host_twin_equals_the_numpy_transcription_bit_for_bit(chain, order, substeps, coupling, mask):
    """200 steps behind the prime of the unequal batch with a synthetic evaluation (energies, forces, virial) at the float32
    coordinates each advance hands out: every array of the state -- atoms, both chains, barostat, the three forms of the cell,
    factors, backup, log -- is bit-equal after every replay.  The barostats are active: the cells move, every kind of factor
    differs from 1 on both sides, and under "axes" the masked axis never moves."""
    s = _unequal_batch()
    host, ref = _drivers(s, (HostMTK, NumpyMTK), chain=chain, order=order, substeps=substeps, coupling=coupling, mask=mask)
    evaluate = _potential(len(s["x"]), s["batch"], 3)
    for p in (host, ref):
        p.state[3] = 1
    low, high = np.zeros(12, dtype=np.int64), np.zeros(12, dtype=np.int64)
    for replay in range(201):
        pos_h, pos_r = host.advance(), ref.advance()
        assert np.array_equal(pos_h, pos_r), replay
        f, e, w = evaluate(pos_r)
        host.finish(f, e, w, total=(100 + replay, 0))
        ref.finish(f, e, w, total=(100 + replay, 0))
        _same(host.snapshot(), ref.snapshot(), replay)
        low, high = low + (host.factors < 1.0).sum(axis=0), high + (host.factors > 1.0).sum(axis=0)
    assert host.state.tolist() == [200, 0, 0, 0] and not host.flag.any() and not host.refused.any()
    moving = [k for k in range(12) if coupling == "isotropic" or mask[k % 3]]
    assert ((low + high)[moving] >= 300).all() and low[6:9].sum() >= 20 and high[6:9].sum() >= 20, (low, high)
    assert (low[:3] >= 20).all() and (high[:3] >= 20).all(), (low, high)
    assert (host.v_xi_b != 0.0).all() and (host.xi_b != 0.0).all() and (host.v_xi != 0.0).all() and not host.v[4].any()
    change = host.volume() / s["volume"] - 1.0
    assert (np.abs(change) > 1e-4).all(), change
    if coupling == "axes":
        assert not host.v_cell[:, 1].any() and (host.factors[:, [7, 10]] == 1.0).all()
        assert np.array_equal(host.cell64.reshape(3, 3, 3)[:, :, 1], s["cell"][:, :, 1])
    else:
        assert (host.v_cell[:, 0] == host.v_cell[:, 1]).all() and (host.v_cell[:, 0] == host.v_cell[:, 2]).all()
    assert np.array_equal(host.cell32, host.cell64.astype(np.float32)) and host.image.any()
    assert host.log[(200 - 1) % 16, :, 2].tolist() == [300.0] * 3
    assert np.array_equal(bits(host.log[(200 - 1) % 16, :, 5]), bits(host.volume()))


def test_tables_of_the_driver_equal_the_reference():
    """`baro_tables` of hermnet_amd/mtk.py against the reference's plain loops, bit for bit; taup = inf gives w = 1 / w = 0 and
    a barostat chain that is off, tau = inf switches that chain off and leaves w."""
    t, dof, p = np.array([300.0, 650.0, 12.5, 77.0]), np.array([21.0, 3.0, 594.0, 93.0]), np.array([0.0, 1e-3, -2e-4, 0.5])
    tau, taup = np.array([100.0, 40.0, np.inf, 7.25]), np.array([1000.0, np.inf, 333.0, 90.0])
    for name, code, mask in (("isotropic", ISOTROPIC, 7), ("axes", AXES, 5), ("axes", AXES, 2)):
        for chain in (1, 3, 8):
            got, want = mtk_module.baro_tables(t, tau, taup, dof, p, name, mask, chain), baro_tables(t, tau, taup, dof, p, code,
                                                                                                    mask, chain)
            for a, b in zip(got, want):
                assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(bits(a), bits(b)), (name, mask, chain)
            par, _, q, inv_q = got
            assert not par[1, :2].any() and not q[1].any() and not inv_q[1].any()
            assert par[2, 0] > 0.0 and not q[2].any() and not inv_q[2].any() and q[0].all() and q[3].all()
    w = mtk_module.baro_tables(t, tau, taup, dof, p, "isotropic", 7, 3)[0][0, 0]
    assert w == (21.0 + 3.0) * (KB * 300.0) * (1000.0 * 1000.0)


def test_taup_inf_is_the_chain_twin_bit_for_bit():
    """The unequal batch with every barostat off (taup = inf) against hermnet_host_nhc_advance / _finish over 100 steps: x, v,
    image, f_prev, pos32, both factors, the chain and the log's first four columns are bit-equal after every step; v_cell
    stays 0, all twelve factors are exactly 1.0 and the three forms of the cell are never written (the inverse stays the one
    the wrapper made with numpy, which the adjugate form would not reproduce bit for bit)."""
    s = _unequal_batch()
    mtk, = _drivers(s, (HostMTK,), taup=np.inf, chain=3, order=3, substeps=2)
    nhc = HostNHC(s["x"], s["v"], s["m"], 0.5, s["temperature"], s["tau"], s["dof"], chain=3, order=3, substeps=2, cell=s["cell"],
                  batch=s["batch"], log_steps=16, num_graphs=3)
    cells = (mtk.cell64.copy(), mtk.cell32.copy(), mtk.inv_cell.copy())
    evaluate = _potential(len(s["x"]), s["batch"], 3)
    for p in (mtk, nhc):
        p.state[3] = 1
    for replay in range(101):
        pos = mtk.advance()
        assert np.array_equal(pos, nhc.advance()), replay
        f, e, w = evaluate(pos)
        mtk.finish(f, e, w, total=(7 * replay, 0))
        nhc.finish(f, e, total=(7 * replay, 0))
        _same(mtk, nhc, replay, ("x", "v", "x0", "v0", "image", "f_prev", "pos32", "xi", "v_xi", "scale", "state"))
        assert not mtk.v_cell.any() and (mtk.factors == 1.0).all() and not mtk.xi_b.any() and not mtk.v_xi_b.any()
        for now, then in zip((mtk.cell64, mtk.cell32, mtk.inv_cell), cells):
            assert now.tobytes() == then.tobytes(), replay
        if replay:
            row, old = mtk.log[(replay - 1) % 16], nhc.log[(replay - 1) % 16]
            assert np.array_equal(bits(row[:, :4]), bits(old)), replay
    assert mtk.state.tolist() == [100, 0, 0, 0] and mtk.image.any() and (mtk.scale != 1.0).all()
    assert np.array_equal(mtk.w_prev, w)


def test_tau_inf_and_taup_inf_is_the_nve_twin_bit_for_bit():
    """Everything off against hermnet_host_md_advance / _finish (NVE) over 100 steps, compared the way test_nhc_host.py
    compares its chain twin: x, v, image, f_prev, pos32 and the log's columns 0 and 2 by bits; column 1 is the canonical sum
    of the NVE twin's own per-atom kinetic energies (hermnet_host_md_finish's sequential sum is frozen with ABI v13)."""
    s = _unequal_batch()
    mtk, = _drivers(s, (HostMTK,), tau=np.inf, taup=np.inf, chain=3, order=3, substeps=2)
    nve = HostMD(s["x"], s["v"], s["m"], 0.5, cell=s["cell"], batch=s["batch"], log_steps=16, num_graphs=3)
    evaluate = _potential(len(s["x"]), s["batch"], 3)
    for p in (mtk, nve):
        p.state[3] = 1
    for replay in range(101):
        pos = mtk.advance()
        assert np.array_equal(pos, nve.advance()), replay
        f, e, w = evaluate(pos)
        mtk.finish(f, e, w, total=(7 * replay, 0))
        nve.finish(f, e, total=(7 * replay, 0))
        _same(mtk, nve, replay, ("x", "v", "image", "f_prev", "pos32", "state"))
        assert not mtk.xi.any() and not mtk.v_xi.any() and (mtk.scale == 1.0).all() and (mtk.factors == 1.0).all()
        if replay:
            row, old = mtk.log[(replay - 1) % 16], nve.log[(replay - 1) % 16]
            assert np.array_equal(bits(row[:, [0, 2]]), bits(old[:, [0, 2]])) and not row[:, 3].any()
            want = [canonical_sum(nve.ke_atom[nve.graph_ptr[g]:nve.graph_ptr[g + 1]]) for g in range(3)]
            assert np.array_equal(bits(row[:, 1]), bits(np.array(want))) and bits(row[0, 1]) == bits(old[0, 1])
    assert mtk.state.tolist() == [100, 0, 0, 0] and mtk.image.any()


# ---- the pair-potential system ----------------------------------------------------------------------------------------------------
PRESSURE, TAU, TAUP, DOF = 0.02, 50.0, 200.0, 93.0        # eV/A^3, fs, fs; 32 atoms with the centre of mass at rest
ARMS = [("isotropic", (1, 1, 1), TAU), ("isotropic", (1, 1, 1), np.inf), ("axes", (1, 1, 0), TAU), ("axes", (1, 1, 0), np.inf)]


def _pair_driver(pairs, x, v, dt, tau, taup, coupling="isotropic", mask=(1, 1, 1), log_steps=64, cls=HostMTK, temperature=300.0,
                 pressure=PRESSURE, wrap=True):
    return cls(x, v, pairs.masses, dt, temperature, tau, DOF, cell=pairs.cell, pressure=pressure, taup=taup, coupling=coupling,
               mask=mask, log_steps=log_steps, max_strain=0.05, wrap=wrap)


def _deviation(pairs, x, v, dt, tau, taup, coupling="isotropic", mask=(1, 1, 1), time=400.0):
    """(max |H - H_0| of the conserved sum over `time` fs of the host twins, the largest relative change of the volume)."""
    steps = int(round(time / dt))
    log = run_pairs(_pair_driver(pairs, x, v, dt, tau, taup, coupling, mask, log_steps=steps), pairs, steps)
    h = conserved_log(log)
    return float(np.abs(h - h[0]).max()), float(np.abs(log[:, 5] / log[0, 5] - 1.0).max())


@pytest.mark.parametrize("shape", ["cubic", "sheared"])
def test_the_extended_energy_is_conserved_to_second_order(shape):
    """32 atoms of unequal masses with the smooth pair potential of mtk_reference.Pairs (float64 numpy, outputs rounded to
    float32 as a step's are) in a cubic and in a sheared cell, 300 K, P0 = 0.02 eV/A^3 (below the start's 0.031: the cell
    expands), tau = 50 fs, taup = 200 fs, M = 3, order 3, 400 fs.  The yardstick is the same twins with everything off (tau =
    taup = inf: NVE bit for bit) on the same system, start and dt: max |E - E_0|.  For both couplings, thermostatted and NPH:
    the conserved sum stays within 3 x that figure, halving dt cuts its deviation between 3.5- and 4.5-fold, and the volume
    moves by more than 1 %.

    Seen (HostMTK; NumpyMTK is bit-identical, the first test), cubic cell, max |H - H_0| in eV and over the yardstick:
        dt    NVE        isotropic        NPH              axes (1,1,0)     axes NPH
        2.0   1.19e-3    2.32e-3 (1.96)   1.57e-3 (1.33)   2.13e-3 (1.80)   1.45e-3 (1.22)
        1.0   2.98e-4    5.72e-4 (1.92)   3.95e-4 (1.33)   5.24e-4 (1.76)   3.65e-4 (1.23)
        cut              4.07             3.97             4.07             3.98
    with the volume growing by 36 to 53 %; sheared cell: NVE 1.06e-3 / 2.68e-4, ratios 1.17 to 1.89, cuts 3.95 to 4.06, the
    volume growing by 34 to 59 %."""
    cell = None if shape == "cubic" else [[7.4, 0.0, 0.0], [0.9, 7.2, 0.0], [-0.5, 0.7, 7.6]]
    pairs = Pairs(cell=cell)
    x, v = pairs.start(300.0, 1)
    seen = {}
    for dt in (2.0, 1.0):
        yardstick, still = _deviation(pairs, x, v, dt, np.inf, np.inf)
        assert still == 0.0
        for coupling, mask, tau in ARMS:
            dev, moved = _deviation(pairs, x, v, dt, tau, TAUP, coupling, mask)
            print("%s dt %.1f %s %s tau %s: NVE max|E - E0| = %.4e eV, MTK max|H - H0| = %.4e eV, ratio %.3f, volume moved "
                  "%.1f %%" % (shape, dt, coupling, mask, tau, yardstick, dev, dev / yardstick, 100.0 * moved))
            assert dev <= 3.0 * yardstick, (dt, coupling, tau, dev, yardstick)
            assert moved > 0.01, (dt, coupling, tau, moved)
            seen[dt, coupling, tau] = dev
    for coupling, mask, tau in ARMS:
        factor = seen[2.0, coupling, tau] / seen[1.0, coupling, tau]
        print("%s %s tau %s: halving dt cuts the deviation %.3f-fold" % (shape, coupling, tau, factor))
        assert 3.5 <= factor <= 4.5, (coupling, tau, factor)


def _reversal(pairs, x, v, steps, tau, taup, coupling="isotropic", mask=(1, 1, 1), moved=0.05):
    """`steps` forward, every velocity of the extended system flipped, `steps` back: the largest error of x (A), of the cell
    (A) and of the chains' positions, and how far the cell had moved at the turning point (A).  The wrap is off: the flow is
    what is reversed.  (A wrap takes a float32 lattice vector off a coordinate whose cell is float64; the scaled drifts behind
    it do not carry that vector to the later float32 cells' own, so a wrapped atom sits 1e-7 A from where the unwrapped flow
    has it -- for the evaluation another, equally good configuration, but not the one the way back retraces.)"""
    host = _pair_driver(pairs, x, v, 2.0, tau, taup, coupling, mask, log_steps=2 * steps, wrap=False)
    run_pairs(host, pairs, 0)
    start = host.snapshot()
    run_pairs(host, pairs, steps, prime=False)
    assert np.abs(host.x - start.x).max() > moved and not host.image.any()
    turned = float(np.abs(host.cell64 - start.cell64).max())
    host.flip()
    run_pairs(host, pairs, steps, prime=False)
    return (float(np.abs(host.x - start.x).max()), float(np.abs(host.cell64 - start.cell64).max()),
            float(max(np.abs(host.xi - start.xi).max(), np.abs(host.xi_b - start.xi_b).max())), turned)


def test_one_step_returns_to_rounding_when_every_velocity_is_flipped():
    """One step and two steps forward, the flip, as many back, both couplings, thermostatted and NPH: the step is a palindrome
    of maps that each invert under the flip, so only rounding is left.  Every quantity passes through fewer than 32 roundings
    of one ulp each per step: x and the cell (below 8 A: ulp 8.9e-16 A) return within 32 ulp per step, the chains' positions
    (below 1) within 1e-15.  A misplaced or wrong-signed factor misses by ten orders and more.
    Seen: x 1.8e-15 A, cell 8.9e-16 A (1.8e-15 after two steps), chains 6.5e-19."""
    pairs = Pairs()
    x, v = pairs.start(300.0, 1)
    for steps in (1, 2):
        for coupling, mask, tau in ARMS:
            err_x, err_cell, err_xi, _ = _reversal(pairs, x, v, steps, tau, TAUP, coupling, mask, moved=1e-3)
            print("%d steps, %s %s tau %s: x %.3e A, cell %.3e A, chains %.3e" % (steps, coupling, mask, tau, err_x, err_cell, err_xi))
            assert err_x <= steps * 32 * 8.9e-16 and err_cell <= steps * 32 * 8.9e-16 and err_xi <= 1e-15


REVERSED = {np.inf: 100, TAU: 30}       # steps each way, by tau: see the test


def test_a_run_returns_when_every_velocity_is_flipped():
    """The pair system at dt = 2 fs: n steps, v, v_cell and both chains' velocities change their sign, n steps.  The yardstick
    is the NVE twin's own reversal error on the same system and the same n (`_reversal` with everything off); x, the cell and
    the chains' positions must return within 100 x that figure, both couplings, thermostatted and NPH.  Both numbers are
    printed.

    n.  Without a thermostat (NPH) n = 100.  With one, the way back runs under the negative of the friction the way out ran
    under, and rounding grows with it whatever is or is not coupled to the cell: the chain twin ALONE (taup = inf: the step of
    hermnet_host_nhc_*, no barostat) returns its chain within 4.2e-15 after 30 steps, 5.8e-13 after 50, 4.2e-7 after 100, and
    not at all after 200.  So the thermostatted arms take n = 30, the longest of these at which that twin itself is inside
    the bound -- asserted here, so that the case cannot silently stop meaning anything.  In 30 steps the cell moves by 0.8 to 1.3 A
    and the atoms by more than 0.05 A: twelve orders above the bound.

    Seen (A; chains dimensionless), NVE twin 8.9e-16 at n = 30 and 1.8e-15 at n = 100 (it retraces: its forces repeat bit for
    bit at the float32 roundings):
        n = 30    isotropic  x 9.8e-15  cell 6.2e-15  chains 7.7e-15      axes (1,1,0)  x 7.1e-15  cell 6.2e-15  chains 9.3e-15
        n = 100   isotropic  x 1.1e-14  cell 2.7e-15                      axes (1,1,0)  x 1.5e-14  cell 6.2e-15
    (With the wrap ON, 100 steps: x 1.8e-6 A thermostatted, 5.9e-7 A NPH -- `_reversal` says why.)"""
    pairs = Pairs()
    x, v = pairs.start(300.0, 1)
    yardstick = {n: _reversal(pairs, x, v, n, np.inf, np.inf)[0] for n in REVERSED.values()}
    alone = _reversal(pairs, x, v, REVERSED[TAU], TAU, np.inf)
    print("the chain twin alone, %d steps: x %.3e A, chains %.3e; NVE %.3e A" % (REVERSED[TAU], alone[0], alone[2], yardstick[REVERSED[TAU]]))
    assert alone[0] <= 100.0 * yardstick[REVERSED[TAU]] and alone[2] <= 100.0 * yardstick[REVERSED[TAU]] and alone[3] == 0.0
    for coupling, mask, tau in ARMS:
        n = REVERSED[tau]
        err_x, err_cell, err_xi, turned = _reversal(pairs, x, v, n, tau, TAUP, coupling, mask)
        print("%s %s tau %s, %d steps: NVE reversal error %.3e A; MTK x %.3e A, cell %.3e A (it had moved %.3e A), chains %.3e" %
              (coupling, mask, tau, n, yardstick[n], err_x, err_cell, turned, err_xi))
        assert 0.0 < yardstick[n] < 1e-12 and turned > 1e-3, (yardstick[n], turned)
        assert err_x <= 100.0 * yardstick[n] and err_cell <= 100.0 * yardstick[n] and err_xi <= 100.0 * yardstick[n]


def test_the_isothermal_isobaric_averages():
    """The pair system (16 atoms) at 300 K and P0 = 0.03 eV/A^3, isotropic, tau = 50 fs, taup = 200 fs, dt = 2 fs: 22,000 steps
    per seed, the first 2,000 dropped, 20 blocks of 1,000.  On each of 4 seeds, within 5 blocked standard errors: <E_kin> = dof
    kB T / 2, and the work-virial identity <(pressure - P0) volume> = -kB T from the log's columns 4 and 5 (the pressure
    column carries the kinetic part of the 3 N velocities, and the ensemble's measure is dV: Martyna, Tobias, Klein 1994).

    Seen (HostMTK = NumpyMTK bit for bit), in standard errors: <E_kin> -2.42, -1.28, +0.20, +0.30; the identity -0.13, +0.57,
    +0.26, -0.14."""
    pairs = Pairs(n=16, cell=np.diag([5.9, 5.9, 5.9]))
    temperature, p0, steps, drop, blocks = 300.0, 0.03, 22000, 2000, 20
    dof = 3.0 * pairs.n - 3.0
    for seed in range(4):
        x, v = pairs.start(temperature, 100 + seed)
        host = HostMTK(x, v, pairs.masses, 2.0, temperature, TAU, dof, cell=pairs.cell, pressure=p0, taup=TAUP, log_steps=steps,
                       max_strain=0.05)
        log = run_pairs(host, pairs, steps)[drop:]
        ke, work = log[:, 1].reshape(blocks, -1), ((log[:, 4] - p0) * log[:, 5]).reshape(blocks, -1)
        for name, series, want in (("<E_kin>", ke, 0.5 * dof * KB * temperature), ("<(P - P0) V>", work, -KB * temperature)):
            mean, err = series.mean(), series.mean(axis=1).std(ddof=1) / math.sqrt(blocks)
            print("seed %d: %s = %.5f +- %.5f eV (want %.5f: %+.2f sigma)" % (seed, name, mean, err, want, (mean - want) / err))
            assert abs(mean - want) <= 5.0 * err, (seed, name, mean, err, want)


# ---- void steps -------------------------------------------------------------------------------------------------------------------
RETURNED = ("x", "v", "image", "f_prev", "pos32", "xi", "v_xi", "xi_b", "v_xi_b", "v_cell", "cell64", "cell32", "inv_cell",
            "w_prev", "log")


@pytest.mark.parametrize("cause", ["energy", "virial", "strain"])
def test_a_void_step_returns_atoms_cell_barostat_and_both_chains(cause):
    """Six steps of the unequal batch, then a step that is fed a NaN energy, a NaN virial entry, or whose barostat was pushed
    beyond max_strain (v_cell of graph 1 written from outside): atoms, both chains, v_cell, the three forms of the cell, f_prev,
    w_prev and the log are those of the step's start bit for bit, `state` records the halt with the non-finite bit, `refused`
    counts the flagged graph alone, and later calls change nothing.  A refused graph's cell never moved: the float32 cell the
    search read is the one the step began with.  After the halt is cleared (and the push taken back) and the prime, the run
    equals one that never saw it."""
    s = _unequal_batch()
    host, twin = _drivers(s, (HostMTK, HostMTK))
    evaluate = _potential(len(s["x"]), s["batch"], 3)
    for p in (host, twin):
        p.state[3] = 1
        for replay in range(6):
            f, e, w = evaluate(p.advance())
            p.finish(f, e, w)
    kept = host.v_cell.copy()
    if cause == "strain":
        host.v_cell[1] = 0.2                              # |v_cell| dt = 0.1 > max_strain = 0.05
    before = host.snapshot()
    moved = host.advance().copy()
    assert not np.array_equal(host.v, before.v) and not np.array_equal(host.xi_b, before.xi_b)
    assert host.flag.tolist() == ([0, 1, 0] if cause == "strain" else [0, 0, 0])
    if cause == "strain":
        assert (host.factors[1] == 1.0).all() and host.cell32[1].tobytes() == before.cell32[1].tobytes()
        assert host.cell64[1].tobytes() == before.cell64[1].tobytes() and not (host.factors[0] == 1.0).any()
    else:
        assert not np.array_equal(host.cell64, before.cell64)
    f, e, w = evaluate(moved)
    bad_e, bad_w = e.copy(), w.copy()
    if cause == "energy":
        bad_e[1] = np.nan
    if cause == "virial":
        bad_w[2, 5] = np.nan
    host.finish(f, bad_e, bad_w)
    after = host.snapshot()
    assert after.state.tolist() == [5, 256, 5, 0]
    assert after.refused.tolist() == ([0, 1, 0] if cause == "strain" else [0, 0, 0])
    for k in RETURNED:
        assert getattr(after, k).tobytes() == getattr(before, k).tobytes(), k
    host.finish(f, e, w)                                  # halted: nothing
    assert np.array_equal(host.advance(), before.pos32)
    for k in STATE_FIELDS:
        assert getattr(host.snapshot(), k).tobytes() == getattr(after, k).tobytes(), k
    host.state[1:3] = 0                                   # resume: the halt cleared, the prime, then the same step
    host.state[3] = 1
    host.v_cell[:] = kept
    f0, e0, w0 = evaluate(host.advance())
    host.finish(f0, e0, w0)
    for p in (host, twin):
        for replay in range(3):
            f, e, w = evaluate(p.advance())
            p.finish(f, e, w)
    _same(host.snapshot(), twin.snapshot(), "resumed", [k for k in STATE_FIELDS if k != "refused"])
    assert host.state.tolist() == [8, 0, 0, 0]


def test_a_prime_fed_a_nan_virial_keeps_the_accepted_forces_and_virial():
    s = _unequal_batch()
    host, = _drivers(s, (HostMTK,))
    evaluate = _potential(len(s["x"]), s["batch"], 3)
    host.state[3] = 1
    f, e, w = evaluate(host.advance())
    w[0, 0] = np.nan
    host.finish(f, e, w)
    assert host.state.tolist() == [0, 256, 0, 0] and not host.f_prev.any() and not host.w_prev.any()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_without_a_gpu():
    z, x = np.full(5, 14), np.arange(15, dtype=np.float64).reshape(5, 3)
    make = lambda **kw: DeviceMTK(None, z, kw.pop("cell", np.eye(3) * 20.0), x, np.full(5, 28.0), 1.0,
                                  **dict(dict(temperature=300.0), **kw))
    with pytest.raises(RuntimeError, match="a barostat needs periodic cells"):
        make(cell=None)
    with pytest.raises(ValueError, match="friction= is Langevin's"):
        make(friction=0.01)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="chain .* in 1..8"):
            make(chain=bad)
    with pytest.raises(ValueError, match="order .* one of 1, 3, 5"):
        make(order=2)
    with pytest.raises(ValueError, match="substeps"):
        make(substeps=0)
    for bad in (None, 0.0, np.inf, [300.0, 0.0]):
        with pytest.raises(ValueError, match="temperature .* positive and finite"):
            make(temperature=bad)
    with pytest.raises(ValueError, match="tau .* > 0"):
        make(tau=-1.0)
    with pytest.raises(ValueError, match="graph 1 has dof = -3 <= 0"):
        make(batch=np.array([0, 0, 0, 1, 1]), num_graphs=2, dof=[6.0, -3.0], cell=np.stack([np.eye(3) * 20.0] * 2))
    for bad in (0.0, -10.0, np.nan, [100.0, -1.0]):
        with pytest.raises(ValueError, match="taup .* > 0 .inf: the barostat is off"):
            make(taup=bad)
    for bad in (np.inf, np.nan, [0.0, -np.inf]):
        with pytest.raises(ValueError, match="pressure .* must be finite"):
            make(pressure=bad)
    for bad in ("full", "berendsen", None):
        with pytest.raises(ValueError, match="coupling is one of .*isotropic.*axes"):
            make(coupling=bad)
    with pytest.raises(ValueError, match="empty mask couples nothing"):
        make(coupling="axes", mask=(0, 0, 0))
    with pytest.raises(ValueError, match="mask has three entries"):
        make(coupling="axes", mask=(1, 1))
    for bad in (0.0, -0.01, 0.11, np.nan):
        with pytest.raises(ValueError, match=r"max_strain must lie in \(0, 0.1\]"):
            make(max_strain=bad)


def test_malformed_calls_are_refused_by_the_argument_checks():
    """HN_ERR_BAD_ARG from the host twins for what the header lists; the device entry points refuse the same before
    anything is launched, so with no GPU."""
    bad_arg = _lib.HN_ERR_BAD_ARG
    x = np.arange(15, dtype=np.float64).reshape(5, 3)
    zero_f = np.zeros((5, 3), dtype=np.float32)

    def fresh():
        return HostMTK(x, np.zeros((5, 3)), np.full(5, 28.0), 1.0, 300.0, 50.0, 12.0, cell=np.eye(3) * 20.0)

    host = fresh()
    host.advance()
    host.finish(zero_f)
    assert host.state.tolist() == [1, 0, 0, 0]
    for name, value in (("chain", 0), ("chain", 9), ("order", 2), ("substeps", 0), ("coupling", 2), ("coupling", -1), ("mask", 0),
                        ("mask", 8), ("mask", 5), ("max_strain", 0.0), ("max_strain", 0.2), ("max_strain", np.nan), ("dt", 0.0),
                        ("flags", 1)):
        host = fresh()
        setattr(host, name, value)
        host.advance(expect=bad_arg)
        if name != "flags":
            host.finish(zero_f, expect=bad_arg)
        assert host.state.tolist() == [0, 0, 0, 0] and np.array_equal(host.x, x)
    for name in ("delta", "kt", "q", "xi", "scale", "par", "dof_kt_b", "q_b", "inv_q_b", "xi_b", "v_xi_b", "scale_b", "v_cell",
                 "cell64", "cell32", "inv_cell", "w_prev", "factors", "backup", "flag", "refused", "e_code"):
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
    h.mask = 0
    rc = lib.hermnet_mtk_advance(5, 1, 0, 1.0, _p(h.x), _p(h.v), _p(h.x0), _p(h.v0), _p(h.image), _p(h.image0), _p(h.f_prev),
                                 _p(h.kick), None, _p(h.pos32), _p(h.state), _p(h.graph_ptr), _p(h.half_mass), *h._chains(),
                                 *h._baro(), None)
    assert rc == bad_arg
    e, tot, w = np.zeros(1, dtype=np.float32), np.zeros(2, dtype=np.int64), np.zeros(9, dtype=np.float32)
    rc = lib.hermnet_mtk_finish(5, 1, _p(h.graph_ptr), None, _p(zero_f), _p(e), _p(w), _p(tot), 100, 1.0, *h._finish_atoms(),
                                *h._chains(), *h._baro(), _p(h.log), 64, _p(h.state), None)
    assert rc == bad_arg
