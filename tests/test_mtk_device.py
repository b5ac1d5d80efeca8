"""GPU: `hermnet_amd.mtk.DeviceMTK` -- the MTK barostat with Nose-Hoover chains inside the replayed hipGraph.  The kernels
against the library's host twins on synthetic state; a run against the host-driven loop it replaces after every step, for a
batch and for one structure; `taup=inf` against `DeviceNHC` with observers; velocities written between two runs; halt on a
list overflow under compression and resume; the launch list; the ASE hand-off."""
from collections import Counter

import numpy as np
import pytest
import torch

from hermnet_amd import _lib
from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep
from hermnet_amd.md import ASE_TIME_FS, HALT_CAPACITY, HALT_NONFINITE, DeviceNPT
from hermnet_amd.mtk import DeviceMTK, conserved
from hermnet_amd.observe import MSD, Frames
from md_reference import AMU, KB, bits
from mtk_reference import HostMTK
import resident_helpers as rh
from resident_helpers import _flat, _put
import test_nhc_device as ndt

pytestmark = pytest.mark.gpu

DT = ndt.DT
T_MTK = ndt.T_NHC                                         # K, per graph
TAU = ndt.TAU                                             # fs, per graph
TAUP = 50.0                                               # fs: short, so that 20 steps move the cells
DOF = ndt.DOF
# eV/A^3 between each graph's start pressure and its target: the barostat's acceleration is 3 dP V / ((dof + 3) kB T taup^2), so
# an offset in proportion to T gives the four cells one acceleration, 8e-5 / fs^2 for V = 450 A^3.  The synthetic weights put up
# next to no resistance, so after 20 steps that is a strain of 1.6e-3 per step (max_strain here: 0.05) and a linear strain of
# 1.6e-2: the volumes move by 5 to 20 %
OFFSET = 0.002 * T_MTK / 1500.0
PARKED = 1 << 20
_CACHE = {}


# ---- 1. the kernels against the host twins ----------------------------------------------------------------------------------------
NAMES = ["x", "v", "x0", "v0", "image", "image0", "f_prev", "kick", "batch", "pos32", "state", "graph_ptr", "half_mass", "ke_atom",
         "log", "delta", "kt", "dof_kt", "q", "inv_q", "xi", "v_xi", "xi0", "v_xi0", "scale", "par", "dof_kt_b", "q_b", "inv_q_b",
         "xi_b", "v_xi_b", "scale_b", "v_cell", "cell64", "cell32", "inv_cell", "w_prev", "factors", "backup", "flag", "refused",
         "e_code"]
CHAIN_NAMES = ("delta", "kt", "dof_kt", "q", "inv_q", "xi", "v_xi", "xi0", "v_xi0", "scale")
BARO_NAMES = ("par", "dof_kt_b", "q_b", "inv_q_b", "xi_b", "v_xi_b", "scale_b", "v_cell", "cell64", "cell32", "inv_cell", "w_prev",
              "factors", "backup", "flag", "refused", "e_code")
COUNTS = [1, 32, 257, 256, 5]


def _replay_on_both(host, d, f_new, energy, virial, total, capacity=5000):
    """One hermnet_mtk_advance + hermnet_mtk_finish and their host twins on the same state and evaluation."""
    lib, P, stream = _lib.load(), _lib.ptr, torch.cuda.current_stream().cuda_stream
    n, B = host.n, host.B
    chains = (host.chain, host.order, host.substeps) + tuple(P(d[k]) for k in CHAIN_NAMES)
    baro = (host.coupling, host.mask, host.max_strain) + tuple(P(d[k]) for k in BARO_NAMES)
    atoms = [P(d[k]) for k in ("x", "v", "x0", "v0", "image", "image0", "f_prev", "kick")]
    _lib.check(lib.hermnet_mtk_advance(n, B, host.flags, host.dt, *atoms, P(d["batch"]), P(d["pos32"]), P(d["state"]),
                                       P(d["graph_ptr"]), P(d["half_mass"]), *chains, *baro, stream), "advance")
    f_d, e_d, w_d, t_d = _put(f_new), _put(energy), _put(virial), _put(np.array(total, dtype=np.int64))
    _lib.check(lib.hermnet_mtk_finish(n, B, P(d["graph_ptr"]), P(d["batch"]), P(f_d), P(e_d), P(w_d), P(t_d), capacity, host.dt,
                                      *atoms, P(d["half_mass"]), P(d["pos32"]), P(d["ke_atom"]), *chains, *baro, P(d["log"]),
                                      host.log_steps, P(d["state"]), stream), "finish")
    torch.cuda.synchronize()
    host.advance()
    host.finish(f_new, energy, virial, total=total, capacity=capacity)


def _equal_everywhere(host, d, what):
    for k in NAMES:
        assert d[k].cpu().numpy().tobytes() == getattr(host, k).tobytes(), (what, k)


@pytest.mark.parametrize("coupling,mask", [("isotropic", (1, 1, 1)), ("axes", (1, 0, 1))])
@pytest.mark.parametrize("chain,order,substeps", [(1, 1, 1), (3, 3, 2), (8, 5, 1)])
def test_device_kernels_equal_the_host_twins(chain, order, substeps, coupling, mask):
    """Graphs of 1, 32, 257, 256 and 5 atoms (one workgroup's tile, one atom more, below a wave) in triclinic cells, an atom of
    infinite mass in the third, per-graph temperatures, pressures and time constants, the last barostat off (taup = inf), on
    synthetic state with chains and barostats in motion: two steps, a void step (NaN energy), a prime, a parked replay, then
    void steps from a NaN virial entry and from a barostat pushed beyond max_strain.  Every array of the state -- backups,
    scratch and the three forms of the cell included -- is bit-equal after each replay; after the refused step the float32
    cell is bit for bit the one the step began with."""
    B, n = len(COUNTS), sum(COUNTS)
    rs = np.random.RandomState(10 * chain + order)
    cell = np.tile(np.array([[9.3, 0.4, -0.7], [2.1, 11.2, 0.3], [-1.6, 3.3, 14.9]]), (B, 1, 1)) * np.linspace(1.0, 1.2, B)[:, None, None]
    batch = np.repeat(np.arange(B), COUNTS)
    m = rs.uniform(10.0, 60.0, n)
    m[40] = np.inf
    x = np.einsum("nk,nkj->nj", rs.uniform(-1.5, 2.5, (n, 3)), cell[batch])
    temperature = np.linspace(300.0, 900.0, B)
    host = HostMTK(x, rs.normal(scale=0.004, size=(n, 3)), m, 0.5, temperature, [15.0, 30.0, 45.0, 60.0, 20.0],
                   [3.0, 93.0, 768.0, 765.0, 12.0], cell, pressure=[0.0, 1e-3, -5e-4, 2e-3, 1e-3],
                   taup=[60.0, 20.0, 10.0, 10.0, np.inf], coupling=coupling, mask=mask, max_strain=0.05, chain=chain, order=order,
                   substeps=substeps, batch=batch, log_steps=4, num_graphs=B)
    host.v[40] = 0.0
    host.f_prev[:] = rs.normal(size=(n, 3)).astype(np.float32)
    host.w_prev[:] = rs.normal(size=(B, 9)).astype(np.float32)
    host.image[:] = rs.randint(-2, 3, (n, 3))
    host.state[0] = 6
    host.xi[:], host.v_xi[:] = rs.normal(scale=0.5, size=(B, chain)), rs.normal(scale=0.02, size=(B, chain))
    host.xi_b[:4], host.v_xi_b[:4] = rs.normal(scale=0.5, size=(4, chain)), rs.normal(scale=0.02, size=(4, chain))
    rate = rs.normal(scale=2e-3, size=(B, 3))
    host.v_cell[:4] = rate[:4, :1] if coupling == "isotropic" else rate[:4] * np.array(mask)
    d = {k: _put(getattr(host, k)) for k in NAMES}
    evaluation = lambda: (rs.normal(size=(n, 3)).astype(np.float32), rs.normal(size=B).astype(np.float32),
                          rs.normal(size=(B, 9)).astype(np.float32))
    start32 = host.cell32.copy()
    for k in (0, 1):
        _replay_on_both(host, d, *evaluation(), (4321 + k, 0))
        _equal_everywhere(host, d, (chain, "step", k))
        coupled = [a for a in range(12) if coupling == "isotropic" or mask[a % 3]]
        assert (host.factors[:4][:, coupled] != 1.0).all() and (host.factors[4] == 1.0).all() and not host.v_cell[4].any()
        assert (host.scale != 1.0).all() and (host.scale_b[:4] != 1.0).all() and not host.flag.any()
    assert host.state.tolist() == [8, 0, 0, 0] and np.abs(host.image).max() >= 2 and not host.v[40].any()
    assert np.all(host.log[7 % 4, :, 2] == 4322) and np.all(host.log[[0, 1]] == -7.0)
    assert not np.array_equal(host.cell32[:4], start32[:4]) and host.cell32[4].tobytes() == start32[4].tobytes()
    returned = ("x", "v", "image", "pos32", "f_prev", "w_prev", "xi", "v_xi", "xi_b", "v_xi_b", "v_cell", "cell64", "cell32",
                "inv_cell", "log")
    code = 256
    for cause in ("energy", "virial", "strain"):
        if cause == "strain":
            host.v_cell[1] = 0.3 if coupling == "isotropic" else [0.3, 0.0, 0.0]
            d["v_cell"].copy_(_put(host.v_cell))
        before = {k: getattr(host, k).copy() for k in returned}
        f, e, w = evaluation()
        if cause == "energy":
            e[B - 1] = np.nan
        if cause == "virial":
            w[2, 7] = np.nan
        _replay_on_both(host, d, f, e, w, (4323, 0))
        _equal_everywhere(host, d, (chain, "void", cause))
        assert host.state.tolist() == [8, code, 8, 0], cause
        assert all(getattr(host, k).tobytes() == v.tobytes() for k, v in before.items()), cause
        assert host.flag.tolist() == [0, int(cause == "strain"), 0, 0, 0] and host.refused.tolist() == host.flag.tolist()
        if cause == "energy":                             # behind the first void step: a prime, then a parked replay
            host.state[:] = (8, 0, 0, 1)
            d["state"].copy_(_put(host.state))
            _replay_on_both(host, d, *evaluation(), (4324, 0))
            _equal_everywhere(host, d, (chain, "prime"))
            assert host.state.tolist() == [8, 0, 0, 0] and host.xi_b.tobytes() == before["xi_b"].tobytes()
            assert host.v.tobytes() == before["v"].tobytes() and host.f_prev.tobytes() != before["f_prev"].tobytes()
            assert host.w_prev.tobytes() != before["w_prev"].tobytes() and host.cell64.tobytes() == before["cell64"].tobytes()
            host.state[:] = (8, PARKED, 0, 0)
            d["state"].copy_(_put(host.state))
            parked = {k: getattr(host, k).copy() for k in NAMES}
            _replay_on_both(host, d, *evaluation(), (4325, 0))
            _equal_everywhere(host, d, (chain, "parked"))
            assert all(getattr(host, k).tobytes() == v.tobytes() for k, v in parked.items())
        host.state[:] = (8, 0, 0, 0)
        d["state"].copy_(_put(host.state))


# ---- the driver on 4 x 32 atoms and on one 32-atom structure --------------------------------------------------------------------------
def _system(name):
    """"batch": test_nhc_device's four different 32-atom alloy cells; "single": the first of them."""
    s = ndt._system()
    if name == "batch":
        return dict(s, B=4, temperature=T_MTK, tau=TAU, offset=OFFSET)
    p = slice(0, 32)
    return dict(pos=s["pos"][p], z=s["z"][p], cell=s["cell"][:1], m=s["m"][p], v=s["v"][p], batch=None, B=1, temperature=T_MTK[3:],
                tau=TAU[3:], offset=OFFSET[3:])


def _evaluator(s):
    """The plain graphed step with the virial, fed the float32 roundings of coordinates and cell: (e, f, edges, virial)."""
    if ("step", s["B"]) not in _CACHE:
        dev, model = rh._dev(), rh._shared_model()
        p0, cell = torch.from_numpy(s["pos"].astype(np.float32)).to(dev), _put(s["cell"].astype(np.float32))
        if s["batch"] is None:
            _CACHE["step", 1] = GraphedMDStep(model, _put(s["z"]), cell.reshape(3, 3), p0, stress=True, variable_cell=True)
        else:
            _CACHE["step", s["B"]] = GraphedBatchMDStep(model, _put(s["z"]), cell, p0, _put(s["batch"]), s["B"], stress=True)
    step, shape = _CACHE["step", s["B"]], (3, 3) if s["batch"] is None else (s["B"], 3, 3)

    def evaluate(p32, cell32):
        step(_put(p32), _put(cell32.reshape(shape)))
        e, f, ok, n, w = step.fetch()
        assert ok
        return e.copy(), f.copy(), n, w.copy().reshape(-1, 9)
    return evaluate


def _start_pressure(s):
    """[B]: (sum m v^2 + tr W) / 3 V of the start, from the plain graphed step: the reference, never the code under test."""
    if ("p", s["B"]) not in _CACHE:
        cell32 = s["cell"].astype(np.float32)
        w = _evaluator(s)(s["pos"].astype(np.float32), cell32)[3]
        b = np.zeros(len(s["z"]), dtype=np.int64) if s["batch"] is None else s["batch"]
        kin = np.bincount(b, weights=s["m"] * AMU * (s["v"] ** 2).sum(axis=1), minlength=s["B"])
        vol = np.abs(np.linalg.det(cell32.astype(np.float64)))
        _CACHE["p", s["B"]] = (kin + w[:, [0, 4, 8]].astype(np.float64).sum(axis=1)) / (3.0 * vol)
    return _CACHE["p", s["B"]]


def _mtk(s, sign=-1.0, cls=DeviceMTK, **kw):
    """The driver at targets OFFSET below (`sign` -1: the cells expand, the list shrinks) or above the start pressures."""
    args = dict(velocities=s["v"], temperature=s["temperature"], tau=s["tau"], taup=TAUP, max_strain=0.05,
                pressure=_start_pressure(s) + sign * s["offset"])
    if s["batch"] is not None:
        args.update(batch=_put(s["batch"]), num_graphs=s["B"])
    args.update(kw)
    cell = s["cell"].astype(np.float32).astype(np.float64)
    return cls(rh._shared_model(), _put(s["z"]), cell if s["batch"] is not None else cell[0], s["pos"], s["m"], DT, **args)


def _host(s, x, v, sign=-1.0, **kw):
    args = dict(pressure=_start_pressure(s) + sign * s["offset"], taup=TAUP, max_strain=0.05, batch=s["batch"], log_steps=64,
                num_graphs=s["B"])
    args.update(kw)
    return HostMTK(x, v, s["m"], DT, s["temperature"], s["tau"], DOF, s["cell"].astype(np.float32).astype(np.float64), **args)


def _equals(snap, host):
    return (np.array_equal(bits(snap.positions), bits(host.x)) and np.array_equal(bits(snap.velocities), bits(host.v))
            and np.array_equal(snap.images, host.image) and np.array_equal(snap.forces, host.f_prev)
            and np.array_equal(bits(snap.cell.reshape(-1, 9)), bits(host.cell64))
            and np.array_equal(bits(snap.v_cell), bits(host.v_cell))
            and np.array_equal(bits(snap.xi), bits(host.xi)) and np.array_equal(bits(snap.v_xi), bits(host.v_xi))
            and np.array_equal(bits(snap.xi_baro), bits(host.xi_b)) and np.array_equal(bits(snap.v_xi_baro), bits(host.v_xi_b))
            and np.array_equal(bits(snap.nhc_scale), bits(host.scale)) and np.array_equal(bits(snap.nhc_scale_baro), bits(host.scale_b))
            and np.array_equal(bits(snap.mtk_factors), bits(host.factors)) and np.array_equal(snap.refused, host.refused))


def _state_bits(snap):
    return ndt._state_bits(snap) + tuple(bits(a).tobytes() for a in (snap.cell, snap.v_cell, snap.xi_baro, snap.v_xi_baro))


@pytest.mark.parametrize("name", ["batch", "single"])
def test_run_equals_the_host_driven_loop_after_every_step(name):
    """4 x 32 atoms at four (T, P) and time constants, and one 32-atom structure (the variable-cell capture): 20 steps against
    the graphed step with the virial + fetch() + the host twins, fed the float32 roundings of coordinates and cell.  Positions,
    images, velocities, forces, the cell, v_cell, both chains, every factor and the log row are bit-equal after EVERY step,
    while the volume changes by more than 1 %; `volume`, `temperature_now` and `conserved` are what their definitions say."""
    s = _system(name)
    B, evaluate = s["B"], _evaluator(s)
    host = _host(s, s["pos"], s["v"])
    host.state[3] = 1
    e, f, n, w = evaluate(host.advance().copy(), host.cell32)
    host.finish(f, e, w, total=(n, 0))
    md = _mtk(s)
    first = md.fetch()
    assert first.step == 0 and np.array_equal(first.forces, host.f_prev) and not first.v_cell.any() and first.log.shape == (0, B, 7)
    assert np.array_equal(md.w_prev.cpu().numpy(), host.w_prev) and md.dof.tolist() == [DOF] * B
    volumes = []
    for k in range(20):
        e, f, n, w = evaluate(host.advance().copy(), host.cell32)
        host.finish(f, e, w, total=(n, 0))
        md.run(1)
        snap = md.fetch()
        assert (snap.step, snap.halted) == (k + 1, False)
        assert _equals(snap, host), k
        assert snap.log.shape == (1, B, 7) and np.array_equal(bits(snap.log[0]), bits(host.log[k % 64])), k
        volumes.append(snap.volume)
    assert np.array_equal(md.step.cell.cpu().numpy().reshape(-1, 9), host.cell32)
    assert np.array_equal(bits(md.inv_cell.cpu().numpy().reshape(-1, 9)), bits(host.inv_cell))
    start = np.abs(np.linalg.det(s["cell"].astype(np.float32).astype(np.float64)))
    print("volume / start volume, the largest of 20 steps:", (np.array(volumes) / start).max(axis=0))
    assert np.all((np.array(volumes) / start).max(axis=0) > 1.01), np.array(volumes) / start
    assert np.allclose(snap.volume, np.abs(np.linalg.det(snap.cell)), rtol=1e-12, atol=0) and np.array_equal(snap.volume, snap.log[0, :, 5])
    assert (snap.mtk_factors != 1.0).all() and (snap.v_xi_baro != 0.0).all() and not snap.refused.any()
    assert np.array_equal(conserved(snap), ((snap.log[..., 0] + snap.log[..., 1]) + snap.log[..., 3]) + snap.log[..., 6])
    b = np.zeros(len(s["z"]), dtype=np.int64) if s["batch"] is None else s["batch"]
    ke = np.bincount(b, weights=0.5 * s["m"] * AMU * (snap.velocities ** 2).sum(axis=1), minlength=B)
    assert np.allclose(snap.temperature_now, 2.0 * ke / (DOF * KB), rtol=1e-13, atol=0.0)


def _observers():
    return [Frames(stride=3, frames=16, velocities=True, images=True), MSD(stride=1, rows=32)]


def test_taup_inf_equals_device_nhc_bit_for_bit_with_observers():
    """`DeviceMTK(taup=inf)` against `DeviceNHC` on the same batch: positions, velocities, images, forces, the chains, the
    log's columns 0 to 3 and everything Frames and MSD recorded are bit-equal after 20 steps; the cell is the start's, v_cell
    = 0, every factor exactly 1."""
    s = _system("batch")
    ours = _mtk(s, taup=np.inf, observers=_observers())
    plain = ndt._nhc(observers=_observers())
    ours.run(20)
    plain.run(20)
    a, b = ours.fetch(), plain.fetch()
    assert (a.step, a.halted, b.step, b.halted) == (20, False, 20, False)
    assert ndt._state_bits(a) == ndt._state_bits(b) and np.array_equal(bits(a.nhc_scale), bits(b.nhc_scale))
    assert a.log.shape == (20, 4, 7) and np.array_equal(bits(a.log[:, :, :4]), bits(b.log)) and a.xi.any()
    assert not a.v_cell.any() and (a.mtk_factors == 1.0).all() and not a.xi_baro.any()
    assert np.array_equal(bits(a.cell), bits(s["cell"].astype(np.float32).astype(np.float64)))
    assert len(a.observers) == 2 and len(a.observers[0].steps) == 7 and a.observers[1].steps.tolist() == list(range(21))
    for p, q in zip(a.observers, b.observers):
        assert _flat(p) == _flat(q)


def test_frames_record_the_moving_cell():
    """The frame of the start and one per step: six different float32 cells, the last one the rounding of the fetched cell."""
    s = _system("single")
    md = _mtk(s, observers=[Frames(stride=1, frames=8)])
    md.run(5)
    snap = md.fetch()
    frames = snap.observers[0]
    assert frames.steps.tolist() == list(range(6)) and frames.cell.shape == (6, 1, 3, 3)
    assert np.array_equal(frames.cell[0], s["cell"].astype(np.float32)) and np.array_equal(frames.cell[-1], snap.cell.astype(np.float32))
    assert len({c.tobytes() for c in frames.cell}) == 6


def test_velocities_written_between_two_runs_steer_the_next_opening_factors():
    """After 3 steps `maxwell_boltzmann` rewrites v; the next step's factors, barostat, chains and atoms are the host twin's from
    the fetched state with the NEW velocities, bit for bit -- and not what the old velocities would have given: the opening
    takes its kinetic sums from v, not from numbers the last finish left."""
    s = _system("batch")
    evaluate = _evaluator(s)
    md = _mtk(s)
    md.run(3)
    old = md.fetch()
    md.maxwell_boltzmann([200.0, 400.0, 2000.0, 3000.0], seed=5)
    start = md.fetch()
    assert not np.array_equal(start.velocities, old.velocities) and np.array_equal(bits(start.v_cell), bits(old.v_cell))
    w_prev = md.w_prev.cpu().numpy()
    factors = []
    for v in (start.velocities, old.velocities):
        host = _host(s, start.positions, v)
        host.image[:], host.f_prev[:], host.w_prev[:], host.state[0] = start.images, start.forces, w_prev, start.step
        host.xi[:], host.v_xi[:], host.xi_b[:], host.v_xi_b[:] = start.xi, start.v_xi, start.xi_baro, start.v_xi_baro
        host.v_cell[:], host.cell64[:] = start.v_cell, start.cell.reshape(-1, 9)
        host.cell32[:] = md.step.cell.cpu().numpy().reshape(-1, 9)
        host.inv_cell[:] = md.inv_cell.cpu().numpy().reshape(-1, 9)
        e, f, n, w = evaluate(host.advance().copy(), host.cell32)
        host.finish(f, e, w, total=(n, 0))
        factors.append(host.factors.copy())
        if v is start.velocities:
            want = host
    md.run(1)
    new = md.fetch()
    assert _equals(new, want) and (factors[0] != factors[1]).all()
    assert np.array_equal(bits(new.log[0]), bits(want.log[start.step % 64]))


def test_halt_on_list_overflow_under_compression_and_resume_continue_to_the_same_bits():
    """Targets above the start pressures and cool velocities: the cells shrink and the list grows.  An uninterrupted 30-step
    run shows the edge count of every step; with a capacity that the list outgrows at step k a second driver halts there with
    the capacity bit in the state of step k -- cell, barostat and chains included --, halted replays change nothing, resume()
    recaptures with more columns and the run ends bit-equal to the uninterrupted one, log included."""
    s = dict(_system("batch"))
    s["v"] = 0.2 * s["v"]
    whole = _mtk(s, sign=1.0)
    snaps = []
    for _ in range(30):
        whole.run(1)
        snaps.append(whole.fetch())
    assert not snaps[-1].halted and np.all(np.min([p.volume for p in snaps], axis=0) < 0.99 * snaps[0].log[0, :, 5])
    counts = [int(p.log[0, 0, 2]) for p in snaps]
    first = _evaluator(s)(s["pos"].astype(np.float32), s["cell"].astype(np.float32))[2]
    at = [k for k in range(2, 30) if counts[k] > max([first] + counts[:k])]
    assert at, "the edge count never exceeded its running maximum: no overflow to test"
    k = at[0]
    capacity = max([first] + counts[:k])
    md = _mtk(s, sign=1.0, capacity=capacity)
    assert md.capacity == capacity
    md.run(30)
    snap = md.fetch()
    assert snap.halted and snap.step == k and snap.halt_step == k and (snap.halt_code & HALT_CAPACITY)
    assert not (snap.halt_code & HALT_NONFINITE) and not snap.refused.any()
    assert _state_bits(snap) == _state_bits(snaps[k - 1]) and snap.v_cell.any() and snap.log.shape[0] == k
    assert np.array_equal(bits(snap.log), bits(np.concatenate([p.log for p in snaps[:k]])))
    md.run(3)                                            # halted: replays change nothing
    again = md.fetch()
    assert _state_bits(again) == _state_bits(snap) and again.log.shape[0] == 0 and again.halted
    md.resume()
    assert md.capacity > capacity
    md.run(30 - k)
    end = md.fetch()
    assert (end.step, end.halted) == (30, False) and _state_bits(end) == _state_bits(snaps[29])
    assert np.array_equal(bits(end.log), bits(np.concatenate([p.log for p in snaps[k:]])))
    assert np.array_equal(bits(end.mtk_factors), bits(snaps[29].mtk_factors))


def test_a_replay_is_device_npts_launch_list_with_the_six_integrator_launches_and_no_copies():
    """The device activity of two replays of `DeviceMTK` and of `DeviceNPT` on the same batch, from the captures' own lists:
    the six kernels of the step are there once per replay, `DeviceNPT`'s integrator kernels are gone, everything else is
    `DeviceNPT`'s, and there is no memcpy or memset."""
    from torch.profiler import ProfilerActivity, profile
    s = _system("batch")
    plain = DeviceNPT(rh._shared_model(), _put(s["z"]), s["cell"].astype(np.float32).astype(np.float64), s["pos"], s["m"], DT,
                      velocities=s["v"], pressure=0.0, compressibility=1e-3, batch=_put(s["batch"]), num_graphs=4)
    ours = _mtk(s)

    def events(driver):
        driver.run(2)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            driver.run(2)
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    a, b = events(ours), events(plain)
    assert sum(a.values()) > 0, "the profiler recorded no device activity for graph launches"
    assert not [k for k in a if "memcpy" in k.lower() or "memset" in k.lower()]
    named = lambda c, word: sum(v for k, v in c.items() if word in k)
    for kernel in ("mtk_open_kernel", "mtk_advance_kernel", "mtk_finish_atoms_kernel", "mtk_close_kernel", "mtk_scale_kernel",
                   "md_commit_kernel"):
        assert named(a, kernel) == 2, (kernel, a)
    assert named(b, "mtk_") == 0 and named(a, "npt_") == 0 and named(a, "md_advance_kernel") == 0
    integrator = lambda k: any(w in k for w in ("mtk_", "npt_", "md_advance_kernel", "md_finish_atoms_kernel", "md_commit_kernel",
                                                "md_log_kernel"))
    rest = lambda c: Counter({k: v for k, v in c.items() if not integrator(k)})
    assert rest(a) == rest(b), (rest(a) - rest(b), rest(b) - rest(a))
    theirs = sum(v for k, v in b.items() if integrator(k))
    print("DeviceNPT's integrator launches per replay: %d (%s); DeviceMTK's: 6" % (theirs // 2, sorted(k for k in b if integrator(k))))
    assert sum(v for k, v in a.items() if integrator(k)) == 12


class _FakeAtoms(rh._FakeAtoms):
    def set_cell(self, cell, scale_atoms=False):
        assert not scale_atoms
        self.cell = np.array(cell)


def test_ase_hand_off_round_trips_the_float64_cell():
    s = _system("single")
    cell = s["cell"][0].astype(np.float64) * (1.0 + 1e-9)                             # not representable in float32
    atoms = _FakeAtoms(s["pos"], s["z"], cell, s["m"], s["v"] * ASE_TIME_FS)
    md = DeviceMTK.from_atoms(atoms, rh._shared_model(), DT, temperature=600.0, tau=30.0, taup=TAUP, chain=2,
                              pressure=float(_start_pressure(s)[0] - 0.004))
    snap = md.fetch()
    assert md.num_graphs == 1 and md.dof.tolist() == [93.0] and snap.xi_baro.shape == (1, 2)
    assert np.array_equal(bits(snap.cell[0]), bits(cell)) and snap.step == 0 and snap.volume.shape == (1,)
    assert np.array_equal(snap.positions, s["pos"]) and np.allclose(snap.velocities, s["v"], rtol=1e-15, atol=0)
    out = _FakeAtoms(np.zeros_like(s["pos"]), s["z"], np.zeros((3, 3)), s["m"], None)
    md.to_atoms(out, snap)
    assert np.array_equal(bits(out.cell), bits(cell)) and np.array_equal(out.positions, s["pos"])
    md.run(2)
    two = md.to_atoms(out)
    assert two.step == 2 and not two.halted and np.array_equal(bits(out.cell), bits(two.cell[0]))
    assert not np.array_equal(out.cell, cell) and np.array_equal(out.positions, two.positions)
    assert np.array_equal(out.get_velocities(), two.velocities * ASE_TIME_FS) and two.log.shape == (2, 1, 7)
