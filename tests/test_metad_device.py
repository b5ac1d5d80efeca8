"""GPU: `hermnet_amd.metad.DeviceMetaD` -- multiple-walker metadynamics inside the replayed hipGraph.  The pair pass and the
library's exp against the host twins bit for bit; a biased trajectory against a host-driven loop after every step; a bias of
zero height against `DeviceMD`, with and without observers; halt at a deposit step and resume; the launch list."""
from collections import Counter

import numpy as np
import pytest
import torch

from hermnet_amd import _lib, synth
from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.md import ASE_TIME_FS, HALT_CAPACITY, DeviceMD
from hermnet_amd.metad import Coordination, DeviceMetaD, Distance, cv_tables
from hermnet_amd.observe import MSD, RDF, Frames
from md_reference import AMU, KB, advance_np, bits
from metad_reference import HostMetaD, host_cv, host_exp
from test_hostile_cells import _skew30
import test_pimd_device as pt
import test_remd_device as rt

pytestmark = pytest.mark.gpu

DT, FRICTION, SEED, T = 1.0, 0.02, (3 << 32) + 19, 2500.0          # K: hot enough that the neighbour list changes
WALKERS = 4
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _put(a):
    return torch.from_numpy(np.array(a)).to(_dev())


# ---- 1. the pair pass alone ---------------------------------------------------------------------------------------------------------
def _device_cv(cvs, B, x, image, cell):
    """hermnet_metad_cv on the device: (values [B,D], grads [D,N,3])."""
    n, D, P = len(x), len(cvs), _lib.ptr
    t = cv_tables(cvs, n // B, cell)
    cell32 = np.ascontiguousarray(np.broadcast_to(np.asarray(cell, dtype=np.float32).reshape(-1, 3, 3), (B, 3, 3)))
    d = dict(ptr=_put((np.arange(B + 1) * (n // B)).astype(np.int32)), x=_put(x), image=_put(image.astype(np.int32)),
             cell=_put(cell32), inv=_put(np.linalg.inv(cell32.astype(np.float64))), kind=_put(t.kind), par=_put(t.par),
             role=_put(t.role), weight=_put(t.weight))
    dev = _dev()
    cv_atom = torch.zeros(D, n, 6, dtype=torch.float64, device=dev)
    cv_walker = torch.zeros(B, 16, dtype=torch.float64, device=dev)
    values = torch.zeros(B, D, dtype=torch.float64, device=dev)
    grads = torch.zeros(D, n, 3, dtype=torch.float64, device=dev)
    _lib.call("hermnet_metad_cv", n, B, D, P(d["ptr"]), P(d["x"]), P(d["image"]), P(d["cell"]), P(d["inv"]), P(d["kind"]),
              P(d["par"]), P(d["role"]), P(d["weight"]), P(cv_atom), P(cv_walker), P(values), P(grads),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return values.cpu().numpy(), grads.cpu().numpy()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_rep", [1, 31, 256, 257, 600])
def test_pair_pass_equals_the_host_twin_bit_for_bit(n_rep, B):
    """hermnet_metad_cv against hermnet_host_metad_cv on the skew30 cell: values and per-atom gradients bit-equal, for walkers
    below, at and above a tile of 256 atoms (257: a one-atom tile; 600: three tiles), groups A != B (overlapping) with a
    distance beside them, and A = B."""
    _, cell, _ = _skew30(np.random.RandomState(0))
    rs = np.random.RandomState(100 * n_rep + B)
    x = rs.uniform(-0.5, 1.5, (B * n_rep, 3)) @ cell           # some atoms outside the cell: the minimum image, not the wrap
    image = rs.randint(-1, 2, (B * n_rep, 3))
    a, b = range(0, (n_rep + 1) // 2 + 1 if n_rep > 1 else 1), range(n_rep // 3, n_rep)
    every = range(n_rep)
    cases = [[Coordination(every, every, 1.6, nn=6, r_cut=2.4, mean=True)],
             [Coordination(a, b, 1.5, nn=8, r_cut=2.3), Distance(a, b, weights_a=rs.uniform(0.5, 2.0, len(a)))]]
    for cvs in cases:
        got_v, got_g = _device_cv(cvs, B, x, image, cell)
        want_v, want_g = host_cv(cvs, B, x, image, cell)
        assert np.array_equal(bits(got_v), bits(want_v)), (n_rep, B, len(cvs))
        assert np.array_equal(bits(got_g), bits(want_g)), (n_rep, B, len(cvs))
        if n_rep > 30:
            assert np.all(want_v[:, 0] > 0.0) and np.abs(want_g[0]).max() > 0.0


# ---- 2. the library's exp on the device ----------------------------------------------------------------------------------------------
def test_device_exp_through_a_one_hill_bias_equals_the_host_twin():
    """256 walkers of two atoms at 256 distances, one hill of height 1 and sigma 0.08 A at 2.0 A: V(s) of walker g IS mt_exp
    of its argument (0 down to -700 and beyond the saturation), read from the walkers' scratch rows after a prime of
    hermnet_metad_bias -- bit-equal to the host twin's rows and to hermnet_host_metad_exp of the same arguments."""
    B, dev, P = 256, _dev(), _lib.ptr
    cell = np.diag([30.0, 30.0, 30.0])
    r = 2.0 + np.concatenate([[0.0], np.linspace(1e-4, 3.2, B - 1)])
    x = np.zeros((2 * B, 3))
    x[0::2] = np.random.RandomState(2).uniform(5.0, 25.0, (B, 3))
    x[1::2] = x[0::2] + r[:, None] * np.array([0.6, 0.0, 0.8])
    hills = (np.array([[2.0]]), np.array([1.0]))
    host = HostMetaD(B, x, np.zeros_like(x), np.full(2 * B, 20.0), 1.0, cell, [Distance([0], [1])], 0.1, [0.08], 10, 300.0,
                     hills=hills, max_hills=4, log_steps=2, wrap=False)
    host.state[3] = 1
    f = np.zeros((2 * B, 3), dtype=np.float32)
    host.finish(f, energy=np.zeros(B))
    t, b = host.tables, host.bias
    d = {k: _put(getattr(host, k)) for k in ("graph_ptr", "x", "image", "cell32", "inv64", "cv_atom", "hill_count", "hill_centres",
                                             "hill_heights", "bias_forces", "cv_log")}
    d.update(kind=_put(t.kind), par=_put(t.par), role=_put(t.role), weight=_put(t.weight), sigma_par=_put(b.sigma_par), f=_put(f),
             energy=_put(np.zeros(B, dtype=np.float32)), total=_put(np.zeros(2, dtype=np.int64)))     # (kept alive past the launch)
    state, walker = _put(np.array([0, 0, 0, 1], dtype=np.int64)), torch.zeros(B, 16, dtype=torch.float64, device=dev)
    forces_b = torch.zeros(2 * B, 3, dtype=torch.float32, device=dev)
    _lib.call("hermnet_metad_bias", 2 * B, B, 1, P(d["graph_ptr"]), P(d["x"]), P(d["image"]), P(d["cell32"]), P(d["inv64"]),
              P(d["kind"]), P(d["par"]), P(d["role"]), P(d["weight"]), P(d["sigma_par"]), b.height, b.inv_kt, b.pace, b.max_hills,
              P(d["f"]), P(d["energy"]), P(d["total"]), 1 << 20, P(state), P(d["cv_atom"]), P(walker), P(d["hill_count"]),
              P(d["hill_centres"]), P(d["hill_heights"]), P(forces_b), P(d["bias_forces"]), P(d["cv_log"]), 2,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = walker.cpu().numpy()
    assert np.array_equal(bits(got), bits(host.cv_walker))
    dd = host.cv_walker[:, 0] - 2.0
    args = -((dd * dd) * b.sigma_par[0, 0])
    assert args.min() < -745.0 and args.max() >= -1e-20 and np.sum((args > -700.0) & (args < -1.0)) > 100
    assert np.array_equal(bits(got[:, 2]), bits(host_exp(args))) and got[0, 2] == 1.0 and got[-1, 2] == 0.0
    assert np.array_equal(forces_b.cpu().numpy(), host.forces_b) and np.abs(host.forces_b).max() > 1.0
    assert d["hill_count"].cpu().numpy()[0] == 1                     # a prime deposits nothing


# ---- the driver on 4 walkers x 32 atoms ------------------------------------------------------------------------------------------------
def _system():
    """Four walkers of one 32-atom alloy cell (7.2 A), spread by 0.02 A, Maxwell-Boltzmann velocities at T."""
    if "system" not in _CACHE:
        pos, cell, z = synth.fcc_alloy_atoms(reps=(2, 2, 2))
        rs = np.random.RandomState(7)
        m = np.tile(np.array([rt.MASS[int(v)] for v in z]), WALKERS)
        x = np.tile(pos, (WALKERS, 1)) + rs.normal(scale=0.02, size=(WALKERS * len(z), 3))
        v = rs.normal(size=(len(m), 3)) * np.sqrt(KB * T / (m * AMU))[:, None]
        _CACHE["system"] = dict(pos=x, z=np.tile(z, WALKERS), cell=np.tile(cell, (WALKERS, 1, 1)), m=m, v=v,
                                batch=np.repeat(np.arange(WALKERS), len(z)), n_rep=len(z), one_cell=cell)
    return _CACHE["system"]


def _cvs():
    return [Distance([0, 1], [2, 3, 4]), Coordination(range(32), range(32), 2.8, nn=6, r_cut=3.5)]


BIAS = dict(height=0.05, sigma=[0.05, 0.5], pace=2, temperature=T, bias_factor=8.0)


def _args(s):
    return (_put(s["z"]), _put(s["cell"].astype(np.float32)), s["pos"], s["m"], DT)


def _metad(friction=FRICTION, **kw):
    s = _system()
    args = dict(BIAS, friction=friction, seed=SEED, velocities=s["v"], batch=_put(s["batch"]), num_graphs=WALKERS, max_hills=512)
    args.update(kw)
    return DeviceMetaD(rt._shared_model(), *_args(s), _cvs(), args.pop("height"), args.pop("sigma"), args.pop("pace"),
                       args.pop("temperature"), **args)


def _device_noise(step, n):
    gauss = torch.zeros(n, 3, dtype=torch.float64, device=_dev())
    _lib.call("hermnet_md_noise", SEED, step, n, None, _lib.ptr(gauss), torch.cuda.current_stream().cuda_stream)
    return gauss.cpu().numpy()


@pytest.mark.parametrize("friction", [None, FRICTION], ids=["nve", "langevin"])
def test_trajectory_equals_the_host_driven_loop_bit_for_bit(friction):
    """20 steps of 4 walkers x 32 atoms (the H = 128, L = 3 model of the other drivers' tests), a distance and a coordination,
    pace 2, well-tempered, against GraphedBatchMDStep + fetch() + hermnet_host_metad_bias + hermnet_host_md_finish: positions,
    velocities, images, (biased) forces, hills, the cv_log row and the bias forces bit-equal after EVERY step.  NVE: the
    advance is hermnet_host_md_advance.  Langevin: the device's Gaussians differ from the host's in the last digits (its
    float64 log / cos / sqrt; tests/test_md_device.py), so the loop's advance is md_step.h's numpy transcription fed with the
    Gaussians of the device's own hermnet_md_noise."""
    s, dev = _system(), _dev()
    z, cell, pos, m, dt = _args(s)
    step = GraphedBatchMDStep(rt._shared_model(), z, cell, torch.from_numpy(pos.astype(np.float32)).to(dev), _put(s["batch"]), WALKERS)

    def forces(p32):
        e, f = step(torch.from_numpy(np.ascontiguousarray(p32)).to(dev))
        e, f = e.cpu().numpy().copy(), f.cpu().numpy().copy()
        ok, n = step.check()
        assert ok
        return e, f, n

    host = HostMetaD(WALKERS, pos, s["v"], m, dt, s["one_cell"], _cvs(), BIAS["height"], BIAS["sigma"], BIAS["pace"], T,
                     friction=friction, bias_factor=BIAS["bias_factor"], max_hills=512, seed=SEED, log_steps=32)
    cell_atom = host.cell32.astype(np.float64)[host.batch]
    inv_atom = host.inv.reshape(-1, 3, 3)[host.batch]

    def advance():
        if friction is None:
            return host.advance().copy()
        host.x0[:], host.v0[:], host.image0[:] = host.x, host.v, host.image
        advance_np(host.x, host.v, host.image, host.f_prev, host.kick, host.dt, host.c1[host.batch], host.sigma,
                   _device_noise(int(host.state[0]), host.n), cell_atom, inv_atom)
        host.pos32[:] = host.x.astype(np.float32)
        return host.pos32.copy()

    host.state[3] = 1                                        # the prime: biased forces of the start
    e, f, n = forces(host.advance().copy())
    host.finish(f, e, total=(n, 0))
    md = _metad(friction=friction)
    first = md.fetch()
    assert first.step == 0 and first.hill_count == 0 and np.array_equal(first.forces, host.f_prev)
    heights = []
    for k in range(20):
        e, f, n = forces(advance())
        host.finish(f, e, total=(n, 0))
        md.run(1)
        snap = md.fetch()
        assert (snap.step, snap.halted) == (k + 1, False)
        assert np.array_equal(bits(snap.positions), bits(host.x)) and np.array_equal(bits(snap.velocities), bits(host.v)), k
        assert np.array_equal(snap.images, host.image) and np.array_equal(snap.forces, host.f_prev), k
        centres, hts = host.hills()
        assert snap.hill_count == len(hts) == WALKERS * ((k + 1) // 2), k
        assert np.array_equal(bits(snap.hill_centres), bits(centres)) and np.array_equal(bits(snap.hill_heights), bits(hts)), k
        assert snap.cv_log.shape == (1, WALKERS, 4) and np.array_equal(bits(snap.cv_log[0]), bits(host.cv_log[k])), k
        assert np.array_equal(bits(snap.bias_forces), bits(host.bias_forces)), k
        heights.append(snap.cv_log[0, :, 3])
    heights = np.array(heights)
    assert np.all(heights[1::2] > 0.0) and not heights[0::2].any() and heights[-1].max() < BIAS["height"]    # tempered
    assert np.abs(snap.bias_forces).max() > 1e-3 and snap.cv_log[0, :, 2].min() > 0.0


def _state_bits(snap):
    return (bits(snap.positions).tobytes(), bits(snap.velocities).tobytes(), snap.images.tobytes(), snap.forces.tobytes(), snap.step)


def _observers():
    return [Frames(stride=3, frames=16, velocities=True, images=True), RDF(r_max=3.5, bins=35, stride=2), MSD(stride=1, rows=32)]


def _flat(entry):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in vars(entry).items()}


@pytest.mark.parametrize("observed", [False, True], ids=["plain", "observers"])
def test_zero_height_equals_device_md_bit_for_bit(observed):
    """`DeviceMetaD(height=0)` (hills of height 0 are deposited every 2 steps) against `DeviceMD` on the same batch and seed:
    positions, velocities, images, forces and the log bit-equal after 20 Langevin steps; with Frames, RDF and MSD attached,
    everything they recorded too."""
    s = _system()
    kw = dict(observers=_observers()) if observed else {}
    ours = _metad(height=0.0, **kw)
    plain = DeviceMD(rt._shared_model(), *_args(s), temperature=T, friction=FRICTION, seed=SEED, velocities=s["v"],
                     batch=_put(s["batch"]), num_graphs=WALKERS, **(dict(observers=_observers()) if observed else {}))
    ours.run(20)
    plain.run(20)
    a, b = ours.fetch(), plain.fetch()
    assert (a.step, a.halted, b.step, b.halted) == (20, False, 20, False)
    assert _state_bits(a) == _state_bits(b) and np.array_equal(bits(a.log), bits(b.log))
    assert a.hill_count == 10 * WALKERS and not a.hill_heights.any() and not a.bias_forces.any()
    assert a.cv_log.shape == (20, WALKERS, 4) and np.all(a.cv_log[:, :, 0] > 0.0) and not a.cv_log[:, :, 2:].any()
    if observed:
        assert len(a.observers) == 3 and len(a.observers[0].steps) == 7 and a.observers[1].counts.sum() > 0
        for x, y in zip(a.observers, b.observers):
            assert _flat(x) == _flat(y)


def test_halt_at_a_deposit_step_and_resume():
    """pace 1: every step deposits.  A capacity that the list outgrows at step k (from an uninterrupted run's edge column; the
    handled list-overflow halt, not a fault): the run halts there with the capacity bit, `hill_count` is that of k completed
    steps and the void step wrote no row; resume() recaptures and the run ends bit-equal to the uninterrupted one, hills,
    cv_log and bias forces included."""
    base = _metad(pace=1)
    _, n0 = base.step.check()
    base.run(30)
    end = base.fetch()
    assert end.step == 30 and not end.halted and end.hill_count == 30 * WALKERS
    counts = end.log[:, 0, 2].astype(int).tolist()
    at = [k for k in range(2, 30) if counts[k] > max([int(n0)] + counts[:k])]
    assert at, "the edge count never exceeded its running maximum: no overflow to test"
    k = at[0]
    capacity = max([int(n0)] + counts[:k])
    md = _metad(pace=1, capacity=capacity)
    md.run(30)
    snap = md.fetch()
    assert snap.halted and snap.step == k and snap.halt_step == k and (snap.halt_code & HALT_CAPACITY)
    assert snap.hill_count == k * WALKERS and snap.cv_log.shape[0] == k
    assert np.array_equal(bits(snap.hill_centres), bits(end.hill_centres[:k * WALKERS]))
    assert np.array_equal(bits(snap.cv_log), bits(end.cv_log[:k]))
    md.run(3)                                                # halted: replays change nothing
    again = md.fetch()
    assert _state_bits(again) == _state_bits(snap) and again.hill_count == k * WALKERS and again.cv_log.shape[0] == 0
    md.resume()
    assert md.capacity > capacity
    md.run(30 - k)
    last = md.fetch()
    assert (last.step, last.halted) == (30, False) and _state_bits(last) == _state_bits(end)
    assert last.hill_count == end.hill_count and np.array_equal(bits(last.hill_centres), bits(end.hill_centres))
    assert np.array_equal(bits(last.hill_heights), bits(end.hill_heights))
    assert np.array_equal(bits(last.cv_log), bits(end.cv_log[k:])) and np.array_equal(bits(last.bias_forces), bits(end.bias_forces))


def test_run_refuses_to_overflow_the_hill_list():
    md = _metad(max_hills=3 * WALKERS)
    md.run(6)                                                # three deposits of four
    with pytest.raises(RuntimeError, match="max_hills=12"):
        md.run(2)
    md.run(1)
    assert md.fetch().hill_count == 12


def test_one_walker_on_a_single_structure_and_the_ase_hand_off():
    """`batch=None` is B = 1, ordinary metadynamics on a `GraphedMDStep`: 6 steps run, deposit and log; the same through
    `from_atoms` (one structure replicated into walkers, or the list of the walkers) and back through `to_atoms`."""
    s, n_rep = _system(), _system()["n_rep"]
    parts = [slice(g * n_rep, (g + 1) * n_rep) for g in range(WALKERS)]
    one = pt._FakeAtoms(s["pos"][parts[0]], s["z"][parts[0]], s["one_cell"], s["m"][parts[0]], s["v"][parts[0]] * ASE_TIME_FS)
    bias = (_cvs(), BIAS["height"], BIAS["sigma"], BIAS["pace"], T)
    kw = dict(friction=FRICTION, bias_factor=BIAS["bias_factor"], seed=SEED, max_hills=64)
    single = DeviceMetaD(rt._shared_model(), _put(s["z"][parts[0]]), _put(s["one_cell"].astype(np.float32)), s["pos"][parts[0]],
                         s["m"][parts[0]], DT, *bias, velocities=s["v"][parts[0]], **kw)
    assert single.num_graphs == 1 and single.n_rep == n_rep and single.batch is None
    single.run(6)
    a = single.fetch()
    assert (a.step, a.halted, a.hill_count) == (6, False, 3) and a.cv_log.shape == (6, 1, 4) and np.abs(a.bias_forces).max() > 0
    same = DeviceMetaD.from_atoms(one, rt._shared_model(), DT, *bias, walkers=1, **kw)
    same.run(6)
    b = same.fetch()
    assert np.allclose(b.positions, a.positions, rtol=0, atol=1e-9) and b.hill_count == 3     # (velocities went through ASE's unit)
    members = [pt._FakeAtoms(s["pos"][p], s["z"][p], s["one_cell"], s["m"][p], s["v"][p] * ASE_TIME_FS) for p in parts]
    md = DeviceMetaD.from_atoms(members, rt._shared_model(), DT, *bias, **kw)
    start = md.fetch()
    assert md.num_graphs == WALKERS and np.array_equal(start.positions, s["pos"])
    assert np.allclose(start.velocities, s["v"], rtol=1e-15, atol=0)
    out = [pt._FakeAtoms(np.zeros((n_rep, 3)), s["z"][p], s["one_cell"], s["m"][p], None) for p in parts]
    assert md.to_atoms(out, start) is start
    for g, p in enumerate(parts):
        assert np.array_equal(out[g].positions, s["pos"][p])
        assert np.allclose(out[g].get_velocities(), s["v"][p] * ASE_TIME_FS, rtol=1e-15, atol=0)
    with pytest.raises(ValueError, match="list of 4 walkers"):
        md.to_atoms(out[:3], start)
    with pytest.raises(ValueError, match="list of the B walkers"):
        DeviceMetaD.from_atoms(members, rt._shared_model(), DT, *bias, walkers=3)


def test_a_replay_has_the_launches_of_a_device_md_replay_plus_four_and_no_copies():
    """The device activity of two replays of `DeviceMetaD` and of `DeviceMD` (Langevin) on the same batch, from the
    captures' own lists: DeviceMD's launches plus exactly four per replay -- the per-atom CV pass, the walkers, the apply, the
    deposit -- and no memcpy or memset."""
    from torch.profiler import ProfilerActivity, profile
    s = _system()
    plain = DeviceMD(rt._shared_model(), *_args(s), temperature=T, friction=FRICTION, seed=SEED, velocities=s["v"],
                     batch=_put(s["batch"]), num_graphs=WALKERS)
    ours = _metad()

    def events(driver):
        driver.run(2)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            driver.run(2)
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    a, b = events(ours), events(plain)
    assert sum(a.values()) > 0, "the profiler recorded no device activity for graph launches"
    assert sum(a.values()) == sum(b.values()) + 8, (a - b, b - a)
    assert not [k for k in a if "memcpy" in k.lower() or "memset" in k.lower()]
    named = lambda c, word: sum(v for k, v in c.items() if word in k)
    for kernel in ("metad_cv_kernel", "metad_walker_kernel", "metad_apply_kernel", "metad_deposit_kernel"):
        assert named(a, kernel) == 2 and named(b, kernel) == 0, kernel
    assert named(a, "metad_") == 8 and a - b == Counter({k: v for k, v in a.items() if "metad_" in k})
