"""GPU: `hermnet_amd.neb.DeviceNEB` -- climbing-image NEB inside the replayed hipGraph -- against the host-driven loop it
replaces (the numpy float64 transcription of tests/neb_reference.py around a plain `GraphedBatchMDStep`), bit for bit after
every evaluation; the three kernels of hermnet_neb_finish against the library's host twin, the scalars that come out of `/`
and sqrt included; end points that never move; the halt-and-resume protocol; convergence; the ASE hand-off; the refusals.

Why bit for bit can be asked: replayed forces equal the plain step's forces bit for bit (tests/test_md_device.py relies on
the same), and the band's arithmetic is contraction-free IEEE float64 in one documented order (tests/test_neb_host.py checks
the transcription on the host twin)."""
import numpy as np
import pytest
import torch

from hermnet_amd import _lib, neb as neb_module, synth
from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.md import HALT_CAPACITY
from hermnet_amd.neb import DeviceNEB
from hermnet_amd._resident import PARKED
from neb_reference import HostNEB, NumpyNEB, bits, layout
from resident_helpers import _shared_model

pytestmark = pytest.mark.gpu

STEPS = 20
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _band(reps, images, seeds):
    """One band: an fcc alloy cell rattled with two seeds as the end points (not wrapped: the band is continuous), the
    images between by linear interpolation.  (pos [images*n,3], cell [images,3,3], z [images*n])."""
    lattice, cell, z = synth.fcc_alloy_atoms(reps=reps, sigma=0.0, seed=seeds[0])
    ends = [lattice + np.random.RandomState(100 + s).normal(scale=0.08, size=lattice.shape) for s in seeds]
    path = neb_module.interpolate(ends[0], ends[1], images)
    return path.reshape(-1, 3), np.tile(cell, (images, 1, 1)), np.tile(z, images)


def _system(name):
    """`one`: 5 images of 32 atoms; `two`: that band and 4 images of 48 atoms."""
    if ("system", name) not in _CACHE:
        parts = [_band((2, 2, 2), 5, (1, 2))] + ([_band((2, 2, 3), 4, (3, 4))] if name == "two" else [])
        sizes, images = ([32, 48], [5, 4]) if name == "two" else ([32], [5])
        graph_ptr, band_ptr, band_of, batch = layout(sizes, images)
        _CACHE[("system", name)] = dict(pos=np.concatenate([p[0] for p in parts]), cell=np.concatenate([p[1] for p in parts]),
                                        z=np.concatenate([p[2] for p in parts]), batch=batch, B=len(band_of), graph_ptr=graph_ptr,
                                        band_ptr=band_ptr, K=len(images))
    return _CACHE[("system", name)]


def _tensors(s):
    dev = _dev()
    return (torch.from_numpy(s["z"]).to(dev), torch.from_numpy(s["cell"].astype(np.float32)).to(dev),
            torch.from_numpy(s["batch"]).to(dev))


def _device_neb(s, **kw):
    z, cell, batch = _tensors(s)
    kw.setdefault("band_ptr", s["band_ptr"])
    return DeviceNEB(_shared_model(), z, cell, s["pos"], batch=batch, num_graphs=s["B"], **kw)


RECORDED = ("x", "v", "f_prev", "gf", "gi", "obs", "climber", "state")


def _reference(name, fmax=1e-6, steps=STEPS):
    """The host-driven loop DeviceNEB replaces, computed once per (system, fmax): NumpyNEB, each evaluation's energies and
    forces from a plain graphed batch step on float32(x).  (system, the NumpyNEB at the end, per-evaluation records)."""
    key = ("reference", name, fmax, steps)
    if key not in _CACHE:
        s, dev = _system(name), _dev()
        z, cell, batch = _tensors(s)
        step = GraphedBatchMDStep(_shared_model(), z, cell, torch.from_numpy(s["pos"].astype(np.float32)).to(dev), batch, s["B"])
        ref = NumpyNEB(s["pos"], s["graph_ptr"], s["band_ptr"], k=0.1, fmax=fmax, climb=True)
        hist = []
        for _ in range(steps):
            e, f = step(torch.from_numpy(ref.advance()).to(dev))
            e, f = e.cpu().numpy().copy(), f.cpu().numpy().copy()
            ok, n = step.check()
            assert ok
            ref.finish(f, e, total=(n, 0))
            rec = {k: getattr(ref, k).copy() for k in RECORDED}
            rec["n"] = n
            hist.append(rec)
        _CACHE[key] = (s, ref, hist)
    return _CACHE[key]


def _equals(snap, rec, s):
    """A fetched snapshot against a record of the reference, bit for bit."""
    lead = s["band_ptr"][:-1] + 1
    gf, gi, obs = rec["gf"], rec["gi"], rec["obs"]
    assert np.array_equal(bits(snap.positions), bits(rec["x"])) and np.array_equal(bits(snap.velocities), bits(rec["v"]))
    assert np.array_equal(snap.forces, rec["f_prev"]) and not snap.images.any()
    for c, name in enumerate(("dt", "a", "scale", "fmax")):
        assert np.array_equal(bits(getattr(snap, name)), bits(gf[lead, c])), name
    assert np.array_equal(snap.nsteps, gi[lead, 0]) and np.array_equal(snap.converged, gi[lead, 2] != 0)
    assert np.array_equal(snap.converged_step, gi[lead, 3]) and np.array_equal(snap.climbing_image, rec["climber"])
    for c, name in enumerate(("energy", "image_fmax", "segment", "tangential_force")):
        assert np.array_equal(bits(getattr(snap, name)), bits(obs[:, c])), name
    assert snap.step == rec["state"][0] and snap.done == bool(rec["state"][3])
    return True


def _state_bits(snap):
    return tuple(bits(getattr(snap, k)).tobytes() for k in ("positions", "velocities", "dt", "a", "scale", "fmax", "energy",
                                                            "image_fmax", "segment", "tangential_force")) + (
        snap.forces.tobytes(), snap.nsteps.tobytes(), snap.converged.tobytes(), snap.converged_step.tobytes(),
        snap.climbing_image.tobytes(), snap.step, snap.done)


def test_device_kernels_equal_the_host_twin():
    """Two advance + finish through hermnet_relax_advance / hermnet_neb_finish and through the host twins on the same random
    inputs: a band of 4 images of 257 atoms (fresh), one of 5 images of 63 atoms (mid-run, with velocities) and one of 3
    images of 1 atom (converges at the first evaluation) -- lanes with 2, 1 and 0 atoms, an image below one wave; held atoms.
    Every array bit-equal, scratch included: the per-image scalars out of `/` and sqrt (obs), the band's out of FIRE (gf)."""
    dev, lib, P = _dev(), _lib.load(), _lib.ptr
    sizes, images = (257, 63, 1), (4, 5, 3)
    graph_ptr, band_ptr, band_of, batch = layout(sizes, images)
    n, B = int(graph_ptr[-1]), len(band_of)
    rs = np.random.RandomState(23)
    x = np.concatenate([np.tile(rs.uniform(0.0, 9.0, (m, 3)), (c, 1)) for m, c in zip(sizes, images)])
    x = x + np.repeat(np.arange(B), np.diff(graph_ptr))[:, None] * np.array([0.3, -0.2, 0.1]) + rs.normal(scale=0.05, size=(n, 3))
    fixed = np.zeros(n, dtype=bool)
    fixed[graph_ptr[:4] + 256] = fixed[graph_ptr[4:9] + 7] = True
    host = HostNEB(x, graph_ptr, band_ptr, fixed=fixed, k=[0.1, 0.25, 0.1], fmax=[0.05, 0.05, 1e3], climb=True, log_steps=4)
    inner1 = np.arange(band_ptr[1] + 1, band_ptr[2] - 1)
    a, b = graph_ptr[inner1[0]], graph_ptr[inner1[-1] + 1]
    host.v[a:b] = rs.normal(scale=0.2, size=(b - a, 3))
    host.v[fixed] = 0.0
    host.gf[inner1, :4] = [0.3, 0.09, 0.02, 1.0]
    host.gi[inner1] = [7, 0, 0, -1]
    host.state[0] = 6                                                                # (log slots 2 and 3)
    names = ["x", "x0", "v", "image", "image0", "f_prev", "fixed", "batch", "pos32", "state", "gf", "gi", "obs", "climber", "g",
             "isum", "csum", "bf_new", "bi_new", "climber_new", "log", "graph_ptr", "band_ptr", "band_of", "k", "fmax"]
    d = {k: torch.from_numpy(getattr(host, k).copy()).to(dev) for k in names}
    stream = torch.cuda.current_stream().cuda_stream
    start = host.x.copy()
    for it in range(2):
        f = rs.normal(scale=2.0, size=(n, 3)).astype(np.float32)
        e = rs.normal(size=B).astype(np.float32)
        tot = np.array([4321 + it, 0], dtype=np.int64)
        f_d, e_d, t_d = (torch.from_numpy(t).to(dev) for t in (f, e, tot))
        _lib.check(lib.hermnet_relax_advance(n, B, 0, P(d["x"]), P(d["x0"]), P(d["v"]), P(d["image"]), P(d["image0"]),
                                             P(d["fixed"]), P(d["batch"]), None, None, P(d["pos32"]), P(d["state"]), P(d["gf"]),
                                             P(d["gi"]), stream), "advance")
        _lib.check(lib.hermnet_neb_finish(n, B, host.K, 1, P(d["graph_ptr"]), P(d["band_ptr"]), P(d["band_of"]), P(f_d), P(e_d),
                                          P(t_d), 5000, host.dt0, host.dtmax, host.maxstep, P(d["k"]), P(d["fmax"]), P(d["x"]),
                                          P(d["v"]), P(d["x0"]), P(d["image"]), P(d["image0"]), P(d["f_prev"]), P(d["fixed"]),
                                          P(d["pos32"]), P(d["gf"]), P(d["gi"]), P(d["obs"]), P(d["climber"]), P(d["g"]),
                                          P(d["isum"]), P(d["csum"]), P(d["bf_new"]), P(d["bi_new"]), P(d["climber_new"]),
                                          P(d["log"]), host.log_steps, P(d["state"]), stream), "finish")
        torch.cuda.synchronize()
        host.advance()
        host.finish(f, e, total=tot, capacity=5000)
        got = {k: d[k].cpu().numpy() for k in names}
        assert got["state"].tolist() == host.state.tolist() == [7 + it, 0, 0, 0]
        for key in ("x", "x0", "v", "gf", "obs", "g", "isum", "csum", "bf_new", "log"):
            assert np.array_equal(bits(got[key]), bits(getattr(host, key))), (it, key)
        for key in ("image", "f_prev", "gi", "bi_new", "climber", "climber_new", "pos32"):
            assert np.array_equal(got[key], getattr(host, key)), (it, key)
    # the inputs did reach: a fresh start, a band in mid-run, one that converged; end points and held atoms stayed
    lead = band_ptr[:-1] + 1
    assert host.gi[lead[2], 2:].tolist() == [1, 6] and host.gi[lead[0], 1] == 0 and host.gi[lead[1], 1] == 0
    assert np.all(host.obs[1:3, 1] > 0.0) and np.all(host.obs[1:3, 2] > 0.0) and np.all(host.climber >= 1)
    ends = np.concatenate([band_ptr[:-1], band_ptr[1:] - 1])
    still = fixed | np.isin(np.repeat(np.arange(B), np.diff(graph_ptr)), ends)
    assert np.array_equal(bits(host.x[still]), bits(start[still])) and np.abs(host.x[~still][:-1] - start[~still][:-1]).min() > 0.0
    assert np.all(got["log"][:2] == -7.0) and np.all(got["log"][2:, :, 3] == [[4321], [4322]])


@pytest.mark.parametrize("name", ["one", "two"])
def test_trajectory_equals_the_host_driven_loop_bit_for_bit(name):
    """20 replays, fetched after every one, against NumpyNEB around a plain graphed batch step: positions, velocities,
    forces, the bands' state, the images' observables and every log row; the end points hold the bits they were given."""
    s, ref, hist = _reference(name)
    nb = _device_neb(s, fmax=1e-6)
    ends = np.isin(s["batch"], np.concatenate([s["band_ptr"][:-1], s["band_ptr"][1:] - 1]))
    for it in range(STEPS):
        nb.run(1)
        snap = nb.fetch()
        assert _equals(snap, hist[it], s) and not snap.halted, it
        assert snap.log.shape == (1, s["B"], 4) and np.array_equal(bits(snap.log[0]), bits(ref.log[it])), it
        assert np.all(snap.log[0, :, 3] == hist[it]["n"])
    assert np.array_equal(bits(snap.positions[ends]), bits(s["pos"][ends]))
    assert not np.array_equal(snap.positions[~ends], s["pos"][~ends])
    assert np.all(snap.climbing_image >= 1) and not snap.done
    assert np.all(snap.fmax < hist[0]["gf"][s["band_ptr"][:-1] + 1, 3])              # FIRE did something: the NEB force fell


def test_halt_on_a_capacity_too_small_and_resume():
    """After 7 evaluations the step is recaptured with fewer columns than the list has pairs: the next replay halts with
    code 4 in the state of evaluation 6 (the void move taken back), later replays change nothing; resume() recaptures with
    more columns and the run ends on the reference's bits."""
    s, ref, hist = _reference("one")
    nb = _device_neb(s, fmax=1e-6)
    nb.run(7)
    assert _equals(nb.fetch(), hist[6], s)
    small = min(rec["n"] for rec in hist) - 1
    nb.state[1].fill_(PARKED)
    nb.step.recapture(capacity=small)
    nb._unpark()
    assert nb.capacity == small
    for _ in range(2):
        nb.run(3)
        snap = nb.fetch()
        assert snap.halted and (snap.halt_code & HALT_CAPACITY) and snap.halt_code < 256
        assert snap.step == snap.halt_step == 7 and snap.log.shape[0] == 0
        assert _equals(snap, hist[6], s)
    nb.resume()
    assert nb.capacity > small
    nb.run(STEPS - 7)
    end = nb.fetch()
    assert _equals(end, hist[-1], s) and not end.halted and end.log.shape[0] == STEPS - 7
    assert np.array_equal(bits(end.log), bits(np.stack(ref.log[7:])))


def test_a_huge_fmax_converges_at_once():
    """fmax far above any force: both bands converge at evaluation 0, nothing has moved, further replays change nothing
    and log nothing."""
    s = _system("two")
    nb = _device_neb(s, fmax=1e6)
    nb.run(3)
    snap = nb.fetch()
    assert snap.done and snap.step == 1 and snap.converged.all() and snap.converged_step.tolist() == [0, 0]
    assert snap.log.shape[0] == 1 and np.array_equal(bits(snap.positions), bits(s["pos"])) and not snap.velocities.any()
    assert np.all(snap.scale == 0.0) and np.all(np.isfinite(snap.energy)) and np.all(snap.fmax > 0.0)
    nb.run(2)
    again = nb.fetch()
    assert _state_bits(again) == _state_bits(snap) and again.log.shape[0] == 0
    assert nb.run_until(10).step == 1


class _FakeAtoms(object):
    """What `from_atoms` / `to_atoms` touch of an ase.Atoms."""

    def __init__(self, positions, numbers, cell, pbc=True):
        self.positions, self.numbers, self.cell, self.pbc = positions.copy(), numbers, cell, np.array([pbc] * 3)


def test_ase_hand_off():
    """from_atoms on the list of a band's duck-typed images is the band; to_atoms writes every image's positions back."""
    s, _, hist = _reference("one")
    ptr = s["graph_ptr"]
    images = [_FakeAtoms(s["pos"][a:b], s["z"][a:b], s["cell"][g]) for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:]))]
    nb = DeviceNEB.from_atoms(images, _shared_model(), fmax=1e-6)
    assert nb.num_graphs == 5 and nb.num_bands == 1 and nb.n == len(s["z"])
    start = nb.fetch()
    assert np.array_equal(start.positions, s["pos"]) and start.step == 0 and not start.halted and not start.done
    nb.run(3)
    snap = nb.to_atoms(images)
    assert _equals(snap, hist[2], s)
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        assert np.array_equal(images[g].positions, hist[2]["x"][a:b])
    with pytest.raises(ValueError, match="do not match"):
        nb.to_atoms(images[:2], snap)
    with pytest.raises(ValueError, match="list"):
        DeviceNEB.from_atoms(images[0], _shared_model())


def test_refusals():
    """ValueError, naming the band, before anything is captured: a band of two images, images that differ, a periodic band
    that is not continuous across a cell face."""
    s = _system("two")
    z, cell, batch = _tensors(s)
    model = _shared_model()
    with pytest.raises(ValueError, match="band 1 has 2 images"):
        DeviceNEB(model, z, cell, s["pos"], batch=batch, num_graphs=s["B"], band_ptr=[0, 7, 9])
    with pytest.raises(ValueError, match="band 0: image 5 differs"):
        DeviceNEB(model, z, cell, s["pos"], batch=batch, num_graphs=s["B"])          # one band of all nine: 32 against 48
    z2 = z.clone()
    z2[40] = 13 if int(z2[40]) != 13 else 28
    with pytest.raises(ValueError, match="band 0: image 1 differs"):
        DeviceNEB(model, z2, cell, s["pos"], batch=batch, num_graphs=s["B"], band_ptr=s["band_ptr"])
    pos = s["pos"].copy()
    pos[32 * 5 + 48 * 2 + 3] += s["cell"][6][0]                                       # an atom of band 1's image 2, a cell over
    with pytest.raises(ValueError, match="band 1: images 1 and 2 are not continuous"):
        DeviceNEB(model, z, cell, pos, batch=batch, num_graphs=s["B"], band_ptr=s["band_ptr"])
    with pytest.raises(ValueError, match="batch"):
        DeviceNEB(model, z[:32], cell[0], s["pos"][:32])
