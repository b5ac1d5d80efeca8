"""CPU: the device-resident FIRE relaxation (hermnet_amd/csrc/relax_kernels.hip, relax_step.h) through its host twins -- the
step against a numpy float64 transcription bit for bit (canonical reduction order included), every branch of the optimiser,
ASE's semantics against a textbook FIRE, the independence of the graphs of a batch, fixed atoms, the void step and the
argument refusals.  No GPU: hermnet_host_relax_advance / _finish run the text the kernels run."""
import numpy as np
import pytest

from hermnet_amd import _lib
from relax_reference import HostRelax, NumpyRelax, _p, bits, lennard_jones, same_state, textbook_fire, wells

TRICLINIC = np.array([[19.3, 0.4, -0.7], [2.1, 21.2, 0.3], [-1.6, 3.3, 24.9]])
SIZES = [1, 255, 257, 600, 0]                 # one atom, a lane short of a row, a lane over, three rows; an empty graph
AMPLITUDES = [0.05, 0.3, 0.3, 0.3, 0.0]
CAP = 200
_CACHE = {}


def _batch_system():
    """Four graphs in wells + an empty one, triclinic cells, a third of the atoms starting outside their cell."""
    if "batch" not in _CACHE:
        cells = np.stack([TRICLINIC * s for s in (1.0, 1.1, 0.9, 1.2, 1.0)])
        parts = [wells(n, 10 + g, AMPLITUDES[g], cell=cells[g], outside=True) for g, n in enumerate(SIZES)]
        x = np.concatenate([p[0] for p in parts])
        batch = np.repeat(np.arange(len(SIZES)), SIZES)
        ptr = np.concatenate([[0], np.cumsum(SIZES)])

        def force(pos32):
            return np.concatenate([parts[g][1](pos32[ptr[g]:ptr[g + 1]]) for g in range(len(SIZES))]).astype(np.float32)

        _CACHE["batch"] = (x, cells, batch, ptr, force, parts)
    return _CACHE["batch"]


def _drive(opt, force, evaluations, every=None):
    for k in range(evaluations):
        opt.finish(force(opt.advance()))
        if every is not None:
            every(k)


def _batch_run():
    """The batch relaxed by the host twin and by NumpyRelax side by side, compared after every evaluation; the histories."""
    if "run" not in _CACHE:
        x, cells, batch, ptr, force, _ = _batch_system()
        host = HostRelax(x, cell=cells, batch=batch, num_graphs=len(SIZES))
        ref = NumpyRelax(x, cell=cells, batch=batch, num_graphs=len(SIZES))
        hist = []

        def both(k):
            ref.finish(force(ref.advance()))
            same_state(host, ref)
            assert np.array_equal(bits(host.log[k]), bits(ref.log[k])) and np.array_equal(host.f_prev, ref.f)
            hist.append(dict(x=host.x.copy(), gf=host.gf.copy(), gi=host.gi.copy(), state=host.state.copy()))

        for k in range(CAP):
            host.finish(force(host.advance()))
            both(k)
            if host.state[3]:
                break
        _CACHE["run"] = (host, ref, hist)
    return _CACHE["run"]


def test_host_twin_equals_the_numpy_transcription_bit_for_bit():
    """x, v, image, pos32, per-graph dt / a / scale / nsteps / converged, the log and the state words after EVERY evaluation
    of the whole relaxation (asserted inside _batch_run); atoms did start outside their cells; all graphs converge."""
    host, ref, hist = _batch_run()
    assert host.state[3] == 1 and np.all(host.gi[:, 2] == 1), "a graph had not converged after %d evaluations" % CAP
    assert np.abs(host.image).max() >= 1
    assert np.all(host.log[len(hist):] == -7.0)                     # no row beyond the evaluations made


def test_the_run_passes_through_every_branch():
    """From the numpy twin's record of what each evaluation did (its state was bit-equal to the host twin's throughout):
    the fresh first step, the uphill reset, the growth behind nsteps > Nmin, dt near dtmax, the maxstep clamp."""
    _, ref, hist = _batch_run()
    for g in (1, 2, 3):
        modes = [m[g] for m in ref.modes]
        assert modes[0] == "fresh" and "fresh" not in modes[1:]
        assert modes.count("stop") >= 1 and modes.count("mix") > 6, (g, modes)
        dts = np.array([row[g, 2] for row in ref.log])
        assert np.any(dts[1:] > dts[:-1] * 1.05)                      # growth
        assert np.any(dts[1:] == 0.5 * dts[:-1])                      # the uphill reset halves it
        assert dts.max() > 0.1 * 1.1 ** 4
        assert any(c[g] for c in ref.clamped) and not all(c[g] for c in ref.clamped)
    # dt reaches dtmax on a long downhill slide: one atom, far up a soft well
    x, force = np.array([[3.0, 0.0, 0.0]]), lambda p: (-0.01 * p.astype(np.float64)).astype(np.float32)
    host, ref = HostRelax(x, fmax=1e-3), NumpyRelax(x, fmax=1e-3)
    for _ in range(60):
        host.finish(force(host.advance()))
        ref.finish(force(ref.advance()))
        same_state(host, ref)
    assert np.max([row[0, 2] for row in ref.log]) == 1.0


@pytest.mark.parametrize("name", ["wells", "lj"])
def test_semantics_are_ases(name):
    """One graph: the twin converges at the same evaluation as the textbook FIRE and evaluates forces within 1e-9 A of its
    positions at every step (they differ in summation order and in where the clamp's scale is applied)."""
    if name == "wells":
        x, force = wells(32, 3, 0.3)
        cell = None
    else:
        x, cell, force = lennard_jones((2, 2, 2), 5)
    count, path = textbook_fire(x, force, cap=CAP)
    assert count is not None and 10 < count <= CAP
    host = HostRelax(x, cell=cell, wrap=False)
    for k in range(count):
        host.advance()
        assert np.abs(host.x - path[k]).max() <= 1e-9, k
        host.finish(force(host.pos32))
        assert bool(host.state[3]) == (k == count - 1), k
    assert host.gi[0, 3] == count - 1 and host.state[0] == count


def test_graphs_of_a_batch_relax_independently():
    """Each graph's trajectory and converged step equal, bit for bit, those of the same graph relaxed alone; the graphs
    converge at different steps; a converged graph's x never changes again; done is set exactly when the last converges and
    later calls change nothing."""
    x, cells, batch, ptr, force, parts = _batch_system()
    host, _, hist = _batch_run()
    conv = host.gi[:, 3]
    assert conv[4] == 0 and len(set(conv[:4].tolist())) > 1
    assert len(hist) == conv.max() + 1 and all(h["state"][3] == 0 for h in hist[:-1]) and hist[-1]["state"][3] == 1
    for g in range(4):
        a, b = ptr[g], ptr[g + 1]
        alone = HostRelax(x[a:b], cell=cells[g])
        for k in range(conv[g] + 1):
            alone.finish(parts[g][1](alone.advance()))
            assert np.array_equal(bits(alone.x), bits(hist[k]["x"][a:b])), (g, k)
            assert np.array_equal(bits(alone.gf[0, :4]), bits(hist[k]["gf"][g, :4]))
        assert alone.state[3] == 1 and alone.gi[0, 3] == conv[g]
        for k in range(conv[g], len(hist)):                             # frozen from its converged step on
            assert np.array_equal(bits(hist[k]["x"][a:b]), bits(hist[conv[g]]["x"][a:b]))
    before = (host.x.copy(), host.v.copy(), host.gf.copy(), host.gi.copy(), host.state.copy(), host.log.copy(), host.pos32.copy())
    for _ in range(3):
        host.finish(force(host.advance()) + 1.0)
    after = (host.x, host.v, host.gf, host.gi, host.state, host.log, host.pos32)
    assert all(np.array_equal(p, q) for p, q in zip(before, after))


def test_fixed_atoms():
    """A fixed atom under a large force never moves, does not enter fmax, P, ff, vv, and does not delay convergence: the
    run equals, bit for bit, the run of the same system with that atom's force set to zero."""
    x, force = wells(48, 7, 0.3)
    fixed = np.zeros(48, dtype=bool)
    fixed[[5, 47]] = True

    def pushed(p):
        f = force(p)
        f[fixed] = 50.0
        return f

    def zeroed(p):
        f = force(p)
        f[fixed] = 0.0
        return f

    a, b, ref = HostRelax(x, fixed=fixed), HostRelax(x, fixed=fixed), NumpyRelax(x, fixed=fixed)
    for k in range(CAP):
        a.finish(pushed(a.advance()))
        b.finish(zeroed(b.advance()))
        ref.finish(pushed(ref.advance()))
        same_state(a, ref)
        assert np.array_equal(bits(a.x), bits(b.x)) and np.array_equal(bits(a.gf[:, :4]), bits(b.gf[:, :4]))
        assert np.array_equal(bits(a.x[fixed]), bits(x[fixed])) and not a.v[fixed].any()
        if a.state[3]:
            break
    assert a.state[3] == 1 and a.gf[0, 3] < 0.05 and 10 < k < 100


@pytest.mark.parametrize("what", ["flags", "capacity", "nan"])
def test_void_step(what):
    """List flags, found > capacity or a NaN energy: x, image and pos32 return to the start of the step, v and the per-graph
    state stay, the halt code and step are recorded, no log row is written, later calls are no-ops."""
    x, cells, batch, ptr, force, _ = _batch_system()
    host = HostRelax(x, cell=cells, batch=batch, num_graphs=len(SIZES))
    _drive(host, force, 6)
    keep = {k: getattr(host, k).copy() for k in ("x", "v", "image", "pos32", "gf", "gi", "log", "f_prev")}
    moved = host.advance().copy()
    assert not np.array_equal(moved, keep["pos32"])
    energy = np.zeros(len(SIZES), dtype=np.float32)
    total, capacity, code = (100, 0), 1 << 30, 0
    if what == "flags":
        total, code = (100, 2), 2
    elif what == "capacity":
        total, capacity, code = (101, 0), 100, 4
    else:
        energy[2], code = np.nan, 256
    host.finish(force(moved), energy=energy, total=total, capacity=capacity)
    assert host.state.tolist() == [6, code, 6, 0]
    for k, want in keep.items():
        assert np.array_equal(getattr(host, k), want, equal_nan=True), k
    host.finish(force(host.advance()))                               # halted: nothing
    assert host.state.tolist() == [6, code, 6, 0]
    for k, want in keep.items():
        assert np.array_equal(getattr(host, k), want, equal_nan=True), k
    # the halt cleared (what resume() does): the run repeats the void move and ends where the unhalted run ends
    host.state[1:3] = 0
    straight = HostRelax(x, cell=cells, batch=batch, num_graphs=len(SIZES))
    _drive(straight, force, 12)
    _drive(host, force, 6)
    assert np.array_equal(bits(host.x), bits(straight.x)) and np.array_equal(bits(host.gf), bits(straight.gf))


@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
@pytest.mark.parametrize("n", [0, 1, 256, 257, 513])
def test_one_graph_on_both_sides_of_the_lane_boundary(n, wrap):
    """No atom, one, a full row of 256 lanes, one over, two rows and one: twelve evaluations bit-equal to the numpy
    transcription (state, log rows, accepted forces), with the wrap and without."""
    x, force = wells(n, 40 + n, 0.3, cell=TRICLINIC, outside=True)
    host, ref = HostRelax(x, cell=TRICLINIC, wrap=wrap), NumpyRelax(x, cell=TRICLINIC, wrap=wrap)
    for k in range(12):
        host.finish(force(host.advance()), energy=[0.25 * k], total=(3 * k, 0))
        ref.finish(force(ref.advance()), energy=[0.25 * k], total=(3 * k, 0))
        same_state(host, ref)
        if k < len(ref.log):
            assert np.array_equal(bits(host.log[k]), bits(ref.log[k])) and np.array_equal(host.f_prev, ref.f)
    assert np.all(host.log[len(ref.log):] == -7.0)
    assert bool(host.image.any()) == (wrap and n > 0)
    assert host.state[0] == len(ref.log) and (n > 0 or host.state.tolist() == [1, 0, 0, 1])


ORTHO = np.diag([18.0, 19.0, 20.0])
HOSTILE_SIZES = (40, 0, 70)
HELD = 45


def _hostile_batch(broken=True, wrap=True):
    """Three graphs, the middle one empty, a triclinic and an orthogonal cell, one held atom under a large force; graph 0
    starts so close to its minimum that it converges at the first evaluation.  `broken`: the first and the last `batch`
    entry out of range on either side (the library clamps them to the graphs they belong to)."""
    cells = np.stack([TRICLINIC, ORTHO, ORTHO])
    near, f_near = wells(HOSTILE_SIZES[0], 31, 0.002, cell=cells[0], outside=True)
    far, f_far = wells(HOSTILE_SIZES[2], 32, 0.3, cell=cells[2], outside=True)
    x, batch = np.concatenate([near, far]), np.repeat([0, 1, 2], HOSTILE_SIZES)
    fixed = np.zeros(len(x), dtype=bool)
    fixed[HELD] = True

    def force(pos32):
        f = np.concatenate([f_near(pos32[:HOSTILE_SIZES[0]]), f_far(pos32[HOSTILE_SIZES[0]:])]).astype(np.float32)
        f[HELD] = 50.0
        return f

    kw = dict(cell=cells, batch=batch, num_graphs=3, fixed=fixed, wrap=wrap)
    host, ref = HostRelax(x, log_steps=16, **kw), NumpyRelax(x, **kw)
    if broken:
        host.batch[0], host.batch[-1] = -7, 99
    return host, ref, force, x


@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
@pytest.mark.parametrize("broken", [False, True], ids=["sound", "broken"])
def test_batch_with_an_empty_graph_and_a_batch_out_of_range(broken, wrap):
    host, ref, force, x = _hostile_batch(broken, wrap)
    assert host.graph_ptr.tolist() == [0, 40, 40, 110]
    for k in range(10):
        host.finish(force(host.advance()), total=(90 + k, 0))
        ref.finish(force(ref.advance()), total=(90 + k, 0))
        same_state(host, ref)
        assert np.array_equal(bits(host.log[k]), bits(ref.log[k])) and np.array_equal(host.f_prev, ref.f)
    assert host.gi[:, 2].tolist() == [1, 1, 0] and host.gi[:, 3].tolist() == [0, 0, -1]
    assert np.array_equal(bits(host.x[HELD]), bits(x[HELD])) and not host.v[HELD].any()
    assert bool(host.image.any()) == wrap


@pytest.mark.parametrize("why", ["flags", "count", "nan", "inf"])
def test_void_step_beside_a_converged_graph(why):
    """Each halt cause on its own, at evaluation 4 of the batch above (broken `batch`, graphs 0 and 1 converged, graph 2 with
    its held atom moving): every array bit-equal to the end of evaluation 3 -- the converged graph's atoms and its gf / gi
    rows among them --, pos32 the rounding of x, state = (4, code, 4, 0), no log row, and a second call changes nothing."""
    host, ref, force, _ = _hostile_batch()
    good = dict(energy=[-1.0, -2.0, -3.0], total=(500, 0), capacity=512)
    for _ in range(4):
        host.finish(force(host.advance()), **good)
        ref.finish(force(ref.advance()), **good)
    assert host.gi[:, 2].tolist() == [1, 1, 0]
    names = ("x", "v", "image", "pos32", "gf", "gi", "log", "f_prev")
    keep = [getattr(host, k).copy() for k in names]
    x0_converged = host.x0[:40].copy()
    bad, code = {"flags": (dict(good, total=(500, 16)), 16), "count": (dict(good, total=(513, 0)), 4),
                 "nan": (dict(good, energy=[-1.0, np.nan, -3.0]), 256),
                 "inf": (dict(good, energy=[np.inf, -2.0, -3.0]), 256)}[why]
    moved = host.advance().copy()
    assert not np.array_equal(moved[40:], keep[3][40:]) and np.array_equal(moved[:40], keep[3][:40])
    ref.advance()
    host.finish(force(moved) + np.float32(2.0), **bad)
    ref.finish(force(moved) + np.float32(2.0), **bad)
    for again in range(2):
        assert host.state.tolist() == [4, code, 4, 0]
        assert all(np.array_equal(getattr(host, k).view(np.uint8), b.view(np.uint8)) for k, b in zip(names, keep))
        assert np.array_equal(host.pos32, host.x.astype(np.float32)) and np.array_equal(bits(host.x0[:40]), bits(x0_converged))
        assert np.all(host.log[4:] == -7.0)
        same_state(host, ref)
        host.finish(force(host.advance()), **good)


def test_argument_refusals():
    """HN_ERR_BAD_ARG for a null state, num_graphs < 1, dt / dtmax / maxstep / fmax not positive, a flag other than the
    wrap; n = 0 is served."""
    lib = _lib.load()
    h = HostRelax(np.zeros((3, 3)) + 1.0, cell=np.eye(3) * 5.0)
    f, e, tot = np.zeros((3, 3), dtype=np.float32), np.zeros(1, dtype=np.float32), np.zeros(2, dtype=np.int64)

    def advance(n=3, B=1, flags=2, state=h.state):
        return lib.hermnet_host_relax_advance(n, B, flags, _p(h.x), _p(h.x0), _p(h.v), _p(h.image), _p(h.image0), None, _p(h.batch),
                                              _p(h.cell), _p(h.inv), _p(h.pos32), _p(state), _p(h.gf), _p(h.gi))

    def finish(n=3, B=1, dt=0.1, dtmax=1.0, maxstep=0.2, fmax=0.05, state=h.state):
        return lib.hermnet_host_relax_finish(n, B, _p(h.graph_ptr), _p(f), _p(e), _p(tot), 10, dt, dtmax, maxstep, fmax, None,
                                             _p(h.x), _p(h.v), _p(h.x0), _p(h.image), _p(h.image0), _p(h.f_prev), None, _p(h.pos32),
                                             _p(h.gf), _p(h.gi), _p(h.gf_new), _p(h.gi_new), _p(h.log), h.log_steps, _p(state))

    bad = 1                                                            # HN_ERR_BAD_ARG
    assert advance(state=None) == bad and advance(B=0) == bad and advance(flags=4) == bad and advance(flags=1) == bad
    assert finish(state=None) == bad and finish(B=0) == bad
    for kw in (dict(dt=0.0), dict(dtmax=-1.0), dict(maxstep=0.0), dict(fmax=0.0), dict(fmax=float("nan"))):
        assert finish(**kw) == bad, kw
    assert h.state.tolist() == [0, 0, 0, 0] and np.all(h.log == -7.0)
    assert advance(n=0) == 0 and finish(n=0) == 0                     # an empty system converges at once
    assert h.state.tolist() == [1, 0, 0, 1]
    # the same checks in front of the device entry points (they return before anything is launched)
    assert lib.hermnet_relax_advance(3, 0, 0, *([None] * 14)) == bad
    assert lib.hermnet_relax_finish(3, 1, None, None, None, None, 10, 0.0, 1.0, 0.2, 0.05, *([None] * 14), 4, None, None) == bad


MANY = 257      # one graph more than the 256 lanes that stride over the GRAPHS: the commit's copy and its `all`, the halt code


def many_graphs():
    """B = 257 with 257 atoms: graph 3 is empty, graph 256 has two atoms, every other graph one.  Graphs 0..255 converged at
    evaluation 0 beforehand; graph 256 is moving (past its first step, velocities and a scale set).  (host twin, numpy
    transcription, the forces of two evaluations: the second puts graph 256 under fmax)."""
    sizes = np.ones(MANY, dtype=np.int64)
    sizes[3], sizes[256] = 0, 2
    n = int(sizes.sum())
    rs = np.random.RandomState(MANY)
    x, batch = rs.uniform(1.0, 9.0, (n, 3)), np.repeat(np.arange(MANY), sizes)
    host = HostRelax(x, batch=batch, num_graphs=MANY, log_steps=4)
    ref = NumpyRelax(x, batch=batch, num_graphs=MANY)
    host.v[-2:] = ref.v[-2:] = rs.normal(scale=0.3, size=(2, 3))
    host.gi[:, 1], host.gi[:256, 2], host.gi[:256, 3], host.gi[256, 0], host.gf[256, 2] = 0, 1, 0, 2, 0.1
    host.gf_new[:], host.gi_new[:] = host.gf, host.gi
    ref.fresh[:], ref.converged[:256], ref.conv_step[:256], ref.nsteps[256], ref.scale[256] = 0, 1, 0, 2, 0.1
    f = rs.normal(size=(n, 3)).astype(np.float32)
    assert (f[-2:].astype(np.float64) ** 2).sum(1).max() > 0.05 ** 2
    return host, ref, f, f * np.float32(1e-3)


def test_more_graphs_than_lanes():
    """Graph 256 -- the second trip of lane 0 through every loop that strides over the graphs -- beside 256 converged graphs:
    after one advance + finish it has moved, is committed (gf / gi, its log row) and is counted in `all` (done stays 0);
    after a second evaluation that puts it under fmax, done is 1.  Bit-equal to the numpy transcription throughout."""
    host, ref, f1, f2 = many_graphs()
    start = host.x.copy()
    for k, f in enumerate((f1, f2)):
        assert np.array_equal(host.advance(), ref.advance())
        host.finish(f, total=(11 + k, 0))
        ref.finish(f, total=(11 + k, 0))
        same_state(host, ref)
        assert np.array_equal(bits(host.log[k]), bits(ref.log[k])) and np.array_equal(host.f_prev, ref.f)
        assert host.state.tolist() == [k + 1, 0, 0, k]
        assert host.gi[256, 1:].tolist() == [[0, 0, -1], [0, 1, 1]][k] and (host.gf[256, 2] > 0.0) == (k == 0)
    assert np.array_equal(bits(host.x[:-2]), bits(start[:-2])) and np.abs(host.x[-2:] - start[-2:]).min() > 1e-4
    assert np.all(host.gi[:256] == [0, 0, 1, 0]) and np.all(host.log[2:] == -7.0)
