"""CPU: the device-resident nudged elastic band (hermnet_amd/csrc/neb_kernels.hip, neb_step.h) through its host twin --
the step against the numpy float64 transcription of tests/neb_reference.py bit for bit, on inputs that reach every tangent
branch, the structure of the NEB force, a real saddle found by the climbing image (and missed without it), the void step
and the argument refusals.  No GPU: hermnet_host_neb_finish runs the text the kernels run."""
import numpy as np
import pytest

from neb_reference import HostNEB, NumpyNEB, _p, bits, layout, same_state

SIZES, IMAGES = (70, 3), (6, 4)           # band 0: 6 images of 70 atoms; band 1: 4 images of 3 atoms
HELD = 11                                  # an atom of every image of band 0 that is held
EARLY = 4                                  # the evaluation at which band 1 converges
_CACHE = {}


def _random_run(climb):
    """Ten evaluations of the host twin beside NumpyNEB on random coordinates, forces and energies, compared after every
    one.  Band 1 starts with its images 1 and 2 coincident under rising energies (T.T == 0), and converges at evaluation
    EARLY; evaluation 2 has Ep == Em on an image.  (host, ref, per-evaluation records)."""
    key = ("run", climb)
    if key in _CACHE:
        return _CACHE[key]
    rs = np.random.RandomState(17 + climb)
    graph_ptr, band_ptr, band_of, batch = layout(SIZES, IMAGES)
    n, B = int(graph_ptr[-1]), len(band_of)
    path = np.repeat(np.arange(B), np.diff(graph_ptr))[:, None] * np.array([0.4, 0.1, -0.2])
    x = np.zeros((n, 3))
    for k in range(2):                                              # every image: the band's template, moved along, rattled
        m = SIZES[k]
        template = rs.uniform(0.0, 8.0, (m, 3))
        for g in range(band_ptr[k], band_ptr[k + 1]):
            x[graph_ptr[g]:graph_ptr[g + 1]] = template
    x = x + path + rs.normal(scale=0.05, size=(n, 3))
    b1 = band_ptr[1]
    x[graph_ptr[b1 + 2]:graph_ptr[b1 + 3]] = x[graph_ptr[b1 + 1]:graph_ptr[b1 + 2]]      # coincident neighbours
    fixed = np.zeros(n, dtype=bool)
    fixed[graph_ptr[:band_ptr[1]] + HELD] = True
    kw = dict(fixed=fixed, k=[0.1, 0.3], fmax=[0.05, 5.0], climb=bool(climb))
    host, ref = HostNEB(x, graph_ptr, band_ptr, **kw), NumpyNEB(x, graph_ptr, band_ptr, **kw)
    hist = []
    for it in range(10):
        assert np.array_equal(host.advance(), ref.advance())
        f = rs.normal(scale=10.0, size=(n, 3)).astype(np.float32)
        e = rs.normal(size=B).astype(np.float32)
        if it == 0:
            e[b1:] = [-1.0, 0.0, 1.0, 2.0]                           # rising through the coincident pair
        if it == 2:
            e[3] = e[1]                                             # Ep == Em on image 2
        if it == EARLY:
            f[graph_ptr[b1]:] *= np.float32(1e-3)
        rec = dict(x=host.x.copy(), f=f, e=e)
        host.finish(f, e, total=(100 + it, 0))
        ref.finish(f, e, total=(100 + it, 0))
        same_state(host, ref)
        assert np.array_equal(bits(host.log[it]), bits(ref.log[it]))
        rec.update(g=host.g.copy(), obs=host.obs.copy(), gi=host.gi.copy(), climber=host.climber.copy())
        hist.append(rec)
    _CACHE[key] = (host, ref, hist, graph_ptr, band_ptr, fixed)
    return _CACHE[key]


@pytest.mark.parametrize("climb", [1, 0], ids=["climb", "plain"])
def test_host_twin_equals_the_numpy_transcription_bit_for_bit(climb):
    """Every array after every one of ten evaluations (asserted inside _random_run), and the inputs did reach: every
    tangent branch, a held atom, T.T == 0 between coincident images, a band that converges early beside one that goes on."""
    host, ref, hist, graph_ptr, band_ptr, fixed = _random_run(climb)
    seen = set(b for per in ref.branches for b in per.values())
    assert seen == {"rising", "falling", "maximum", "minimum", "equal"}, seen
    b1 = band_ptr[1]
    a, b = graph_ptr[b1 + 1], graph_ptr[b1 + 2]
    assert hist[0]["obs"][b1 + 1, 2] == 0.0 and hist[0]["obs"][b1 + 1, 3] == 0.0          # |t2| = 0, T = 0: ft = 0
    assert np.array_equal(hist[0]["g"][a:b], hist[0]["f"][a:b].astype(np.float64))      # ... and g = F
    lead0, lead1 = band_ptr[0] + 1, b1 + 1
    assert host.gi[lead1, 2:].tolist() == [1, EARLY] and host.gi[lead0, 2] == 0 and host.state.tolist() == [10, 0, 0, 0]
    assert np.array_equal(bits(host.x[graph_ptr[b1]:]), bits(hist[EARLY]["x"][graph_ptr[b1]:]))     # frozen since
    assert not host.v[graph_ptr[b1]:].any() and host.v[:graph_ptr[b1]].any()
    assert np.array_equal(bits(host.x[fixed]), bits(hist[0]["x"][fixed])) and not host.v[fixed].any()
    for k in range(2):                                               # end points never move
        for g in (band_ptr[k], band_ptr[k + 1] - 1):
            a, b = graph_ptr[g], graph_ptr[g + 1]
            assert np.array_equal(bits(host.x[a:b]), bits(hist[0]["x"][a:b]))
    assert np.all((host.climber >= 1) & (host.climber <= np.array(IMAGES) - 2)) if climb else np.all(host.climber == -1)
    assert np.all(host.log[10:] == -7.0)


@pytest.mark.parametrize("climb", [1, 0], ids=["climb", "plain"])
def test_structure_of_the_neb_force(climb):
    """From the run above, per interior image of band 0 and evaluation, against plain numpy sums: g - F is parallel to T;
    on a non-climbing image (g - F).tau = spring - ft, on the climbing image g.tau = -ft: to 1e-12 relative (float64
    rounding of a few hundred terms)."""
    from neb_reference import tangent_coef
    host, ref, hist, graph_ptr, band_ptr, fixed = _random_run(climb)
    climbing = 0
    for rec in hist:
        e = rec["e"].astype(np.float64)
        for g in range(1, IMAGES[0] - 1):
            a, b, am, ap = graph_ptr[g], graph_ptr[g + 1], graph_ptr[g - 1], graph_ptr[g + 1]
            free = ~fixed[a:b, None]
            t1, t2 = (rec["x"][a:b] - rec["x"][am:a]) * free, (rec["x"][ap:ap + b - a] - rec["x"][a:b]) * free
            c1, c2 = tangent_coef(e[g - 1], e[g], e[g + 1])
            T = c2 * t2 + c1 * t1
            tau = T / np.sqrt((T * T).sum())
            F = rec["f"][a:b].astype(np.float64) * free
            G = rec["g"][a:b]
            ft = (F * tau).sum()
            spring = 0.1 * (np.sqrt((t2 * t2).sum()) - np.sqrt((t1 * t1).sum()))
            scale = np.sqrt((F * F).sum())
            d = G - F
            along = (d * tau).sum()
            assert np.abs(d - along * tau).max() <= 1e-12 * scale
            if rec["climber"][0] == g:
                climbing += 1
                assert abs((G * tau).sum() + ft) <= 1e-12 * scale
            else:
                assert abs(along - (spring - ft)) <= 1e-12 * scale
            assert abs(rec["obs"][g, 3] - ft) <= 1e-12 * scale
    assert climbing == (len(hist) if climb else 0)


# ---- a real saddle ------------------------------------------------------------------------------------------------------------
SADDLE = np.array([0.0, 0.6, 0.0])
FMAX = 1e-3


def _surface(pos32):
    """E = (x^2 - 1)^2 + 2 (y - 0.6 (1 - x^2))^2 + 2 z^2 on the first atom of every image (the second is held, under a
    force that must not matter): minima (+-1, 0, 0), the saddle (0, 0.6, 0) with E = 1 and Hessian eigenvalues +-4.
    (energies [B], forces [2B,3]) rounded to float32."""
    p = pos32.astype(np.float64).reshape(-1, 2, 3)[:, 0]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    u = y - 0.6 * (1.0 - x * x)
    e = (x * x - 1.0) ** 2 + 2.0 * u * u + 2.0 * z * z
    f = np.zeros((len(p), 2, 3))
    f[:, 0] = -np.stack([4.0 * x * (x * x - 1.0) + 4.8 * u * x, 4.0 * u, 4.0 * z], axis=1)
    f[:, 1] = (1.0, -2.0, 3.0)
    return e.astype(np.float32), f.reshape(-1, 3).astype(np.float32)


def _saddle_run(climb):
    if ("saddle", climb) not in _CACHE:
        images = 8
        t = np.linspace(0.0, 1.0, images)
        mobile = np.stack([-1.0 + 2.0 * t, np.zeros(images), np.where((t > 0) & (t < 1), 0.02, 0.0)], axis=1)
        x = np.stack([mobile, np.tile([5.0, 5.0, 5.0], (images, 1))], axis=1).reshape(-1, 3)
        graph_ptr, band_ptr, _, _ = layout((2,), (images,))
        fixed = np.tile([False, True], images)
        host = HostNEB(x, graph_ptr, band_ptr, fixed=fixed, k=0.1, fmax=FMAX, climb=climb, log_steps=256)
        for _ in range(200):
            e, f = _surface(host.advance())
            host.finish(f, e)
            if host.state[3]:
                break
        _CACHE[("saddle", climb)] = (host, x)
    return _CACHE[("saddle", climb)]


def test_the_climbing_image_finds_the_saddle():
    """Eight images (an even count: none sits on the saddle by symmetry), k = 0.1, fmax = 1e-3: the band converges within
    200 evaluations (2x what a numpy prototype took); the climbing image lies within fmax / 2 of the saddle (|g| / |lambda|
    = fmax / 4 per component) and its energy within fmax^2 of 1; end points and the held atoms have not moved."""
    host, x = _saddle_run(True)
    evaluations = int(host.state[0])
    top = int(host.climber[0])
    at = host.x[2 * top]
    print("evaluations %d, climbing image %d at %s, |at - saddle| %.3e, E - 1 %.3e"
          % (evaluations, top, at, np.linalg.norm(at - SADDLE), host.obs[top, 0] - 1.0))
    assert host.state[3] == 1 and evaluations <= 200
    assert host.gi[1, 2:].tolist() == [1, evaluations - 1] and host.gf[1, 3] < FMAX
    assert np.linalg.norm(at - SADDLE) < FMAX / 2
    assert abs(host.obs[top, 0] - 1.0) < FMAX ** 2
    assert top == int(np.argmax(host.obs[1:-1, 0])) + 1
    assert np.array_equal(bits(host.x[1::2]), bits(x[1::2])) and np.array_equal(bits(host.x[[0, 14]]), bits(x[[0, 14]]))


def test_without_the_climbing_image_the_saddle_is_missed():
    """climb=False on the same band: the highest image stays more than 0.1 from the saddle (prototype: 0.17) -- the
    climbing branch is what found it."""
    host, _ = _saddle_run(False)
    top = int(np.argmax(host.obs[1:-1, 0])) + 1
    print("evaluations %d, highest image %d, |at - saddle| %.3e" % (host.state[0], top, np.linalg.norm(host.x[2 * top] - SADDLE)))
    assert host.climber[0] == -1
    assert np.linalg.norm(host.x[2 * top] - SADDLE) > 0.1


# ---- the void step and the refusals ---------------------------------------------------------------------------------------------
def _small(log_steps=8):
    rs = np.random.RandomState(5)
    graph_ptr, band_ptr, band_of, _ = layout((9,), (4,))
    x = rs.uniform(0.0, 5.0, (9, 3))
    x = np.concatenate([x + 0.3 * g + rs.normal(scale=0.05, size=(9, 3)) for g in range(4)])
    host = HostNEB(x, graph_ptr, band_ptr, k=0.2, fmax=0.05, log_steps=log_steps)
    force = lambda: (rs.normal(size=(36, 3)).astype(np.float32), rs.normal(size=4).astype(np.float32))
    return host, force


@pytest.mark.parametrize("what", ["nan", "capacity"])
def test_void_step(what):
    """A NaN energy or more pairs than columns: the coordinates return to the start of the step, velocities, band state,
    observables and log are untouched, the halt is recorded, later calls are no-ops; with the halt cleared (what resume()
    does) the run repeats the void move and ends on the bits of the run that never halted."""
    host, force = _small()
    straight, _ = _small()
    inputs = [force() for _ in range(7)]
    for f, e in inputs[:3]:
        host.advance()
        host.finish(f, e, total=(50, 0), capacity=60)
    names = ("x", "v", "image", "pos32", "gf", "gi", "obs", "climber", "log", "f_prev")
    keep = {k: getattr(host, k).copy() for k in names}
    moved = host.advance().copy()
    assert not np.array_equal(moved, keep["pos32"])
    f, e = inputs[3]
    bad_e, total, code = e.copy(), (50, 0), 256
    if what == "nan":
        bad_e[0] = np.nan                                            # an end point's energy counts too
    else:
        total, code = (61, 0), 4
    host.finish(f, bad_e, total=total, capacity=60)
    for again in range(2):
        assert host.state.tolist() == [3, code, 3, 0]
        for k, want in keep.items():
            assert np.array_equal(getattr(host, k).view(np.uint8), want.view(np.uint8)), k
        host.advance()
        host.finish(f, e, total=(50, 0), capacity=60)
    host.state[1:3] = 0
    for f, e in inputs[3:]:
        host.advance()
        host.finish(f, e, total=(50, 0), capacity=60)
    for f, e in inputs:
        straight.advance()
        straight.finish(f, e, total=(50, 0), capacity=60)
    assert host.state.tolist() == straight.state.tolist() == [7, 0, 0, 0]
    for k in names:
        assert np.array_equal(getattr(host, k).view(np.uint8), getattr(straight, k).view(np.uint8)), k


def test_argument_refusals():
    """HN_ERR_BAD_ARG, with nothing written: a null state, fewer than three graphs, no band, dt / dtmax / maxstep not
    positive, climb not 0 or 1, a band of two images, images of unequal size, a band_of that disagrees, fmax = 0; the device
    entry point refuses what it can see before anything is launched."""
    host, force = _small()
    f, e = force()
    tot = np.array([5, 0], dtype=np.int64)
    lib, bad = host.lib, 1

    def finish(**change):
        args = host.finish_args(f, e, tot, 10)
        for at, value in change.items():
            args[int(at[1:])] = value
        return lib.hermnet_host_neb_finish(*args)

    assert finish(_36=None) == bad and finish(_1=2) == bad and finish(_2=0) == bad and finish(_3=2) == bad
    for at in ("_11", "_12", "_13"):
        assert finish(**{at: 0.0}) == bad and finish(**{at: float("nan")}) == bad, at
    assert finish(_35=0) == bad and finish(_10=-1) == bad and finish(_4=None) == bad and finish(_26=None) == bad
    two = np.array([0, 2, 4], dtype=np.int32)
    assert finish(_2=2, _5=_p(two)) == bad                                                    # bands of two images
    uneven = np.array([0, 9, 19, 27, 36], dtype=np.int32)
    assert finish(_4=_p(uneven)) == bad
    wrong = np.array([0, 0, 1, 0], dtype=np.int32)
    assert finish(_6=_p(wrong)) == bad
    zero = np.zeros(1)
    assert finish(_15=_p(zero)) == bad
    assert host.state.tolist() == [0, 0, 0, 0] and np.all(host.log == -7.0)
    assert finish() == 0 and host.state.tolist() == [1, 0, 0, 0]
    assert lib.hermnet_neb_finish(36, 2, 1, 1, *([None] * 6), 10, 0.1, 1.0, 0.2, *([None] * 21), 8, None, None) == bad
    assert lib.hermnet_neb_finish(36, 4, 1, 1, *([None] * 6), 10, 0.0, 1.0, 0.2, *([None] * 21), 8, None, None) == bad
