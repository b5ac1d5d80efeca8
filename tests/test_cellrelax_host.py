"""CPU: the device-resident cell relaxation (hermnet_amd/csrc/cellrelax_kernels.hip, cellrelax_step.h) through its host twins
-- the step against a numpy float64 transcription bit for bit, ASE's UnitCellFilter + FIRE semantics against a textbook
version, the filter's options, fixed atoms, the independence of the graphs of a batch, the void step for each cause (the
cell is taken back), the lane boundaries and the argument refusals.  No GPU: hermnet_host_cellrelax_advance / _finish run
the text the kernels run."""
import numpy as np
import pytest

from hermnet_amd import _lib
from cellrelax_reference import (HostCellRelax, NumpyCellRelax, _p, bits, cell_force_np, drive, lj_evaluation, lj_fcc, lj_one,
                                 same_state, textbook_cell_fire)

STRAINS = [np.array([[0.03, 0.01, 0.0], [0.0, -0.02, 0.015], [0.01, 0.0, 0.025]]),
           np.array([[-0.03, 0.0, 0.01], [0.02, 0.03, 0.0], [0.0, -0.01, -0.02]]),
           np.array([[0.02, 0.02, 0.0], [0.0, 0.02, 0.0], [0.0, 0.0, 0.04]])]
REPS = [(2, 2, 2), (2, 2, 3), (2, 3, 3)]          # 32, 48 and 72 atoms; the fourth graph is empty
RATTLE = [0.12, 0.002, 0.08]                     # graph 1 barely rattled: its cell rows carry the largest force
CAP = 300
_CACHE = {}


def _batch_system():
    """Three triclinic LJ cells of unequal sizes + an empty graph, a third of the atoms starting outside their cell."""
    if "batch" not in _CACHE:
        parts = [lj_fcc(REPS[g], 10 + g, RATTLE[g], STRAINS[g], outside=True) for g in range(3)]
        sizes = [len(p[0]) for p in parts] + [0]
        x = np.concatenate([p[0] for p in parts])
        cells = np.stack([p[1] for p in parts] + [np.eye(3) * 9.0])
        batch = np.repeat(np.arange(4), sizes)
        ptr = np.concatenate([[0], np.cumsum(sizes)])
        _CACHE["batch"] = (x, cells, batch, ptr, lj_evaluation(ptr))
    return _CACHE["batch"]


def _side_by_side(host, ref, evaluate, evaluations, hist=None, first=0):
    """Host twin and numpy transcription through `evaluations` evaluations, compared after every one."""
    for k in range(first, first + evaluations):
        pos32, cell32 = host.advance()
        rp, rc = ref.advance()
        assert np.array_equal(pos32, rp) and np.array_equal(cell32, rc)
        e, f, w = evaluate(pos32, cell32)
        host.finish(f, w, energy=e, total=(7 * k, 0))
        ref.finish(f, w, energy=e, total=(7 * k, 0))
        same_state(host, ref)
        if k < len(ref.log):
            assert np.array_equal(bits(host.log[k]), bits(ref.log[k])) and np.array_equal(host.f_prev, ref.f)
        if hist is not None:
            hist.append(dict(x=host.x.copy(), q=host.q.copy(), rows=host.rows.copy(), cell32=host.cell32.copy(),
                             gf=host.gf.copy(), gi=host.gi.copy(), state=host.state.copy()))
        if host.state[3]:
            break


def _batch_run():
    if "run" not in _CACHE:
        x, cells, batch, ptr, evaluate = _batch_system()
        host = HostCellRelax(x, cells, batch=batch, num_graphs=4)
        ref = NumpyCellRelax(x, cells, batch=batch, num_graphs=4)
        hist = []
        _side_by_side(host, ref, evaluate, CAP, hist)
        _CACHE["run"] = (host, ref, hist)
    return _CACHE["run"]


def test_host_twin_equals_the_numpy_transcription_bit_for_bit():
    """q, x, v, image, pos32, the rows G and their velocities, F, F^-1, C, cell32, obs, the per-graph FIRE state, the log and
    the state words after EVERY evaluation of the whole relaxation (asserted inside _batch_run); atoms did start outside
    their cells; all graphs converge."""
    host, ref, hist = _batch_run()
    assert host.state[3] == 1 and np.all(host.gi[:, 2] == 1), "a graph had not converged after %d evaluations" % CAP
    assert np.abs(host.image).max() >= 1
    assert np.all(host.log[len(hist):] == -7.0)                     # no row beyond the evaluations made
    assert np.abs(host.deform[:3] - np.eye(3).reshape(9)).max() > 5e-3         # the cells did move


def test_the_run_passes_through_every_branch():
    """From the numpy twin's record (its state was bit-equal to the host twin's throughout): fresh, mix, stop, dt growth, the
    maxstep clamp, and an evaluation whose largest generalised force was a cell row's."""
    _, ref, hist = _batch_run()
    for g in range(3):
        modes = [m[g] for m in ref.modes]
        assert modes[0] == "fresh" and "fresh" not in modes[1:]
        assert modes.count("stop") >= 1 and modes.count("mix") > 6, (g, modes)
        dts = np.array([row[g, 2] for row, m in zip(ref.log, modes) if m != "frozen"])
        assert np.any(dts[1:] > dts[:-1] * 1.05) and np.any(dts[1:] == 0.5 * dts[:-1]) and dts.max() > 0.1 * 1.1 ** 4
        assert any(c[g] for c in ref.clamped) and not all(c[g] for c in ref.clamped)
        assert any(c[g] for c in ref.cell_led)
    assert ref.cell_led[0][1] and not ref.cell_led[0][0]            # at the start: graph 1 led by its cell, graph 0 by an atom


@pytest.mark.parametrize("case", [0, 1])
def test_semantics_are_ases_unit_cell_filter_under_fire(case):
    """One strained and rattled LJ cell: the twin converges at the same evaluation as the textbook, positions and cell stay
    within 1e-9 A of the textbook's at every evaluation (they differ in summation order, in the inverse and in where the
    clamp's scale is applied); at the end an independent float64 evaluation gives max |f| and the largest row of S F^-T /
    cell_factor below fmax, and the enthalpy fell."""
    p = [0.0, 0.02][case]
    x, cell = lj_fcc(REPS[case], 20 + case, 0.06, STRAINS[case + 1])
    n = len(x)
    evaluate = lj_evaluation(np.array([0, n]))
    count, path, enthalpy = textbook_cell_fire(x, cell, evaluate, scalar_pressure=p, cap=CAP)
    assert count is not None and 10 < count <= CAP
    host = HostCellRelax(x, cell, wrap=False, scalar_pressure=p)
    for k in range(count):
        pos32, cell32 = host.advance()
        assert np.abs(host.x - path[k][0]).max() <= 1e-9 and np.abs(host.cell64.reshape(3, 3) - path[k][1]).max() <= 1e-9, k
        e, f, w = evaluate(pos32, cell32)
        host.finish(f, w, energy=e)
        assert bool(host.state[3]) == (k == count - 1), k
        assert abs(host.gf[0, 4] - enthalpy[k]) <= 1e-9 * max(1.0, abs(enthalpy[k]))
    assert host.gi[0, 3] == count - 1 and host.state[0] == count
    C, F = host.cell64.reshape(3, 3), host.deform.reshape(3, 3)
    e, f, w = lj_one(host.x, C)
    vol = abs(np.linalg.det(C))
    S = 0.5 * (w + w.T) - p * vol * np.eye(3)
    cell_force = S @ np.linalg.inv(F).T / n
    assert np.sqrt((f ** 2).sum(1).max()) < 0.05 and np.sqrt((cell_force ** 2).sum(1).max()) < 0.05
    assert e + p * vol < enthalpy[0] - 0.1 and host.gf[0, 4] < host.log[0, 0, 0]


def _option_run(**kw):
    """The first LJ cell relaxed to convergence under the filter's options; (host, evaluations, per-evaluation record)."""
    x, cell = lj_fcc(REPS[0], 30, 0.06, STRAINS[0])
    evaluate = lj_evaluation(np.array([0, len(x)]))
    host = HostCellRelax(x, cell, **kw)
    rec = []

    def every(k):
        rec.append(dict(rows_v=host.rows_v.copy(), obs=host.obs.copy(), cell64=host.cell64.copy(), finv=host.deform_inv.copy()))

    made = drive(host, evaluate, CAP, until_done=True, every=every)
    assert host.state[3] == 1 and made > 10
    return host, made, rec


def test_mask_zeros_leave_those_entries_of_F_at_the_identity():
    mask = np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    host, _, _ = _option_run(mask=mask)
    F = host.deform.reshape(3, 3)
    assert np.array_equal(F[mask == 0.0], np.eye(3)[mask == 0.0])                  # exactly
    assert np.all(np.abs(F - np.eye(3))[mask == 1.0] > 1e-4)
    voigt, _, _ = _option_run(mask=[1, 1, 0, 0, 1, 0])                             # xx, yy, zz, yz, xz, xy
    assert np.array_equal(bits(voigt.deform), bits(host.deform)) and np.array_equal(bits(voigt.x), bits(host.x))


def test_hydrostatic_strain_keeps_F_a_multiple_of_the_identity():
    host, _, _ = _option_run(hydrostatic_strain=True)
    F = host.deform.reshape(3, 3)
    assert F[0, 0] == F[1, 1] == F[2, 2] != 1.0 and np.array_equal(F - np.diag(np.diag(F)), np.zeros((3, 3)))


def test_constant_volume_keeps_the_trace_of_F():
    """tr(F - I) stays 0 to rounding.  The bound, from the arithmetic (eps = 2^-52, K evaluations, U the largest operand):
    the projection a_kk - t leaves a trace of at most 4 eps max |a| (t carries two roundings, each subtraction one), so
    tr fG <= 4 eps max |fG_unprojected|; a velocity update (keep v + cf f, + dt f: four roundings per entry, dt <= 1) adds at
    most 16 eps U to tr vG with U >= max |vG| + max |fG_unprojected|, so |tr vG| <= 16 K eps U; the move G += scale vG (scale <=
    1) passes that on and rounds three diagonal entries of size <= 1.1 cf; F = G / cf and the trace's own additions round
    once more each: |tr(F - I)| <= eps (4 K + 8 + 16 K^2 U / cf)."""
    host, K, rec = _option_run(constant_volume=True)
    cf = host.cf[0]
    raw = [cell_force_np(-r["obs"][0, 2:] * r["obs"][0, 0], r["cell64"][0], r["finv"][0], cf, 0.0, np.ones(9), 0)[0] for r in rec]
    U = max(np.abs(r["rows_v"]).max() for r in rec) + max(np.abs(a).max() for a in raw)
    F = host.deform.reshape(3, 3)
    bound = 2.0 ** -52 * (4 * K + 8 + 16 * K * K * U / cf)
    assert bound < 1e-10 and abs((F[0, 0] - 1.0) + (F[1, 1] - 1.0) + (F[2, 2] - 1.0)) <= bound
    assert np.abs(F - np.eye(3)).max() > 1e-3                                       # the shape did relax


def test_scalar_pressure_ends_at_a_smaller_volume():
    free, _, _ = _option_run()
    pressed, _, _ = _option_run(scalar_pressure=0.05)
    assert pressed.obs[0, 0] < 0.99 * free.obs[0, 0]
    assert abs(pressed.obs[0, 1] - 0.05) < 0.01 and abs(free.obs[0, 1]) < 0.01       # tr W / 3V balances p


def test_fixed_atoms_keep_q_and_ride_the_cell():
    x, cell = lj_fcc(REPS[0], 31, 0.06, STRAINS[0])
    fixed = np.zeros(len(x), dtype=bool)
    fixed[[5, 31]] = True
    evaluate = lj_evaluation(np.array([0, len(x)]))
    host = HostCellRelax(x, cell, fixed=fixed)
    ref = NumpyCellRelax(x, cell, fixed=fixed)
    _side_by_side(host, ref, evaluate, 40)
    assert np.array_equal(bits(host.q[fixed]), bits(x[fixed])) and not host.v[fixed].any()
    F = host.deform.reshape(3, 3)
    assert np.abs(F - np.eye(3)).max() > 5e-3
    assert np.allclose(host.x[fixed], x[fixed] @ F.T, rtol=0, atol=1e-12) and np.abs(host.x[fixed] - x[fixed]).max() > 1e-3
    assert np.abs(host.q[~fixed] - x[~fixed]).max() > 1e-3


def test_graphs_of_a_batch_relax_independently():
    """Each graph's trajectory (q, G, the FIRE state) and converged step equal, bit for bit, those of the same graph relaxed
    alone; the graphs converge at different steps; a converged graph is never written again, its cell included; done is set
    exactly when the last converges and later calls change nothing."""
    x, cells, batch, ptr, evaluate = _batch_system()
    host, _, hist = _batch_run()
    conv = host.gi[:, 3]
    assert conv[3] == 0 and len(set(conv[:3].tolist())) > 1
    assert len(hist) == conv.max() + 1 and all(h["state"][3] == 0 for h in hist[:-1]) and hist[-1]["state"][3] == 1
    for g in range(3):
        a, b = ptr[g], ptr[g + 1]
        alone = HostCellRelax(x[a:b], cells[g])
        one = lj_evaluation(np.array([0, b - a]))
        for k in range(conv[g] + 1):
            pos32, cell32 = alone.advance()
            e, f, w = one(pos32, cell32)
            alone.finish(f, w, energy=e)
            assert np.array_equal(bits(alone.q), bits(hist[k]["q"][a:b])) and np.array_equal(bits(alone.x), bits(hist[k]["x"][a:b]))
            assert np.array_equal(bits(alone.rows[0]), bits(hist[k]["rows"][g]))
            assert np.array_equal(bits(alone.gf[0]), bits(hist[k]["gf"][g]))
        assert alone.state[3] == 1 and alone.gi[0, 3] == conv[g]
        for k in range(conv[g], len(hist)):                             # frozen from its converged step on
            assert np.array_equal(bits(hist[k]["x"][a:b]), bits(hist[conv[g]]["x"][a:b]))
            assert np.array_equal(hist[k]["cell32"][g], hist[conv[g]]["cell32"][g])
            assert np.array_equal(bits(hist[k]["rows"][g]), bits(hist[conv[g]]["rows"][g]))
    names = ("q", "x", "v", "rows", "rows_v", "cell32", "cell64", "gf", "gi", "state", "log", "pos32")
    before = [getattr(host, k).copy() for k in names]
    for _ in range(3):
        pos32, cell32 = host.advance()
        e, f, w = evaluate(pos32, cell32)
        host.finish(f + 1.0, w + 1.0, energy=e)
    assert all(np.array_equal(p, getattr(host, k)) for p, k in zip(before, names))


VOID_AT = 6


@pytest.mark.parametrize("why", ["flags", "count", "nan_energy", "nan_virial", "det"])
def test_void_step(why):
    """Each cause on its own at evaluation 6, beside a converged graph (graph 1, by a loose threshold of its own, and the
    empty graph 3): q, x, image, G, F, F^-1, C, cell32 and pos32 return to the start of the step bit for bit, velocities and
    the per-graph state stay, the converged graphs are untouched, state = (6, code, 6, 0), no log row, later calls are no-ops
    -- and once the halt is cleared the run repeats the void move and ends where an uninterrupted run ends."""
    x, cells, batch, ptr, evaluate = _batch_system()
    kw = dict(batch=batch, num_graphs=4, fmax=[0.05, 3.0, 0.05, 0.05], log_steps=16)
    host, ref = HostCellRelax(x, cells, **kw), NumpyCellRelax(x, cells, **{k: v for k, v in kw.items() if k != "log_steps"})
    good = dict(total=(500, 0), capacity=512)

    def evaluation(opt, **bad):
        pos32, cell32 = opt.advance()
        e, f, w = evaluate(pos32, cell32)
        if "energy" in bad:
            e = e.copy()
            e[bad.pop("energy")] = np.nan
        if "virial" in bad:
            w = w.copy()
            w[bad.pop("virial"), 1, 2] = np.inf
        moved = (pos32.copy(), cell32.copy())
        opt.finish(f, w, energy=e, **dict(good, **bad))
        return moved

    for _ in range(VOID_AT):
        evaluation(host)
        evaluation(ref)
    assert host.gi[:, 2].tolist() == [0, 1, 0, 1]
    names = ("q", "x", "v", "image", "pos32", "rows", "rows_v", "deform", "deform_inv", "cell64", "cell32", "obs", "gf", "gi", "log",
             "f_prev")
    keep = [getattr(host, k).copy() for k in names]
    bad, code = {"flags": (dict(total=(500, 16)), 16), "count": (dict(total=(513, 0)), 4), "nan_energy": (dict(energy=1), 256),
                 "nan_virial": (dict(virial=3), 256), "det": ({}, 256)}[why]
    if why == "det":                                                # graph 2's rows thrown through zero: det F < 0
        for opt, scale in ((host, host.gf[2, 2]), (ref, ref.scale[2])):
            opt.rows_v[2] = -1e3 * opt.cf[2] * np.eye(3).reshape(9) / scale
        keep[names.index("rows_v")] = host.rows_v.copy()
    pos32, cell32 = evaluation(host, **dict(bad))
    evaluation(ref, **dict(bad))
    old_pos, old_cell = keep[names.index("pos32")], keep[names.index("cell32")].reshape(4, 3, 3)
    assert not np.array_equal(pos32[ptr[2]:ptr[3]], old_pos[ptr[2]:ptr[3]])
    assert not np.array_equal(cell32[2], old_cell[2])
    assert np.array_equal(pos32[ptr[1]:ptr[2]], old_pos[ptr[1]:ptr[2]]) and np.array_equal(cell32[1], old_cell[1])
    assert (host.det_f[2] < 0.0) == (why == "det")
    for again in range(2):
        assert host.state.tolist() == [VOID_AT, code, VOID_AT, 0]
        for k, want in zip(names, keep):
            assert np.array_equal(getattr(host, k).view(np.uint8), want.view(np.uint8)), k
        assert np.array_equal(host.pos32, host.x.astype(np.float32)) and np.array_equal(host.cell32, host.cell64.astype(np.float32))
        assert np.all(host.log[VOID_AT:] == -7.0)
        same_state(host, ref)
        evaluation(host)                                             # halted: nothing
    if why == "det":
        return
    host.state[1:3] = 0                                              # what resume() does
    straight = HostCellRelax(x, cells, **kw)
    for _ in range(VOID_AT + 4):
        evaluation(straight)
    for _ in range(4):
        evaluation(host)
    for k in ("q", "x", "rows", "cell32", "gf"):
        assert np.array_equal(getattr(host, k).view(np.uint8), getattr(straight, k).view(np.uint8)), k


def _well(n, seed, cell):
    """(start coordinates, evaluation) of a cheap synthetic field for the bit-for-bit tests: harmonic wells at fixed
    fractional sites of the current cell and a harmonic pull of the cell towards a target."""
    rs = np.random.RandomState(seed)
    sites, k = rs.uniform(0.1, 0.9, (n, 3)), rs.uniform(1.0, 6.0, (n, 3))
    target = cell * np.array([1.03, 0.98, 1.01])
    x = sites @ cell + rs.uniform(-0.25, 0.25, (n, 3))
    x[::3] += np.array([2, -1, 1]) @ cell

    def evaluate(pos32, cell32):
        c = np.asarray(cell32, dtype=np.float64).reshape(3, 3)
        d = pos32.astype(np.float64) - sites @ c
        d = d - np.round(d @ np.linalg.inv(c)) @ c
        w = -np.einsum("na,nb->ab", k * d, d) - 0.8 * (c - target).T @ c
        return (np.array([0.5 * (k * d * d).sum()], dtype=np.float32), (-k * d).astype(np.float32),
                w.astype(np.float32).reshape(1, 3, 3))

    return x, evaluate


TRICLINIC = np.array([[19.3, 0.4, -0.7], [2.1, 21.2, 0.3], [-1.6, 3.3, 24.9]])


@pytest.mark.parametrize("wrap", [True, False], ids=["wrap", "nowrap"])
@pytest.mark.parametrize("n", [0, 1, 256, 257, 513])
def test_one_graph_on_both_sides_of_the_lane_boundary(n, wrap):
    """No atom, one, a full row of 256 lanes, one over, two rows and one: twelve evaluations bit-equal to the numpy
    transcription (state, log rows, accepted forces), with the wrap and without."""
    x, evaluate = _well(n, 40 + n, TRICLINIC)
    host, ref = HostCellRelax(x, TRICLINIC, wrap=wrap, log_steps=16), NumpyCellRelax(x, TRICLINIC, wrap=wrap)
    _side_by_side(host, ref, evaluate, 12)
    assert host.state[0] == len(ref.log) == 12 and np.all(host.log[12:] == -7.0)
    assert bool(host.image.any()) == (wrap and n > 0)
    assert np.abs(host.deform - np.eye(3).reshape(9)).max() > 1e-5


def test_argument_refusals():
    """HN_ERR_BAD_ARG without a GPU: null pointers, num_graphs < 1, unknown flags, dt / dtmax / maxstep / fmax not positive,
    cell_factor <= 0 (the host twins read it), a mask entry that is not finite (every entry point reads it)."""
    lib = _lib.load()
    h = HostCellRelax(np.zeros((3, 3)) + 1.0, np.eye(3) * 5.0)
    f, e, w, tot = np.zeros((3, 3), dtype=np.float32), np.zeros(1, dtype=np.float32), np.zeros((1, 9), dtype=np.float32), \
        np.zeros(2, dtype=np.int64)
    A, F = h.advance_args, lambda: h.finish_args(f, e, w, tot, 10)

    def advance(**kw):
        a = list(A())
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.hermnet_host_cellrelax_advance(*a)

    def finish(**kw):
        a = list(F())
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.hermnet_host_cellrelax_finish(*a)

    bad = 1                                                            # HN_ERR_BAD_ARG
    assert advance(_1=0) == bad and advance(_2=4) == bad and advance(_2=1) == bad
    for i in (3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26):      # every array but fixed, batch
        assert advance(**{"_%d" % i: None}) == bad, i
    assert finish(_1=0) == bad and finish(_2=4) == bad
    for i, v in ((9, 0.0), (10, -1.0), (11, 0.0), (12, 0.0), (12, float("nan")), (43, 0)):
        assert finish(**{"_%d" % i: v}) == bad, i
    for i in [3, 4, 5, 6, 7, 14, 15, 16, 17, 18] + list(range(19, 27)) + list(range(28, 43)) + [44]:   # every array but fmax_graph, fixed
        assert finish(**{"_%d" % i: None}) == bad, i
    for value in (0.0, -2.0, np.nan, np.inf):
        cf = np.array([value])
        assert advance(_14=_p(cf)) == bad and finish(_18=_p(cf)) == bad, value
    for value in (np.nan, np.inf):
        mask = np.ones(9)
        mask[5] = value
        assert finish(_15=_p(mask)) == bad
    assert h.state.tolist() == [0, 0, 0, 0] and np.all(h.log == -7.0)
    # the same checks in front of the device entry points (they return before anything is launched)
    dev_a, dev_f = list(A()) + [None], list(F()) + [None]
    mask = np.ones(9)
    mask[0] = np.nan
    assert lib.hermnet_cellrelax_advance(*(dev_a[:3] + [None] * 25)) == bad
    assert lib.hermnet_cellrelax_finish(*(dev_f[:15] + [_p(mask)] + dev_f[16:])) == bad
    assert lib.hermnet_cellrelax_finish(*(dev_f[:15] + [None] + dev_f[16:])) == bad
    assert lib.hermnet_cellrelax_finish(*(dev_f[:6] + [None] + dev_f[7:])) == bad


MANY = 257      # one graph more than the 256 lanes that stride over the GRAPHS: in the commit's copy and its `all`, in the halt
#                 code, in the advance's lane-per-graph kernel (a second block)


def many_graphs():
    """B = 257 with 257 atoms: graph 3 is empty, graph 256 has two atoms, every other graph one.  Graphs 0..255 converged at
    evaluation 0 beforehand; graph 256 is moving (past its first step; velocities of atoms and cell rows and a scale set).
    (host twin, numpy transcription, (forces, virial) of two evaluations: the second puts graph 256 under fmax)."""
    sizes = np.ones(MANY, dtype=np.int64)
    sizes[3], sizes[256] = 0, 2
    n = int(sizes.sum())
    rs = np.random.RandomState(MANY)
    cells = TRICLINIC[None] * rs.uniform(0.4, 0.6, (MANY, 1, 1))
    batch = np.repeat(np.arange(MANY), sizes)
    x = np.einsum("nk,nkj->nj", rs.uniform(-0.5, 1.5, (n, 3)), cells[batch])
    host = HostCellRelax(x, cells, batch=batch, num_graphs=MANY, log_steps=4)
    ref = NumpyCellRelax(x, cells, batch=batch, num_graphs=MANY)
    host.v[-2:] = ref.v[-2:] = rs.normal(scale=0.3, size=(2, 3))
    host.rows_v[256] = ref.rows_v[256] = rs.normal(scale=0.1, size=9)
    host.gi[:, 1], host.gi[:256, 2], host.gi[:256, 3], host.gi[256, 0], host.gf[256, 2] = 0, 1, 0, 2, 0.1
    host.gf_new[:], host.gi_new[:] = host.gf, host.gi
    ref.fresh[:], ref.converged[:256], ref.conv_step[:256], ref.nsteps[256], ref.scale[256] = 0, 1, 0, 2, 0.1
    f, w = rs.normal(size=(n, 3)).astype(np.float32), rs.normal(scale=5.0, size=(MANY, 3, 3)).astype(np.float32)
    return host, ref, (f, w), (f * np.float32(1e-3), w * np.float32(1e-4))


MANY_NAMES = ("q", "x", "v", "image", "pos32", "rows", "rows_v", "deform", "deform_inv", "cell64", "cell32", "obs", "gf", "gi",
              "log", "f_prev")


def test_more_graphs_than_lanes():
    """Graph 256 -- the second trip of lane 0 through every loop that strides over the graphs, and the second block of the
    advance's lane-per-graph kernel -- beside 256 converged graphs: after one advance + finish its atoms and cell have moved,
    it is committed (gf / gi, its log row) and is counted in `all` (done stays 0); after a second evaluation that puts it
    under fmax, done is 1.  Bit-equal to the numpy transcription throughout; graphs 0..255 are never written."""
    host, ref, first, second = many_graphs()
    start = {k: getattr(host, k).copy() for k in ("x", "cell32", "rows", "gi")}
    for k, (f, w) in enumerate((first, second)):
        (pos32, cell32), (rp, rc) = host.advance(), ref.advance()
        assert np.array_equal(pos32, rp) and np.array_equal(cell32, rc)
        host.finish(f, w, total=(11 + k, 0))
        ref.finish(f, w, total=(11 + k, 0))
        same_state(host, ref)
        assert np.array_equal(bits(host.log[k]), bits(ref.log[k])) and np.array_equal(host.f_prev, ref.f)
        assert host.state.tolist() == [k + 1, 0, 0, k]
        assert host.gi[256, 1:].tolist() == [[0, 0, -1], [0, 1, 1]][k] and (host.gf[256, 2] > 0.0) == (k == 0)
    for name in ("x", "cell32", "rows"):
        a, b = getattr(host, name), start[name]
        rows = slice(-2, None) if name == "x" else slice(256, None)
        keep = slice(None, -2) if name == "x" else slice(None, 256)
        assert np.array_equal(a[keep].view(np.uint8), b[keep].view(np.uint8)) and not np.array_equal(a[rows], b[rows]), name
    assert np.array_equal(host.gi[:256], start["gi"][:256]) and np.all(host.log[2:] == -7.0)


def test_more_graphs_than_lanes_void_on_the_last_virial():
    """The virial of graph 256 alone is NaN: halt code 256 at evaluation 0, graph 256's atoms and cell back to the start of
    the step bit for bit, graphs 0..255 untouched, no log row; equal to the numpy transcription."""
    host, ref, (f, w), _ = many_graphs()
    keep = [getattr(host, k).copy() for k in MANY_NAMES]
    (pos32, cell32), _ = host.advance(), ref.advance()
    moved = (pos32.copy(), cell32.reshape(MANY, 9).copy())
    old_pos, old_cell = keep[MANY_NAMES.index("pos32")], keep[MANY_NAMES.index("cell32")]
    assert not np.array_equal(moved[0][-2:], old_pos[-2:]) and not np.array_equal(moved[1][256], old_cell[256])
    assert np.array_equal(moved[0][:-2], old_pos[:-2]) and np.array_equal(moved[1][:256], old_cell[:256])
    w = w.copy()
    w[256, 1, 2] = np.nan
    host.finish(f, w, total=(11, 0))
    ref.finish(f, w, total=(11, 0))
    assert host.state.tolist() == [0, 256, 0, 0]
    for k, want in zip(MANY_NAMES, keep):
        assert np.array_equal(getattr(host, k).view(np.uint8), want.view(np.uint8)), k
    same_state(host, ref)
