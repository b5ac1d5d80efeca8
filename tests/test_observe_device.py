"""GPU: the MD observers (`hermnet_amd.observe`: Frames, RDF, MSD) inside the replayed step of `DeviceMD`, `DeviceNPT`,
`DeviceREMD` and `DevicePIMD` -- against a second, unobserved driver that is fetched after every step and the numpy
transcription (tests/observe_reference.py) applied to what it showed: frames as equal float32, pair counts as equal integers,
displacement sums as equal bits; the observers leave the trajectory alone; void replays and resume() leave the observers
alone; run() refuses to overwrite ring entries that were not fetched."""
from collections import Counter

import numpy as np
import pytest
import torch

from hermnet_amd import synth
from hermnet_amd.md import _inverse3
from hermnet_amd.observe import MSD, RDF, Frames
from md_reference import KB, AMU, bits
from observe_reference import NumpyFrames, NumpyMSD, NumpyRDF, state_words
import test_md_device as mdt
import test_npt_device as nptt
import test_pimd_device as pt
import test_remd_device as rt

pytestmark = pytest.mark.gpu

R_MAX, BINS = 3.5, 35          # the smallest box of these systems is 7.2 A


def _big():
    """32 and 300 atoms: the second graph spans two tiles of the pair kernel."""
    parts = [synth.fcc_alloy_atoms(reps=r, seed=s) for s, r in enumerate([(2, 2, 2), (3, 5, 5)])]
    pos, z = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
    batch = np.repeat(np.arange(2), [len(p[0]) for p in parts])
    m = np.array([mdt.MASS[int(v)] for v in z])
    v = np.random.RandomState(5).normal(size=(len(m), 3)) * np.sqrt(KB * mdt.HOT / (m * AMU))[:, None]
    return dict(pos=pos, cell=np.stack([p[1] for p in parts]), z=z, m=m, v=v, batch=batch)


SYSTEMS = {"single": mdt._single, "batch": mdt._batched, "big": _big}


def _ptr(s):
    n = len(s["z"])
    return np.array([0, n]) if s["batch"] is None else np.searchsorted(s["batch"], np.arange(int(s["batch"][-1]) + 2))


def _all_three():
    return [Frames(stride=3, frames=16, velocities=True, images=True), RDF(r_max=R_MAX, bins=BINS, stride=2), MSD(stride=1, rows=32)]


def _walk(driver, steps):
    """The snapshots of an unobserved driver at the steps 0..steps: one fetch behind every step."""
    snaps = [driver.fetch()]
    for _ in range(steps):
        driver.run(1)
        snaps.append(driver.fetch())
    assert [s.step for s in snaps] == list(range(steps + 1))
    return snaps


def _references(s, snaps, cells=None, invs=None, slot_of=None, observers=None):
    """The numpy observers offered every snapshot; cells / invs: per step (default: the constant float32 cell and the
    inverse DeviceMD makes of it)."""
    ptr, B = _ptr(s), len(_ptr(s)) - 1
    c32 = s["cell"].astype(np.float32).reshape(B, 3, 3)
    inv0 = np.linalg.inv(c32.astype(np.float64))
    f = NumpyFrames(len(s["z"]), B, 3, 16, velocities=True, images=True)
    r = NumpyRDF(s["z"], ptr, R_MAX, BINS, 2)
    m = NumpyMSD(s["z"], ptr, 1, 32)
    for k, snap in enumerate(snaps):
        state = state_words(snap.step)
        cell, inv = (c32, inv0) if cells is None else (cells[k], invs[k])
        f.offer(state, snap.positions, snap.velocities, snap.images, cell)
        r.offer(state, snap.positions, cell, inv, None if slot_of is None else slot_of[k])
        m.offer(state, snap.positions, snap.images, cell)
    return f, r, m


def _check(got, want, k_frames, k_rows):
    """The fetched observers `got` against the numpy ones (rings not yet wrapped)."""
    f, r, m = got
    nf, nr, nm = want
    assert f.steps.tolist() == nf.steps[:k_frames].tolist() and len(f.steps) == k_frames
    assert np.array_equal(f.positions, nf.positions[:k_frames]) and np.array_equal(f.velocities, nf.velocities[:k_frames])
    assert np.array_equal(f.images, nf.images[:k_frames]) and np.array_equal(f.cell, nf.cells[:k_frames])
    assert np.array_equal(r.counts, nr.counts) and r.counts.sum() > 0
    assert np.array_equal(r.samples, nr.samples) and np.array_equal(r.skipped, nr.skipped)
    assert np.array_equal(bits(r.volume_sum), bits(nr.volume_sum))
    assert m.steps.tolist() == nm.steps[:k_rows].tolist() and len(m.steps) == k_rows
    assert np.array_equal(bits(m.sums), bits(nm.sums[:k_rows]))


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_nve_run_with_all_three_observers(name):
    """20 NVE steps: positions and velocities bit-equal to the same driver without observers; frames = float32 of what the
    unobserved driver shows when fetched after every step; RDF counts = numpy's over those configurations, as integers; MSD
    rows bit-equal to numpy's; g is finite and averages near 1 at the far end."""
    s = SYSTEMS[name]()
    md = mdt._device_md(s, observers=_all_three())
    md.run(20)
    snap = md.fetch()
    snaps = _walk(mdt._device_md(s), 20)
    assert mdt._state_bits(snap) == mdt._state_bits(snaps[-1]) and not snap.halted
    _check(snap.observers, _references(s, snaps), 7, 21)
    r = snap.observers[1]
    assert r.samples.tolist() == [11] * len(r.samples) and r.g.shape == r.counts.shape
    assert len(r.pairs) == 6 and r.pairs[0] == (13, 13) and r.pairs[-1] == (29, 29) and len(r.r) == BINS
    msd = snap.observers[2].msd
    assert msd.shape == (21, len(r.samples), 3) and not msd[0].any() and np.all(msd[-1] > 0)
    # nothing pending: the next fetch carries no ring entries; the counts are cumulative
    again = md.fetch().observers
    assert len(again[0].steps) == 0 and len(again[2].steps) == 0 and np.array_equal(again[1].counts, r.counts)


def test_void_replays_and_resume_leave_the_observers_as_an_uninterrupted_run_does():
    """A capacity the list outgrows at step k (the existing halt test's construction: ordinary padded searches that report
    a flag): the void replays record nothing; after resume() the observers' totals equal the uninterrupted run's, no frame
    twice."""
    s = mdt._single()
    full = mdt._device_md(s, observers=_all_three())
    _, first = full.step.check()
    full.run(30)
    whole = full.fetch()
    counts = whole.log[:, 0, 2].astype(np.int64).tolist()
    at = [k for k in range(2, 30) if counts[k] > max([int(first)] + counts[:k])]
    assert at, "the edge count never exceeded its running maximum: no overflow to test"
    k = at[0]
    md = mdt._device_md(s, capacity=max([int(first)] + counts[:k]), observers=_all_three())
    md.run(30)
    halted = md.fetch()
    assert halted.halted and halted.step == k and (halted.halt_code & mdt.HALT_CAPACITY)
    f, r, m = halted.observers
    assert f.steps.tolist() == list(range(0, k + 1, 3)) and m.steps.tolist() == list(range(k + 1))
    assert r.samples.tolist() == [k // 2 + 1]
    md.run(3)                                            # halted: replays change nothing
    idle = md.fetch().observers
    assert len(idle[0].steps) == 0 and len(idle[2].steps) == 0 and np.array_equal(idle[1].counts, r.counts)
    assert np.array_equal(idle[1].samples, r.samples)
    md.resume()
    md.run(30 - k)
    end = md.fetch()
    assert (end.step, end.halted) == (30, False) and mdt._state_bits(end) == mdt._state_bits(whole)
    f2, r2, m2 = end.observers
    wf, wr, wm = whole.observers
    assert f.steps.tolist() + f2.steps.tolist() == wf.steps.tolist() == list(range(0, 31, 3))
    assert np.array_equal(np.concatenate([f.positions, f2.positions]), wf.positions)
    assert np.array_equal(np.concatenate([f.velocities, f2.velocities]), wf.velocities)
    assert np.array_equal(r2.counts, wr.counts) and np.array_equal(r2.samples, wr.samples) and r2.samples.tolist() == [16]
    assert m.steps.tolist() + m2.steps.tolist() == wm.steps.tolist() == list(range(31))
    assert np.array_equal(bits(np.concatenate([m.sums, m2.sums])), bits(wm.sums))


def test_under_a_barostat_frames_carry_their_cell_and_counts_follow_it():
    """`DeviceNPT`, 12 steps: each frame's cell is the (float32) cell fetched at that step, the counts are numpy's with the
    per-step cells and the inverses the driver keeps, the MSD rows numpy's with the current cell."""
    name = "single"
    s = nptt._system(name)
    kw = dict(pressure=nptt._target(name), compressibility=nptt._compressibility(name))
    md = nptt._npt(s, observers=_all_three(), **kw)
    md.run(12)
    snap = md.fetch()
    snaps = _walk(nptt._npt(s, **kw), 12)
    assert mdt._state_bits(snap) == mdt._state_bits(snaps[-1]) and np.array_equal(bits(snap.cell), bits(snaps[-1].cell))
    cells = [t.cell.astype(np.float32) for t in snaps]
    assert not np.array_equal(cells[0], cells[-1])
    invs = [_inverse3(c.astype(np.float64)) for c in cells]
    _check(snap.observers, _references(s, snaps, cells, invs), 5, 13)
    f = snap.observers[0]
    for k, step in enumerate(f.steps):
        assert np.array_equal(f.cell[k], cells[step])


def test_remd_histograms_by_rung_follow_the_temperatures():
    """`DeviceREMD`, exchange every 2 steps, RDF(by_rung=True): the counts of slot r are numpy's accumulated with the rung
    each replica held behind the previous step's exchange (the log's last column)."""
    s = rt._hot_system()
    remd = rt._remd(2, observers=[RDF(r_max=R_MAX, bins=BINS, stride=1, by_rung=True)])
    remd.run(20)
    snap = remd.fetch()
    snaps = _walk(rt._remd(2), 20)
    assert rt._state_bits(snap) == rt._state_bits(snaps[-1])
    rungs = [np.arange(4)] + [snap.log[k, :, 4].astype(np.int64) for k in range(20)]
    assert any(not np.array_equal(r, np.arange(4)) for r in rungs), "no exchange was accepted: nothing by_rung to test"
    ref = NumpyRDF(s["z"], _ptr(s), R_MAX, BINS, 1)
    c32 = s["cell"].astype(np.float32)
    inv = np.linalg.inv(c32.astype(np.float64))
    for k, t in enumerate(snaps):
        ref.offer(state_words(t.step), t.positions, c32, inv, rungs[k])
    got = snap.observers[0]
    assert np.array_equal(got.counts, ref.counts) and got.samples.tolist() == [21] * 4
    by_replica = NumpyRDF(s["z"], _ptr(s), R_MAX, BINS, 1)
    for t in snaps:
        by_replica.offer(state_words(t.step), t.positions, c32, inv)
    assert not np.array_equal(by_replica.counts, ref.counts)
    with pytest.raises(ValueError, match="DeviceREMD alone"):
        mdt._device_md(mdt._batched(), observers=[RDF(r_max=R_MAX, bins=BINS, by_rung=True)])


def test_pimd_counts_per_bead():
    """`DevicePIMD`, four beads, thermostatted: per-bead counts equal numpy's over the configurations an unobserved ring
    polymer shows (beads sit slightly outside the cell: the fractional difference does not mind)."""
    s = pt._system()
    pimd = pt._pimd(observers=[RDF(r_max=R_MAX, bins=BINS, stride=2), Frames(stride=5, frames=8)])
    pimd.run(10)
    snap = pimd.fetch()
    snaps = _walk(pt._pimd(), 10)
    assert pt._state_bits(snap) == pt._state_bits(snaps[-1])
    ref = NumpyRDF(s["z"], _ptr(s), R_MAX, BINS, 2)
    c32 = s["cell"].astype(np.float32)
    inv = np.linalg.inv(c32.astype(np.float64))
    for t in snaps:
        ref.offer(state_words(t.step), t.positions, c32, inv)
    got, frames = snap.observers
    assert np.array_equal(got.counts, ref.counts) and got.samples.tolist() == [6] * pt.BEADS
    assert len(set(c.tobytes() for c in got.counts)) == pt.BEADS                   # the beads really differ
    assert frames.steps.tolist() == [0, 5, 10]
    assert np.array_equal(frames.positions, np.stack([snaps[k].positions.astype(np.float32) for k in (0, 5, 10)]))


def test_run_refuses_to_overwrite_ring_entries_and_the_rings_wrap():
    s = mdt._batched()
    md = mdt._device_md(s, observers=[Frames(stride=2, frames=4), MSD(stride=3, rows=2)])
    with pytest.raises(RuntimeError, match="frames not fetched"):
        md.run(8)                                        # steps 0, 2, 4, 6, 8: five frames
    with pytest.raises(RuntimeError, match="MSD rows not fetched"):
        md.run(6)                                        # four frames fit, the rows of steps 0, 3, 6 do not
    md.run(5)
    with pytest.raises(RuntimeError, match="MSD rows not fetched"):
        md.run(2)
    first = md.fetch().observers
    assert first[0].steps.tolist() == [0, 2, 4] and first[1].steps.tolist() == [0, 3]
    with pytest.raises(RuntimeError, match="MSD rows not fetched"):
        md.run(8)                                        # 6, 9, 12
    md.run(6)                                            # 6, 8, 10 and 6, 9: both rings wrap
    snap = md.fetch()
    f, m = snap.observers
    assert snap.step == 11 and f.steps.tolist() == [6, 8, 10] and m.steps.tolist() == [6, 9]
    assert np.all(m.msd > 0) and not np.array_equal(f.positions[0], f.positions[2])
    with pytest.raises(ValueError, match="one per driver"):
        mdt._device_md(s, observers=md._observers)
    # the driver's constructor refuses an r_max above half a cell height (7.2 A boxes): rounding would miss images
    with pytest.raises(ValueError, match="half the smallest cell height of graph 0"):
        mdt._device_md(s, observers=[RDF(r_max=3.7, bins=BINS)])


def test_an_observed_replay_adds_six_kernels_and_no_copies():
    """The device activity of two replays with and without the three observers: two kernels more per observer and replay,
    no memcpy or memset."""
    from torch.profiler import ProfilerActivity, profile
    s = mdt._batched()

    def events(driver):
        driver.run(2)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            driver.run(2)
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    plain, ours = events(mdt._device_md(s)), events(mdt._device_md(s, observers=_all_three()))
    assert sum(plain.values()) > 0, "the profiler recorded no device activity for graph launches"
    assert sum(ours.values()) == sum(plain.values()) + 12, (ours - plain, plain - ours)
    assert not [k for k in ours if "memcpy" in k.lower() or "memset" in k.lower()]
    assert sum(v for k, v in ours.items() if "obs_" in k) == 12
