#!/usr/bin/env python3
"""What the MD observers (hermnet_amd/observe.py: Frames, RDF, MSD inside the replayed step) cost, and what they replace.
Three arms in ONE process, alternating, same cell, model and start state; a window ends in a synchronisation:

    (a) plain       `DeviceMD` without observers: run(steps) + one fetch() per window
    (b) observed    `DeviceMD` with Frames(stride 10) + RDF(stride 5) + MSD(stride 5): run(steps) + one fetch() per window
    (c) host loop   `DeviceMD` without observers, a fetch() every 5 steps and the numpy analysis of tests/observe_reference.py
                    on what it shows (a frame every second fetch): the round trip the observers remove

and the pair-histogram kernel alone on the largest cell (hip events around its two launches).  Behind the windows arms (a) and
(b) must stand at bit-equal states, and (b)'s counts must be (c)'s wherever (c) ran the same steps.

    python tools/observe_bench.py [--steps 200] [--rounds 5] [--out profiles/device_observe.json]
    python tools/observe_bench.py --plain-only          # arm (a) alone (it needs no observers: runs on older trees too)
    python tools/observe_bench.py --parent plain.json   # ... and that run's --out, recorded beside every case
    python tools/observe_bench.py --launches profiles/device_observe_launches.txt

Cases: 108 atoms (3x3x3), 1008 atoms (6x6x7), a batch of 64 x 32 atoms (2x2x2), BASELINE configs[1] (10x10x25: 10,000 atoms --
its host loop runs `--big-steps` steps in one round: numpy walks 5e7 pairs per sample); NVE, model of configs[1]."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from hermnet_amd import synth  # noqa: E402
from hermnet_amd.md import AMU_A2_FS2_TO_EV, KB, DeviceMD  # noqa: E402
from hermnet_amd.neighbor import neighbor_search, padded_capacity  # noqa: E402
from relax_bench import model_for  # noqa: E402

MASS = {13: 26.9815, 28: 58.6934, 29: 63.546}
CASES = [("108 atoms", [(3, 3, 3)], 5.0), ("1008 atoms", [(6, 6, 7)], 5.0), ("64 x 32 atoms", [(2, 2, 2)] * 64, 3.5),
         ("configs[1], 10000 atoms", [(10, 10, 25)], 6.0)]
BINS, STRIDE, FRAME_STRIDE = 120, 5, 10


def system(members, temp):
    """(pos, cells [B,3,3], z, masses, batch, velocities) of a batch of rattled alloy cells."""
    parts = [synth.fcc_alloy_atoms(reps=r, seed=s) for s, r in enumerate(members)]
    pos, z = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
    batch = np.repeat(np.arange(len(parts)), [len(p[0]) for p in parts])
    m = np.array([MASS[int(v)] for v in z])
    v = np.random.RandomState(1).normal(size=pos.shape) * np.sqrt(KB * temp / (m * AMU_A2_FS2_TO_EV))[:, None]
    return pos, np.stack([p[1] for p in parts]), z, m, batch, v


def ms(ts):
    return [statistics.median(ts), min(ts), max(ts)]


class HostLoop(object):
    """Arm (c): fetch every STRIDE steps, analyse on the host."""

    def __init__(self, md, z, ptr, cells, r_max):
        from observe_reference import NumpyFrames, NumpyMSD, NumpyRDF, state_words
        B = len(ptr) - 1
        self.md, self.words = md, state_words
        self.cell = cells.astype(np.float32)
        self.inv = np.linalg.inv(self.cell.astype(np.float64))
        self.frames = NumpyFrames(len(z), B, FRAME_STRIDE, 64)
        self.rdf = NumpyRDF(z, ptr, r_max, BINS, STRIDE)
        self.msd = NumpyMSD(z, ptr, STRIDE, 64)
        self._look()

    def _look(self):
        s = self.md.fetch()
        state = self.words(s.step, s.halt_code)
        self.frames.offer(state, s.positions, cell=self.cell)
        self.rdf.offer(state, s.positions, self.cell, self.inv)
        self.msd.offer(state, s.positions, s.images, self.cell)
        return s

    def run(self, n):
        for _ in range(n // STRIDE):
            self.md.run(STRIDE)
            s = self._look()
        return s


def rdf_kernel_ms(md, ob, repeats=20):
    """ms of the RDF observer's two launches on the state `md` stands at (every call made due by hand)."""
    ob.stride = 1
    start, stop, ts = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), []
    for _ in range(repeats):
        ob.obs[0].fill_(-1)
        torch.cuda.synchronize()
        start.record()
        ob._launch(md, md.step)
        stop.record()
        torch.cuda.synchronize()
        ts.append(start.elapsed_time(stop))
    return ms(ts)


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per MD step (NVE, dt %.2f fs, %g K start): (a) DeviceMD.run(n) + one fetch() per window, (b) the same with "
                   "Frames(stride %d) + RDF(stride %d, %d bins) + MSD(stride %d) inside the replay, (c) DeviceMD + fetch() every "
                   "%d steps + the numpy analysis; %d alternating rounds of %d steps, median (min, max)"
                   % (a.dt, a.temp, FRAME_STRIDE, STRIDE, BINS, STRIDE, STRIDE, a.rounds, a.steps), "cases": []}
    for name, members, r_max in CASES:
        if a.only and a.only not in name:
            continue
        pos, cells, z, m, batch, v = system(members, a.temp)
        B, big = len(members), len(z) > 5000
        z_t, cells_t, batch_t = torch.from_numpy(z).to(dev), torch.from_numpy(cells.astype(np.float32)).to(dev), torch.from_numpy(batch).to(dev)
        p0 = torch.from_numpy(pos.astype(np.float32)).to(dev)
        first = int(neighbor_search(p0, 5.0, cells_t, batch=batch_t, num_graphs=B)[0].size(1))
        kw = dict(velocities=v, batch=batch_t, num_graphs=B, log_steps=max(a.steps, 64), capacity=padded_capacity(first, margin=a.margin))
        plain = DeviceMD(model, z_t, cells_t, pos, m, a.dt, **kw)
        row = {"case": name, "atoms": int(len(z)), "graphs": B, "edges_at_start": first, "capacity": kw["capacity"]}
        if a.plain_only:
            observed = host = None
        else:
            from hermnet_amd.observe import MSD, RDF, Frames
            obs = [Frames(stride=FRAME_STRIDE, frames=64), RDF(r_max=r_max, bins=BINS, stride=STRIDE), MSD(stride=STRIDE, rows=64)]
            observed = DeviceMD(model, z_t, cells_t, pos, m, a.dt, observers=obs, **kw)
            host = HostLoop(DeviceMD(model, z_t, cells_t, pos, m, a.dt, **kw), z, np.searchsorted(batch, np.arange(B + 1)), cells, r_max)
            row.update(r_max=r_max, rdf_workgroups=int(obs[1].work.shape[0]))
        t_a, t_b, t_c, sa, sb, sc = [], [], [], None, None, None
        for r in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plain.run(a.steps)
            sa = plain.fetch()
            t_a.append((time.perf_counter() - t0) / a.steps * 1e3)
            if observed is None:
                continue
            t0 = time.perf_counter()
            observed.run(a.steps)
            sb = observed.fetch()
            t_b.append((time.perf_counter() - t0) / a.steps * 1e3)
            steps_c = a.big_steps if big else a.steps
            if not big or r == 0:
                t0 = time.perf_counter()
                sc = host.run(steps_c)
                t_c.append((time.perf_counter() - t0) / steps_c * 1e3)
        row.update(plain_ms=ms(t_a), steps_done=int(sa.step), halted=bool(sa.halted))
        if observed is not None:
            same = bool(np.array_equal(sa.positions.view(np.uint64), sb.positions.view(np.uint64)) and sa.step == sb.step)
            rdf = sb.observers[1]
            counts_equal = None
            if sc.step == sb.step:
                counts_equal = bool(np.array_equal(rdf.counts, host.rdf.counts))
            elif sc.step < a.steps:              # the host loop stopped inside the first window: compare nothing cumulative
                counts_equal = "host loop ran %d steps only: not compared" % sc.step
            row.update(observed_ms=ms(t_b), host_loop_ms=ms(t_c), host_loop_steps_per_round=steps_c,
                       observers_cost_ms=statistics.median(t_b) - statistics.median(t_a),
                       observers_cost_percent=100.0 * (statistics.median(t_b) / statistics.median(t_a) - 1.0),
                       ratio_host_loop_over_observed=statistics.median(t_c) / statistics.median(t_b),
                       observed_state_bit_equal_to_plain=same, rdf_samples=int(rdf.samples[0]), rdf_skipped=int(rdf.skipped.sum()),
                       rdf_pairs_counted=int(rdf.counts.sum()), rdf_counts_equal_host_loop=counts_equal)
            if big:
                row["rdf_kernel_alone_ms"] = rdf_kernel_ms(observed, observed._observers[1])
                n = len(z)
                row["rdf_kernel_pairs"] = n * (n - 1) // 2
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    if a.parent:
        with open(a.parent) as fh:
            add_parent(out, json.load(fh))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


def add_parent(out, parent):
    """Beside every case of `out`: arm (a) as `--plain-only` measured it on the parent commit (same box), and the observed
    arm's cost against that."""
    theirs = {row["case"]: row["plain_ms"] for row in parent["cases"]}
    for row in out["cases"]:
        if row["case"] in theirs and "observed_ms" in row:
            row["parent_commit_plain_ms"] = theirs[row["case"]]
            row["observers_cost_percent_of_parent_plain"] = 100.0 * (row["observed_ms"][0] / theirs[row["case"]][0] - 1.0)
            row["plain_over_parent_plain"] = row["plain_ms"][0] / theirs[row["case"]][0]


def launches(a):
    """Device activity of two replays of DeviceMD without and with the three observers (108 atoms): the kernels by name and
    count, and every memcpy / memset the profiler saw."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    from hermnet_amd.observe import MSD, RDF, Frames
    dev = torch.device("cuda:0")
    model = model_for(dev)
    pos, cells, z, m, batch, v = system([(3, 3, 3)], a.temp)
    z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cells[0].astype(np.float32)).to(dev)
    plain_md = DeviceMD(model, z_t, cell_t, pos, m, a.dt, velocities=v)
    observed = DeviceMD(model, z_t, cell_t, pos, m, a.dt, velocities=v,
                        observers=[Frames(stride=FRAME_STRIDE), RDF(r_max=5.0, bins=BINS, stride=STRIDE), MSD(stride=STRIDE)])
    plain_md.run(4)
    observed.run(4)
    torch.cuda.synchronize()

    def device_events(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    plain, ours = device_events(lambda: plain_md.run(2)), device_events(lambda: observed.run(2))
    lines = ["device activity of 2 replays, 108 atoms: DeviceMD.run(2) | DeviceMD(observers=[Frames, RDF, MSD]).run(2)    (count name)"]
    for name in sorted(set(plain) | set(ours)):
        lines.append("%4d %4d  %s" % (plain.get(name, 0), ours.get(name, 0), name[:150]))
    extra = {k[:100]: c - plain.get(k, 0) for k, c in ours.items() if c != plain.get(k, 0)}
    copies = {k: c for k, c in ours.items() if "memcpy" in k.lower() or "memset" in k.lower()}
    lines.append("kernels: plain %d, observed %d; difference: %s" % (sum(plain.values()), sum(ours.values()), extra))
    lines.append("memcpy / memset activities inside the observed run(2): %d %s" % (sum(copies.values()), copies))
    if not ours:
        lines.append("(the profiler recorded no device activity for graph launches)")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.launches, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--big-steps", type=int, default=10, help="steps of the host loop's one round on the 10,000-atom cell")
    ap.add_argument("--dt", type=float, default=0.5)
    ap.add_argument("--temp", type=float, default=300.0)
    ap.add_argument("--margin", type=float, default=0.25, help="columns of the padded list beyond the first count")
    ap.add_argument("--only", default=None, help="cases whose name contains this")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--parent", default=None, help="the --out of a --plain-only run on the parent commit: recorded beside every case")
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("observe_bench: needs the GPU (nothing is measured without one)")
    launches(a) if a.launches else bench(a)
