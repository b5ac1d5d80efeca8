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
import json
import statistics

import numpy as np
from resident_bench import cells, fetched, launch_table, main, model_for, ms, on_device, time_arms  # (sets the path)
import torch

from hermnet_amd.md import DeviceMD

CASES = [("108 atoms", [(3, 3, 3)], 5.0), ("1008 atoms", [(6, 6, 7)], 5.0), ("64 x 32 atoms", [(2, 2, 2)] * 64, 3.5),
         ("configs[1], 10000 atoms", [(10, 10, 25)], 6.0)]
BINS, STRIDE, FRAME_STRIDE = 120, 5, 10


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
        pos, cell, z, m, batch, v = cells(members, a.temp)
        B, big = len(members), len(z) > 5000
        z_t, cells_t, _, kw, first, capacity = on_device(dev, pos, cell, z, batch, a.margin)
        kw.update(velocities=v, log_steps=max(a.steps, 64), capacity=capacity)
        plain = DeviceMD(model, z_t, cells_t, pos, m, a.dt, **kw)
        row = {"case": name, "atoms": int(len(z)), "graphs": B, "edges_at_start": first, "capacity": capacity}
        arms = [("a", a.steps, fetched(plain))]
        if a.plain_only:
            observed = None
        else:
            from hermnet_amd.observe import MSD, RDF, Frames
            obs = [Frames(stride=FRAME_STRIDE, frames=64), RDF(r_max=r_max, bins=BINS, stride=STRIDE), MSD(stride=STRIDE, rows=64)]
            observed = DeviceMD(model, z_t, cells_t, pos, m, a.dt, observers=obs, **kw)
            host = HostLoop(DeviceMD(model, z_t, cells_t, pos, m, a.dt, **kw), z, np.searchsorted(batch, np.arange(B + 1)), cell, r_max)
            row.update(r_max=r_max, rdf_workgroups=int(obs[1].work.shape[0]))
            steps_c = a.big_steps if big else a.steps
            # (the host loop's window ends in its last fetch(); on the big cell it takes part in the first round alone)
            arms += [("b", a.steps, fetched(observed)), ("c", steps_c, host.run, dict(rounds=lambda r: not big or r == 0))]
        t, last = time_arms(arms, a.rounds)
        t_a, sa = t["a"], last["a"]
        row.update(plain_ms=ms(t_a), steps_done=int(sa.step), halted=bool(sa.halted))
        if observed is not None:
            t_b, t_c, sb, sc = t["b"], t["c"], last["b"], last["c"]
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
    return out


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
    from hermnet_amd.observe import MSD, RDF, Frames
    dev = torch.device("cuda:0")
    model = model_for(dev)
    pos, cell, z, m, batch, v = cells([(3, 3, 3)], a.temp)
    z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell[0].astype(np.float32)).to(dev)
    plain_md = DeviceMD(model, z_t, cell_t, pos, m, a.dt, velocities=v)
    observed = DeviceMD(model, z_t, cell_t, pos, m, a.dt, velocities=v,
                        observers=[Frames(stride=FRAME_STRIDE), RDF(r_max=5.0, bins=BINS, stride=STRIDE), MSD(stride=STRIDE)])
    plain_md.run(4)
    observed.run(4)
    torch.cuda.synchronize()
    launch_table("device activity of 2 replays, 108 atoms: DeviceMD.run(2) | DeviceMD(observers=[Frames, RDF, MSD]).run(2)",
                 "plain", lambda: plain_md.run(2), "observed", lambda: observed.run(2), a.launches, inside="the observed run(2)")


if __name__ == "__main__":
    main("observe_bench", bench, launches,
         flags=[("--steps", dict(type=int, default=200)),
                ("--big-steps", dict(type=int, default=10, help="steps of the host loop's one round on the 10,000-atom cell")),
                ("--dt", dict(type=float, default=0.5)), ("--temp", dict(type=float, default=300.0)),
                ("--only", dict(default=None, help="cases whose name contains this")), ("--plain-only", dict(action="store_true")),
                ("--parent", dict(default=None, help="the --out of a --plain-only run on the parent commit: recorded beside every case"))])
