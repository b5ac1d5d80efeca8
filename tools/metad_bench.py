#!/usr/bin/env python3
"""ms per time step of multiple-walker metadynamics: `DeviceMetaD.run(n)` (hermnet_amd/metad.py: CVs, bias and deposits
inside the replayed graph) against the same batch without bias, and against the host-driven loop it replaces.  Three arms in
ONE process, alternating, same walkers, model, seed and start state; a window ends in a synchronisation (a `fetch()`):

    (1) DeviceMD     Langevin on the same uncoupled batch, run(steps) + one fetch(): (2) - (1) is what the feature costs
    (2) DeviceMetaD  run(steps) + one fetch() per window
    (3) host loop    `GraphedBatchMDStep` + its fetch() every step, the integrator, the CVs and the bias in numpy
                     (tests/metad_reference.py: NumpyMetaD, the same arithmetic), the coordinates uploaded for the next step;
                     `--host-steps` steps per window (its cost per step does not depend on the window)

    python tools/metad_bench.py [--steps 200] [--rounds 5] [--out profiles/device_metad.json]
    python tools/metad_bench.py --launches profiles/device_metad_launches.txt     # device activity of the replays, and the
                                                                                  # pair kernel's time alone

Cases: 8 walkers of 32 atoms (2x2x2) and 8 of 108 atoms (3x3x3) of the fcc alloy cell at 600 K, friction 0.01 /fs, dt 1 fs,
one `Distance` and one `Coordination` over all atoms, each at 0 and at max_hills / 2 = 8192 preloaded hills (pace beyond the
run: the list stays as long as it is); model of BASELINE configs[1]."""
import json
import re
import statistics

import numpy as np
from resident_bench import copies, device_events, fetched, launch_table, main, model_for, ms, on_device, time_arms  # (sets the path)
import torch

from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.md import DeviceMD
from hermnet_amd.metad import Coordination, DeviceMetaD, Distance
from metad_reference import NumpyMetaD

WALKERS, DT, FRICTION, SEED, T, MAX_HILLS = 8, 1.0, 0.01, 2024, 600.0, 16384
CASES = [("8 x 32 atoms", (2, 2, 2)), ("8 x 108 atoms", (3, 3, 3))]
HEIGHT, SIGMA, PACE = 0.01, [0.05, 1.0], 10 ** 9


def cvs_for(n_rep):
    return [Distance([0], [1]), Coordination(range(n_rep), range(n_rep), 2.8, nn=6, r_cut=3.5)]


def preloaded(count, n_rep):
    """`count` low hills scattered around the start's CV values (a distance of 2.5 A, a coordination of 6.5 per atom)."""
    if count == 0:
        return None
    rs = np.random.RandomState(3)
    return np.stack([rs.normal(2.5, 0.3, count), rs.normal(6.5 * n_rep, 0.1 * n_rep, count)], axis=1), rs.uniform(0.0, 1e-3, count)


class HostLoop(object):
    """Arm (3): the integrator, the CVs and the bias in numpy around a captured evaluation that knows nothing of them."""

    def __init__(self, model, z_t, cell_t, pos, cell, m, batch_t, v, hills, capacity, n_rep):
        p0 = torch.from_numpy(pos.astype(np.float32)).to(z_t.device)
        self.step = GraphedBatchMDStep(model, z_t, cell_t, p0, batch_t, WALKERS, capacity=capacity)
        self.ref = NumpyMetaD(WALKERS, pos, v, m, DT, cell[0], cvs_for(n_rep), HEIGHT, SIGMA, PACE, T, friction=FRICTION,
                              max_hills=MAX_HILLS, hills=hills, seed=SEED, log_steps=64)
        self.ref.state[3] = 1
        self._finish(self.ref.advance())

    def _finish(self, pos32):
        self.step(torch.from_numpy(np.ascontiguousarray(pos32)))       # the upload
        e, f, ok, n = self.step.fetch()                                 # the download
        self.ref.finish(f, e, total=(n, 0 if ok else 1), capacity=self.step.capacity)

    def run(self, n):
        for _ in range(n):
            self._finish(self.ref.advance())


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per time step of %d walkers (dt %g fs, Langevin %g /fs at %g K, one Distance and one Coordination over all "
                   "atoms, well-tempered off, no deposit inside the windows): (1) DeviceMD.run(n) + one fetch() per window, (2) "
                   "DeviceMetaD.run(n) + one fetch() per window, (3) GraphedBatchMDStep + fetch() + NumpyMetaD + upload every "
                   "step (%d steps per window); %d alternating rounds of %d steps, median (min, max)"
                   % (WALKERS, DT, FRICTION, T, a.host_steps, a.rounds, a.steps), "cases": []}
    for name, reps in CASES:
        pos, cell, z, m, batch, v = copies(reps, [T] * WALKERS)
        n_rep = len(z) // WALKERS
        z_t, cell_t, _, kw, first, capacity = on_device(dev, pos, cell, z, batch, a.margin)    # every arm on the same column count
        batch_t = kw["batch"]
        kw.update(seed=SEED, velocities=v, log_steps=max(a.steps, 64), capacity=capacity)
        for count in (0, MAX_HILLS // 2):
            hills = preloaded(count, n_rep)
            plain = DeviceMD(model, z_t, cell_t, pos, m, DT, temperature=T, friction=FRICTION, **kw)
            ours = DeviceMetaD(model, z_t, cell_t, pos, m, DT, cvs_for(n_rep), HEIGHT, SIGMA, PACE, T, friction=FRICTION,
                               max_hills=MAX_HILLS, hills=hills, **kw)
            host = HostLoop(model, z_t, cell_t, pos, cell, m, batch_t, v, hills, capacity, n_rep)
            t, last = time_arms([("plain", a.steps, fetched(plain)), ("ours", a.steps, fetched(ours)),
                                 ("host", a.host_steps, host.run, dict(sync=True))], a.rounds)
            t_plain, t_ours, t_host, psnap, snap = t["plain"], t["ours"], t["host"], last["plain"], last["ours"]
            row = {"case": name, "atoms": int(len(z)), "walkers": WALKERS, "hills": count, "edges_at_start": first,
                   "capacity": capacity, "device_md_ms": ms(t_plain), "device_metad_ms": ms(t_ours), "host_loop_ms": ms(t_host),
                   "bias_cost_ms": statistics.median(t_ours) - statistics.median(t_plain),
                   "ratio_metad_over_md": statistics.median(t_ours) / statistics.median(t_plain),
                   "ratio_host_over_device": statistics.median(t_host) / statistics.median(t_ours),
                   "steps_done": [int(psnap.step), int(snap.step), int(host.ref.state[0])],
                   "halted": [bool(psnap.halted), bool(snap.halted), bool(host.ref.state[1] != 0)],
                   "hill_count": int(snap.hill_count), "last_cv_row": snap.cv_log[-1, 0].tolist(),
                   "largest_bias_force": float(np.abs(snap.bias_forces).max())}
            out["cases"].append(row)
            print(json.dumps(row), flush=True)
    return out


def launches(a):
    """Device activity of two DeviceMD replays and of two DeviceMetaD replays on the same batch of 8 x 32 atoms: the kernels
    by name and count, every memcpy / memset the profiler saw, and the mean device time of the stage's four kernels in both
    cases at 0 and at 8192 hills (the pair kernel is metad_cv_kernel)."""
    dev = torch.device("cuda:0")
    model = model_for(dev)
    lines = []
    for name, reps in CASES:
        pos, cell, z, m, batch, v = copies(reps, [T] * WALKERS)
        n_rep = len(z) // WALKERS
        z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
        kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=WALKERS, seed=SEED, velocities=v)
        for count in (0, MAX_HILLS // 2):
            biased = DeviceMetaD(model, z_t, cell_t, pos, m, DT, cvs_for(n_rep), HEIGHT, SIGMA, PACE, T, friction=FRICTION,
                                 max_hills=MAX_HILLS, hills=preloaded(count, n_rep), **kw)
            biased.run(4)
            torch.cuda.synchronize()
            times = {}
            for ev in device_events(lambda: biased.run(20)):
                kernel = re.search(r"metad_\w+", ev.name)
                if kernel:
                    times.setdefault(kernel.group(0), []).append(ev.device_time)
            lines.append("%s, %d hills: mean device time per launch over 20 replays (us): %s"
                         % (name, count, {k: round(statistics.mean(t), 2) for k, t in sorted(times.items())}))
            if name == CASES[0][0] and count == 0:
                plain_md = DeviceMD(model, z_t, cell_t, pos, m, DT, temperature=T, friction=FRICTION, **kw)
                plain_md.run(4)
                torch.cuda.synchronize()
                launch_table("device activity of 2 replays, batch of 8 x 32 atoms: DeviceMD.run(2) | DeviceMetaD.run(2)",
                             "DeviceMD", lambda: plain_md.run(2), "DeviceMetaD", lambda: biased.run(2), a.launches)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.launches, "a") as fh:                   # behind the table
        fh.write(text)


if __name__ == "__main__":
    main("metad_bench", bench, launches,
         flags=[("--steps", dict(type=int, default=200)),
                ("--host-steps", dict(type=int, default=10, help="steps of the host-loop arm per window"))])
