#!/usr/bin/env python3
"""ms per NEB evaluation (= one force evaluation of every image): `DeviceNEB.run(n)` (hermnet_amd/neb.py: the projection and
FIRE on the band inside the replayed graph) against the host-driven loop it replaces -- `GraphedBatchMDStep(pos)` on the
images + `fetch()` + the numpy NEB of the tests (tests/neb_reference.py: NumpyNEB, the same arithmetic in the same order) per
evaluation.  Both arms in ONE process, alternating, same band, model and start state; a window ends in a synchronisation (the
device arm's in `fetch()`).  `fmax` is set out of reach, so every evaluation of a window moves every interior image.

    python tools/neb_bench.py [--steps 100] [--rounds 5] [--out profiles/device_neb.json]
    python tools/neb_bench.py --launches profiles/device_neb_launches.txt      # device activity of the replays

Cases: one band of 8 images of 32 atoms (2x2x2) and one of 8 images of 108 atoms (3x3x3): an fcc alloy cell rattled with two
seeds as the end points, linear interpolation between them, climbing image on; model of BASELINE configs[1]."""
import json
import statistics

import numpy as np
from resident_bench import FMAX, fetched, launch_table, main, model_for, ms, on_device, time_arms  # (sets the path)
import torch

from hermnet_amd import neb, synth
from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.relax import DeviceRelax
from neb_reference import NumpyNEB, layout

IMAGES = 8
CASES = [("8 x 32 atoms", (2, 2, 2)), ("8 x 108 atoms", (3, 3, 3))]


def band(reps, sigma, images=IMAGES):
    """(pos [images*n,3], cell [images,3,3], z, batch, graph_ptr, band_ptr): the lattice rattled with two seeds (not wrapped),
    the images between by `neb.interpolate`."""
    lattice, cell, z = synth.fcc_alloy_atoms(reps=reps, sigma=0.0, seed=0)
    ends = [lattice + np.random.RandomState(s).normal(scale=sigma, size=lattice.shape) for s in (1, 2)]
    graph_ptr, band_ptr, _, batch = layout([len(z)], [images])
    return (neb.interpolate(ends[0], ends[1], images).reshape(-1, 3), np.tile(cell, (images, 1, 1)), np.tile(z, images), batch,
            graph_ptr, band_ptr)


class HostLoop(object):
    """One evaluation = upload float32(x), replay, `fetch()` (one copy + synchronisation), NumpyNEB on the host."""

    def __init__(self, model, pos, cell_t, z_t, batch_t, graph_ptr, band_ptr, dev, capacity):
        p0 = torch.from_numpy(pos.astype(np.float32)).to(dev)
        self.step = GraphedBatchMDStep(model, z_t, cell_t, p0, batch_t, len(graph_ptr) - 1, capacity=capacity)
        self.opt = NumpyNEB(pos, graph_ptr, band_ptr, k=0.1, fmax=FMAX, climb=True)
        self.ok = True

    def run(self, n):
        for _ in range(n):
            self.step(torch.from_numpy(self.opt.advance()))
            e, f, ok, found = self.step.fetch()
            self.ok = self.ok and ok
            self.opt.finish(f, e, total=(found, 0))


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per NEB evaluation of the whole band (improved tangents, climbing image, k 0.1, FIRE with ASE defaults, end "
                   "points rattled by %.2f A, fmax out of reach): DeviceNEB.run(n) + one fetch() per window vs graphed batch step + "
                   "fetch() + numpy NEB (tests/neb_reference.py: NumpyNEB, a Python loop over the images) per evaluation; %d "
                   "alternating rounds of %d evaluations, median (min, max)" % (a.sigma, a.rounds, a.steps), "cases": []}
    for name, reps in CASES:
        pos, cell, z, batch, graph_ptr, band_ptr = band(reps, a.sigma)
        z_t, cell_t, _, kw, first, capacity = on_device(dev, pos, cell, z, batch, a.margin)    # both arms on the same column count
        host = HostLoop(model, pos, cell_t, z_t, kw["batch"], graph_ptr, band_ptr, dev, capacity)
        nb = neb.DeviceNEB(model, z_t, cell_t, pos, k=0.1, climb=True, fmax=FMAX, log_steps=max(a.steps, 64), capacity=capacity, **kw)
        host.run(10)
        nb.run(10)
        nb.fetch()
        t, last = time_arms([("host", a.steps, host.run, dict(sync=True)), ("dev", a.steps, fetched(nb))], a.rounds)
        snap = last["dev"]
        same = bool(np.array_equal(snap.positions, host.opt.x) and np.array_equal(snap.velocities, host.opt.v))
        row = {"case": name, "atoms": int(len(z)), "images": IMAGES, "edges_at_start": first, "capacity": capacity,
               "host_loop_ms": ms(t["host"]), "device_neb_ms": ms(t["dev"]),
               "ratio_host_over_device": statistics.median(t["host"]) / statistics.median(t["dev"]),
               "device_steps_done": snap.step, "device_halted": bool(snap.halted), "host_loop_lists_complete": bool(host.ok),
               "fmax_at_end": float(snap.fmax.max()), "climbing_image": int(snap.climbing_image[0]), "arms_end_bit_equal": same}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    return out


def launches(a):
    """Device activity of two DeviceRelax replays and of two DeviceNEB replays on the same batch of 5 x 32 atoms: the kernels
    by name and count, and every memcpy / memset the profiler saw."""
    dev = torch.device("cuda:0")
    model = model_for(dev)
    pos, cell, z, batch, graph_ptr, band_ptr = band((2, 2, 2), a.sigma, images=5)
    z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
    kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=5, fmax=FMAX)
    plain_rx = DeviceRelax(model, z_t, cell_t, pos, **kw)
    band_nb = neb.DeviceNEB(model, z_t, cell_t, pos, **kw)
    plain_rx.run(4)
    band_nb.run(4)
    torch.cuda.synchronize()
    launch_table("device activity of 2 replays, batch of 5 x 32 atoms: DeviceRelax.run(2) | DeviceNEB.run(2)",
                 "DeviceRelax", lambda: plain_rx.run(2), "DeviceNEB", lambda: band_nb.run(2), a.launches)


if __name__ == "__main__":
    main("neb_bench", bench, launches,
         flags=[("--steps", dict(type=int, default=100)),
                ("--sigma", dict(type=float, default=0.08, help="rattle of the two end points (A)"))])
