#!/usr/bin/env python3
"""ms per time step of a ring polymer: `DevicePIMD.run(n)` (hermnet_amd/pimd.py: the normal-mode propagation inside the
replayed graph) against the host-driven loop it replaces, and against the same batch without the springs.  Three arms in ONE
process, alternating, same beads, model and start state; a window ends in a synchronisation:

    (a) host loop    a plain `GraphedBatchMDStep`; every step the float32 coordinates go up, energies and forces come down,
                     and the ring's step is numpy (tests/pimd_reference.py: NumpyPIMD, the same arithmetic)
    (b) DevicePIMD   run(steps) + one fetch() per window
    (c) DeviceMD     Langevin on the same, uncoupled batch at P T, run(steps) + one fetch(): (b) - (c) is what the coupling costs

The timed windows run the PILE-L thermostat (the Gaussians of arm (a) are the library's host form; the device's differ in
the last digits, so those arms end close, not equal).  Behind them both PIMD arms run `--check` steps WITHOUT the thermostat
from one start and must end bit-equal.

    python tools/pimd_bench.py [--steps 200] [--rounds 5] [--out profiles/device_pimd.json]
    python tools/pimd_bench.py --launches profiles/device_pimd_launches.txt      # device activity of the replays

Cases: 8 beads of 32 atoms (2x2x2) and 8 of 108 atoms (3x3x3) of the fcc alloy cell, T = 300 K, tau0 = 100 fs, dt 0.5 fs; model
of BASELINE configs[1]."""
import json
import statistics
import sys

import numpy as np
from resident_bench import copies, fetched, launch_table, main, model_for, ms, on_device, time_arms  # (sets the path)
import torch

from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.md import DeviceMD
from hermnet_amd.pimd import DevicePIMD
from pimd_reference import NumpyPIMD

BEADS, DT, T, TAU0, SEED = 8, 0.5, 300.0, 100.0, 2024
CASES = [("8 x 32 atoms", (2, 2, 2)), ("8 x 108 atoms", (3, 3, 3))]


def ring(reps, beads):
    """(pos, cells [P,3,3], z, masses, batch, velocities) of P beads of one rattled cell, spread by 0.02 A around their atom,
    Maxwell-Boltzmann velocities at P T."""
    return copies(reps, [beads * T] * beads, spread=0.02)


class HostLoop(object):
    """Arm (a): the ring polymer's step on the host around a graphed step that knows nothing of it."""

    def __init__(self, model, z_t, cells_t, batch_t, x, v, m, cell, capacity, thermostat, dev):
        self.dev = dev
        self.ref = NumpyPIMD(BEADS, x, v, m, DT, T, tau0=TAU0, thermostat=thermostat, seed=SEED, cell=cell, log_steps=8)
        self.step = GraphedBatchMDStep(model, z_t, cells_t, torch.from_numpy(self.ref.pos32).to(dev), batch_t, BEADS,
                                       capacity=capacity)
        _, self.ref.f_prev = self._forces(self.ref.pos32)

    def _forces(self, pos32):
        e, f = self.step(torch.from_numpy(pos32).to(self.dev))
        return e.cpu().numpy(), f.cpu().numpy()

    def run(self, n):
        for _ in range(n):
            e, f = self._forces(self.ref.advance())
            ok, found = self.step.check()
            if not ok:
                sys.exit("pimd_bench: the host loop's list overflowed -- raise --margin")
            self.ref.finish(f, e, total=(found, 0))


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per time step of a ring polymer of %d beads (T %g K, dt %g fs, PILE-L, tau0 %g fs): (a) GraphedBatchMDStep + "
                   "download + NumpyPIMD + upload every step, (b) DevicePIMD.run(n) + one fetch() per window, (c) DeviceMD "
                   "Langevin on the same uncoupled batch at P T, run(n) + one fetch() per window; %d alternating rounds of %d "
                   "steps, median (min, max)" % (BEADS, T, DT, TAU0, a.rounds, a.steps),
           "cases": []}
    for name, reps in CASES:
        x, cells, z, m, batch, v = ring(reps, BEADS)
        cell = cells[0]
        z_t, cells_t, _, kw, first, capacity = on_device(dev, x, cells, z, batch, a.margin)    # every arm on the same column count
        batch_t = kw["batch"]
        kw.update(seed=SEED, velocities=v, log_steps=max(a.steps, a.check, 64), capacity=capacity)
        pimd = DevicePIMD(model, z_t, cells_t, x, m, DT, T, tau0=TAU0, **kw)
        plain = DeviceMD(model, z_t, cells_t, x, m, DT, temperature=BEADS * T, friction=1.0 / TAU0, **kw)
        host = HostLoop(model, z_t, cells_t, batch_t, x, v, m, cell, capacity, True, dev)
        t, last = time_arms([("host", a.steps, host.run, dict(sync=True)), ("pimd", a.steps, fetched(pimd)), ("plain", a.steps, fetched(plain))],
                            a.rounds)
        snap, psnap = last["pimd"], last["plain"]
        close = float(np.abs(snap.positions - host.ref.x).max())
        # thermostat off, both arms from one start: bit-equal
        rpmd = DevicePIMD(model, z_t, cells_t, x, m, DT, T, thermostat=False, **kw)
        href = HostLoop(model, z_t, cells_t, batch_t, x, v, m, cell, capacity, False, dev)
        rpmd.run(a.check)
        href.run(a.check)
        end = rpmd.fetch()
        same = bool(np.array_equal(end.positions.view(np.uint64), href.ref.x.view(np.uint64))
                    and np.array_equal(end.velocities.view(np.uint64), href.ref.v.view(np.uint64))
                    and np.array_equal(end.images, href.ref.image) and end.step == a.check and not end.halted)
        row = {"case": name, "atoms": int(len(z)), "beads": BEADS, "edges_at_start": first, "capacity": capacity,
               "host_loop_ms": ms(t["host"]), "device_pimd_ms": ms(t["pimd"]), "device_md_ms": ms(t["plain"]),
               "ratio_host_over_device": statistics.median(t["host"]) / statistics.median(t["pimd"]),
               "coupling_cost_ms": statistics.median(t["pimd"]) - statistics.median(t["plain"]),
               "steps_done": [int(host.ref.state[0]), int(snap.step), int(psnap.step)],
               "halted": [bool(host.ref.state[1]), bool(snap.halted), bool(psnap.halted)],
               "thermostatted_arms_max_position_difference": close,
               "rpmd_check_steps": a.check, "rpmd_arms_end_bit_equal": same}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    return out


def launches(a):
    """Device activity of two DeviceMD replays and of two DevicePIMD replays on the same batch of 5 x 32 atoms: the kernels by
    name and count, and every memcpy / memset the profiler saw."""
    dev, beads = torch.device("cuda:0"), 5
    model = model_for(dev)
    x, cells, z, m, batch, v = ring((2, 2, 2), beads)
    z_t, cells_t = torch.from_numpy(z).to(dev), torch.from_numpy(cells.astype(np.float32)).to(dev)
    kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=beads, seed=SEED, velocities=v)
    plain_md = DeviceMD(model, z_t, cells_t, x, m, DT, temperature=beads * T, friction=1.0 / TAU0, **kw)
    polymer = DevicePIMD(model, z_t, cells_t, x, m, DT, T, tau0=TAU0, **kw)
    plain_md.run(4)
    polymer.run(4)
    torch.cuda.synchronize()
    launch_table("device activity of 2 replays, batch of 5 x 32 atoms: DeviceMD.run(2) | DevicePIMD.run(2)",
                 "DeviceMD", lambda: plain_md.run(2), "DevicePIMD", lambda: polymer.run(2), a.launches)


if __name__ == "__main__":
    main("pimd_bench", bench, launches,
         flags=[("--steps", dict(type=int, default=200)),
                ("--check", dict(type=int, default=20, help="steps of the bit-equality run without the thermostat"))])
