#!/usr/bin/env python3
"""ms per MD step: `DeviceMD.run(n)` (hermnet_amd/md.py: the integrator inside the replayed graph) against the host-driven
loop it replaces -- `GraphedMDStep(pos)` + `fetch()` + the torch integrator of tools/md_nve.py (device tensors, one
synchronisation per step for the list check).  Both arms in ONE process, alternating, same cell, model and start state; a
window ends in a synchronisation (the device arm's in `fetch()`).

    python tools/md_device_bench.py [--steps 300] [--rounds 5] [--out profiles/device_md.json]
    python tools/md_device_bench.py --launches profiles/device_md_launches.txt      # device activity of the replays

Cells: 108 atoms (3x3x3), 1008 atoms (6x6x7), BASELINE configs[1] (10x10x25: 10,000 atoms); model of configs[1]."""
import json
import statistics

import numpy as np
from resident_bench import fetched, launch_table, main, model_for, ms, on_device, setup, time_arms  # (sets the path)
import torch

from hermnet_amd.graph import GraphedMDStep
from hermnet_amd.md import AMU_A2_FS2_TO_EV, DeviceMD

CELLS = [("108 atoms", (3, 3, 3)), ("1008 atoms", (6, 6, 7)), ("configs[1], 10000 atoms", (10, 10, 25))]


class HostLoop(object):
    """tools/md_nve.py's velocity Verlet in torch ops around a captured step; forces stay on the device, `fetch()` is the
    step's one copy + synchronisation (energy and the list's flags reach the host, as a driver needs them)."""

    def __init__(self, model, pos, cell, z, m, v, dt, dev, capacity=None):
        self.pos = torch.from_numpy(pos.astype(np.float32)).to(dev)
        self.v = torch.from_numpy(v.astype(np.float32)).to(dev)
        self.m = torch.from_numpy((m * AMU_A2_FS2_TO_EV).astype(np.float32)).to(dev)[:, None]
        cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
        self.box, self.dt = torch.diagonal(cell_t).clone(), dt
        self.step = GraphedMDStep(model, torch.from_numpy(z).to(dev), cell_t, self.pos, capacity=capacity)
        self.f = self.step(self.pos)[1].clone()
        self.ok = True

    def run(self, n):
        dt, m, box, step = self.dt, self.m, self.box, self.step
        for _ in range(n):
            self.v = self.v + 0.5 * dt * self.f / m
            self.pos = self.pos + dt * self.v
            self.pos = self.pos - torch.floor(self.pos / box) * box
            self.f = step(self.pos)[1]
            self.ok = step.fetch()[2] and self.ok
            self.v = self.v + 0.5 * dt * self.f / m


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per MD step (NVE, dt %.2f fs, %g K start): DeviceMD.run(n) + one fetch() per window vs GraphedMDStep + "
                   "fetch() + torch integrator per step; %d alternating rounds of %d steps, median (min, max)"
                   % (a.dt, a.temp, a.rounds, a.steps), "cells": []}
    for name, reps in CELLS:
        pos, cell, z, m, v = setup(reps, a.temp)
        # both arms on the same column count, with room for the list to grow while the random-weight model heats the cell
        # (a list that outgrows it halts the device arm and fails the host arm's check: the row says so)
        z_t, cell_t, _, _, first, capacity = on_device(dev, pos, cell, z, margin=a.margin)
        host = HostLoop(model, pos, cell, z, m, v, a.dt, dev, capacity=capacity)
        md = DeviceMD(model, z_t, cell_t, pos, m, a.dt, velocities=v, log_steps=max(a.steps, 64), capacity=capacity)
        host.run(20)
        md.run(20)
        md.fetch()
        t, last = time_arms([("host", a.steps, host.run, dict(sync=True)), ("dev", a.steps, fetched(md))], a.rounds)
        snap = last["dev"]
        row = {"cell": name, "atoms": int(len(z)), "edges_at_start": first, "capacity": capacity,
               "host_loop_ms": ms(t["host"]), "device_md_ms": ms(t["dev"]),
               "ratio_host_over_device": statistics.median(t["host"]) / statistics.median(t["dev"]),
               "device_md_steps_done": snap.step, "device_md_halted": bool(snap.halted), "host_loop_lists_complete": bool(host.ok)}
        out["cells"].append(row)
        print(json.dumps(row), flush=True)
    return out


def launches(a):
    """Device activity of two replays of the plain captured step and of two DeviceMD steps (108-atom cell): the kernels by
    name and count, and every memcpy / memset the profiler saw."""
    dev = torch.device("cuda:0")
    model = model_for(dev)
    pos, cell, z, m, v = setup((3, 3, 3), a.temp)
    host = HostLoop(model, pos, cell, z, m, v, a.dt, dev)
    md = DeviceMD(model, torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev), pos, m, a.dt, velocities=v)
    md.run(4)
    host.step()
    torch.cuda.synchronize()
    launch_table("device activity of 2 replays, 108-atom cell: GraphedMDStep() | DeviceMD.run(2)",
                 "plain", lambda: (host.step(), host.step()), "DeviceMD", lambda: md.run(2), a.launches)


if __name__ == "__main__":
    main("md_device_bench", bench, launches, flags=[("--steps", dict(type=int, default=300)), ("--dt", dict(type=float, default=0.5)),
                                                    ("--temp", dict(type=float, default=300.0))])
