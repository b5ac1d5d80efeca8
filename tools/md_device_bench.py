#!/usr/bin/env python3
"""ms per MD step: `DeviceMD.run(n)` (hermnet_amd/md.py: the integrator inside the replayed graph) against the host-driven
loop it replaces -- `GraphedMDStep(pos)` + `fetch()` + the torch integrator of tools/md_nve.py (device tensors, one
synchronisation per step for the list check).  Both arms in ONE process, alternating, same cell, model and start state; a
window ends in a synchronisation (the device arm's in `fetch()`).

    python tools/md_device_bench.py [--steps 300] [--rounds 5] [--out profiles/device_md.json]
    python tools/md_device_bench.py --launches profiles/device_md_launches.txt      # device activity of the replays

Cells: 108 atoms (3x3x3), 1008 atoms (6x6x7), BASELINE configs[1] (10x10x25: 10,000 atoms); model of configs[1]."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import hermnet_amd as hn  # noqa: E402
from hermnet_amd import synth  # noqa: E402
from hermnet_amd.graph import GraphedMDStep  # noqa: E402
from hermnet_amd.md import AMU_A2_FS2_TO_EV, KB, DeviceMD  # noqa: E402
from hermnet_amd.neighbor import neighbor_search, padded_capacity  # noqa: E402

MASS = {13: 26.9815, 28: 58.6934, 29: 63.546}
CELLS = [("108 atoms", (3, 3, 3)), ("1008 atoms", (6, 6, 7)), ("configs[1], 10000 atoms", (10, 10, 25))]


def setup(reps, dev, temp, seed=0):
    pos, cell, z = synth.fcc_alloy_atoms(reps=reps, seed=seed)
    m = np.array([MASS[int(v)] for v in z])
    v = np.random.RandomState(seed + 1).normal(size=pos.shape) * np.sqrt(KB * temp / (m * AMU_A2_FS2_TO_EV))[:, None]
    return pos, cell, z, m, v


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


def model_for(dev):
    model = hn.HVNet(["Al", "Ni", "Cu"], rc=5.0, num_layers=5, hidden_channels=128, num_rbf=128).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
    model = model.to(dev)
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per MD step (NVE, dt %.2f fs, %g K start): DeviceMD.run(n) + one fetch() per window vs GraphedMDStep + "
                   "fetch() + torch integrator per step; %d alternating rounds of %d steps, median (min, max)"
                   % (a.dt, a.temp, a.rounds, a.steps), "cells": []}
    for name, reps in CELLS:
        pos, cell, z, m, v = setup(reps, dev, a.temp)
        # both arms on the same column count, with room for the list to grow while the random-weight model heats the cell
        # (a list that outgrows it halts the device arm and fails the host arm's check: the row says so)
        cell_t = torch.from_numpy(cell.astype(np.float32)).to(dev)
        first = int(neighbor_search(torch.from_numpy(pos.astype(np.float32)).to(dev), 5.0, cell_t)[0].size(1))
        capacity = padded_capacity(first, margin=a.margin)
        host = HostLoop(model, pos, cell, z, m, v, a.dt, dev, capacity=capacity)
        md = DeviceMD(model, torch.from_numpy(z).to(dev), cell_t, pos, m, a.dt, velocities=v, log_steps=max(a.steps, 64),
                      capacity=capacity)
        host.run(20)
        md.run(20)
        md.fetch()
        t_host, t_dev, snap = [], [], None
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host.run(a.steps)
            torch.cuda.synchronize()
            t_host.append((time.perf_counter() - t0) / a.steps * 1e3)
            t0 = time.perf_counter()
            md.run(a.steps)
            snap = md.fetch()
            t_dev.append((time.perf_counter() - t0) / a.steps * 1e3)
        row = {"cell": name, "atoms": int(len(z)), "edges_at_start": first, "capacity": capacity,
               "host_loop_ms": [statistics.median(t_host), min(t_host), max(t_host)],
               "device_md_ms": [statistics.median(t_dev), min(t_dev), max(t_dev)],
               "ratio_host_over_device": statistics.median(t_host) / statistics.median(t_dev),
               "device_md_steps_done": snap.step, "device_md_halted": bool(snap.halted), "host_loop_lists_complete": bool(host.ok)}
        out["cells"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


def launches(a):
    """Device activity of two replays of the plain captured step and of two DeviceMD steps (108-atom cell): the kernels by
    name and count, and every memcpy / memset the profiler saw."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda:0")
    model = model_for(dev)
    pos, cell, z, m, v = setup((3, 3, 3), dev, a.temp)
    host = HostLoop(model, pos, cell, z, m, v, a.dt, dev)
    md = DeviceMD(model, torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev), pos, m, a.dt, velocities=v)
    md.run(4)
    host.step()
    torch.cuda.synchronize()

    def device_events(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    plain = device_events(lambda: (host.step(), host.step()))
    ours = device_events(lambda: md.run(2))
    lines = ["device activity of 2 replays, 108-atom cell: GraphedMDStep() | DeviceMD.run(2)    (count name)"]
    for name in sorted(set(plain) | set(ours)):
        lines.append("%4d %4d  %s" % (plain.get(name, 0), ours.get(name, 0), name[:150]))
    extra = {k: c - plain.get(k, 0) for k, c in ours.items() if c != plain.get(k, 0)}
    copies = {k: c for k, c in ours.items() if "memcpy" in k.lower() or "memset" in k.lower()}
    lines.append("kernels: plain %d, DeviceMD %d; only in DeviceMD: %s" % (sum(plain.values()), sum(ours.values()), extra))
    lines.append("memcpy / memset activities inside DeviceMD.run(2): %d %s" % (sum(copies.values()), copies))
    if not ours:
        lines.append("(the profiler recorded no device activity for graph launches)")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.launches, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dt", type=float, default=0.5)
    ap.add_argument("--temp", type=float, default=300.0)
    ap.add_argument("--margin", type=float, default=0.25, help="columns of the padded list beyond the first count")
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("md_device_bench: needs the GPU (nothing is measured without one)")
    launches(a) if a.launches else bench(a)
