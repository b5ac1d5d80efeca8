#!/usr/bin/env python3
"""ms per NPT step: `DeviceNPT.run(n)` (hermnet_amd/md.py: the Berendsen barostat inside the replayed graph) against
  (a) `DeviceMD.run(n)` on the same system -- what the virial kernels and the barostat's two launches cost --, and
  (b) the host-driven NPT loop it replaces: `GraphedMDStep(stress=True, variable_cell=True)` / `GraphedBatchMDStep(stress=True)`
      fed float32(x) and float32(cell), `fetch()` (forces and virial in one copy), numpy float64 velocity Verlet + barostat.
The three arms run in ONE process, alternating, on the same cell, model and start state; a window ends in a synchronisation
(the device arms' in `fetch()`).

    python tools/npt_bench.py [--steps 200] [--rounds 5] [--out profiles/device_npt.json]
    python tools/npt_bench.py --launches profiles/device_npt_launches.txt      # device activity of the replays

Systems: 108 atoms (3x3x3), 1008 atoms (6x6x7), a batch of 64 replicas of 32 atoms (2x2x2); model of BASELINE configs[1]."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep  # noqa: E402
from hermnet_amd.md import AMU_A2_FS2_TO_EV, DeviceMD, DeviceNPT  # noqa: E402
from hermnet_amd.neighbor import neighbor_search, padded_capacity  # noqa: E402
from md_device_bench import model_for, setup  # noqa: E402

SYSTEMS = [("108 atoms", (3, 3, 3), 1), ("1008 atoms", (6, 6, 7), 1), ("64 x 32 atoms", (2, 2, 2), 64)]


def system(reps, copies, dev, temp):
    pos, cell, z, m, v = setup(reps, dev, temp)
    if copies == 1:
        return dict(pos=pos, cell=cell, z=z, m=m, v=v, batch=None, B=1)
    n = len(z)
    vs = np.concatenate([setup(reps, dev, temp, seed=g)[4] for g in range(copies)])
    return dict(pos=np.tile(pos, (copies, 1)), cell=np.stack([cell] * copies), z=np.tile(z, copies), m=np.tile(m, copies), v=vs,
                batch=np.repeat(np.arange(copies), n), B=copies)


class HostNPTLoop(object):
    """Velocity Verlet + isotropic Berendsen scaling in numpy float64 around a captured step with the virial: per step one
    upload of coordinates and cells, one replay, one packed `fetch()`."""

    def __init__(self, model, s, dt, dev, pressure, c, capacity):
        self.dev, self.dt, self.p0, self.c, self.B = dev, dt, pressure, c, s["B"]
        self.x, self.v = s["pos"].astype(np.float64).copy(), s["v"].astype(np.float64).copy()
        self.cell = s["cell"].astype(np.float64).reshape(self.B, 3, 3).copy()
        self.m = (s["m"] * AMU_A2_FS2_TO_EV)[:, None]
        self.b = np.zeros(len(self.x), dtype=np.int64) if s["batch"] is None else s["batch"]
        z = torch.from_numpy(s["z"]).to(dev)
        p0 = torch.from_numpy(self.x.astype(np.float32)).to(dev)
        c0 = torch.from_numpy(self.cell.astype(np.float32)).to(dev)
        if s["batch"] is None:
            self.step = GraphedMDStep(model, z, c0[0], p0, capacity=capacity, stress=True, variable_cell=True)
        else:
            self.step = GraphedBatchMDStep(model, z, c0, p0, torch.from_numpy(s["batch"]).to(dev), self.B, capacity=capacity,
                                           stress=True)
        self.f, self.ok = self._evaluate()[0], True

    def _evaluate(self):
        cell32 = self.cell.astype(np.float32)
        self.step(torch.from_numpy(self.x.astype(np.float32)).to(self.dev),
                  torch.from_numpy(cell32 if self.B > 1 else cell32[0]).to(self.dev))
        _, f, ok, _, w = self.step.fetch()
        return f.astype(np.float64), w.astype(np.float64), ok

    def run(self, n):
        dt, m, b = self.dt, self.m, self.b
        for _ in range(n):
            self.v += 0.5 * dt * self.f / m
            self.x += dt * self.v
            inv = np.linalg.inv(self.cell)
            s = np.einsum("nk,nkj->nj", self.x, inv[b])
            self.x -= np.einsum("nk,nkj->nj", np.floor(s), self.cell[b])
            self.f, w, ok = self._evaluate()
            self.ok = self.ok and ok
            self.v += 0.5 * dt * self.f / m
            vol = np.abs(np.linalg.det(self.cell))
            kin = np.bincount(b, weights=(m * self.v * self.v).sum(axis=1), minlength=self.B)
            p = (kin + np.trace(w, axis1=1, axis2=2)) / (3.0 * vol)
            mu = np.clip(1.0 - self.c * (self.p0 - p), 0.99, 1.01)
            self.cell *= mu[:, None, None]
            self.x *= mu[b][:, None]


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    c = (a.dt / a.taup) * a.compressibility / 3.0
    out = {"what": "ms per step (dt %.2f fs, %g K start, Berendsen isotropic, taup %g fs, compressibility %g A^3/eV, target %g "
                   "eV/A^3): DeviceNPT.run(n) + one fetch() per window vs DeviceMD.run(n) + fetch() vs the host-driven NPT loop "
                   "(graphed step with virial + fetch() + numpy barostat per step); %d alternating rounds of %d steps, median "
                   "(min, max)" % (a.dt, a.temp, a.taup, a.compressibility, a.pressure, a.rounds, a.steps), "systems": []}
    for name, reps, copies in SYSTEMS:
        s = system(reps, copies, dev, a.temp)
        z = torch.from_numpy(s["z"]).to(dev)
        cell_t = torch.from_numpy(s["cell"].astype(np.float32)).to(dev)
        kw = {} if s["batch"] is None else dict(batch=torch.from_numpy(s["batch"]).to(dev), num_graphs=s["B"])
        first = neighbor_search(torch.from_numpy(s["pos"].astype(np.float32)).to(dev), 5.0, cell_t, **kw)[0].size(1)
        capacity = padded_capacity(int(first), margin=a.margin)
        common = dict(velocities=s["v"], log_steps=max(a.steps, 64), capacity=capacity, **kw)
        host = HostNPTLoop(model, s, a.dt, dev, a.pressure, c, capacity)
        md = DeviceMD(model, z, cell_t, s["pos"], s["m"], a.dt, **common)
        npt = DeviceNPT(model, z, s["cell"], s["pos"], s["m"], a.dt, pressure=a.pressure, compressibility=a.compressibility,
                        taup=a.taup, **common)
        for arm in (host, md, npt):
            arm.run(20)
        md.fetch(), npt.fetch()
        t = {"host": [], "md": [], "npt": []}
        snaps = {}
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host.run(a.steps)
            torch.cuda.synchronize()
            t["host"].append((time.perf_counter() - t0) / a.steps * 1e3)
            for key, arm in (("md", md), ("npt", npt)):
                t0 = time.perf_counter()
                arm.run(a.steps)
                snaps[key] = arm.fetch()
                t[key].append((time.perf_counter() - t0) / a.steps * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {"system": name, "atoms": int(len(s["z"])), "graphs": s["B"], "edges_at_start": int(first), "capacity": capacity,
               "host_npt_loop_ms": [med["host"], min(t["host"]), max(t["host"])],
               "device_md_ms": [med["md"], min(t["md"]), max(t["md"])],
               "device_npt_ms": [med["npt"], min(t["npt"]), max(t["npt"])],
               "ratio_device_npt_over_device_md": med["npt"] / med["md"],
               "ratio_host_loop_over_device_npt": med["host"] / med["npt"],
               "device_npt_steps_done": snaps["npt"].step, "device_npt_halted": bool(snaps["npt"].halted),
               "device_npt_clamped": int(snaps["npt"].clamped.sum()), "device_md_halted": bool(snaps["md"].halted),
               "host_loop_lists_complete": bool(host.ok),
               "volume_ratio_device_npt": float(np.median(snaps["npt"].volume / np.abs(np.linalg.det(s["cell"].reshape(-1, 3, 3)))))}
        out["systems"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


def launches(a):
    """Device activity of two DeviceMD steps and of two DeviceNPT steps (108-atom cell): the kernels by name and count, and
    every memcpy / memset the profiler saw."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda:0")
    model = model_for(dev)
    s = system((3, 3, 3), 1, dev, a.temp)
    z = torch.from_numpy(s["z"]).to(dev)
    md = DeviceMD(model, z, torch.from_numpy(s["cell"].astype(np.float32)).to(dev), s["pos"], s["m"], a.dt, velocities=s["v"])
    npt = DeviceNPT(model, z, s["cell"], s["pos"], s["m"], a.dt, velocities=s["v"], pressure=a.pressure,
                    compressibility=a.compressibility, taup=a.taup)
    md.run(4)
    npt.run(4)
    torch.cuda.synchronize()

    def device_events(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    plain = device_events(lambda: md.run(2))
    ours = device_events(lambda: npt.run(2))
    lines = ["device activity of 2 replays, 108-atom cell: DeviceMD.run(2) | DeviceNPT.run(2)    (count name)"]
    for name in sorted(set(plain) | set(ours)):
        lines.append("%4d %4d  %s" % (plain.get(name, 0), ours.get(name, 0), name[:150]))
    extra = {k: c - plain.get(k, 0) for k, c in ours.items() if c != plain.get(k, 0)}
    copies = {k: c for k, c in ours.items() if "memcpy" in k.lower() or "memset" in k.lower()}
    lines.append("kernels: DeviceMD %d, DeviceNPT %d; difference: %s" % (sum(plain.values()), sum(ours.values()), extra))
    lines.append("memcpy / memset activities inside DeviceNPT.run(2): %d %s" % (sum(copies.values()), copies))
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
    ap.add_argument("--dt", type=float, default=0.5)
    ap.add_argument("--temp", type=float, default=300.0)
    ap.add_argument("--pressure", type=float, default=0.0, help="target, eV/A^3")
    ap.add_argument("--compressibility", type=float, default=73.2, help="A^3/eV (4.57e-5 / bar: ASE's default, water)")
    ap.add_argument("--taup", type=float, default=1000.0, help="fs")
    ap.add_argument("--margin", type=float, default=0.25, help="columns of the padded list beyond the first count")
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("npt_bench: needs the GPU (nothing is measured without one)")
    launches(a) if a.launches else bench(a)
