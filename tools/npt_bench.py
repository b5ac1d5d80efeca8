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
import json

import numpy as np
from resident_bench import fetched, launch_table, main, model_for, ms, on_device, setup, time_arms  # (sets the path)
import torch

from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep
from hermnet_amd.md import AMU_A2_FS2_TO_EV, DeviceMD, DeviceNPT

SYSTEMS = [("108 atoms", (3, 3, 3), 1), ("1008 atoms", (6, 6, 7), 1), ("64 x 32 atoms", (2, 2, 2), 64)]


def system(reps, copies, temp):
    """md_device_bench's cell, or `copies` of it with velocities of their own (copy g: the stream of a cell of seed g)."""
    pos, cell, z, m, v = setup(reps, temp)
    if copies == 1:
        return dict(pos=pos, cell=cell, z=z, m=m, v=v, batch=None, B=1)
    n = len(z)
    vs = np.concatenate([setup(reps, temp, seed=g)[4] for g in range(copies)])
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
        s = system(reps, copies, a.temp)
        z, cell_t, _, kw, first, capacity = on_device(dev, s["pos"], s["cell"], s["z"], s["batch"], a.margin)
        common = dict(velocities=s["v"], log_steps=max(a.steps, 64), capacity=capacity, **kw)
        host = HostNPTLoop(model, s, a.dt, dev, a.pressure, c, capacity)
        md = DeviceMD(model, z, cell_t, s["pos"], s["m"], a.dt, **common)
        npt = DeviceNPT(model, z, s["cell"], s["pos"], s["m"], a.dt, pressure=a.pressure, compressibility=a.compressibility,
                        taup=a.taup, **common)
        for arm in (host, md, npt):
            arm.run(20)
        md.fetch(), npt.fetch()
        t, snaps = time_arms([("host", a.steps, host.run, dict(sync=True)), ("md", a.steps, fetched(md)), ("npt", a.steps, fetched(npt))],
                             a.rounds)
        t = {k: ms(v) for k, v in t.items()}
        row = {"system": name, "atoms": int(len(s["z"])), "graphs": s["B"], "edges_at_start": first, "capacity": capacity,
               "host_npt_loop_ms": t["host"], "device_md_ms": t["md"], "device_npt_ms": t["npt"],
               "ratio_device_npt_over_device_md": t["npt"][0] / t["md"][0],
               "ratio_host_loop_over_device_npt": t["host"][0] / t["npt"][0],
               "device_npt_steps_done": snaps["npt"].step, "device_npt_halted": bool(snaps["npt"].halted),
               "device_npt_clamped": int(snaps["npt"].clamped.sum()), "device_md_halted": bool(snaps["md"].halted),
               "host_loop_lists_complete": bool(host.ok),
               "volume_ratio_device_npt": float(np.median(snaps["npt"].volume / np.abs(np.linalg.det(s["cell"].reshape(-1, 3, 3)))))}
        out["systems"].append(row)
        print(json.dumps(row), flush=True)
    return out


def launches(a):
    """Device activity of two DeviceMD steps and of two DeviceNPT steps (108-atom cell): the kernels by name and count, and
    every memcpy / memset the profiler saw."""
    dev = torch.device("cuda:0")
    model = model_for(dev)
    s = system((3, 3, 3), 1, a.temp)
    z = torch.from_numpy(s["z"]).to(dev)
    md = DeviceMD(model, z, torch.from_numpy(s["cell"].astype(np.float32)).to(dev), s["pos"], s["m"], a.dt, velocities=s["v"])
    npt = DeviceNPT(model, z, s["cell"], s["pos"], s["m"], a.dt, velocities=s["v"], pressure=a.pressure,
                    compressibility=a.compressibility, taup=a.taup)
    md.run(4)
    npt.run(4)
    torch.cuda.synchronize()
    launch_table("device activity of 2 replays, 108-atom cell: DeviceMD.run(2) | DeviceNPT.run(2)",
                 "DeviceMD", lambda: md.run(2), "DeviceNPT", lambda: npt.run(2), a.launches)


if __name__ == "__main__":
    main("npt_bench", bench, launches,
         flags=[("--steps", dict(type=int, default=200)), ("--dt", dict(type=float, default=0.5)),
                ("--temp", dict(type=float, default=300.0)), ("--pressure", dict(type=float, default=0.0, help="target, eV/A^3")),
                ("--compressibility", dict(type=float, default=73.2, help="A^3/eV (4.57e-5 / bar: ASE's default, water)")),
                ("--taup", dict(type=float, default=1000.0, help="fs"))])
