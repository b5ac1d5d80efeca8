#!/usr/bin/env python3
"""ms per time step of Nose-Hoover chain NVT: `DeviceNHC.run(n)` (hermnet_amd/nhc.py: the chains inside the replayed graph)
against `DeviceMD` Langevin on the same batch and against the host-driven loop it replaces.  Three arms in ONE process,
alternating, same batch, model and start state; a window ends in a synchronisation (a `fetch()`):

    (a) DeviceMD     Langevin, run(steps) + one fetch(): the yardstick -- (b) - (a) is what the chain costs per replay (two
                     launches more, lane 0's serial half steps, one more streaming pass over v; no noise drawn)
    (b) DeviceNHC    M = 3, order 3, substeps 1: run(steps) + one fetch()
    (c) host loop    per step: velocity Verlet and the chains' two half steps in numpy float64 (vectorised over the graphs,
                     numpy's exp), a plain `GraphedBatchMDStep` on the float32 coordinates + its `fetch()`

    python tools/nhc_bench.py [--steps 200] [--rounds 5] [--out profiles/device_nhc.json]
    python tools/nhc_bench.py --launches profiles/device_nhc_launches.txt      # device activity of the replays

Cases: 1 x 108 atoms (3x3x3), 1 x 1008 atoms (6x6x7) and 64 x 32 atoms (2x2x2; 64 DIFFERENT cells) of the fcc alloy; 600 K,
tau 100 fs (Langevin: friction 0.01 /fs), dt 1 fs; model of BASELINE configs[1]."""
import json
import statistics

import numpy as np
from resident_bench import cells, fetched, launch_table, main, model_for, ms, on_device, time_arms  # (sets the path)
import torch

from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.md import AMU_A2_FS2_TO_EV, DeviceMD
from hermnet_amd.nhc import DeviceNHC, chain_tables

DT, FRICTION, SEED, T, TAU, CHAIN, ORDER = 1.0, 0.01, 2024, 600.0, 100.0, 3, 3
CASES = [("1 x 108 atoms", 1, (3, 3, 3)), ("1 x 1008 atoms", 1, (6, 6, 7)), ("64 x 32 atoms", 64, (2, 2, 2))]


class HostLoop(object):
    """Arm (c): velocity Verlet and the chains in numpy around a plain graphed step; one upload and one fetch per step."""

    def __init__(self, step, pos, v, m, batch, cell, dof):
        B = len(cell)
        self.step, self.batch, self.B = step, batch, B
        self.x, self.v = pos.copy(), v.copy()
        self.m = m * AMU_A2_FS2_TO_EV
        self.cell, self.inv = cell.astype(np.float32).astype(np.float64), np.linalg.inv(cell.astype(np.float32).astype(np.float64))
        self.delta, self.kt, self.dof_kt, self.q, self.inv_q = chain_tables(np.full(B, T), np.full(B, TAU), dof, DT, CHAIN, ORDER, 1)
        self.xi, self.v_xi = np.zeros((B, CHAIN)), np.zeros((B, CHAIN))
        self.f = self._forces()
        self.steps = 0

    def _forces(self):
        self.step(torch.from_numpy(self.x.astype(np.float32)))
        e, f, ok, _ = self.step.fetch()
        assert ok
        self.e = e
        return f.astype(np.float64)

    def _force(self, j, k2):
        if j == 0:
            return (k2 - self.dof_kt) * self.inv_q[:, 0]
        return (self.q[:, j - 1] * self.v_xi[:, j - 1] ** 2 - self.kt) * self.inv_q[:, j]

    def _half(self):
        """csrc/nhc_step.h: NHC(dt/2) of every graph at once; scales v."""
        M, v = CHAIN, self.v_xi
        k2 = np.bincount(self.batch, weights=self.m * (self.v ** 2).sum(axis=1), minlength=self.B)
        s = np.ones(self.B)
        for d in self.delta:
            v[:, M - 1] += self._force(M - 1, k2) * 0.5 * d
            for j in range(M - 2, -1, -1):
                e = np.exp(-0.25 * d * v[:, j + 1])
                v[:, j] = (v[:, j] * e + self._force(j, k2) * 0.5 * d) * e
            a = np.exp(-d * v[:, 0])
            s, k2 = s * a, k2 * a * a
            self.xi += d * v
            for j in range(M - 1):
                e = np.exp(-0.25 * d * v[:, j + 1])
                v[:, j] = (v[:, j] * e + self._force(j, k2) * 0.5 * d) * e
            v[:, M - 1] += self._force(M - 1, k2) * 0.5 * d
        self.v *= s[self.batch, None]

    def run(self, steps):
        kick = (0.5 * DT / self.m)[:, None]
        for _ in range(steps):
            self._half()
            self.v += kick * self.f
            self.x += DT * self.v
            n = np.floor(np.einsum("nk,nkj->nj", self.x, self.inv[self.batch]))
            self.x -= np.einsum("nk,nkj->nj", n, self.cell[self.batch])
            self.f = self._forces()
            self.v += kick * self.f
            self._half()
        self.steps += steps


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per time step (dt %g fs, %g K): (a) DeviceMD Langevin (friction %g /fs) run(n) + one fetch() per window, "
                   "(b) DeviceNHC (tau %g fs, M = %d, order %d) run(n) + one fetch() per window, (c) numpy velocity Verlet + numpy "
                   "chains + GraphedBatchMDStep + fetch() every step; %d alternating rounds of %d steps, median (min, max)"
                   % (DT, T, FRICTION, TAU, CHAIN, ORDER, a.rounds, a.steps), "cases": []}
    for name, B, reps in CASES:
        pos, cell, z, m, batch, v = cells([reps] * B, T)
        z_t, cell_t, p0, kw, first, capacity = on_device(dev, pos, cell, z, batch, a.margin)    # every arm on the same column count
        batch_t = kw["batch"]
        kw.update(velocities=v, log_steps=max(a.steps, 64), capacity=capacity, temperature=T)
        plain = DeviceMD(model, z_t, cell_t, pos, m, DT, friction=FRICTION, seed=SEED, **kw)
        ours = DeviceNHC(model, z_t, cell_t, pos, m, DT, tau=TAU, chain=CHAIN, order=ORDER, **kw)
        host = HostLoop(GraphedBatchMDStep(model, z_t, cell_t, p0, batch_t, B, capacity=capacity), pos, v, m, batch, cell, ours.dof)
        # (the host loop's window ends in its last step's fetch())
        t, last = time_arms([("plain", a.steps, fetched(plain)), ("ours", a.steps, fetched(ours)), ("host", a.steps, host.run)],
                            a.rounds)
        t_plain, t_ours, t_host, psnap, snap = t["plain"], t["ours"], t["host"], last["plain"], last["ours"]
        md_ms, ours_ms = statistics.median(t_plain), statistics.median(t_ours)
        row = {"case": name, "atoms": int(len(z)), "graphs": B, "edges_at_start": first, "capacity": capacity,
               "device_md_langevin_ms": ms(t_plain), "device_nhc_ms": ms(t_ours), "host_loop_ms": ms(t_host),
               "nhc_minus_md_us": 1e3 * (ours_ms - md_ms), "nhc_over_md_percent": 100.0 * (ours_ms - md_ms) / md_ms,
               "ratio_host_over_device": statistics.median(t_host) / ours_ms,
               "steps_done": [int(psnap.step), int(snap.step), host.steps], "halted": [bool(psnap.halted), bool(snap.halted)],
               "temperature_now_mean": float(snap.temperature_now.mean()),
               "host_loop_max_abs_dx_vs_device": float(np.abs(host.x - snap.positions).max())}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    return out


def launches(a):
    """Device activity of two DeviceMD (NVE) replays and of two DeviceNHC replays on the same batch of 5 x 32 atoms: the kernels
    by name and count, and every memcpy / memset the profiler saw."""
    dev = torch.device("cuda:0")
    model = model_for(dev)
    pos, cell, z, m, batch, v = cells([(2, 2, 2)] * 5, T)
    z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
    kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=5, velocities=v)
    plain_md = DeviceMD(model, z_t, cell_t, pos, m, DT, **kw)
    nhc_md = DeviceNHC(model, z_t, cell_t, pos, m, DT, temperature=T, tau=TAU, chain=CHAIN, order=ORDER, **kw)
    plain_md.run(2)
    nhc_md.run(2)
    torch.cuda.synchronize()
    launch_table("device activity of 2 replays, batch of 5 x 32 atoms: DeviceMD.run(2) (NVE) | DeviceNHC.run(2)",
                 "DeviceMD", lambda: plain_md.run(2), "DeviceNHC", lambda: nhc_md.run(2), a.launches)


if __name__ == "__main__":
    main("nhc_bench", bench, launches, flags=[("--steps", dict(type=int, default=200))])
