#!/usr/bin/env python3
"""ms per time step of MTK NPT: `DeviceMTK.run(n)` (hermnet_amd/mtk.py: barostat and both chains inside the replayed graph)
against `DeviceNPT` with Langevin on the same batch and against the host-driven loop it replaces.  Three arms in ONE process,
alternating, same batch, model and start state; a window ends in a synchronisation (a `fetch()`):

    (a) DeviceNPT    Berendsen + Langevin, run(steps) + one fetch(): the yardstick -- (b) - (a) is what the integrator costs
                     per replay (one launch more in the finish, two serial chains on lane 0; no noise drawn)
    (b) DeviceMTK    isotropic, M = 3, order 3, substeps 1: run(steps) + one fetch()
    (c) host loop    per step: the numpy transcription of the step (tests/mtk_reference.py: NumpyMTK), a plain
                     `GraphedBatchMDStep(stress=True)` on the float32 coordinates and cell + its `fetch()`

    python tools/mtk_bench.py [--steps 200] [--rounds 5] [--out profiles/device_mtk.json]
    python tools/mtk_bench.py --launches profiles/device_mtk_launches.txt      # device activity of the replays

Cases: 1 x 108 atoms (3x3x3), 1 x 1008 atoms (6x6x7) and 64 x 32 atoms (2x2x2; 64 DIFFERENT cells) of the fcc alloy; 600 K,
tau 100 fs (Langevin: friction 0.01 /fs), the target pressure each cell starts at, dt 1 fs; model of BASELINE configs[1].
taup is 1e5 fs for both barostats: the model's synthetic weights give a cell no stiffness, so at a physical taup the volumes run
away within the windows (with taup 1000 fs: x 2 to x 4 in 1000 steps, fewer edges every step, and one of the 64 small cells
until its energy was not finite and the run halted) and the arms would no longer be timed on the same lists.  The kernels do
the same work whatever the factors' values are."""
import json
import os
import statistics
import sys

import numpy as np
from resident_bench import ROOT, cells, fetched, launch_table, main, model_for, ms, on_device, time_arms  # (sets the path)
import torch

from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.md import AMU_A2_FS2_TO_EV, DeviceNPT
from hermnet_amd.mtk import DeviceMTK

DT, FRICTION, SEED, T, TAU, TAUP, CHAIN, ORDER, COMPRESSIBILITY = 1.0, 0.01, 2024, 600.0, 100.0, 1e5, 3, 3, 1e-2
CASES = [("1 x 108 atoms", 1, (3, 3, 3)), ("1 x 1008 atoms", 1, (6, 6, 7)), ("64 x 32 atoms", 64, (2, 2, 2))]


class HostLoop(object):
    """Arm (c): the numpy transcription of the step around a plain graphed step with the virial; one upload and one fetch
    per step."""

    def __init__(self, step, pos, v, m, batch, cell, dof, pressure):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from mtk_reference import NumpyMTK
        B = len(cell)
        self.step, self.B = step, B
        self.ref = NumpyMTK(pos, v, m, DT, np.full(B, T), np.full(B, TAU), dof, cell.astype(np.float32).astype(np.float64),
                            pressure=pressure, taup=TAUP, chain=CHAIN, order=ORDER, batch=batch, log_steps=64, num_graphs=B)
        self.ref.state[3] = 1
        self._replay()
        self.steps = 0

    def _replay(self):
        pos32 = self.ref.advance()
        self.step(torch.from_numpy(pos32), torch.from_numpy(self.ref.cell32.reshape(self.B, 3, 3)))
        e, f, ok, n, w = self.step.fetch()
        assert ok
        self.ref.finish(f, e, w.reshape(self.B, 9), total=(n, 0))

    def run(self, steps):
        for _ in range(steps):
            self._replay()
        self.steps += steps

    @property
    def x(self):
        return self.ref.x


def start_pressure(step, pos, cell, m, v, batch, B):
    """[B]: (sum m v^2 + tr W) / 3 V of the start configuration, from the plain graphed step."""
    cell32 = cell.astype(np.float32)
    step(torch.from_numpy(pos.astype(np.float32)), torch.from_numpy(cell32))
    w = step.fetch()[4].reshape(B, 9).astype(np.float64)
    kin = np.bincount(batch, weights=m * AMU_A2_FS2_TO_EV * (v ** 2).sum(axis=1), minlength=B)
    return (kin + w[:, [0, 4, 8]].sum(axis=1)) / (3.0 * np.abs(np.linalg.det(cell32.astype(np.float64))))


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per time step (dt %g fs, %g K, target pressure = the start's): (a) DeviceNPT Berendsen (compressibility %g "
                   "A^3/eV) + Langevin (friction %g /fs) run(n) + one fetch() per window, (b) DeviceMTK (tau %g fs, taup %g fs, "
                   "isotropic, M = %d, order %d) run(n) + one fetch() per window, (c) NumpyMTK + GraphedBatchMDStep(stress=True) + "
                   "fetch() every step; %d alternating rounds of %d steps, median (min, max)"
                   % (DT, T, COMPRESSIBILITY, FRICTION, TAU, TAUP, CHAIN, ORDER, a.rounds, a.steps), "cases": []}
    for name, B, reps in CASES:
        pos, cell, z, m, batch, v = cells([reps] * B, T)
        z_t, cell_t, p0, kw, first, capacity = on_device(dev, pos, cell, z, batch, a.margin)    # every arm on the same column count
        plain_step = GraphedBatchMDStep(model, z_t, cell_t, p0, kw["batch"], B, capacity=capacity, stress=True)
        pressure = start_pressure(plain_step, pos, cell, m, v, batch, B)
        cell64 = cell.astype(np.float32).astype(np.float64)
        kw.update(velocities=v, log_steps=max(a.steps, 64), capacity=capacity, temperature=T, pressure=pressure, taup=TAUP)
        plain = DeviceNPT(model, z_t, cell64, pos, m, DT, friction=FRICTION, seed=SEED, compressibility=COMPRESSIBILITY, **kw)
        ours = DeviceMTK(model, z_t, cell64, pos, m, DT, tau=TAU, chain=CHAIN, order=ORDER, **kw)
        host = HostLoop(plain_step, pos, v, m, batch, cell, ours.dof, pressure)
        t, last = time_arms([("plain", a.steps, fetched(plain)), ("ours", a.steps, fetched(ours)), ("host", a.steps, host.run)],
                            a.rounds)
        t_plain, t_ours, t_host, psnap, snap = t["plain"], t["ours"], t["host"], last["plain"], last["ours"]
        npt_ms, ours_ms = statistics.median(t_plain), statistics.median(t_ours)
        row = {"case": name, "atoms": int(len(z)), "graphs": B, "edges_at_start": first, "capacity": capacity,
               "device_npt_langevin_ms": ms(t_plain), "device_mtk_ms": ms(t_ours), "host_loop_ms": ms(t_host),
               "mtk_minus_npt_us": 1e3 * (ours_ms - npt_ms), "mtk_over_npt_percent": 100.0 * (ours_ms - npt_ms) / npt_ms,
               "ratio_host_over_device": statistics.median(t_host) / ours_ms,
               "steps_done": [int(psnap.step), int(snap.step), host.steps], "halted": [bool(psnap.halted), bool(snap.halted)],
               "temperature_now_mean": float(snap.temperature_now.mean()), "refused": int(snap.refused.sum()),
               "volume_over_start_min_max": [float((snap.volume / np.abs(np.linalg.det(cell64))).min()),
                                             float((snap.volume / np.abs(np.linalg.det(cell64))).max())],
               "host_loop_max_abs_dx_vs_device": float(np.abs(host.x - snap.positions).max())}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    return out


def launches(a):
    """Device activity of two DeviceNPT replays and of two DeviceMTK replays on the same batch of 5 x 32 atoms: the kernels by
    name and count, and every memcpy / memset the profiler saw."""
    dev = torch.device("cuda:0")
    model = model_for(dev)
    pos, cell, z, m, batch, v = cells([(2, 2, 2)] * 5, T)
    z_t, cell64 = torch.from_numpy(z).to(dev), cell.astype(np.float32).astype(np.float64)
    kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=5, velocities=v, taup=TAUP)
    plain_md = DeviceNPT(model, z_t, cell64, pos, m, DT, compressibility=COMPRESSIBILITY, **kw)
    mtk_md = DeviceMTK(model, z_t, cell64, pos, m, DT, temperature=T, tau=TAU, chain=CHAIN, order=ORDER, **kw)
    plain_md.run(2)
    mtk_md.run(2)
    torch.cuda.synchronize()
    launch_table("device activity of 2 replays, batch of 5 x 32 atoms: DeviceNPT.run(2) | DeviceMTK.run(2)",
                 "DeviceNPT", lambda: plain_md.run(2), "DeviceMTK", lambda: mtk_md.run(2), a.launches)


if __name__ == "__main__":
    main("mtk_bench", bench, launches, flags=[("--steps", dict(type=int, default=200))])
