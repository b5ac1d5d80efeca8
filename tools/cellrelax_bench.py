#!/usr/bin/env python3
"""ms per cell-relaxation step (= force-and-stress evaluation): `DeviceCellRelax.run(n)` (hermnet_amd/relax.py: FIRE on atoms
and cell inside the replayed graph) against the host-driven loop it replaces -- `GraphedMDStep(stress=True,
variable_cell=True)` / `GraphedBatchMDStep(stress=True)` fed float32(x) and float32(C), `fetch()`, and the numpy cell filter +
FIRE of the tests (tests/cellrelax_reference.py: NumpyCellRelax, the same arithmetic in the same order) per evaluation.  Both
arms in ONE process, alternating, same structures, model and start state; a window ends in a synchronisation (the device
arm's in `fetch()`).  `fmax` is set out of reach, so every evaluation of a window moves every structure and its cell.

    python tools/cellrelax_bench.py [--steps 100] [--rounds 5] [--out profiles/device_cellrelax.json]
    python tools/cellrelax_bench.py --launches profiles/device_cellrelax_launches.txt      # device activity of the replays

Cases: 108 atoms (3x3x3), 1008 atoms (6x6x7), a batch of 64 structures of 32 atoms (2x2x2), every cell strained by 2 %; model
of BASELINE configs[1]."""
import json
import statistics

import numpy as np
from resident_bench import FMAX, RELAX_CASES as CASES, fetched, launch_table, main, model_for, ms, on_device, structures, time_arms  # (sets the path)
import torch

from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep
from hermnet_amd.relax import DeviceCellRelax, DeviceRelax
from cellrelax_reference import NumpyCellRelax

STRAIN = np.array([[0.02, 0.006, 0.0], [0.0, -0.018, 0.004], [0.005, 0.0, 0.021]])


def strained(members, sigma):
    """relax_bench's structures, cells and atoms deformed by I + STRAIN; cells [B,3,3] float64."""
    pos, cell, z, batch = structures(members, sigma)
    d = np.eye(3) + STRAIN
    return pos @ d, np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3) @ d, z, batch


class HostLoop(object):
    """One evaluation = upload float32(x) and float32(C), replay, `fetch()` (one copy + synchronisation), NumpyCellRelax."""

    def __init__(self, model, pos, cell, z, batch, dev, capacity):
        z_t = torch.from_numpy(z).to(dev)
        p0 = torch.from_numpy(pos.astype(np.float32)).to(dev)
        B = self.B = len(cell)
        if batch is None:
            self.step = GraphedMDStep(model, z_t, torch.from_numpy(cell[0].astype(np.float32)).to(dev), p0, capacity=capacity,
                                      stress=True, variable_cell=True)
        else:
            self.step = GraphedBatchMDStep(model, z_t, torch.from_numpy(cell.astype(np.float32)).to(dev), p0,
                                           torch.from_numpy(batch).to(dev), B, capacity=capacity, stress=True)
        self.shape = (3, 3) if batch is None else (B, 3, 3)
        self.opt = NumpyCellRelax(pos, cell, batch=batch, num_graphs=B, fmax=FMAX)
        self.ok = True

    def run(self, n):
        for _ in range(n):
            p32, c32 = self.opt.advance()
            self.step(torch.from_numpy(p32), torch.from_numpy(c32.reshape(self.shape)))
            e, f, ok, found, w = self.step.fetch()
            self.ok = self.ok and ok
            self.opt.finish(f, w, energy=e, total=(found, 0))


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per cell-relaxation step (UnitCellFilter + FIRE, ASE defaults, cells strained by 2 %%, start rattled by %.2f A, "
                   "fmax out of reach): DeviceCellRelax.run(n) + one fetch() per window vs graphed step with virial + fetch() + "
                   "numpy filter and FIRE (tests/cellrelax_reference.py: NumpyCellRelax, a Python loop over the graphs) per step; "
                   "%d alternating rounds of %d steps, median (min, max)" % (a.sigma, a.rounds, a.steps), "cases": []}
    for name, members in CASES:
        pos, cell, z, batch = strained(members, a.sigma)
        B = len(members)
        own = cell[0] if batch is None else cell
        z_t, _, _, kw, first, capacity = on_device(dev, pos, own, z, batch, a.margin)    # both arms on the same column count
        host = HostLoop(model, pos, cell, z, batch, dev, capacity)
        rx = DeviceCellRelax(model, z_t, own, pos, fmax=FMAX, log_steps=max(a.steps, 64), capacity=capacity, **kw)
        host.run(10)
        rx.run(10)
        rx.fetch()
        t, last = time_arms([("host", a.steps, host.run, dict(sync=True)), ("dev", a.steps, fetched(rx))], a.rounds)
        snap = last["dev"]
        same = bool(np.array_equal(snap.positions, host.opt.x) and np.array_equal(snap.cell.reshape(B, 9), host.opt.cell64)
                    and np.array_equal(snap.velocities, host.opt.v))
        row = {"case": name, "atoms": int(len(z)), "graphs": B, "edges_at_start": first, "capacity": capacity,
               "host_loop_ms": ms(t["host"]), "device_cellrelax_ms": ms(t["dev"]),
               "ratio_host_over_device": statistics.median(t["host"]) / statistics.median(t["dev"]),
               "device_steps_done": snap.step, "device_halted": bool(snap.halted), "host_loop_lists_complete": bool(host.ok),
               "fmax_at_end": float(snap.fmax.max()), "volume_change": float((snap.volume / np.abs(np.linalg.det(cell))).mean() - 1.0),
               "arms_end_bit_equal": same}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    return out


def launches(a):
    """Device activity of two DeviceRelax replays and of two DeviceCellRelax replays (a batch of 3 x 32 atoms): the kernels by
    name and count, and every memcpy / memset the profiler saw."""
    dev = torch.device("cuda:0")
    model = model_for(dev)
    pos, cell, z, batch = strained([(2, 2, 2)] * 3, a.sigma)
    kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=3, fmax=FMAX)
    z_t = torch.from_numpy(z).to(dev)
    plain_rx = DeviceRelax(model, z_t, torch.from_numpy(cell.astype(np.float32)).to(dev), pos, **kw)
    cell_rx = DeviceCellRelax(model, z_t, cell, pos, **kw)
    plain_rx.run(4)
    cell_rx.run(4)
    torch.cuda.synchronize()
    launch_table("device activity of 2 replays, batch of 3 x 32 atoms: DeviceRelax.run(2) | DeviceCellRelax.run(2)",
                 "DeviceRelax", lambda: plain_rx.run(2), "DeviceCellRelax", lambda: cell_rx.run(2), a.launches)


if __name__ == "__main__":
    main("cellrelax_bench", bench, launches,
         flags=[("--steps", dict(type=int, default=100)),
                ("--sigma", dict(type=float, default=0.05, help="rattle of the start coordinates (A)"))])
