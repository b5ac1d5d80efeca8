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
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep  # noqa: E402
from hermnet_amd.neighbor import neighbor_search, padded_capacity  # noqa: E402
from hermnet_amd.relax import DeviceCellRelax, DeviceRelax  # noqa: E402
from cellrelax_reference import NumpyCellRelax  # noqa: E402
from relax_bench import CASES, FMAX, model_for, setup  # noqa: E402

STRAIN = np.array([[0.02, 0.006, 0.0], [0.0, -0.018, 0.004], [0.005, 0.0, 0.021]])


def strained(members, sigma):
    """relax_bench's structures, cells and atoms deformed by I + STRAIN; cells [B,3,3] float64."""
    pos, cell, z, batch = setup(members, sigma)
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
        z_t = torch.from_numpy(z).to(dev)
        p0 = torch.from_numpy(pos.astype(np.float32)).to(dev)
        kw = {} if batch is None else dict(batch=torch.from_numpy(batch).to(dev), num_graphs=B)
        cell_t = torch.from_numpy((cell[0] if batch is None else cell).astype(np.float32)).to(dev)
        first = int(neighbor_search(p0, 5.0, cell_t, **kw)[0].size(1))
        capacity = padded_capacity(first, margin=a.margin)                # both arms on the same column count
        host = HostLoop(model, pos, cell, z, batch, dev, capacity)
        rx = DeviceCellRelax(model, z_t, cell[0] if batch is None else cell, pos, fmax=FMAX, log_steps=max(a.steps, 64),
                             capacity=capacity, **kw)
        host.run(10)
        rx.run(10)
        rx.fetch()
        t_host, t_dev, snap = [], [], None
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host.run(a.steps)
            torch.cuda.synchronize()
            t_host.append((time.perf_counter() - t0) / a.steps * 1e3)
            t0 = time.perf_counter()
            rx.run(a.steps)
            snap = rx.fetch()
            t_dev.append((time.perf_counter() - t0) / a.steps * 1e3)
        same = bool(np.array_equal(snap.positions, host.opt.x) and np.array_equal(snap.cell.reshape(B, 9), host.opt.cell64)
                    and np.array_equal(snap.velocities, host.opt.v))
        row = {"case": name, "atoms": int(len(z)), "graphs": B, "edges_at_start": first, "capacity": capacity,
               "host_loop_ms": [statistics.median(t_host), min(t_host), max(t_host)],
               "device_cellrelax_ms": [statistics.median(t_dev), min(t_dev), max(t_dev)],
               "ratio_host_over_device": statistics.median(t_host) / statistics.median(t_dev),
               "device_steps_done": snap.step, "device_halted": bool(snap.halted), "host_loop_lists_complete": bool(host.ok),
               "fmax_at_end": float(snap.fmax.max()), "volume_change": float((snap.volume / np.abs(np.linalg.det(cell))).mean() - 1.0),
               "arms_end_bit_equal": same}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


def launches(a):
    """Device activity of two DeviceRelax replays and of two DeviceCellRelax replays (a batch of 3 x 32 atoms): the kernels by
    name and count, and every memcpy / memset the profiler saw."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
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

    def device_events(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    plain = device_events(lambda: plain_rx.run(2))
    ours = device_events(lambda: cell_rx.run(2))
    lines = ["device activity of 2 replays, batch of 3 x 32 atoms: DeviceRelax.run(2) | DeviceCellRelax.run(2)    (count name)"]
    for name in sorted(set(plain) | set(ours)):
        lines.append("%4d %4d  %s" % (plain.get(name, 0), ours.get(name, 0), name[:150]))
    extra = {k: c - plain.get(k, 0) for k, c in ours.items() if c != plain.get(k, 0)}
    copies = {k: c for k, c in ours.items() if "memcpy" in k.lower() or "memset" in k.lower()}
    lines.append("kernels: DeviceRelax %d, DeviceCellRelax %d; difference: %s" % (sum(plain.values()), sum(ours.values()), extra))
    lines.append("memcpy / memset activities inside DeviceCellRelax.run(2): %d %s" % (sum(copies.values()), copies))
    if not ours:
        lines.append("(the profiler recorded no device activity for graph launches)")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.launches, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.05, help="rattle of the start coordinates (A)")
    ap.add_argument("--margin", type=float, default=0.25, help="columns of the padded list beyond the first count")
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cellrelax_bench: needs the GPU (nothing is measured without one)")
    launches(a) if a.launches else bench(a)
