#!/usr/bin/env python3
"""ms per relaxation step (= force evaluation): `DeviceRelax.run(n)` (hermnet_amd/relax.py: FIRE inside the replayed graph)
against the host-driven loop it replaces -- `GraphedMDStep(pos)` / `GraphedBatchMDStep(pos)` + `fetch()` + the numpy FIRE of
the tests (tests/relax_reference.py: NumpyRelax, the same arithmetic in the same order) per evaluation.  Both arms in ONE
process, alternating, same structures, model and start state; a window ends in a synchronisation (the device arm's in
`fetch()`).  `fmax` is set out of reach, so every evaluation of a window moves every structure.

    python tools/relax_bench.py [--steps 100] [--rounds 5] [--out profiles/device_relax.json]

Cases: 108 atoms (3x3x3), 1008 atoms (6x6x7), a batch of 64 structures of 32 atoms (2x2x2); model of BASELINE configs[1]."""
import json
import statistics

import numpy as np
from resident_bench import FMAX, RELAX_CASES as CASES, fetched, main, model_for, ms, on_device, structures, time_arms  # (sets the path)
import torch

from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep
from hermnet_amd.relax import DeviceRelax
from relax_reference import NumpyRelax


class HostLoop(object):
    """One evaluation = upload float32(x), replay, `fetch()` (one copy + synchronisation), NumpyRelax on the host."""

    def __init__(self, model, pos, cell, z, batch, dev, capacity):
        z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
        p0 = torch.from_numpy(pos.astype(np.float32)).to(dev)
        B = 1 if batch is None else int(batch[-1]) + 1
        if batch is None:
            self.step = GraphedMDStep(model, z_t, cell_t, p0, capacity=capacity)
        else:
            self.step = GraphedBatchMDStep(model, z_t, cell_t, p0, torch.from_numpy(batch).to(dev), B, capacity=capacity)
        self.opt = NumpyRelax(pos, cell=cell, batch=batch, num_graphs=B, fmax=FMAX)
        self.ok = True

    def run(self, n):
        for _ in range(n):
            self.step(torch.from_numpy(self.opt.advance()))
            e, f, ok, found = self.step.fetch()
            self.ok = self.ok and ok
            self.opt.finish(f, energy=e, total=(found, 0))


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per relaxation step (FIRE, ASE defaults, start rattled by %.2f A, fmax out of reach): DeviceRelax.run(n) + "
                   "one fetch() per window vs graphed step + fetch() + numpy FIRE (tests/relax_reference.py: NumpyRelax, a "
                   "Python loop over the graphs) per step; %d alternating rounds of %d steps, median (min, max)"
                   % (a.sigma, a.rounds, a.steps), "cases": []}
    for name, members in CASES:
        pos, cell, z, batch = structures(members, a.sigma)
        B = len(members)
        z_t, cell_t, _, kw, first, capacity = on_device(dev, pos, cell, z, batch, a.margin)    # both arms on the same column count
        host = HostLoop(model, pos, cell, z, batch, dev, capacity)
        rx = DeviceRelax(model, z_t, cell_t, pos, fmax=FMAX, log_steps=max(a.steps, 64), capacity=capacity, **kw)
        host.run(10)
        rx.run(10)
        rx.fetch()
        t, last = time_arms([("host", a.steps, host.run, dict(sync=True)), ("dev", a.steps, fetched(rx))], a.rounds)
        snap = last["dev"]
        same = bool(np.array_equal(snap.positions, host.opt.x))
        row = {"case": name, "atoms": int(len(z)), "graphs": B, "edges_at_start": first, "capacity": capacity,
               "host_loop_ms": ms(t["host"]), "device_relax_ms": ms(t["dev"]),
               "ratio_host_over_device": statistics.median(t["host"]) / statistics.median(t["dev"]),
               "device_steps_done": snap.step, "device_halted": bool(snap.halted), "host_loop_lists_complete": bool(host.ok),
               "fmax_at_end": float(snap.fmax.max()), "arms_end_bit_equal": same}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    return out


if __name__ == "__main__":
    main("relax_bench", bench, flags=[("--steps", dict(type=int, default=100)),
                                      ("--sigma", dict(type=float, default=0.05, help="rattle of the start coordinates (A)"))])
