#!/usr/bin/env python3
"""ms per relaxation step (= force evaluation): `DeviceRelax.run(n)` (hermnet_amd/relax.py: FIRE inside the replayed graph)
against the host-driven loop it replaces -- `GraphedMDStep(pos)` / `GraphedBatchMDStep(pos)` + `fetch()` + the numpy FIRE of
the tests (tests/relax_reference.py: NumpyRelax, the same arithmetic in the same order) per evaluation.  Both arms in ONE
process, alternating, same structures, model and start state; a window ends in a synchronisation (the device arm's in
`fetch()`).  `fmax` is set out of reach, so every evaluation of a window moves every structure.

    python tools/relax_bench.py [--steps 100] [--rounds 5] [--out profiles/device_relax.json]

Cases: 108 atoms (3x3x3), 1008 atoms (6x6x7), a batch of 64 structures of 32 atoms (2x2x2); model of BASELINE configs[1]."""
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
import torch  # noqa: E402

import hermnet_amd as hn  # noqa: E402
from hermnet_amd import synth  # noqa: E402
from hermnet_amd.graph import GraphedBatchMDStep, GraphedMDStep  # noqa: E402
from hermnet_amd.neighbor import neighbor_search, padded_capacity  # noqa: E402
from hermnet_amd.relax import DeviceRelax  # noqa: E402
from relax_reference import NumpyRelax  # noqa: E402

CASES = [("108 atoms", [(3, 3, 3)]), ("1008 atoms", [(6, 6, 7)]), ("64 x 32 atoms", [(2, 2, 2)] * 64)]
FMAX = 1e-6


def model_for(dev):
    model = hn.HVNet(["Al", "Ni", "Cu"], rc=5.0, num_layers=5, hidden_channels=128, num_rbf=128).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
    model = model.to(dev)
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def setup(members, sigma):
    parts = [synth.fcc_alloy_atoms(reps=r, seed=s, sigma=sigma) for s, r in enumerate(members)]
    pos, z = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
    if len(members) == 1:
        return pos, parts[0][1], z, None
    return pos, np.stack([p[1] for p in parts]), z, np.repeat(np.arange(len(parts)), [len(p[0]) for p in parts])


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
        pos, cell, z, batch = setup(members, a.sigma)
        B = len(members)
        z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
        p0 = torch.from_numpy(pos.astype(np.float32)).to(dev)
        kw = {} if batch is None else dict(batch=torch.from_numpy(batch).to(dev), num_graphs=B)
        first = int(neighbor_search(p0, 5.0, cell_t, **kw)[0].size(1))
        capacity = padded_capacity(first, margin=a.margin)                # both arms on the same column count
        host = HostLoop(model, pos, cell, z, batch, dev, capacity)
        rx = DeviceRelax(model, z_t, cell_t, pos, fmax=FMAX, log_steps=max(a.steps, 64), capacity=capacity, **kw)
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
        same = bool(np.array_equal(snap.positions, host.opt.x))
        row = {"case": name, "atoms": int(len(z)), "graphs": B, "edges_at_start": first, "capacity": capacity,
               "host_loop_ms": [statistics.median(t_host), min(t_host), max(t_host)],
               "device_relax_ms": [statistics.median(t_dev), min(t_dev), max(t_dev)],
               "ratio_host_over_device": statistics.median(t_host) / statistics.median(t_dev),
               "device_steps_done": snap.step, "device_halted": bool(snap.halted), "host_loop_lists_complete": bool(host.ok),
               "fmax_at_end": float(snap.fmax.max()), "arms_end_bit_equal": same}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.05, help="rattle of the start coordinates (A)")
    ap.add_argument("--margin", type=float, default=0.25, help="columns of the padded list beyond the first count")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("relax_bench: needs the GPU (nothing is measured without one)")
    bench(a)
