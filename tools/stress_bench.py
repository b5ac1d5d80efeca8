#!/usr/bin/env python3
"""What a stress step costs, three forms interleaved in one process, on the configs[1] cell (10k atoms, built as bench.py
builds it) and on a 108-atom alloy cell (same model):

    P: the plain step (relation build + forward + forces), for scale
    A: the two-backward path -- `plugin.ase_interface._evaluate(want_virial=True)`: autograd.grad(E, pos), then
       `utils.virial_calc`'s autograd.grad(E, cell)
    B: `hermnet_amd.energy_forces_stress`, eager: one forward, one backward, the virial kernels alongside
    C: the replayed `GraphedMDStep(stress=True, variable_cell=True)` -- ONE graph launch that ALSO contains the neighbour
       search (positions and cell uploaded per call), which P / A / B do not pay for here
    G: the replayed plain `GraphedMDStep` (fixed cell, no stress), for scale of C

then the kernels' times from a separate `rocprofv3 --kernel-trace --stats` run of A and B (a child process).  Writes
profiles/stress_step.json.

    python tools/stress_bench.py [--steps 50] [--rounds 6] [--out profiles/stress_step.json] [--no-profile]
    python tools/stress_bench.py --only AB --steps 20      (the workload the profiled child runs)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hermnet_amd as hn  # noqa: E402
from hermnet_amd import synth  # noqa: E402
from hermnet_amd.graph import GraphedMDStep  # noqa: E402
from hermnet_amd.plugin import ase_interface as A  # noqa: E402

CELLS = {"configs1_10k": (10, 10, 25), "alloy108": (3, 3, 3)}


def setup(dev, reps):
    """bench.py's configs[1] model on an fcc alloy cell of `reps`."""
    model = hn.HVNet(["Al", "Ni", "Cu"], rc=5.0, num_layers=5, hidden_channels=128, num_rbf=128).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
    model = model.to(dev)
    for p in model.parameters():
        p.requires_grad_(False)
    return model, synth.fcc_alloy(reps=reps, seed=0, device=dev)


def forms(model, d, dev, replay=True):
    def plain():
        d.pos.requires_grad_(True)
        e = model(d)
        return e, -torch.autograd.grad(e.sum(), d.pos)[0]

    # (A asks for the cell's gradient: on tensors of its own, so that P and B do not pay for the [E,3,3] outer product)
    da = hn.Data(**{k: v.detach().clone() for k, v in d})
    out = {"P": plain,
           "A": lambda: A._evaluate(model, da, dev, True, True),
           "B": lambda: hn.energy_forces_stress(model, d)}
    if replay:
        cell, pos = d.cell[0].detach().clone(), d.pos.detach().clone()
        c = GraphedMDStep(model, d.atomic_number, cell, pos, stress=True, variable_cell=True)
        g = GraphedMDStep(model, d.atomic_number, cell, pos)
        out["C"] = lambda: c(pos, cell)
        out["G"] = lambda: g(pos)
    return out


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_stats(steps, cell):
    """rocprofv3 --kernel-trace --stats of `--only AB` in a child process -> {kernel: (calls, average us)} of the geometry
    backward and virial kernels."""
    outdir = tempfile.mkdtemp(prefix="stress_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--only", "AB", "--steps", str(steps), "--warmup", "3", "--cell", cell]
    subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
    shown = " ".join(cmd[:6] + ["<tmpdir>"] + cmd[7:10] + ["python", "tools/stress_bench.py"] + cmd[12:])
    out = {}
    for f in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "edge_geometry" in row["Name"] or "graph_virial" in row["Name"]:
                    out[row["Name"]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    return shown, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--cell", default=None, choices=sorted(CELLS), help="one cell only (default: both)")
    ap.add_argument("--only", default=None, help="just run these forms, e.g. AB (profiled child)")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stress_step.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"command": "python tools/stress_bench.py --steps %d --rounds %d" % (args.steps, args.rounds),
           "forms": {"P": "plain energy + forces", "A": "_evaluate(want_virial=True): two backward passes",
                     "B": "energy_forces_stress, eager: one backward", "C": "replayed GraphedMDStep(stress, variable_cell), "
                     "neighbour search included", "G": "replayed plain GraphedMDStep, neighbour search included"},
           "cells": {}}
    for name in ([args.cell] if args.cell else sorted(CELLS)):
        model, data = setup(dev, CELLS[name])
        fn = forms(model, data, dev, replay=not args.only)
        for _ in range(args.warmup):
            for k in fn:
                fn[k]()
        if args.only:
            for _ in range(args.steps):
                for k in args.only:
                    fn[k]()
            torch.cuda.synchronize()
            continue
        ms = {k: [] for k in fn}
        order = sorted(fn)
        for r in range(args.rounds):              # interleaved, the order alternating round by round
            for k in (order if r % 2 == 0 else order[::-1]):
                ms[k].append(timed(fn[k], args.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = {"workload": "%d atoms, %d edges, HVNet hidden=128 num_rbf=128 layers=5" % (data.pos.size(0), data.edge_index.size(1)),
               "ms_per_step": med, "rounds_ms": ms, "A_minus_B_ms": med["A"] - med["B"], "B_minus_P_ms": med["B"] - med["P"],
               "A_over_B": med["A"] / med["B"], "C_minus_G_ms": med["C"] - med["G"]}
        if not args.no_profile:
            rec["profile_command"], rec["kernels"] = kernel_stats(20, name)
        res["cells"][name] = rec
    if args.only:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
