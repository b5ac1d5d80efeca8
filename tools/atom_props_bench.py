#!/usr/bin/env python3
"""What per-atom energies + virials cost on the bench step: configs[1] cell (10k atoms, built as bench.py builds it), step =
relation build + forward + forces.  Interleaved A/B in one process -- A: the plain step, B: the same step through
`hermnet_amd.atom_properties` (energies and virials) -- then the kernels' times from a separate
`rocprofv3 --kernel-trace --stats` run of both steps (a child process).  Writes profiles/atom_properties.json.

    python tools/atom_props_bench.py [--steps 50] [--rounds 6] [--out profiles/atom_properties.json] [--no-profile]
    python tools/atom_props_bench.py --only AB --steps 20      (the workload the profiled child runs)
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


def setup(dev):
    """bench.py's configs[1] model and cell."""
    model = hn.HVNet(["Al", "Ni", "Cu"], rc=5.0, num_layers=5, hidden_channels=128, num_rbf=128).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
    model = model.to(dev)
    for p in model.parameters():
        p.requires_grad_(False)
    return model, synth.fcc_alloy(reps=(10, 10, 25), seed=0, device=dev)


def step_a(model, d):
    d.pos.requires_grad_(True)
    e = model(d)
    return e, -torch.autograd.grad(e.sum(), d.pos)[0]


def step_b(model, d):
    out = hn.atom_properties(model, d)
    return out["energy"], out["forces"]


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_stats(steps):
    """rocprofv3 --kernel-trace --stats of `--only AB` in a child process -> {kernel: (calls, average us)} of the geometry
    backward kernels."""
    outdir = tempfile.mkdtemp(prefix="atom_props_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--only", "AB", "--steps", str(steps), "--warmup", "3"]
    subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
    shown = " ".join(cmd[:6] + ["<tmpdir>"] + cmd[7:10] + ["python", "tools/atom_props_bench.py"] + cmd[12:])
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    out = {}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "edge_geometry" in row["Name"]:
                    out[row["Name"]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    return shown, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--only", default=None, choices=["A", "B", "AB"], help="just run these steps (profiled child)")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atom_properties.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model, data = setup(dev)
    fa, fb = (lambda: step_a(model, data)), (lambda: step_b(model, data))
    for _ in range(args.warmup):
        fa()
        fb()
    if args.only:
        for _ in range(args.steps):
            if "A" in args.only:
                fa()
            if "B" in args.only:
                fb()
        torch.cuda.synchronize()
        return
    a_ms, b_ms = [], []
    for r in range(args.rounds):              # interleaved, the order alternating round by round
        for which in (("A", "B") if r % 2 == 0 else ("B", "A")):
            (a_ms if which == "A" else b_ms).append(timed(fa if which == "A" else fb, args.steps))
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    res = {"workload": "configs[1] cell (%d atoms, %d edges), HVNet hidden=128 num_rbf=128 layers=5; step = relation build + "
                       "forward + forces" % (data.pos.size(0), data.edge_index.size(1)),
           "command": "python tools/atom_props_bench.py --steps %d --rounds %d" % (args.steps, args.rounds),
           "ms_per_step": {"A_plain": a, "B_energies_virials": b}, "rounds_ms": {"A": a_ms, "B": b_ms},
           "overhead_ms": b - a, "overhead_pct": 100.0 * (b - a) / a}
    if not args.no_profile:
        res["profile_command"], res["kernels"] = kernel_stats(20)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
