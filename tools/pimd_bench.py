#!/usr/bin/env python3
"""ms per time step of a ring polymer: `DevicePIMD.run(n)` (hermnet_amd/pimd.py: the normal-mode propagation inside the
replayed graph) against the host-driven loop it replaces, and against the same batch without the springs.  Three arms in ONE
process, alternating, same beads, model and start state; a window ends in a synchronisation:

    (a) host loop    a plain `GraphedBatchMDStep`; every step the float32 coordinates go up, energies and forces come down,
                     and the ring's step is numpy (tests/pimd_reference.py: NumpyPIMD, the same arithmetic)
    (b) DevicePIMD   run(steps) + one fetch() per window
    (c) DeviceMD     Langevin on the same, uncoupled batch at P T, run(steps) + one fetch(): (b) - (c) is what the coupling costs

The timed windows run the PILE-L thermostat (the Gaussians of arm (a) are the library's host form; the device's differ in
the last digits, so those arms end close, not equal).  Behind them both PIMD arms run `--check` steps WITHOUT the thermostat
from one start and must end bit-equal.

    python tools/pimd_bench.py [--steps 200] [--rounds 5] [--out profiles/device_pimd.json]
    python tools/pimd_bench.py --launches profiles/device_pimd_launches.txt      # device activity of the replays

Cases: 8 beads of 32 atoms (2x2x2) and 8 of 108 atoms (3x3x3) of the fcc alloy cell, T = 300 K, tau0 = 100 fs, dt 0.5 fs; model
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

from hermnet_amd import synth  # noqa: E402
from hermnet_amd.graph import GraphedBatchMDStep  # noqa: E402
from hermnet_amd.md import AMU_A2_FS2_TO_EV, KB, DeviceMD  # noqa: E402
from hermnet_amd.neighbor import neighbor_search, padded_capacity  # noqa: E402
from hermnet_amd.pimd import DevicePIMD  # noqa: E402
from pimd_reference import NumpyPIMD  # noqa: E402
from relax_bench import model_for  # noqa: E402

BEADS, DT, T, TAU0, SEED = 8, 0.5, 300.0, 100.0, 2024
CASES = [("8 x 32 atoms", (2, 2, 2)), ("8 x 108 atoms", (3, 3, 3))]
MASS = {13: 26.9815, 28: 58.6934, 29: 63.546}


def ring(reps, beads):
    """(pos, cell [3,3], cells [P,3,3], z, masses, batch, velocities) of P beads of one rattled cell, spread by 0.02 A around
    their atom, Maxwell-Boltzmann velocities at P T."""
    pos, cell, z = synth.fcc_alloy_atoms(reps=reps)
    rs = np.random.RandomState(1)
    m = np.tile(np.array([MASS[int(v)] for v in z]), beads)
    x = np.tile(pos, (beads, 1)) + rs.normal(scale=0.02, size=(beads * len(z), 3))
    v = rs.normal(size=(len(m), 3)) * np.sqrt(KB * beads * T / (m * AMU_A2_FS2_TO_EV))[:, None]
    return x, cell, np.tile(cell, (beads, 1, 1)), np.tile(z, beads), m, np.repeat(np.arange(beads), len(z)), v


class HostLoop(object):
    """Arm (a): the ring polymer's step on the host around a graphed step that knows nothing of it."""

    def __init__(self, model, z_t, cells_t, batch_t, x, v, m, cell, capacity, thermostat, dev):
        self.dev = dev
        self.ref = NumpyPIMD(BEADS, x, v, m, DT, T, tau0=TAU0, thermostat=thermostat, seed=SEED, cell=cell, log_steps=8)
        self.step = GraphedBatchMDStep(model, z_t, cells_t, torch.from_numpy(self.ref.pos32).to(dev), batch_t, BEADS,
                                       capacity=capacity)
        _, self.ref.f_prev = self._forces(self.ref.pos32)

    def _forces(self, pos32):
        e, f = self.step(torch.from_numpy(pos32).to(self.dev))
        return e.cpu().numpy(), f.cpu().numpy()

    def run(self, n):
        for _ in range(n):
            e, f = self._forces(self.ref.advance())
            ok, found = self.step.check()
            if not ok:
                sys.exit("pimd_bench: the host loop's list overflowed -- raise --margin")
            self.ref.finish(f, e, total=(found, 0))


def ms(ts):
    return [statistics.median(ts), min(ts), max(ts)]


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    out = {"what": "ms per time step of a ring polymer of %d beads (T %g K, dt %g fs, PILE-L, tau0 %g fs): (a) GraphedBatchMDStep + "
                   "download + NumpyPIMD + upload every step, (b) DevicePIMD.run(n) + one fetch() per window, (c) DeviceMD "
                   "Langevin on the same uncoupled batch at P T, run(n) + one fetch() per window; %d alternating rounds of %d "
                   "steps, median (min, max)" % (BEADS, T, DT, TAU0, a.rounds, a.steps),
           "cases": []}
    for name, reps in CASES:
        x, cell, cells, z, m, batch, v = ring(reps, BEADS)
        z_t, cells_t = torch.from_numpy(z).to(dev), torch.from_numpy(cells.astype(np.float32)).to(dev)
        batch_t = torch.from_numpy(batch).to(dev)
        p0 = torch.from_numpy(x.astype(np.float32)).to(dev)
        first = int(neighbor_search(p0, 5.0, cells_t, batch=batch_t, num_graphs=BEADS)[0].size(1))
        capacity = padded_capacity(first, margin=a.margin)               # every arm on the same column count
        kw = dict(batch=batch_t, num_graphs=BEADS, seed=SEED, velocities=v, log_steps=max(a.steps, a.check, 64), capacity=capacity)
        pimd = DevicePIMD(model, z_t, cells_t, x, m, DT, T, tau0=TAU0, **kw)
        plain = DeviceMD(model, z_t, cells_t, x, m, DT, temperature=BEADS * T, friction=1.0 / TAU0, **kw)
        host = HostLoop(model, z_t, cells_t, batch_t, x, v, m, cell, capacity, True, dev)
        t_host, t_pimd, t_plain, snap, psnap = [], [], [], None, None
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host.run(a.steps)
            torch.cuda.synchronize()
            t_host.append((time.perf_counter() - t0) / a.steps * 1e3)
            t0 = time.perf_counter()
            pimd.run(a.steps)
            snap = pimd.fetch()
            t_pimd.append((time.perf_counter() - t0) / a.steps * 1e3)
            t0 = time.perf_counter()
            plain.run(a.steps)
            psnap = plain.fetch()
            t_plain.append((time.perf_counter() - t0) / a.steps * 1e3)
        close = float(np.abs(snap.positions - host.ref.x).max())
        # thermostat off, both arms from one start: bit-equal
        rpmd = DevicePIMD(model, z_t, cells_t, x, m, DT, T, thermostat=False, **kw)
        href = HostLoop(model, z_t, cells_t, batch_t, x, v, m, cell, capacity, False, dev)
        rpmd.run(a.check)
        href.run(a.check)
        end = rpmd.fetch()
        same = bool(np.array_equal(end.positions.view(np.uint64), href.ref.x.view(np.uint64))
                    and np.array_equal(end.velocities.view(np.uint64), href.ref.v.view(np.uint64))
                    and np.array_equal(end.images, href.ref.image) and end.step == a.check and not end.halted)
        row = {"case": name, "atoms": int(len(z)), "beads": BEADS, "edges_at_start": first, "capacity": capacity,
               "host_loop_ms": ms(t_host), "device_pimd_ms": ms(t_pimd), "device_md_ms": ms(t_plain),
               "ratio_host_over_device": statistics.median(t_host) / statistics.median(t_pimd),
               "coupling_cost_ms": statistics.median(t_pimd) - statistics.median(t_plain),
               "steps_done": [int(host.ref.state[0]), int(snap.step), int(psnap.step)],
               "halted": [bool(host.ref.state[1]), bool(snap.halted), bool(psnap.halted)],
               "thermostatted_arms_max_position_difference": close,
               "rpmd_check_steps": a.check, "rpmd_arms_end_bit_equal": same}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


def device_events(fn):
    """The device activities of `fn()` by name, as the profiler saw them."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)


def launch_lists(model, dev, beads=5):
    """(DeviceMD's, DevicePIMD's) device activity of two replays on the same batch of `beads` x 32 atoms."""
    x, _, cells, z, m, batch, v = ring((2, 2, 2), beads)
    z_t, cells_t = torch.from_numpy(z).to(dev), torch.from_numpy(cells.astype(np.float32)).to(dev)
    kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=beads, seed=SEED, velocities=v)
    plain_md = DeviceMD(model, z_t, cells_t, x, m, DT, temperature=beads * T, friction=1.0 / TAU0, **kw)
    polymer = DevicePIMD(model, z_t, cells_t, x, m, DT, T, tau0=TAU0, **kw)
    plain_md.run(4)
    polymer.run(4)
    torch.cuda.synchronize()
    return device_events(lambda: plain_md.run(2)), device_events(lambda: polymer.run(2))


def launches(a):
    """Device activity of two DeviceMD replays and of two DevicePIMD replays on the same batch of 5 x 32 atoms: the kernels by
    name and count, and every memcpy / memset the profiler saw."""
    dev = torch.device("cuda:0")
    plain, ours = launch_lists(model_for(dev), dev)
    lines = ["device activity of 2 replays, batch of 5 x 32 atoms: DeviceMD.run(2) | DevicePIMD.run(2)    (count name)"]
    for name in sorted(set(plain) | set(ours)):
        lines.append("%4d %4d  %s" % (plain.get(name, 0), ours.get(name, 0), name[:150]))
    extra = {k[:100]: c - plain.get(k, 0) for k, c in ours.items() if c != plain.get(k, 0)}
    extra.update({k[:100]: -c for k, c in plain.items() if k not in ours})
    copies = {k: c for k, c in ours.items() if "memcpy" in k.lower() or "memset" in k.lower()}
    lines.append("kernels: DeviceMD %d, DevicePIMD %d; difference: %s" % (sum(plain.values()), sum(ours.values()), extra))
    lines.append("memcpy / memset activities inside DevicePIMD.run(2): %d %s" % (sum(copies.values()), copies))
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
    ap.add_argument("--check", type=int, default=20, help="steps of the bit-equality run without the thermostat")
    ap.add_argument("--margin", type=float, default=0.25, help="columns of the padded list beyond the first count")
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pimd_bench: needs the GPU (nothing is measured without one)")
    launches(a) if a.launches else bench(a)
