#!/usr/bin/env python3
"""ms per replay of hybrid swap Monte Carlo / MD: `DeviceSwapMD.run(n)` (hermnet_amd/swapmc.py: the trials inside the
replayed graph) against `DeviceMD` on the same batch and against the host-driven loop it replaces.  Three arms in ONE
process, alternating, same batch, model, seed and start state; a window ends in a synchronisation (a `fetch()`):

    (a) DeviceMD       run(replays) + one fetch(): the yardstick -- a trial replay costs a full step, so (b) - (a) is what the
                       two hooks' extra work costs per replay
    (b) DeviceSwapMD   run(replays) + one fetch(): `interval` MD steps, `swaps` trial replays, and again
    (c) host loop      `DeviceMD.run(interval)` + `fetch()`, then per trial: the exchange in numpy (the pairs and uniforms of
                       tests/swapmc_reference.py, drawn ahead of the window -- the same arithmetic), a plain
                       `GraphedBatchMDStep` on the trial coordinates + its `fetch()`, the decisions in numpy, and where a graph
                       accepted the upload of coordinates, images and forces

    python tools/swapmc_bench.py [--replays 200] [--rounds 5] [--interval 10] [--swaps 10] [--out profiles/device_swapmc.json]
    python tools/swapmc_bench.py --launches profiles/device_swapmc_launches.txt      # device activity of the replays

Cases: 8 x 32 atoms (2x2x2), 8 x 108 atoms (3x3x3) -- eight DIFFERENT cells -- and 1 x 1008 atoms (6x6x7) of the fcc alloy;
Langevin at 600 K, friction 0.01 /fs, dt 1 fs, swaps at 800 K; model of BASELINE configs[1]."""
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
from hermnet_amd.swapmc import DeviceSwapMD  # noqa: E402
from relax_bench import model_for  # noqa: E402
from swapmc_reference import pick_pair, trial_uniform  # noqa: E402

DT, FRICTION, SEED, T_MD, T_MC = 1.0, 0.01, 2024, 600.0, 800.0
CASES = [("8 x 32 atoms", 8, (2, 2, 2)), ("8 x 108 atoms", 8, (3, 3, 3)), ("1 x 1008 atoms", 1, (6, 6, 7))]
MASS = {13: 26.9815, 28: 58.6934, 29: 63.546}


def members(B, reps):
    """(pos, cell [B,3,3], z, masses, batch, velocities) of B different rattled cells, Maxwell-Boltzmann velocities."""
    parts = [synth.fcc_alloy_atoms(reps=reps, seed=g) for g in range(B)]
    pos, z = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
    m = np.array([MASS[int(v)] for v in z])
    v = np.random.RandomState(1).normal(size=(len(m), 3)) * np.sqrt(KB * T_MD / (m * AMU_A2_FS2_TO_EV))[:, None]
    return pos, np.stack([p[1] for p in parts]), z, m, np.repeat(np.arange(B), [len(p[0]) for p in parts]), v


class HostLoop(object):
    """Arm (c): the swaps on the host around a `DeviceMD` that knows nothing of them and a plain graphed step."""

    def __init__(self, md, step, ref, interval, swaps):
        self.md, self.step, self.interval, self.swaps = md, step, interval, swaps
        self.cand, self.ptr, self.beta = ref.cand.cpu().numpy(), ref.cand_ptr.cpu().numpy(), ref.beta.cpu().numpy()
        self.batch = md._batch_h
        self.t = self.accepted = 0
        self.drawn = {}

    def prepare(self, trials):
        """The pairs and log(u) of the next `trials` trials, OUTSIDE the timed window: they depend on (seed, t, g) alone, and
        the pure-Python Philox of the tests is no part of what a host loop costs."""
        B = self.md.num_graphs
        for t in range(self.t, self.t + trials):
            self.drawn[t] = ([pick_pair(SEED, t, g, self.cand, self.ptr[g]) for g in range(B)],
                             [float(np.log(trial_uniform(SEED, t, g))) for g in range(B)])

    def run(self, blocks):
        """`blocks` times (`interval` MD steps, `swaps` trials); returns the last snapshot."""
        snap = None
        for _ in range(blocks):
            self.md.run(self.interval)
            snap = self.md.fetch()
            x, image, f_prev, e_ref = snap.positions, snap.images, snap.forces, snap.log[-1, :, 0].copy()
            for _ in range(self.swaps):
                pairs, log_u = self.drawn.pop(self.t)
                for p in pairs:
                    if p is not None:
                        x[list(p)], image[list(p)] = x[list(p)[::-1]], image[list(p)[::-1]]
                self.step(torch.from_numpy(x.astype(np.float32)))
                e, f, _, _ = self.step.fetch()
                kept = False
                for g, p in enumerate(pairs):
                    if p is None:
                        continue
                    delta = -self.beta[g] * (np.float64(e[g]) - e_ref[g])
                    if delta >= 0.0 or log_u[g] < delta:
                        mine = self.batch == g
                        f_prev[mine], e_ref[g], kept = f[mine], np.float64(e[g]), True
                        self.accepted += 1
                    else:
                        x[list(p)], image[list(p)] = x[list(p)[::-1]], image[list(p)[::-1]]
                if kept:
                    self.md.x.copy_(torch.from_numpy(x))
                    self.md.image.copy_(torch.from_numpy(image))
                    self.md.f_prev.copy_(torch.from_numpy(f_prev))
                self.t += 1
        return snap


def ms(ts):
    return [statistics.median(ts), min(ts), max(ts)]


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    block = a.interval + a.swaps
    if a.replays % block:
        sys.exit("swapmc_bench: --replays must be a multiple of --interval + --swaps")
    out = {"what": "ms per replay (dt %g fs, Langevin %g K, friction %g /fs; %d MD steps then %d trial replays at %g K, and "
                   "again): (a) DeviceMD.run(n) + one fetch() per window, (b) DeviceSwapMD.run(n) + one fetch() per window, (c) "
                   "DeviceMD + fetch() every block, then per trial numpy pairs + GraphedBatchMDStep + fetch() + numpy decisions + "
                   "uploads; %d alternating rounds of %d replays, median (min, max)"
                   % (DT, T_MD, FRICTION, a.interval, a.swaps, T_MC, a.rounds, a.replays), "cases": []}
    for name, B, reps in CASES:
        pos, cell, z, m, batch, v = members(B, reps)
        z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
        batch_t = torch.from_numpy(batch).to(dev)
        p0 = torch.from_numpy(pos.astype(np.float32)).to(dev)
        first = int(neighbor_search(p0, 5.0, cell_t, batch=batch_t, num_graphs=B)[0].size(1))
        capacity = padded_capacity(first, margin=a.margin)                       # every arm on the same column count
        kw = dict(batch=batch_t, num_graphs=B, seed=SEED, velocities=v, log_steps=max(a.replays, 64), capacity=capacity,
                  temperature=T_MD, friction=FRICTION)
        plain = DeviceMD(model, z_t, cell_t, pos, m, DT, **kw)
        ours = DeviceSwapMD(model, z_t, cell_t, pos, m, DT, a.interval, a.swaps, mc_temperature=T_MC, **kw)
        host = HostLoop(DeviceMD(model, z_t, cell_t, pos, m, DT, **kw),
                        GraphedBatchMDStep(model, z_t, cell_t, p0, batch_t, B, capacity=capacity), ours, a.interval, a.swaps)
        t_plain, t_ours, t_host = [], [], []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plain.run(a.replays)
            psnap = plain.fetch()
            t_plain.append((time.perf_counter() - t0) / a.replays * 1e3)
            t0 = time.perf_counter()
            ours.run(a.replays)
            snap = ours.fetch()
            t_ours.append((time.perf_counter() - t0) / a.replays * 1e3)
            host.prepare(a.replays // block * a.swaps)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hsnap = host.run(a.replays // block)
            torch.cuda.synchronize()
            t_host.append((time.perf_counter() - t0) / a.replays * 1e3)
        # (the host arm's last uploads are not in its last snapshot: compare what both arms hold on the device)
        same = bool(torch.equal(host.md.x, ours.x) and torch.equal(host.md.v, ours.v) and torch.equal(host.md.f_prev, ours.f_prev))
        md_ms, ours_ms = statistics.median(t_plain), statistics.median(t_ours)
        row = {"case": name, "atoms": int(len(z)), "graphs": B, "interval": a.interval, "swaps": a.swaps, "edges_at_start": first,
               "capacity": capacity, "device_md_ms": ms(t_plain), "device_swapmd_ms": ms(t_ours), "host_loop_ms": ms(t_host),
               "overhead_ms": ours_ms - md_ms, "overhead_percent": 100.0 * (ours_ms - md_ms) / md_ms,
               "ratio_host_over_device": statistics.median(t_host) / ours_ms,
               "steps_done": [int(psnap.step), int(snap.step), int(hsnap.step)], "trials_done": int(snap.swap_trials),
               "halted": [bool(psnap.halted), bool(snap.halted), bool(hsnap.halted)],
               "attempts": snap.swap_attempts.tolist(), "accepts": snap.swap_accepts.tolist(), "host_loop_accepts": host.accepted,
               "arms_end_bit_equal": same}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


def launches(a):
    """Device activity of two DeviceMD replays and of two DeviceSwapMD replays (an MD step and a trial: interval 1, swaps 1)
    on the same batch of 5 x 32 atoms: the kernels by name and count, and every memcpy / memset the profiler saw."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda:0")
    model = model_for(dev)
    pos, cell, z, m, batch, v = members(5, (2, 2, 2))
    z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
    kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=5, seed=SEED, velocities=v, temperature=T_MD, friction=FRICTION)
    plain_md = DeviceMD(model, z_t, cell_t, pos, m, DT, **kw)
    swap_md = DeviceSwapMD(model, z_t, cell_t, pos, m, DT, 1, 1, mc_temperature=T_MC, **kw)
    plain_md.run(4)
    swap_md.run(4)
    torch.cuda.synchronize()

    def device_events(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    plain = device_events(lambda: plain_md.run(2))
    ours = device_events(lambda: swap_md.run(2))
    lines = ["device activity of 2 replays, batch of 5 x 32 atoms: DeviceMD.run(2) | DeviceSwapMD.run(2), an MD step and a trial"
             "    (count name)"]
    for name in sorted(set(plain) | set(ours)):
        lines.append("%4d %4d  %s" % (plain.get(name, 0), ours.get(name, 0), name[:150]))
    extra = {k[:100]: c - plain.get(k, 0) for k, c in ours.items() if c != plain.get(k, 0)}
    extra.update({k[:100]: -c for k, c in plain.items() if k not in ours})
    copies = {k: c for k, c in ours.items() if "memcpy" in k.lower() or "memset" in k.lower()}
    lines.append("kernels: DeviceMD %d, DeviceSwapMD %d; difference: %s" % (sum(plain.values()), sum(ours.values()), extra))
    lines.append("memcpy / memset activities inside DeviceSwapMD.run(2): %d %s" % (sum(copies.values()), copies))
    if not ours:
        lines.append("(the profiler recorded no device activity for graph launches)")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.launches, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--swaps", type=int, default=10)
    ap.add_argument("--margin", type=float, default=0.25, help="columns of the padded list beyond the first count")
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("swapmc_bench: needs the GPU (nothing is measured without one)")
    launches(a) if a.launches else bench(a)
