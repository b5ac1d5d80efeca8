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
import json
import statistics
import sys

import numpy as np
from resident_bench import cells, fetched, launch_table, main, model_for, ms, on_device, time_arms  # (sets the path)
import torch

from hermnet_amd.graph import GraphedBatchMDStep
from hermnet_amd.md import DeviceMD
from hermnet_amd.swapmc import DeviceSwapMD
from swapmc_reference import pick_pair, trial_uniform

DT, FRICTION, SEED, T_MD, T_MC = 1.0, 0.01, 2024, 600.0, 800.0
CASES = [("8 x 32 atoms", 8, (2, 2, 2)), ("8 x 108 atoms", 8, (3, 3, 3)), ("1 x 1008 atoms", 1, (6, 6, 7))]


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
        pos, cell, z, m, batch, v = cells([reps] * B, T_MD)
        z_t, cell_t, p0, kw, first, capacity = on_device(dev, pos, cell, z, batch, a.margin)    # every arm on the same column count
        kw.update(seed=SEED, velocities=v, log_steps=max(a.replays, 64), capacity=capacity, temperature=T_MD, friction=FRICTION)
        plain = DeviceMD(model, z_t, cell_t, pos, m, DT, **kw)
        ours = DeviceSwapMD(model, z_t, cell_t, pos, m, DT, a.interval, a.swaps, mc_temperature=T_MC, **kw)
        host = HostLoop(DeviceMD(model, z_t, cell_t, pos, m, DT, **kw),
                        GraphedBatchMDStep(model, z_t, cell_t, p0, kw["batch"], B, capacity=capacity), ours, a.interval, a.swaps)

        def drawn_ahead(r):                                                      # (untimed, and its own synchronisation)
            host.prepare(a.replays // block * a.swaps)
            torch.cuda.synchronize()

        t, last = time_arms([("plain", a.replays, fetched(plain)), ("ours", a.replays, fetched(ours)),
                             ("host", a.replays, lambda n: host.run(n // block), dict(sync=True, before=drawn_ahead))], a.rounds)
        t_plain, t_ours, t_host, psnap, snap, hsnap = t["plain"], t["ours"], t["host"], last["plain"], last["ours"], last["host"]
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
    return out


def launches(a):
    """Device activity of two DeviceMD replays and of two DeviceSwapMD replays (an MD step and a trial: interval 1, swaps 1)
    on the same batch of 5 x 32 atoms: the kernels by name and count, and every memcpy / memset the profiler saw."""
    dev = torch.device("cuda:0")
    model = model_for(dev)
    pos, cell, z, m, batch, v = cells([(2, 2, 2)] * 5, T_MD)
    z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
    kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=5, seed=SEED, velocities=v, temperature=T_MD, friction=FRICTION)
    plain_md = DeviceMD(model, z_t, cell_t, pos, m, DT, **kw)
    swap_md = DeviceSwapMD(model, z_t, cell_t, pos, m, DT, 1, 1, mc_temperature=T_MC, **kw)
    plain_md.run(4)
    swap_md.run(4)
    torch.cuda.synchronize()
    launch_table("device activity of 2 replays, batch of 5 x 32 atoms: DeviceMD.run(2) | DeviceSwapMD.run(2), an MD step and a trial",
                 "DeviceMD", lambda: plain_md.run(2), "DeviceSwapMD", lambda: swap_md.run(2), a.launches)


if __name__ == "__main__":
    main("swapmc_bench", bench, launches, flags=[("--replays", dict(type=int, default=200)), ("--interval", dict(type=int, default=10)),
                                                 ("--swaps", dict(type=int, default=10))])
