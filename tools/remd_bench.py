#!/usr/bin/env python3
"""ms per time step of a replica-exchange ladder: `DeviceREMD.run(n)` (hermnet_amd/remd.py: the exchanges inside the
replayed graph) against the host-driven loop it replaces, and against the same batch without exchange.  Three arms in ONE
process, alternating, same replicas, model, seed and start state; a window ends in a synchronisation (a `fetch()`):

    (a) host loop    `DeviceMD` on the batch; every `interval` steps `fetch()`, the decisions in numpy (tests/remd_reference.py:
                     decide, the same arithmetic), then velocities and `sigma` uploaded where a pair was accepted
    (b) DeviceREMD   run(steps) + one fetch() per window
    (c) DeviceMD     the same batch at the ladder's temperatures without exchange, run(steps) + one fetch(): (b) - (c) is
                     what the feature costs

    python tools/remd_bench.py [--steps 200] [--rounds 5] [--interval 10] [--out profiles/device_remd.json]
    python tools/remd_bench.py --launches profiles/device_remd_launches.txt      # device activity of the replays

Cases: 8 replicas of 32 atoms (2x2x2) and 8 of 108 atoms (3x3x3) of the fcc alloy cell, temperatures 600 K x 1.08^r, friction
0.01 /fs, dt 1 fs; model of BASELINE configs[1]."""
import json
import statistics
import sys

import numpy as np
from resident_bench import copies, fetched, launch_table, main, model_for, ms, on_device, time_arms  # (sets the path)
import torch

from hermnet_amd.md import DeviceMD
from hermnet_amd.remd import DeviceREMD
from remd_reference import decide

REPLICAS, DT, FRICTION, SEED = 8, 1.0, 0.01, 2024
CASES = [("8 x 32 atoms", (2, 2, 2)), ("8 x 108 atoms", (3, 3, 3))]


class HostLoop(object):
    """Arm (a): the ladder's bookkeeping on the host around a `DeviceMD` that knows nothing of it."""

    def __init__(self, md, ref, interval):
        self.md, self.interval, self.step = md, interval, 0
        self.beta, self.up, self.down = (t.cpu().numpy() for t in (ref.beta, ref.up, ref.down))
        self.table, self.n_rep = ref.sigma_table.cpu().numpy(), ref.n_rep
        self.rung = np.arange(md.num_graphs)
        self.accepted = 0

    def run(self, n):
        """`n` steps (a multiple of the interval); returns the last snapshot."""
        snap = None
        for _ in range(n // self.interval):
            self.md.run(self.interval)
            snap = self.md.fetch()
            self.step += self.interval
            pairs = decide(SEED, self.step - 1, self.interval, self.beta, snap.log[-1, :, 0].astype(np.float32),
                           np.argsort(self.rung))
            if any(p[5] for p in pairs):
                v = snap.velocities
                for r, ga, gb, _, _, yes in pairs:
                    if yes:
                        self.rung[ga], self.rung[gb] = r + 1, r
                        v[ga * self.n_rep:(ga + 1) * self.n_rep] *= self.up[r]
                        v[gb * self.n_rep:(gb + 1) * self.n_rep] *= self.down[r]
                        self.accepted += 1
                self.md.set_velocities(v)
                self.md.sigma.copy_(torch.from_numpy(np.ascontiguousarray(self.table[self.rung].reshape(-1))))
        return snap


def bench(a):
    dev = torch.device("cuda:0")
    model = model_for(dev)
    temps = 600.0 * 1.08 ** np.arange(REPLICAS)
    if a.steps % a.interval:
        sys.exit("remd_bench: --steps must be a multiple of --interval")
    out = {"what": "ms per time step of %d Langevin replicas (dt %g fs, friction %g /fs, temperatures 600 K x 1.08^r, an exchange "
                   "attempt every %d steps): (a) DeviceMD + fetch() + numpy decisions + uploads every interval, (b) "
                   "DeviceREMD.run(n) + one fetch() per window, (c) DeviceMD.run(n) + one fetch() per window, no exchange; %d "
                   "alternating rounds of %d steps, median (min, max)" % (REPLICAS, DT, FRICTION, a.interval, a.rounds, a.steps),
           "cases": []}
    for name, reps in CASES:
        pos, cell, z, m, batch, v = copies(reps, temps)
        z_t, cell_t, _, kw, first, capacity = on_device(dev, pos, cell, z, batch, a.margin)    # every arm on the same column count
        kw.update(seed=SEED, velocities=v, log_steps=max(a.steps, 64), capacity=capacity)
        remd = DeviceREMD(model, z_t, cell_t, pos, m, DT, temps, FRICTION, a.interval, **kw)
        plain = DeviceMD(model, z_t, cell_t, pos, m, DT, temperature=temps, friction=FRICTION, **kw)
        host = HostLoop(DeviceMD(model, z_t, cell_t, pos, m, DT, temperature=temps, friction=FRICTION, **kw), remd, a.interval)
        t, last = time_arms([("host", a.steps, host.run, dict(sync=True)), ("remd", a.steps, fetched(remd)), ("plain", a.steps, fetched(plain))],
                            a.rounds)
        hsnap, snap, psnap = last["host"], last["remd"], last["plain"]
        # (the host arm's last upload is not in its last snapshot: compare what both arms hold on the device)
        same = bool(torch.equal(host.md.x, remd.x) and torch.equal(host.md.v, remd.v) and torch.equal(host.md.sigma, remd.sigma)
                    and np.array_equal(host.rung, snap.rung))
        row = {"case": name, "atoms": int(len(z)), "replicas": REPLICAS, "interval": a.interval, "edges_at_start": first,
               "capacity": capacity, "host_loop_ms": ms(t["host"]), "device_remd_ms": ms(t["remd"]), "device_md_ms": ms(t["plain"]),
               "ratio_host_over_device": statistics.median(t["host"]) / statistics.median(t["remd"]),
               "exchange_cost_ms": statistics.median(t["remd"]) - statistics.median(t["plain"]),
               "steps_done": [int(hsnap.step), int(snap.step), int(psnap.step)],
               "halted": [bool(hsnap.halted), bool(snap.halted), bool(psnap.halted)],
               "attempts": snap.attempts.tolist(), "accepts": snap.accepts.tolist(), "host_loop_accepts": host.accepted,
               "arms_end_bit_equal": same}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    return out


def launches(a):
    """Device activity of two DeviceMD replays and of two DeviceREMD replays (an attempt in each: interval 1) on the same
    batch of 5 x 32 atoms: the kernels by name and count, and every memcpy / memset the profiler saw."""
    dev = torch.device("cuda:0")
    model = model_for(dev)
    temps = 600.0 * 1.08 ** np.arange(5)
    pos, cell, z, m, batch, v = copies((2, 2, 2), temps)
    z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
    kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=5, seed=SEED, velocities=v)
    plain_md = DeviceMD(model, z_t, cell_t, pos, m, DT, temperature=temps, friction=FRICTION, **kw)
    ladder = DeviceREMD(model, z_t, cell_t, pos, m, DT, temps, FRICTION, 1, **kw)
    plain_md.run(4)
    ladder.run(4)
    torch.cuda.synchronize()
    launch_table("device activity of 2 replays, batch of 5 x 32 atoms: DeviceMD.run(2) | DeviceREMD.run(2), interval 1",
                 "DeviceMD", lambda: plain_md.run(2), "DeviceREMD", lambda: ladder.run(2), a.launches)


if __name__ == "__main__":
    main("remd_bench", bench, launches, flags=[("--steps", dict(type=int, default=200)), ("--interval", dict(type=int, default=10))])
