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
from hermnet_amd.md import AMU_A2_FS2_TO_EV, KB, DeviceMD  # noqa: E402
from hermnet_amd.neighbor import neighbor_search, padded_capacity  # noqa: E402
from hermnet_amd.remd import DeviceREMD  # noqa: E402
from relax_bench import model_for  # noqa: E402
from remd_reference import decide  # noqa: E402

REPLICAS, DT, FRICTION, SEED = 8, 1.0, 0.01, 2024
CASES = [("8 x 32 atoms", (2, 2, 2)), ("8 x 108 atoms", (3, 3, 3))]
MASS = {13: 26.9815, 28: 58.6934, 29: 63.546}


def replicas(reps, temperatures):
    """(pos, cell [R,3,3], z, masses, batch, velocities) of R copies of one rattled cell, Maxwell-Boltzmann velocities."""
    R = len(temperatures)
    pos, cell, z = synth.fcc_alloy_atoms(reps=reps)
    m = np.tile(np.array([MASS[int(v)] for v in z]), R)
    v = (np.random.RandomState(1).normal(size=(len(m), 3))
         * np.sqrt(KB * np.repeat(temperatures, len(z)) / (m * AMU_A2_FS2_TO_EV))[:, None])
    return np.tile(pos, (R, 1)), np.tile(cell, (R, 1, 1)), np.tile(z, R), m, np.repeat(np.arange(R), len(z)), v


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


def ms(ts):
    return [statistics.median(ts), min(ts), max(ts)]


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
        pos, cell, z, m, batch, v = replicas(reps, temps)
        z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
        batch_t = torch.from_numpy(batch).to(dev)
        p0 = torch.from_numpy(pos.astype(np.float32)).to(dev)
        first = int(neighbor_search(p0, 5.0, cell_t, batch=batch_t, num_graphs=REPLICAS)[0].size(1))
        kw = dict(batch=batch_t, num_graphs=REPLICAS, seed=SEED, velocities=v, log_steps=max(a.steps, 64),
                  capacity=padded_capacity(first, margin=a.margin))              # every arm on the same column count
        remd = DeviceREMD(model, z_t, cell_t, pos, m, DT, temps, FRICTION, a.interval, **kw)
        plain = DeviceMD(model, z_t, cell_t, pos, m, DT, temperature=temps, friction=FRICTION, **kw)
        host = HostLoop(DeviceMD(model, z_t, cell_t, pos, m, DT, temperature=temps, friction=FRICTION, **kw), remd, a.interval)
        t_host, t_remd, t_plain, snap, hsnap = [], [], [], None, None
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hsnap = host.run(a.steps)
            torch.cuda.synchronize()
            t_host.append((time.perf_counter() - t0) / a.steps * 1e3)
            t0 = time.perf_counter()
            remd.run(a.steps)
            snap = remd.fetch()
            t_remd.append((time.perf_counter() - t0) / a.steps * 1e3)
            t0 = time.perf_counter()
            plain.run(a.steps)
            psnap = plain.fetch()
            t_plain.append((time.perf_counter() - t0) / a.steps * 1e3)
        # (the host arm's last upload is not in its last snapshot: compare what both arms hold on the device)
        same = bool(torch.equal(host.md.x, remd.x) and torch.equal(host.md.v, remd.v) and torch.equal(host.md.sigma, remd.sigma)
                    and np.array_equal(host.rung, snap.rung))
        row = {"case": name, "atoms": int(len(z)), "replicas": REPLICAS, "interval": a.interval, "edges_at_start": first,
               "capacity": kw["capacity"], "host_loop_ms": ms(t_host), "device_remd_ms": ms(t_remd), "device_md_ms": ms(t_plain),
               "ratio_host_over_device": statistics.median(t_host) / statistics.median(t_remd),
               "exchange_cost_ms": statistics.median(t_remd) - statistics.median(t_plain),
               "steps_done": [int(hsnap.step), int(snap.step), int(psnap.step)],
               "halted": [bool(hsnap.halted), bool(snap.halted), bool(psnap.halted)],
               "attempts": snap.attempts.tolist(), "accepts": snap.accepts.tolist(), "host_loop_accepts": host.accepted,
               "arms_end_bit_equal": same}
        out["cases"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


def launches(a):
    """Device activity of two DeviceMD replays and of two DeviceREMD replays (an attempt in each: interval 1) on the same
    batch of 5 x 32 atoms: the kernels by name and count, and every memcpy / memset the profiler saw."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device("cuda:0")
    model = model_for(dev)
    temps = 600.0 * 1.08 ** np.arange(5)
    pos, cell, z, m, batch, v = replicas((2, 2, 2), temps)
    z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
    kw = dict(batch=torch.from_numpy(batch).to(dev), num_graphs=5, seed=SEED, velocities=v)
    plain_md = DeviceMD(model, z_t, cell_t, pos, m, DT, temperature=temps, friction=FRICTION, **kw)
    ladder = DeviceREMD(model, z_t, cell_t, pos, m, DT, temps, FRICTION, 1, **kw)
    plain_md.run(4)
    ladder.run(4)
    torch.cuda.synchronize()

    def device_events(fn):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return Counter(ev.name for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)

    plain = device_events(lambda: plain_md.run(2))
    ours = device_events(lambda: ladder.run(2))
    lines = ["device activity of 2 replays, batch of 5 x 32 atoms: DeviceMD.run(2) | DeviceREMD.run(2), interval 1    (count name)"]
    for name in sorted(set(plain) | set(ours)):
        lines.append("%4d %4d  %s" % (plain.get(name, 0), ours.get(name, 0), name[:150]))
    extra = {k[:100]: c - plain.get(k, 0) for k, c in ours.items() if c != plain.get(k, 0)}
    extra.update({k[:100]: -c for k, c in plain.items() if k not in ours})
    copies = {k: c for k, c in ours.items() if "memcpy" in k.lower() or "memset" in k.lower()}
    lines.append("kernels: DeviceMD %d, DeviceREMD %d; difference: %s" % (sum(plain.values()), sum(ours.values()), extra))
    lines.append("memcpy / memset activities inside DeviceREMD.run(2): %d %s" % (sum(copies.values()), copies))
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
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--margin", type=float, default=0.25, help="columns of the padded list beyond the first count")
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("remd_bench: needs the GPU (nothing is measured without one)")
    launches(a) if a.launches else bench(a)
