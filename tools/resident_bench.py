"""What the resident drivers' bench tools (md_device, npt, relax, cellrelax, neb, remd, pimd, observe, metad, swapmc, nhc
`_bench.py`) share: the model, the samples, the device preparation, the timing protocol, the launch list and the command
line.  Imported by those tools, never run; the only module under tools/ that another tool imports.

A tool keeps its docstring, constants and cases, its host-loop arm, a `bench(a)` that declares arms for `time_arms` and
returns the record, and a `launches(a)` that builds two drivers for `launch_table`; `main` does the rest."""
import argparse
import json
import os
import statistics
import sys
import time
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import hermnet_amd as hn  # noqa: E402
from hermnet_amd import synth  # noqa: E402
from hermnet_amd.md import AMU_A2_FS2_TO_EV, KB  # noqa: E402
from hermnet_amd.neighbor import neighbor_search, padded_capacity  # noqa: E402

MASS = {13: 26.9815, 28: 58.6934, 29: 63.546}
FMAX = 1e-6                 # the relaxations' (relax, cellrelax, neb) convergence bound: out of reach, every evaluation moves
RELAX_CASES = [("108 atoms", [(3, 3, 3)]), ("1008 atoms", [(6, 6, 7)]), ("64 x 32 atoms", [(2, 2, 2)] * 64)]   # relax, cellrelax


def model_for(dev):
    """The model of BASELINE configs[1], synthetic weights, on `dev`."""
    model = hn.HVNet(["Al", "Ni", "Cu"], rc=5.0, num_layers=5, hidden_channels=128, num_rbf=128).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
    model = model.to(dev)
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def ms(ts):
    return [statistics.median(ts), min(ts), max(ts)]


def maxwell(rs, m, temperature):
    """Maxwell-Boltzmann velocities drawn from `rs`; `temperature` a number or one per atom."""
    return rs.normal(size=(len(m), 3)) * np.sqrt(KB * temperature / (m * AMU_A2_FS2_TO_EV))[:, None]


def setup(reps, temp, seed=0):
    """(pos, cell [3,3], z, masses, velocities) of one rattled cell."""
    pos, cell, z = synth.fcc_alloy_atoms(reps=reps, seed=seed)
    m = np.array([MASS[int(v)] for v in z])
    return pos, cell, z, m, maxwell(np.random.RandomState(seed + 1), m, temp)


def cells(members, temp=None, sigma=0.05):
    """(pos, cell [B,3,3], z, masses, batch, velocities) of B DIFFERENT cells, graph g of `members[g]` repeats rattled with
    seed g; velocities at `temp` from one stream over all atoms, or None."""
    parts = [synth.fcc_alloy_atoms(reps=r, seed=s, sigma=sigma) for s, r in enumerate(members)]
    pos, z = np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts])
    m = np.array([MASS[int(v)] for v in z])
    v = None if temp is None else maxwell(np.random.RandomState(1), m, temp)
    return pos, np.stack([p[1] for p in parts]), z, m, np.repeat(np.arange(len(parts)), [len(p[0]) for p in parts]), v


def structures(members, sigma):
    """(pos, cell, z, batch) of `cells` as the relaxations take them: one structure comes with its [3,3] cell and no batch."""
    pos, cell, z, _, batch, _ = cells(members, sigma=sigma)
    return (pos, cell[0], z, None) if len(members) == 1 else (pos, cell, z, batch)


def copies(reps, temperatures, spread=0.0):
    """(pos, cell [R,3,3], z, masses, batch, velocities) of R copies of ONE rattled cell, copy r's velocities at
    `temperatures[r]`; `spread`: the copies' atoms scattered by that much (A) around their place."""
    R = len(temperatures)
    pos, cell, z = synth.fcc_alloy_atoms(reps=reps)
    rs = np.random.RandomState(1)
    m = np.tile(np.array([MASS[int(v)] for v in z]), R)
    x = np.tile(pos, (R, 1))
    if spread:
        x = x + rs.normal(scale=spread, size=x.shape)
    return x, np.tile(cell, (R, 1, 1)), np.tile(z, R), m, np.repeat(np.arange(R), len(z)), maxwell(rs, m, np.repeat(temperatures, len(z)))


def on_device(dev, pos, cell, z, batch=None, margin=0.25):
    """(z_t, cell_t, p0, kw, edges_at_start, capacity) of a sample: its tensors, the drivers' `batch=, num_graphs=` (nothing
    for one structure without a batch), the columns of the first list and the padded count every arm is given."""
    z_t, cell_t = torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev)
    p0 = torch.from_numpy(pos.astype(np.float32)).to(dev)
    kw = {} if batch is None else dict(batch=torch.from_numpy(batch).to(dev), num_graphs=len(cell))
    first = int(neighbor_search(p0, 5.0, cell_t, **kw)[0].size(1))
    return z_t, cell_t, p0, kw, first, padded_capacity(first, margin=margin)


def time_arms(arms, rounds, sync=None, clock=time.perf_counter):
    """The family's timing protocol.  `arms`: ordered (key, steps, fn[, options]); `fn(steps)` runs one window and returns what
    the row needs.  A window ENDS in a synchronisation: a device arm's `fetch()` (`fetched`), a host arm's own last `fetch()`,
    or `sync()`, called here inside the window for an arm with `sync=True`.  Per round: one `sync()`, then every arm in the
    declared order, `clock()` around it, divided by its own `steps`.  The options, a dict:
        sync=True      the window ends in `sync()`
        before=f       `f(round)` runs untimed ahead of the arm's window (whatever it returns)
        rounds=p       the arm takes part in the rounds where `p(round)` holds
    -> ({key: [ms per step, one per round it took part in]}, {key: fn's last return value})"""
    sync = sync or torch.cuda.synchronize
    times, last = {arm[0]: [] for arm in arms}, {arm[0]: None for arm in arms}
    for r in range(rounds):
        sync()
        for key, steps, fn, *options in arms:
            opt = options[0] if options else {}
            if "rounds" in opt and not opt["rounds"](r):
                continue
            if "before" in opt:
                opt["before"](r)
            t0 = clock()
            last[key] = fn(steps)
            if opt.get("sync"):
                sync()
            times[key].append((clock() - t0) / steps * 1e3)
    return times, last


def fetched(driver):
    """A device arm's `fn`: run(n), then the `fetch()` that ends the window; returns the snapshot."""
    def fn(n):
        driver.run(n)
        return driver.fetch()
    return fn


def device_events(fn):
    """The device activities of `fn()`, as the profiler saw them."""
    from torch import profiler
    with profiler.profile(activities=[profiler.ProfilerActivity.CPU, profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]


def launch_table(title, left_name, left_fn, right_name, right_fn, path, inside=None,
                 events=lambda fn: Counter(ev.name for ev in device_events(fn))):
    """The device activity of `left_fn()` (the plain driver's replays) beside `right_fn()`'s (ours) by name and count, the
    difference, and every memcpy / memset inside ours; printed and written to `path`.  Both drivers come warmed up."""
    plain, ours = events(left_fn), events(right_fn)
    lines = ["%s    (count name)" % title]
    for name in sorted(set(plain) | set(ours)):
        lines.append("%4d %4d  %s" % (plain.get(name, 0), ours.get(name, 0), name[:150]))
    extra = {k[:100]: c - plain.get(k, 0) for k, c in ours.items() if c != plain.get(k, 0)}
    extra.update({k[:100]: -c for k, c in plain.items() if k not in ours})
    copies = {k: c for k, c in ours.items() if "memcpy" in k.lower() or "memset" in k.lower()}
    lines.append("kernels: %s %d, %s %d; difference: %s" % (left_name, sum(plain.values()), right_name, sum(ours.values()), extra))
    lines.append("memcpy / memset activities inside %s: %d %s" % (inside or right_name + ".run(2)", sum(copies.values()), copies))
    if not ours:
        lines.append("(the profiler recorded no device activity for graph launches)")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "w") as fh:
        fh.write(text)
    return text


def main(name, bench, launches=None, flags=()):
    """The tools' command line: `flags` ((option, add_argument's keywords) of the tool's own), then the family's; `bench(a)`
    returns the record that --out takes."""
    ap = argparse.ArgumentParser()
    for flag, kw in flags:
        ap.add_argument(flag, **kw)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--margin", type=float, default=0.25, help="columns of the padded list beyond the first count")
    ap.add_argument("--out", default=None)
    if launches:
        ap.add_argument("--launches", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("%s: needs the GPU (nothing is measured without one)" % name)
    if launches and a.launches:
        return launches(a)
    out = bench(a)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
