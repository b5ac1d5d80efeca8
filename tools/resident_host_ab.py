"""CPU only: the host twins of the resident drivers (hermnet_host_md_advance / _finish, hermnet_host_relax_advance /
_finish) of TWO builds of the library, driven side by side over random cases, every output array compared as raw bytes.

    python tools/resident_host_ab.py OLD/libhermnet_hip.so NEW/libhermnet_hip.so [--cases 300] [--seed 0]

A case is a multi-step sequence: one graph of 0, 1, 256, 257, 513 or a random number of atoms, or three graphs with the
middle one empty; `batch` entries out of range; the wrap on (a triclinic and an orthogonal cell) or off; NVE or Langevin /
held atoms; a halt of a random cause at a random step, further calls behind it, the halt cleared (MD: primed) and the run
continued.  Prints one line per driver and exits 1 on any differing byte."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from hermnet_amd import _lib  # noqa: E402
from md_reference import HostMD  # noqa: E402
from relax_reference import HostRelax  # noqa: E402

TRICLINIC = np.array([[19.3, 0.4, -0.7], [2.1, 21.2, 0.3], [-1.6, 3.3, 24.9]])
ORTHO = np.diag([18.0, 19.0, 20.0])
MD_ARRAYS = ("x", "v", "x0", "v0", "image", "image0", "f_prev", "pos32", "ke_atom", "log", "state")
RELAX_ARRAYS = ("x", "v", "x0", "image", "image0", "f_prev", "pos32", "gf", "gi", "gf_new", "gi_new", "log", "state")


def open_library(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith(("hermnet_host_md_", "hermnet_host_relax_")):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def shape(rs):
    """(sizes of the graphs, cells or None, batch, the batch with entries out of range or None)."""
    if rs.rand() < 0.5:
        sizes = [int(rs.choice([0, 1, 256, 257, 513, rs.randint(2, 600)]))]
    else:
        sizes = [int(rs.randint(1, 300)), 0, int(rs.randint(1, 300))]
    B, n = len(sizes), sum(sizes)
    cells = np.stack([TRICLINIC, ORTHO, ORTHO][:B]) * rs.uniform(0.8, 1.2) if rs.rand() < 0.7 else None
    batch = np.repeat(np.arange(B), sizes)
    broken = None
    if n and rs.rand() < 0.5:
        broken = batch.copy()
        broken[0], broken[-1] = -int(rs.randint(1, 9)), B + int(rs.randint(0, 9))
    return sizes, cells, batch, broken


def bad_evaluation(rs, B):
    """(energy, total, capacity) of an evaluation that halts, one cause alone."""
    energy, why = rs.normal(size=B).astype(np.float32), rs.randint(4)
    if why == 0:
        return energy, (400, int(rs.choice([1, 2, 8, 16]))), 512
    if why == 1:
        return energy, (513, 0), 512
    energy[rs.randint(B)] = [np.nan, np.inf, -np.inf][rs.randint(3)]
    return energy, (400, 0), 512


def compare(pair, names, where):
    diff = 0
    for k in names:
        a, b = (np.ascontiguousarray(getattr(h, k)).view(np.uint8) for h in pair)
        d = int(np.count_nonzero(a != b)) if a.shape == b.shape else max(a.size, b.size)
        if d:
            print("DIFF %s: %s, %d bytes" % (where, k, d))
        diff += d
    return diff


def run_case(kind, libs, rs, case):
    sizes, cells, batch, broken = shape(rs)
    n, B = sum(sizes), len(sizes)
    box = ORTHO if cells is None else cells[0]
    x = rs.uniform(-1.0, 2.0, (n, 3)) @ box
    centre, stiff = rs.uniform(0.3, 0.7, (n, 3)) @ box, rs.uniform(0.2, 5.0, (n, 1))
    steps, halt_at = int(rs.randint(4, 16)), int(rs.randint(1, 16))
    if kind == "md":
        langevin = rs.rand() < 0.5
        m = rs.uniform(5.0, 80.0, n)
        m[rs.rand(n) < 0.05] = np.inf
        kw = dict(cell=cells, batch=batch, friction=0.03 if langevin else None, seed=int(rs.randint(1 << 30)), log_steps=5,
                  temperature=rs.uniform(100.0, 900.0, B) if langevin else None, num_graphs=B)
        v = rs.normal(scale=0.02, size=(n, 3))
        pair = [HostMD(x, v, m, 0.5, **kw) for _ in libs]
        names = MD_ARRAYS
    else:
        fixed = rs.rand(n) < 0.05 if rs.rand() < 0.5 else None
        kw = dict(cell=cells, batch=batch, num_graphs=B, fixed=fixed, fmax=rs.uniform(0.02, 0.5, B), log_steps=5)
        pair = [HostRelax(x, **kw) for _ in libs]
        names = RELAX_ARRAYS
    prime = kind == "md" and rs.rand() < 0.3                          # start with a prime evaluation
    for h, lib in zip(pair, libs):
        h.lib = lib
        if broken is not None:
            h.batch[:] = broken
        h.state[3] = int(prime)
    diff, calls = 0, 0
    for step in range(steps):
        good = (rs.normal(size=B).astype(np.float32), (int(rs.randint(0, 500)), 0), 512)
        energy, total, capacity = bad_evaluation(rs, B) if step == halt_at else good
        for h in pair:
            p = h.advance().astype(np.float64)
            h.finish((-stiff * (p - centre)).astype(np.float32), energy=energy, total=total, capacity=capacity)
        calls += 2
        diff += compare(pair, names, "%s case %d step %d" % (kind, case, step))
        if step == halt_at + 2:                                        # what resume() does
            for h in pair:
                h.state[1:3] = 0
                if kind == "md":
                    h.state[3] = 1
    return diff, calls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    libs = [open_library(args.old), open_library(args.new)]
    for which, lib in zip(("old", "new"), libs):
        lib.hermnet_build_info.restype = ctypes.c_char_p
        print("%s: %s" % (which, lib.hermnet_build_info().decode()))
    total = 0
    for kind in ("md", "relax"):
        rs = np.random.RandomState(args.seed)
        diff = calls = 0
        for case in range(args.cases):
            d, c = run_case(kind, libs, rs, case)
            diff, calls = diff + d, calls + c
        print("%s: %d cases, %d advance/finish calls per library, %d differing bytes" % (kind, args.cases, calls, diff))
        total += diff
    sys.exit(1 if total else 0)


if __name__ == "__main__":
    main()
