"""CPU only: the resident drivers' bench harness (tools/resident_bench.py) and the eleven tools on it.  The samples are pinned
by sha256 digests recorded from the tools as they stood BEFORE the harness (each tool's own builder, run at the parent
commit), the launch list and the timing protocol by outputs written out here, the command lines by the option strings the
parent's tools printed.  Nothing touches a device."""
import hashlib
import importlib
import os
import re
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")


@pytest.fixture
def tool(monkeypatch):
    """`tool("nhc_bench")`: that module of tools/, imported the way the tools import the harness."""
    monkeypatch.syspath_prepend(TOOLS)
    return importlib.import_module


def digest(arrays):
    """sha256 prefix over the C-contiguous bytes of the arrays in order (a None, as relax's batch of one structure, adds nothing)."""
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def _npt(t, reps, copies):
    s = t("npt_bench").system(reps, copies, 300.0)
    return [s[k] for k in ("pos", "cell", "z", "m", "v", "batch")]


def _ring(t, reps, beads):
    x, cells, z, m, batch, v = t("pimd_bench").ring(reps, beads)
    return x, cells[0], cells, z, m, batch, v                   # the parent's ring() handed the one cell out too


def _ladder(n):
    return 600.0 * 1.08 ** np.arange(n)


R2, R3, R67, BIG = (2, 2, 2), (3, 3, 3), (6, 6, 7), (10, 10, 25)
RB = "resident_bench"
# (what the parent called, its digest, the same sample from today's code)
SAMPLES = [
    ("md_device_bench.setup((2,2,2), None, 300)", "23f4a1fcb058766b", lambda t: t(RB).setup(R2, 300.0)),
    ("md_device_bench.setup((3,3,3), None, 300)", "d87c0abb627d676a", lambda t: t(RB).setup(R3, 300.0)),
    ("md_device_bench.setup((6,6,7), None, 300)", "f170c2754e0cc4e5", lambda t: t(RB).setup(R67, 300.0)),
    ("md_device_bench.setup((10,10,25), None, 300)", "f5e75c990f638b71", lambda t: t(RB).setup(BIG, 300.0)),
    ("relax_bench.setup([(3,3,3)], 0.05)", "0c2498d9fef9b57b", lambda t: t(RB).structures([R3], 0.05)),
    ("relax_bench.setup([(6,6,7)], 0.05)", "f8ddf10348537c9b", lambda t: t(RB).structures([R67], 0.05)),
    ("relax_bench.setup([(2,2,2)] * 64, 0.05)", "250ab58d3ec7e4e1", lambda t: t(RB).structures([R2] * 64, 0.05)),
    ("relax_bench.setup([(2,2,2)] * 3, 0.05)", "8480f1cfd65b48d8", lambda t: t(RB).structures([R2] * 3, 0.05)),
    ("cellrelax_bench.strained([(3,3,3)], 0.05)", "3db93ff2df827ee6", lambda t: t("cellrelax_bench").strained([R3], 0.05)),
    ("cellrelax_bench.strained([(6,6,7)], 0.05)", "b992606b711dbc0b", lambda t: t("cellrelax_bench").strained([R67], 0.05)),
    ("cellrelax_bench.strained([(2,2,2)] * 64, 0.05)", "44d63d55d0137d3a", lambda t: t("cellrelax_bench").strained([R2] * 64, 0.05)),
    ("cellrelax_bench.strained([(2,2,2)] * 3, 0.05)", "e750b06f207d0e20", lambda t: t("cellrelax_bench").strained([R2] * 3, 0.05)),
    ("npt_bench.system((3,3,3), 1, None, 300)", "d87c0abb627d676a", lambda t: _npt(t, R3, 1)),
    ("npt_bench.system((6,6,7), 1, None, 300)", "f170c2754e0cc4e5", lambda t: _npt(t, R67, 1)),
    ("npt_bench.system((2,2,2), 64, None, 300)", "a7fc5a6aed43ab5f", lambda t: _npt(t, R2, 64)),
    ("observe_bench.system([(3,3,3)], 300)", "914d10bbf7110d0c", lambda t: t(RB).cells([R3], 300.0)),
    ("observe_bench.system([(6,6,7)], 300)", "b8d42ef20f48be84", lambda t: t(RB).cells([R67], 300.0)),
    ("observe_bench.system([(2,2,2)] * 64, 300)", "3cd9384273ff44c2", lambda t: t(RB).cells([R2] * 64, 300.0)),
    ("observe_bench.system([(10,10,25)], 300)", "a4d7b5e9e3158650", lambda t: t(RB).cells([BIG], 300.0)),
    ("nhc_bench.members(1, (3,3,3))", "f19fa4fb7ba64de6", lambda t: t(RB).cells([R3], 600.0)),
    ("nhc_bench.members(1, (6,6,7)) = swapmc_bench's", "8441904fb937b101", lambda t: t(RB).cells([R67], 600.0)),
    ("nhc_bench.members(2, (2,2,2)) = swapmc_bench's", "3004e55ce056cd07", lambda t: t(RB).cells([R2] * 2, 600.0)),
    ("nhc_bench.members(5, (2,2,2)) = swapmc_bench's", "e1e117fdc6173859", lambda t: t(RB).cells([R2] * 5, 600.0)),
    ("nhc_bench.members(64, (2,2,2))", "7f302091a511a049", lambda t: t(RB).cells([R2] * 64, 600.0)),
    ("swapmc_bench.members(8, (2,2,2))", "4c8ab3535dfe9d4d", lambda t: t(RB).cells([R2] * 8, 600.0)),
    ("swapmc_bench.members(8, (3,3,3))", "141bf6d74367c5c0", lambda t: t(RB).cells([R3] * 8, 600.0)),
    ("remd_bench.replicas((2,2,2), 600 * 1.08 ** arange(3))", "9348f1d048501de5", lambda t: t(RB).copies(R2, _ladder(3))),
    ("remd_bench.replicas((2,2,2), 600 * 1.08 ** arange(5))", "531d9fd5e9bf9f92", lambda t: t(RB).copies(R2, _ladder(5))),
    ("remd_bench.replicas((2,2,2), 600 * 1.08 ** arange(8))", "85dff5afdd33e292", lambda t: t(RB).copies(R2, _ladder(8))),
    ("remd_bench.replicas((3,3,3), 600 * 1.08 ** arange(8))", "9d24a14928c7b199", lambda t: t(RB).copies(R3, _ladder(8))),
    ("metad_bench.walkers((2,2,2))", "b176386b032dc258", lambda t: t(RB).copies(R2, [600.0] * 8)),
    ("metad_bench.walkers((3,3,3))", "103aee5f1229f129", lambda t: t(RB).copies(R3, [600.0] * 8)),
    ("pimd_bench.ring((2,2,2), 5)", "d08d0c5d7aa50d85", lambda t: _ring(t, R2, 5)),
    ("pimd_bench.ring((2,2,2), 8)", "b0a17202dc1f8294", lambda t: _ring(t, R2, 8)),
    ("pimd_bench.ring((3,3,3), 8)", "cfbdf04cb06b375c", lambda t: _ring(t, R3, 8)),
    ("neb_bench.band((2,2,2), 0.08, images=5)", "e30091cdc30f02f2", lambda t: t("neb_bench").band(R2, 0.08, images=5)),
    ("neb_bench.band((2,2,2), 0.08)", "0150689d5d7f3b64", lambda t: t("neb_bench").band(R2, 0.08)),
    ("neb_bench.band((3,3,3), 0.08)", "22d5e87eac0293cb", lambda t: t("neb_bench").band(R3, 0.08)),
]


@pytest.mark.parametrize("parent_call, parent_digest, build", SAMPLES, ids=[s[0] for s in SAMPLES])
def test_samples_are_bit_equal_to_the_parents(tool, parent_call, parent_digest, build):
    assert digest(build(tool)) == parent_digest


LONG = "k" + "x" * 160
TITLE = "device activity of 2 replays, a batch: Plain.run(2) | Ours.run(2)"
TABLE = """device activity of 2 replays, a batch: Plain.run(2) | Ours.run(2)    (count name)
   1    2  Memcpy DtoD (Device -> Device)
   2    2  both_kernel
   0    1  k%s
   3    0  left_only_kernel
   0    4  right_only
kernels: Plain 6, Ours 9; difference: {'right_only': 4, 'k%s': 1, 'Memcpy DtoD (Device -> Device)': 1, 'left_only_kernel': -3}
memcpy / memset activities inside Ours.run(2): 2 {'Memcpy DtoD (Device -> Device)': 2}
""" % ("x" * 149, "x" * 99)
EMPTY = """device activity of 2 replays, a batch: Plain.run(2) | Ours.run(2)    (count name)
   1    0  Memcpy DtoD (Device -> Device)
   2    0  both_kernel
kernels: Plain 3, Ours 0; difference: {'both_kernel': -2, 'Memcpy DtoD (Device -> Device)': -1}
memcpy / memset activities inside the right run(2): 0 {}
(the profiler recorded no device activity for graph launches)
"""


def test_launch_table(tool, tmp_path, capsys):
    """A kernel in both lists, one on either side alone (the left one negative in the difference), a name cut at 150 in its row
    and at 100 in the summary, a memcpy, and an empty right list."""
    rb = tool(RB)
    plain = Counter({"both_kernel": 2, "left_only_kernel": 3, "Memcpy DtoD (Device -> Device)": 1})
    ours = Counter({"both_kernel": 2, "right_only": 4, LONG: 1, "Memcpy DtoD (Device -> Device)": 2})
    path = tmp_path / "launches.txt"
    text = rb.launch_table(TITLE, "Plain", lambda: plain, "Ours", lambda: ours, str(path), events=lambda fn: fn())
    assert text == TABLE
    assert path.read_text() == TABLE
    assert capsys.readouterr().out == TABLE + "\n"
    few = Counter({"both_kernel": 2, "Memcpy DtoD (Device -> Device)": 1})
    text = rb.launch_table(TITLE, "Plain", lambda: few, "Ours", Counter, str(path), inside="the right run(2)", events=lambda fn: fn())
    assert text == EMPTY
    assert path.read_text() == EMPTY


def _clock():
    """A clock that steps 0, 1, 3, 6, 10, ...: the k-th timed window (from 0) lasts 2 k + 1."""
    ticks = iter(k * (k + 1) // 2 for k in range(1000))
    return lambda: float(next(ticks))


def test_time_arms(tool):
    rb = tool(RB)
    calls = []

    def arm(key):
        def fn(steps):
            calls.append((key, steps))
            return key, len(calls)
        return fn

    times, last = rb.time_arms([("a", 2, arm("a")), ("b", 5, arm("b")), ("c", 10, arm("c"))], 2, sync=lambda: calls.append("sync"),
                               clock=_clock())
    assert calls == ["sync", ("a", 2), ("b", 5), ("c", 10), "sync", ("a", 2), ("b", 5), ("c", 10)]
    assert times == {"a": [1 / 2 * 1e3, 7 / 2 * 1e3], "b": [3 / 5 * 1e3, 9 / 5 * 1e3], "c": [5 / 10 * 1e3, 11 / 10 * 1e3]}
    assert last == {"a": ("a", 6), "b": ("b", 7), "c": ("c", 8)}


def test_time_arms_options(tool):
    """`sync=True`: the harness's own `sync` ends the window, inside the timing.  `before` runs untimed ahead of its arm's window,
    and what it returns (False here) decides nothing.  `rounds` alone says in which rounds an arm takes part."""
    rb = tool(RB)
    calls, clock = [], _clock()

    def timed_sync():
        calls.append("sync")
        clock()                                       # (a tick of its own: a sync inside a window lengthens that window)

    arms = [("a", 1, lambda n: calls.append("a")),
            ("b", 4, lambda n: calls.append("b"), dict(sync=True, before=lambda r: calls.append("ahead of b") or False)),
            ("c", 1, lambda n: calls.append("c") or "seen", dict(rounds=lambda r: r == 0))]
    times, last = rb.time_arms(arms, 2, sync=timed_sync, clock=clock)
    assert calls == ["sync", "a", "ahead of b", "b", "sync", "c", "sync", "a", "ahead of b", "b", "sync"]
    # ticks: round 0: sync 0 | a 1..3 | b 6 (its sync 10) ..15 | c 21..28; round 1: sync 36 | a 45..55 | b 66 (78) ..91
    assert times == {"a": [2e3, 10e3], "b": [9 / 4 * 1e3, 25 / 4 * 1e3], "c": [7e3]}
    assert last == {"a": None, "b": None, "c": "seen"}


COMMON = ["--help", "--margin", "--out", "--rounds"]
OPTIONS = {                                                     # as the parent's tools printed them, sorted
    "md_device_bench": COMMON + ["--launches", "--dt", "--steps", "--temp"],
    "npt_bench": COMMON + ["--launches", "--compressibility", "--dt", "--pressure", "--steps", "--taup", "--temp"],
    "relax_bench": COMMON + ["--sigma", "--steps"],
    "cellrelax_bench": COMMON + ["--launches", "--sigma", "--steps"],
    "neb_bench": COMMON + ["--launches", "--sigma", "--steps"],
    "remd_bench": COMMON + ["--launches", "--interval", "--steps"],
    "pimd_bench": COMMON + ["--launches", "--check", "--steps"],
    "observe_bench": COMMON + ["--launches", "--big-steps", "--dt", "--only", "--parent", "--plain-only", "--steps", "--temp"],
    "metad_bench": COMMON + ["--launches", "--host-steps", "--steps"],
    "swapmc_bench": COMMON + ["--launches", "--interval", "--replays", "--swaps"],
    "nhc_bench": COMMON + ["--launches", "--steps"],
}


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_command_line(name):
    """--help exits 0 with the parent's option strings; without a GPU the tool exits 1 and says what it needs."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # on any machine
    cmd = [sys.executable, os.path.join(TOOLS, name + ".py")]
    asked = subprocess.Popen(cmd + ["--help"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    bare = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out, err = asked.communicate(timeout=120)
    assert asked.returncode == 0, err
    assert sorted(set(re.findall(r"(?<![\w-])--[a-z][a-z-]*", out))) == sorted(OPTIONS[name])
    out, err = bare.communicate(timeout=120)
    assert bare.returncode == 1, (out, err)
    assert err.strip().splitlines()[-1] == "%s: needs the GPU (nothing is measured without one)" % name
