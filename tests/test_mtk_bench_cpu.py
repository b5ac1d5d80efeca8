"""CPU: the command line of tools/mtk_bench.py (the harness is tests/test_resident_bench_cpu.py's subject)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = ["--help", "--margin", "--out", "--rounds", "--launches", "--steps"]


def test_command_line():
    """--help exits 0 with the family's option strings; without a GPU the tool exits 1 with the family's message."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # on any machine
    cmd = [sys.executable, os.path.join(ROOT, "tools", "mtk_bench.py")]
    asked = subprocess.Popen(cmd + ["--help"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    bare = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out, err = asked.communicate(timeout=120)
    assert asked.returncode == 0, err
    assert sorted(set(re.findall(r"(?<![\w-])--[a-z][a-z-]*", out))) == sorted(OPTIONS)
    out, err = bare.communicate(timeout=120)
    assert bare.returncode == 1, (out, err)
    assert err.strip().splitlines()[-1] == "mtk_bench: needs the GPU (nothing is measured without one)"
