"""CPU: the gedge-only backward message kernels (csrc/message_bwd_cl.hip: message_edge_bwd_cl_kernel, NEED_GXH = false) keep
their register budget, on the code hipcc generates for gfx950 with the library's flags for the unit -- no GPU.

They are launched with 1024 threads, 16 waves, four per SIMD: that needs at most 128 VGPRs, and scratch would put spilled
registers into the per-edge loop.  Found when this test was written (the compiler's kernel-resource-usage remarks): 87 VGPRs for
the whole-tile instance and 89 for the one over tap-row windows, no scratch, no spills (89 and 90 before part s of the tap
contraction became a scalar sum there)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gedge_only_backward_kernels_fit_their_register_budget():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "hermnet_amd", "csrc", "message_bwd_cl.hip")
    run = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                         check=True, capture_output=True, timeout=600)
    blocks = re.findall(r"remark: Function Name: (\S*message_edge_bwd_cl_kernel\S*)(.*?)LDS Size", run.stderr.decode(), flags=re.S)
    found = {}
    for name, body in blocks:
        get = lambda key: int(re.search(r"remark:\s+%s: (\d+)" % re.escape(key), body).group(1))
        found[name] = (get("VGPRs"), get("ScratchSize [bytes/lane]"), get("VGPRs Spill"), get("SGPRs Spill"))
        print(name, found[name])
    assert len(found) == 2 and sorted("ILb1E" in n for n in found) == [False, True]      # whole tile, tap-row windows
    for name, (vgprs, scratch, vspill, sspill) in found.items():
        assert vgprs <= 128, (name, vgprs)                       # 4 waves per SIMD at 1024 threads
        assert scratch == 0 and vspill == 0, (name, scratch, vspill)
        if "ILb0E" in name:                                      # the whole-tile instance: what every default-sized model runs
            assert sspill == 0, (name, sspill)
