#!/usr/bin/env python3
"""The routes of the fused layer (hermnet_amd/layer.py):
    python tools/layer_routes.py launches CASE ...  per case "== CASE", then the kernel names of one warm energy+forces step in
                                                    launch order
    python tools/layer_routes.py eager64 [STEPS]    ms per eager step of the 64-atom cell (host-bound: ~0.8 ms, most of it Python)
CASE: default (configs[1]) | boundary1 .. boundary4 (switches.boundary_mode) | gemm (switches.node_chain = False) | w192 (padded
channels) | htnet | halo0, halo1, halo2 (one rank whose halo peer is itself over RCCL, HERMNET_HALO_OVERLAP = 0 / 1 / 2).
Two trees run the same launches when the outputs of `launches` are equal line by line."""
import json
import os
import sys
import tempfile
import time

import torch
from torch.profiler import ProfilerActivity, profile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hermnet_amd as hn  # noqa: E402
from hermnet_amd import switches, synth  # noqa: E402

dev = torch.device("cuda")


def make_step(case):
    width, reps, Model = 128, (10, 10, 25), hn.HVNet
    switches.boundary_mode, switches.node_chain = 0, True
    os.environ.pop("HERMNET_HALO_OVERLAP", None)
    if case.startswith("boundary"):
        switches.boundary_mode = int(case[len("boundary"):])
    elif case == "gemm":
        switches.node_chain = False
    elif case == "w192":
        width = 192
    elif case == "htnet":
        Model = hn.HTNet
    elif case == "eager64":
        reps = (2, 2, 4)
    elif case.startswith("halo"):
        os.environ["HERMNET_HALO_OVERLAP"] = case[len("halo"):]
    elif case != "default":
        raise SystemExit(__doc__)
    model = Model(["Al", "Ni", "Cu"], rc=5.0, num_layers=5, hidden_channels=width, num_rbf=128).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 10))
    model = model.to(dev)
    for p in model.parameters():
        p.requires_grad_(False)
    if case.startswith("halo"):        # as bench.py --self-peer 1: the production exchange with real rows on ONE GPU
        import numpy as np
        import torch.distributed as dist
        from hermnet_amd.sharding import SlabStepper
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29544")
        torch.cuda.set_device(0)
        if not dist.is_initialized():
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        pos, cell, z = synth.fcc_alloy_atoms(reps=reps, seed=0)
        stepper = SlabStepper(torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev), 5.0, 0, 1,
                              skin=1.0, group=dist.group.WORLD, deferred=True, self_peer=1)
        data, _plan = stepper(torch.from_numpy(pos.astype(np.float32)).to(dev))
    else:
        data = synth.fcc_alloy(reps=reps, seed=0, device=dev)

    def step():
        data.pos.requires_grad_(True)
        e = model(data)
        return e, -torch.autograd.grad(e.sum(), data.pos)[0]
    return step


def launches(case):
    print("== " + case, flush=True)
    step = make_step(case)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    # (ordered by the host call that launched them: the kernels of the exchange run on a stream of their own)
    with tempfile.TemporaryDirectory() as tmp:
        prof.export_chrome_trace(os.path.join(tmp, "trace.json"))
        with open(os.path.join(tmp, "trace.json")) as fh:
            events = [e for e in json.load(fh)["traceEvents"] if "correlation" in e.get("args", {})]
    on_device = lambda e: e.get("cat") == "kernel" or str(e.get("cat")).startswith("gpu_")       # (+ memcpy, memset)
    called = {e["args"]["correlation"]: e["ts"] for e in events if not on_device(e)}
    for _, _, name in sorted((called.get(e["args"]["correlation"], e["ts"]), e["ts"], e["name"]) for e in events if on_device(e)):
        print(name)
    sys.stdout.flush()


def eager64(steps):
    step = make_step("eager64")
    for _ in range(20):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    print("eager64 %.4f ms per step (%d steps)" % ((time.perf_counter() - t0) / steps * 1e3, steps))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "launches":
        for case in sys.argv[2:]:
            launches(case)
    elif len(sys.argv) > 1 and sys.argv[1] == "eager64":
        eager64(int(sys.argv[2]) if len(sys.argv) > 2 else 2000)
    else:
        raise SystemExit(__doc__)
