"""Both resident drivers for a few replays (DeviceMD: 108 atoms, Langevin; DeviceRelax: a batch of 3 x 32 atoms), for a
launch list by kernel name and count:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/resident_launch_probe.py [TREE]

TREE: the checkout to import hermnet_amd and the bench tools' set-up from (default: this one)."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import resident_bench as rb  # noqa: E402
from hermnet_amd.md import DeviceMD  # noqa: E402
from hermnet_amd.relax import DeviceRelax  # noqa: E402

dev = torch.device("cuda:0")
model = rb.model_for(dev)
pos, cell, z, m, v = rb.setup((3, 3, 3), 300.0)
md = DeviceMD(model, torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev), pos, m, 0.5, velocities=v,
              friction=0.01, temperature=300.0)
md.run(5)
s = md.fetch()
print("md", ROOT, s.step, s.halted, float(s.log[-1, 0, 0]), float(s.log[-1, 0, 1]))
pos, cell, z, batch = rb.structures([(2, 2, 2)] * 3, 0.05)
rx = DeviceRelax(model, torch.from_numpy(z).to(dev), torch.from_numpy(cell.astype(np.float32)).to(dev), pos,
                 batch=torch.from_numpy(batch).to(dev), num_graphs=3, fmax=1e-6)
rx.run(5)
s = rx.fetch()
print("relax", ROOT, s.step, s.halted, s.energy.tolist(), s.fmax.tolist())
