"""tests/golden/message_scatter_host.npz: one call of trainops.message_scatter_generic on host tensors (float64, the torch route:
per-relation TallLinear, GatherRows, the torch message algebra, SumRows, the residual), with and without vec -- inputs and
results, recorded once at the commit before the row keys became declared objects (tests/test_host_logic.py compares to the
last bit).

12 atoms of three elements, one of them without atoms, 3 atoms of an element the model does not know, H = 8, 6 radial
functions.  Every row of the basis holds ONE nonzero entry, a power of two: the projection's sums then have one term that is
exact, so the recorded bits do not depend on the order in which a BLAS adds.

    python tests/golden/gen_message_scatter_host.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from hermnet_amd import trainops                              # noqa: E402
from hermnet_amd.relations import RelationalGraph             # noqa: E402

Z_LIST, H, RADIAL = [13, 28, 29], 8, 6


def inputs():
    gen = torch.Generator().manual_seed(2024)
    z = torch.tensor([13] * 5 + [29] * 4 + [1] * 3)[torch.randperm(12, generator=gen)]
    src, tgt = torch.randint(0, 12, (2, 60), generator=gen)
    keep = src != tgt
    edge_index = torch.stack([src[keep], tgt[keep]])
    g = RelationalGraph.build(z, edge_index, Z_LIST)
    T, N, E = g.T, g.N, g.E
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    emb = torch.zeros(E, RADIAL, dtype=torch.float64)
    emb[torch.arange(E), torch.randint(0, RADIAL, (E,), generator=gen)] = 2.0 ** torch.randint(-2, 3, (E,), generator=gen).double()
    edge = torch.cat([torch.nn.functional.normalize(rnd(E, 3), dim=1), 1.0 + rnd(E, 1).abs()], dim=1)
    return dict(z=z, edge_index=edge_index, xh=rnd(T, N, 3 * H), vec=rnd(N, 3, H), x=rnd(N, H), edge=edge, edge_embed=emb,
                w_rbf=rnd(T, 3 * H, RADIAL), b_rbf=rnd(T, 3 * H))


def run(t, with_vec):
    g = RelationalGraph.build(t["z"], t["edge_index"], Z_LIST)
    return trainops.message_scatter_generic(t["xh"], t["vec"] if with_vec else None, t["x"], t["edge"], t["edge_embed"],
                                            list(t["w_rbf"]), list(t["b_rbf"]), g)


if __name__ == "__main__":
    t = inputs()
    out = {k: v.numpy() for k, v in t.items()}
    for with_vec in (False, True):
        x1, vec1 = run(t, with_vec)
        out["x1_vec%d" % with_vec], out["vec1_vec%d" % with_vec] = x1.numpy(), vec1.numpy()
    np.savez(os.path.join(HERE, "message_scatter_host.npz"), **out)
    print({k: v.shape for k, v in out.items()})
