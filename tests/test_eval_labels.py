"""GPU: the timer labels of one energy + force evaluation, in launch order, against tests/golden/eval_launch_labels.json.

The fixture was recorded with `eval_labels` below on the hand-written call sites of the evaluation path (a closure per launch, the
C name typed twice) before they moved onto `ops._call`: a label that changes, a launch that leaves the labelled path or joins
it, or another order shows here.  bench.py counts and times launches by these labels.  (The training step's labels:
tests/test_training_routes.py.)  Recording again, from the repository root: PYTHONPATH=. python tests/test_eval_labels.py"""
import json
import os

import pytest
import torch

from helpers import GOLDEN, Golden

FIXTURE = os.path.join(GOLDEN, "eval_launch_labels.json")
CASES = ["mol16", "alloy108_unknown_type"]


class _Labels(object):
    """ops.set_kernel_timer hook that records the label of every library launch."""

    def __init__(self):
        self.names = []

    def launch(self, name, fn):
        self.names.append(name)
        return fn()


def eval_labels(name):
    """The ordered labels of model(d) and autograd.grad(E, pos) on fixture `name`: H = 128, boundary_mode 0, defaults otherwise."""
    from hermnet_amd import ops, switches
    dev = torch.device("cuda:0")
    g = Golden(name)
    assert g.model_kw["hidden_channels"] == 128
    old, switches.boundary_mode = switches.boundary_mode, 0
    rec = _Labels()
    try:
        model = g.model().to(dev)
        d = g.data().to(dev)
        d.pos.requires_grad_(True)
        ops.set_kernel_timer(rec)
        e = model(d)
        f = -torch.autograd.grad(e.sum(), d.pos)[0]
    finally:
        ops.set_kernel_timer(None)
        switches.boundary_mode = old
    torch.cuda.synchronize()
    assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(f).all())
    return rec.names


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_evaluation_launch_labels_in_order(name):
    with open(FIXTURE) as fh:
        want = json.load(fh)[name]
    got = eval_labels(name)
    assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:5] + [len(got), len(want)]
    assert any(n.startswith("message_scatter_fwd") for n in got) and any(n.startswith("message_scatter_bwd") for n in got)
    assert "edge_radial_table" in got


if __name__ == "__main__":
    with open(FIXTURE, "w") as fh:
        json.dump({name: eval_labels(name) for name in CASES}, fh, indent=1)
        fh.write("\n")
