"""What the resident drivers' GPU tests (tests/test_*_device.py) share: the H = 128, L = 3 model, built once per session, the
stand-in for an ase.Atoms, and the two small conversions.  The names keep their underscore: the test files import them as
they used to define them."""
import numpy as np
import torch

import hermnet_amd as hn
from hermnet_amd import synth

MASS = {13: 26.9815, 28: 58.6934, 29: 63.546}
_CACHE = {}


def _dev():
    return torch.device("cuda:0")


def _model(seed=8):
    """The model of test_md_step_with_list_rebuild_replays_as_one_graph."""
    model = hn.HVNet(["Al", "Ni", "Cu"], rc=5.0, num_layers=3, hidden_channels=128, num_rbf=64).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed))
    model = model.to(_dev())
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def _shared_model():
    if "model" not in _CACHE:
        _CACHE["model"] = _model()
    return _CACHE["model"]


class _FakeAtoms(object):
    """What `from_atoms` / `to_atoms` touch of an ase.Atoms."""

    def __init__(self, positions, numbers, cell, masses, velocities):
        self.positions, self.numbers, self.cell, self.pbc = positions.copy(), numbers, cell, np.array([True, True, True])
        self._m, self._v = masses, velocities

    def get_masses(self):
        return self._m

    def get_velocities(self):
        return self._v

    def set_velocities(self, v):
        self._v = np.array(v)


def _put(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _flat(entry):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in vars(entry).items()}
