"""Energy, forces and stress from ONE forward and ONE force backward ("Stress").

    energy [B], forces [N,3]   exactly what `model(data)` and `-autograd.grad(E.sum(), pos)` give, bit for bit
    virial [B,3,3]             W_b = sum_{atoms i of b} W_i = -sum_{e in b} D_e (x) dE/dD_e, energy units, unsymmetrised
                               ([a,b] = D_a g_b): the ordered per-graph sums (hermnet_graph_virial) of the per-atom rows
                               that the position backward writes alongside the forces (hermnet_edge_geometry_bwd_virial)
    stress [B,3,3]             -sym(W_b) / V_b with V_b = |det cell_b| (ASE's sign: sigma = (1/V) dE/d(strain)); zeros for
                               graphs without a cell

`cell.requires_grad` is not needed and no second backward runs (the cell gradient of `utils.virial_calc` costs a second
pass through every layer).  Nothing here reads the host, so the call may be captured into a hipGraph (graph.GraphedStep /
GraphedMDStep with `stress=True`).

Refused (NotImplementedError): atom-sharded data, HTNet, train() / eval_param_grads (create_graph).
"""
import copy

import torch

from .ops import AtomSink


def stress_of_virial(virial, cell):
    """-sym(W_b) / |det cell_b| for W [B,3,3] and cell [B,3,3] (or [3,3] with B = 1); a singular / missing (all-zero) cell
    gives zeros.  Pure tensor algebra (any device, no host read)."""
    w = virial.reshape(-1, 3, 3)
    if cell is None:
        return torch.zeros_like(w)
    c = cell.detach().reshape(-1, 3, 3).to(w.dtype)
    vol = torch.linalg.det(c).abs()
    inv = torch.where(vol > 0, 1.0 / vol.clamp(min=torch.finfo(w.dtype).tiny), torch.zeros_like(vol))
    return -0.5 * (w + w.transpose(1, 2)) * inv[:, None, None]


def evaluate_with_sink(model, data, sink, pos=None):
    """One forward of `model` and ONE `autograd.grad(E.sum(), pos)` with `sink` (ops.AtomSink) travelling on the Data for this
    call only -> (d, pos, energy [B] detached, forces [N,3]).  `pos` None: the caller's `data` is not modified, the call runs
    on a shallow copy `d` whose `pos` is a leaf; else `data` is the caller's own copy and `pos` its leaf.  No host read."""
    d = data
    if pos is None:
        d, pos = copy.copy(data), data.pos
        if not (pos.requires_grad and pos.is_leaf):
            pos = d.pos = pos.detach().requires_grad_(True)
    d._hn_atom_props = sink
    try:
        with torch.enable_grad():
            energy = model(d)
            g = torch.autograd.grad(energy.sum(), pos, allow_unused=True)[0] if energy.requires_grad else None
    finally:
        d._hn_atom_props = None
    return d, pos, energy.detach(), (torch.zeros_like(pos) if g is None else -g).detach()


def energy_forces_virial(model, d, pos):
    """(energy [B] detached, forces [N,3], virial [B,3,3]) of `model` on `d`, whose `pos` is the leaf `pos` (None: any `d`, which
    is not modified).  (The body shared by `energy_forces_stress` and the captured steps.)"""
    sink = AtomSink(virials=False, graph_virial=True, energies=False)
    _, pos, energy, forces = evaluate_with_sink(model, d, sink, pos)
    virial = sink.graph_virial
    if virial is None:           # (no gradient reached the edge geometry -- e.g. no edge at all: the virial is zero)
        virial = torch.zeros(energy.numel(), 3, 3, dtype=pos.dtype, device=pos.device)
    return energy, forces, virial


def energy_forces_stress(model, data, *, trn_mean=0.0):
    """One eval() evaluation of `model` on `data` (GPU tensors) -> dict with `energy` [B], `forces` [N,3], `virial` [B,3,3]
    and `stress` [B,3,3] (module docstring).  The model must be in eval(); the caller's `data` is not modified."""
    from .hermnet import HTNet
    if isinstance(model, HTNet):
        raise NotImplementedError("energy_forces_stress: HTNet's triadic graphs are not supported")
    if model.training or getattr(model, "eval_param_grads", False):
        raise NotImplementedError("energy_forces_stress is a first-order eval() result: not in train() or with "
                                  "eval_param_grads (call model.eval())")
    if data.get("_hn_shard") is not None:
        raise NotImplementedError("energy_forces_stress of atom-sharded data: the ghost atoms' shares would have to be sent "
                                  "back to their owners, which is not implemented")
    if not data.pos.is_cuda:
        raise RuntimeError("hermnet_amd.energy_forces_stress runs on MI355X only (data is on %s); there is no CPU fallback"
                           % data.pos.device)
    energy, forces, virial = energy_forces_virial(model, data, None)
    if trn_mean:
        energy = energy + trn_mean
    return {"energy": energy, "forces": forces, "virial": virial, "stress": stress_of_virial(virial, data.get("cell"))}
