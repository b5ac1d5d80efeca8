"""Per-atom energies and per-atom virials of an eval() evaluation ("Per-atom outputs").

    energy [B], forces [N,3]   exactly what `model(data)` and `-autograd.grad(E.sum(), pos)` give
    energies [N]               the read-out term of every atom (hermnet.py:129), atom order; intensive models divide it by
                               the atom count of its graph, `trn_mean` is spread as trn_mean / N_graph per atom, so the
                               terms of a graph sum to its energy
    virials [N,3,3]            W_i = -1/2 sum_{e touching i} D_e (x) dE/dD_e, energy units, unsymmetrised ([a,b] = D_a g_b);
                               each edge is split equally between its two atoms (a convention: the pair split of LAMMPS
                               `compute stress/atom` and of ASE's pair calculators).  Summed over a graph, the symmetric
                               part is the virial of `utils.virial_calc(..., units='lj')`.

Refused (NotImplementedError): atom-sharded data, HTNet, train() / create_graph.  (With `trn_mean` on a batch of several
graphs the call reads the host -- a bincount -- and cannot be captured into a hipGraph; without it nothing does.)
"""
import torch

from .ops import AtomSink
from .stress import evaluate_with_sink


def atom_properties(model, data, *, virials=True, trn_mean=0.0):
    """One eval() evaluation of `model` on `data` (GPU tensors) with per-atom outputs -> dict with `energy` [B],
    `forces` [N,3], `energies` [N] and, with `virials=True`, `virials` [N,3,3].  Like the ASE calculator, the model is put
    in eval() and the forces come from ONE `autograd.grad(E.sum(), pos)`; the caller's `data` is not modified."""
    pos = data.pos
    if not pos.is_cuda:
        raise RuntimeError("hermnet_amd.atom_properties runs on MI355X only (data is on %s); there is no CPU fallback"
                           % pos.device)
    if model.training:
        model.eval()
    sink = AtomSink(virials)
    d, pos, energy, forces = evaluate_with_sink(model, data, sink)
    n = pos.size(0)
    batch = d.batch.long() if d.get("batch") is not None else torch.zeros(n, dtype=torch.long, device=pos.device)
    energies = sink.energies
    if trn_mean:
        energy = energy + trn_mean
        cnt = torch.bincount(batch, minlength=energy.numel()).clamp(min=1).to(energies.dtype)
        energies = energies + trn_mean / cnt.index_select(0, batch)
    out = {"energy": energy, "forces": forces, "energies": energies}
    if virials:
        # (no gradient reached the edge geometry -- e.g. no edge at all: every virial is zero)
        out["virials"] = sink.virials if sink.virials is not None else torch.zeros(n, 3, 3, dtype=pos.dtype, device=pos.device)
    return out
