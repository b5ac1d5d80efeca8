"""GPU: layer 0's node projection from the per-species table (layer.SpeciesTable + hermnet_species_expand) against the per-atom
launch of hermnet_node_pre_fwd, bit for bit.

In an energy / force evaluation x of the first layer is the embedding gather, so xh of a row depends on its species only: the
table holds hermnet_node_pre_fwd's xh of the embedding rows, the expand launch copies table[t][z_rows[r]] into xh[t][r].  A row's
result of the chain kernel does not depend on the other rows of its tile, so both forms must hold the same bits.

Shapes: the 53-atom graphs of tests/test_dead_ends.py (28 / 22 / 3 atoms of three elements; in-degrees 0, 1, 3, 5 and 70; atoms of
an unknown element -- rows past type_rowptr[T] --, an element without atoms, the NULL edges of a padded list); H = 128 and 64;
embeddings of 1, 100 and the model's own number of rows.  "Bit for bit" compares the int32 views."""
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import _lib, nodeops, switches, synth
from hermnet_amd.layer import LayerWeights
from hermnet_amd.ops import _stream
from test_dead_ends import ELEMS, KINDS, _alloy53, _dev, _energy_forces, _graph, _same_bits

pytestmark = pytest.mark.gpu
P = _lib.ptr
_CACHE = {}


def _layer(H, dev):
    """(embedding weight [V, H] of the model, kernel-ready weights of one layer of the three elements) at width H."""
    if H not in _CACHE:
        model = hn.HVNet(ELEMS, rc=5.0, num_layers=1, hidden_channels=H, num_rbf=16).eval()
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 11))
        model = model.to(dev)
        _CACHE[H] = (model, model.embed.weight.detach(), LayerWeights(model.hermconvs[0].mods.values()).refresh())
    return _CACHE[H][1:]


def _expand(table, z_rows, N, fill=float("nan")):
    """hermnet_species_expand into a pre-filled buffer -> (return code, xh)."""
    T, V, W = table.shape
    xh = torch.full((T, N, W), fill, device=table.device)
    rc = _lib.load().hermnet_species_expand(P(table), P(z_rows), P(xh), N, T, V, W, _stream())
    return rc, xh


@pytest.mark.parametrize("H,V", [(128, None), (64, None), (128, 1), (128, 100)], ids=["h128", "h64", "one_row", "100_rows"])
@pytest.mark.parametrize("kind", KINDS)
def test_table_and_expand_give_the_per_atom_launchs_bits(kind, H, V):
    """xh [T, N, 3H] of the two forms for x = embed(z_rows): every row, pad rows and rows of an unknown element included; the
    expand launch leaves nothing of its output unwritten (the buffer starts as NaN)."""
    dev = _dev()
    graph = _graph(kind, dev)
    emb, w = _layer(H, dev)
    z_rows = graph.z_rows
    if V is not None:
        emb = emb[:V].contiguous()
        z_rows = z_rows.clamp(max=V - 1)
    assert z_rows.dtype == torch.int64 and z_rows.numel() == graph.N and int(z_rows.max()) < emb.size(0)
    x = torch.nn.functional.embedding(z_rows, emb).contiguous()
    want = nodeops.node_pre_fwd(x, w, graph.T)[1]
    table = nodeops.species_table(emb, w, graph.T)
    assert table.shape == (graph.T, emb.size(0), 3 * H)
    rc, got = _expand(table, z_rows, graph.N)
    assert rc == 0
    assert torch.isfinite(got).all() and torch.isfinite(want).all() and float(want.abs().max()) > 1e-3
    assert _same_bits(got, want)
    assert _same_bits(nodeops.species_expand(table, z_rows, graph.N), want)      # (the wrapper the layer calls)
    if V is None and kind == "unknown":
        nk = graph.type_rowptr_host[graph.T]
        assert nk < graph.N and _same_bits(got[:, nk:], want[:, nk:])


def test_species_outside_the_table_are_clamped_into_it():
    """The kernel never reads outside the table: a species below 0 or at / above V takes the first / last row."""
    dev = _dev()
    emb, w = _layer(128, dev)
    table = nodeops.species_table(emb[:7].contiguous(), w, 3)
    z = torch.tensor([0, 6, 7, 1000, -1, -2 ** 40, 2 ** 40, 3], device=dev)
    rc, got = _expand(table, z, z.numel())
    assert rc == 0
    assert _same_bits(got, table[:, z.clamp(0, 6)])


def test_refusals():
    """HN_ERR_BAD_ARG in front of any launch: the output keeps its fill."""
    dev = _dev()
    emb, w = _layer(128, dev)
    table = nodeops.species_table(emb[:5].contiguous(), w, 3)
    T, V, W = table.shape
    z = torch.zeros(9, dtype=torch.int64, device=dev)
    xh = torch.full((T, 9, W), 7.0, device=dev)
    lib = _lib.load()
    good = (P(table), P(z), P(xh), 9, T, V, W)
    bad = {"no table": (None,) + good[1:], "no species": good[:1] + (None,) + good[2:], "no output": good[:2] + (None,) + good[3:],
           "negative rows": good[:3] + (-1,) + good[4:], "no relation": good[:4] + (0,) + good[5:],
           "empty table": good[:5] + (0, W), "width 0": good[:6] + (0,), "width not a multiple of 4": good[:6] + (W - 2,)}
    for name, args in bad.items():
        assert lib.hermnet_species_expand(*args, _stream()) == 1, name
    assert lib.hermnet_species_expand(*(good[:3] + (0,) + good[4:]), _stream()) == 0          # no rows: nothing to do
    torch.cuda.synchronize()
    assert bool((xh == 7.0).all())
    assert lib.hermnet_species_expand(*good, _stream()) == 0
    assert _same_bits(xh, table[:, z])


def _model(layers, dev, H=128):
    key = ("model", layers, H)
    if key not in _CACHE:
        model = hn.HVNet(ELEMS, rc=3.0, num_layers=layers, hidden_channels=H, num_rbf=128).eval()
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 7))
        model = model.to(dev)
        for prm in model.parameters():
            prm.requires_grad_(False)
        _CACHE[key] = model
    return _CACHE[key]


def _data(kind, dev):
    """test_dead_ends' 53-atom alloy; "padded": the same atoms with the device search's padded list (21 NULL edges)."""
    d = _alloy53(kind)
    if kind != "padded":
        return d
    from hermnet_amd.neighbor import neighbor_search_padded, padded_list_ok
    E = d.edge_index.size(1)
    pos, cell = d.pos.to(dev), d.cell[0].to(dev).contiguous()
    ei, sh, total = neighbor_search_padded(pos, 3.0, cell, E + 21)
    assert padded_list_ok(total) == (True, E) and bool((ei[:, E:] == -1).all())
    out = hn.Data(pos=pos, atomic_number=d.atomic_number.to(dev), batch=d.batch.to(dev), cell=d.cell.to(dev), edge_index=ei,
                  edge_shift=sh)
    out._hn_edge_count = total
    return out


def _counted(monkeypatch):
    """Counts the calls of the two forms of layer 0's projection as the layer makes them."""
    import hermnet_amd.layer as lmod
    calls = []
    for name in ("species_expand", "node_pre_fwd"):
        def wrap(*a, _f=getattr(nodeops, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(lmod.nodeops, name, wrap)
    return calls


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layers", [1, 2, 5])
def test_model_with_and_without_the_table_gives_the_same_bits(layers, kind, monkeypatch):
    """HVNet with 1, 2 and 5 layers: switches.species_table on (one expand launch, L - 1 per-atom projections) against off."""
    dev = _dev()
    model = _model(layers, dev)
    calls = _counted(monkeypatch)
    e1, f1, _ = _energy_forces(model, _data(kind, dev), dev)
    assert sorted(calls) == ["node_pre_fwd"] * (layers - 1) + ["species_expand"]
    del calls[:]
    monkeypatch.setattr(switches, "species_table", False)
    e0, f0, _ = _energy_forces(model, _data(kind, dev), dev)
    assert calls == ["node_pre_fwd"] * layers
    assert float(f0.abs().max()) > 1e-4
    assert _same_bits(e1, e0) and _same_bits(f1, f0)


@pytest.mark.parametrize("H", [64, 100])
def test_model_at_other_chain_widths_gives_the_same_bits(H, monkeypatch):
    """Width 64 (the message backward's general form runs at layer 0: the deferred sums are width 128's) and width 100 (padded to
    128 channels: the table is made from the padded embedding rows), two layers: the switch on against off."""
    dev = _dev()
    model = _model(2, dev, H)
    calls = _counted(monkeypatch)
    e1, f1, _ = _energy_forces(model, _data("unknown", dev), dev)
    assert sorted(calls) == ["node_pre_fwd", "species_expand"]
    assert model._species.table.shape == (3, model.embed.weight.size(0), 3 * ((H + 63) // 64 * 64))
    monkeypatch.setattr(switches, "species_table", False)
    e0, f0, _ = _energy_forces(model, _data("unknown", dev), dev)
    assert float(f0.abs().max()) > 1e-4
    assert _same_bits(e1, e0) and _same_bits(f1, f0)


@pytest.mark.parametrize("layers", [1, 2, 5])
def test_the_replayed_step_gives_the_eager_bits(layers):
    """GraphedStep (warm-up steps build the table, the captured step holds the expand launch) against the eager evaluation."""
    from hermnet_amd.graph import GraphedStep
    dev = _dev()
    model = _model(layers, dev)
    e, f, _ = _energy_forces(model, _alloy53("unknown"), dev)
    builds = model._species.builds
    step = GraphedStep(model, _alloy53("unknown").to(dev), warmup=2)
    eg, fg = step()
    assert _same_bits(eg, e) and _same_bits(fg, f)
    assert model._species.builds == builds and model._species.table is not None      # (nothing was rebuilt for the capture)


def test_a_layer_with_a_forward_hook_gets_the_per_atom_launch(monkeypatch):
    """A hook on the first layer is somebody who may read what it works on: the general form, the same bits."""
    dev = _dev()
    model = _model(2, dev)
    calls = _counted(monkeypatch)
    handle = model.hermconvs[0].register_forward_hook(lambda mod, args, out: None)
    try:
        e1, f1, _ = _energy_forces(model, _alloy53("plain"), dev)
    finally:
        handle.remove()
    assert calls == ["node_pre_fwd"] * 2
    del calls[:]
    e0, f0, _ = _energy_forces(model, _alloy53("plain"), dev)
    assert sorted(calls) == ["node_pre_fwd", "species_expand"]
    assert _same_bits(e1, e0) and _same_bits(f1, f0)


def test_the_table_follows_the_embedding_and_layer_0s_projection(monkeypatch):
    """After an in-place change of one embedding row, and after one of a single weight of layer 0's projection, the next
    evaluation's xh is the per-atom launch's again (and not the one from before)."""
    import hermnet_amd.layer as lmod
    dev = _dev()
    model = hn.HVNet(ELEMS, rc=3.0, num_layers=2, hidden_channels=128, num_rbf=128).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 9))
    model = model.to(dev)
    for prm in model.parameters():
        prm.requires_grad_(False)
    seen = []

    def expand(*a, _f=nodeops.species_expand, **k):
        seen.append(_f(*a, **k))
        return seen[-1]
    monkeypatch.setattr(lmod.nodeops, "species_expand", expand)

    def xh_pair():
        """(xh the evaluation's expand launch wrote, xh of the per-atom launch on the same x with the model's current copies)"""
        del seen[:]
        e, f, d = _energy_forces(model, _alloy53("unknown"), dev)
        assert len(seen) == 1 and bool(torch.isfinite(e).all())
        graph, w0 = d._hn_step.graph, model.hermconvs[0]._weights
        x = torch.nn.functional.embedding(graph.z_rows, model.embed.weight.detach()).contiguous()
        return seen[0], nodeops.node_pre_fwd(x, w0, graph.T)[1]

    got0, want0 = xh_pair()
    assert _same_bits(got0, want0) and model._species.builds == 1
    again, _ = xh_pair()
    assert _same_bits(again, got0) and model._species.builds == 1          # an unchanged model: no rebuild
    with torch.no_grad():
        model.embed.weight[13] += 0.25                                      # Al: 28 of the 53 atoms
    got1, want1 = xh_pair()
    assert _same_bits(got1, want1) and not _same_bits(got1, got0) and model._species.builds == 2
    with torch.no_grad():
        model.hermconvs[0].mods["Ni"].message_layer.x_proj[0].weight[3, 5] += 0.5
    got2, want2 = xh_pair()
    assert _same_bits(got2, want2) and not _same_bits(got2, got1) and model._species.builds == 3
    with torch.no_grad():                                                   # (another layer's weight: the table stays)
        model.hermconvs[1].mods["Ni"].message_layer.x_proj[0].weight[3, 5] += 0.5
    got3, _ = xh_pair()
    assert _same_bits(got3, got2) and model._species.builds == 3
