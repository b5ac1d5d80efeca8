"""The kernel-ready parameter copies (layer.LayerWeights, layer.HeadWeights) as host objects: every copy a declared field,
each model the only owner of its own, and the one choice of the update launches' weight stream.  CPU only: the copies are
built with plain torch ops."""
import pytest
import torch

import hermnet_amd as hn
from hermnet_amd import _lib, nodeops
from hermnet_amd.layer import HeadWeights, LayerWeights
from hermnet_amd.rmnet import PaiNNModule, ScaledSiLU
from test_host_logic import _layer_weights_and_graph


def _is_set(v):
    """A built copy: a tensor, or the per-relation list of them."""
    return torch.is_tensor(v) or (isinstance(v, list) and len(v) > 0 and all(torch.is_tensor(t) for t in v))


def _group(w, names):
    """True / False: every field of the group is built / is None; anything mixed fails."""
    got = [_is_set(getattr(w, n)) for n in names]
    assert all(got) or (not any(got) and all(getattr(w, n) is None for n in names)), dict(zip(names, got))
    return all(got)


# hidden_channels -> (dense, frag, frag16): 100 pads to 128 (every group), 520 pads to 576 (no chain kernels)
@pytest.mark.parametrize("H,groups", [(64, (True, True, False)), (100, (True, True, True)), (520, (True, False, False))])
def test_layer_weights_fields_are_declared_and_built_by_group(H, groups):
    torch.manual_seed(0)
    w = LayerWeights([PaiNNModule(hidden_channels=H, num_rbf=16) for _ in range(3)])
    declared = LayerWeights.STATE + LayerWeights.DENSE + LayerWeights.FRAG + LayerWeights.FRAG16
    assert tuple(LayerWeights.__slots__) == declared and len(set(declared)) == len(declared)
    assert len(LayerWeights.FRAG) == 10 and LayerWeights.FRAG16 == tuple(n + "16" for n in LayerWeights.FRAG)
    for built in (False, True):         # every slot is set from the start; a refresh fills the groups of this width
        if built:
            assert w.refresh() is w and w.builds == 1
        for n in declared:
            getattr(w, n)               # (an unset slot raises AttributeError)
        want = groups if built else (False, False, False)
        assert (_group(w, LayerWeights.DENSE), _group(w, LayerWeights.FRAG), _group(w, LayerWeights.FRAG16)) == want
    assert w.chain == groups[1] and w.h_real == (H if H % 64 else 0)
    assert set(vars(w)) == set(declared)
    with pytest.raises(AttributeError):
        w.wvf32 = None
    with pytest.raises(AttributeError):
        w.frag16 = {}


@pytest.mark.parametrize("H,mfma", [(128, True), (100, False)])
def test_head_weights_fields_are_declared(H, mfma):
    torch.manual_seed(0)
    head = torch.nn.Sequential(torch.nn.Linear(H, H // 2), ScaledSiLU(), torch.nn.Linear(H // 2, 1))
    hw = HeadWeights(head)
    for n in HeadWeights.__slots__:
        getattr(hw, n)
    assert hw.w0 is None and hw.builds == 0
    assert hw.refresh() is hw and hw.builds == 1 and hw.refresh().builds == 1
    assert all(torch.is_tensor(getattr(hw, n)) for n in ("w0", "b0", "w2v", "b2"))
    assert hw.w0.shape == (H // 2, H) and hw.w0.is_contiguous() and hw.w2v.shape == (H // 2,)
    assert nodeops.head16_supported(H, H // 2) == mfma
    assert hw.w0t is None                       # (the fused form's copy: 128 takes the matrix-pipe form, 100 has neither)
    if mfma:
        assert torch.equal(hw.w0f16, nodeops.weight_fragments16(head[0].weight.detach()))
        assert torch.equal(hw.w0tf16, nodeops.weight_fragments16(head[0].weight.detach().t().contiguous()))
    else:
        assert hw.w0f16 is None and hw.w0tf16 is None
    with pytest.raises(AttributeError):
        hw.w0f = None
    # loose tensors, for one call: the fused form's transpose where that kernel exists, and no key
    w0 = torch.randn(64, 256)
    one = HeadWeights().build(w0, torch.randn(64), torch.randn(1, 64), torch.randn(1))
    assert nodeops.head_fused_supported(256, 64) and torch.equal(one.w0t, w0.t()) and one.w0t.is_contiguous()
    assert one.w0f16 is None and one.key is None and one.builds == 0


def _model(seed, H=128):
    torch.manual_seed(seed)
    return hn.HVNet(["Si"], rc=5.0, num_layers=1, hidden_channels=H, num_rbf=16).eval()


def _head_copies(model):
    ws, hw = model._refresh_weights(torch.device("cpu"))
    assert hw is model._head and len(ws) == 1
    return hw, (hw.w0, hw.b0, hw.w2v, hw.b2, hw.w0f16, hw.w0tf16)


def test_a_models_read_out_copies_are_its_own():
    """Nothing another model does drops or evicts a model's copies (a captured step has their addresses baked in): not its
    `invalidate_caches()`, not its train() / eval() transitions, not any number of other read-outs evaluated since."""
    A, B = _model(1), _model(2)
    hw_a, kept_a = _head_copies(A)
    hw_b, kept_b = _head_copies(B)
    assert all(torch.is_tensor(t) for t in kept_a) and hw_a is not hw_b and hw_a.builds == 1
    B.invalidate_caches()
    B.train()
    B.eval()
    others = [_model(10 + k) for k in range(5)]
    for m in others:
        _head_copies(m)
    again = _head_copies(A)[1]
    assert all(s is t for s, t in zip(again, kept_a)) and hw_a.builds == 1
    hw_b, kept_b = _head_copies(B)
    builds_b = hw_b.builds
    A.invalidate_caches()
    hw_a2, rebuilt = _head_copies(A)
    assert hw_a2 is hw_a and hw_a.builds == 2
    assert rebuilt[4] is not kept_a[4] and rebuilt[5] is not kept_a[5] and torch.equal(rebuilt[4], kept_a[4])
    assert all(s is t for s, t in zip(_head_copies(B)[1], kept_b)) and hw_b.builds == builds_b
    import hermnet_amd.layer as lmod            # no process-wide weight cache is left to share
    assert not hasattr(lmod, "_T_CACHE")


@pytest.mark.parametrize("H,T,counts,tile16,picks16", [(128, 3, (20, 31, 9), 1, True), (128, 3, (20, 31, 9), 0, False),
                                                       (64, 2, (40, 3), 1, False)])
def test_update_stream_is_the_triple_the_kernels_were_handed(H, T, counts, tile16, picks16):
    """`nodeops.update_stream`: 16-row tiles and the frag16 copies where the row layout picks them and the width has them,
    else the base tiles (tile_rows 0) and the frag copies -- the forward's triple and the backward's in the entry points' order."""
    w, g = _layer_weights_and_graph(H, T, counts)
    with _lib.options(update_tile16=tile16):
        assert (nodeops.update_tile_rows(g, H) == 16) == picks16
        tile, fwd, bwd = nodeops.update_stream(g, H, w)
        want = (16, (w.wvf16, w.wx0f16, w.wx2f16), (w.wx2tf16, w.wx0tf16, w.wvtf16)) if picks16 else \
            (0, (w.wvf, w.wx0f, w.wx2f), (w.wx2tf, w.wx0tf, w.wvtf))
        assert tile == want[0] and all(a is b for a, b in zip(fwd + bwd, want[1] + want[2]))
        assert all(torch.is_tensor(t) for t in fwd + bwd)
        assert nodeops.last_update_supported(g, H, w) == picks16
        assert nodeops.fused_boundary_supported(g, H, w) == picks16 == nodeops.fused_boundary_supported(g, H, w, w)
