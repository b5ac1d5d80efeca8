"""GPU: the stage kernels (csrc/node_kernels.hip), the read-out in its three forms, HTNet's pair mean, and the layer built
from the stage kernels (layer.GemmRelationalLayer) against float64 restatements, every row on its own scale.

Inputs, references and rules are those of tests/test_stage_reference.py, which checks them on the CPU: a row passes at
err <= max(floor, 8 x base) (helpers.judge_rows; floors 2e-6 forward, 5e-6 backward; base = the error of the fp32
restatement on that row); rows defined as zero must be exactly zero; every output buffer is NaN-filled before its launch
(the wrappers of hermnet_amd.nodeops allocate through `nodeops._new`, which is replaced here), and what the contract
leaves undefined stays out of the judgement.  On the "plain" set 8 x base may decide on at most CAP of an output's rows.

Measured on the MI355X: see each test's docstring."""
import copy
import math
from types import SimpleNamespace

import pytest
import torch

from hermnet_amd import nodeops
from helpers import rel_err, judge_rows, FLT_MIN
import ref_ops
import test_message_reference as mr
import test_stage_reference as sr
from test_stage_reference import CAP, OPERAND_SETS, FWD

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def nan_outputs(monkeypatch):
    """Every buffer a nodeops wrapper allocates for a kernel to write starts as NaN."""
    monkeypatch.setattr(nodeops, "_new", lambda like, *shape: torch.full(shape, float("nan"), dtype=like.dtype, device=like.device))


def _report(case, opset, figures, cap=True):
    per_kernel = sr.worst_by_kernel(figures, {})
    for k, (share, worst) in sorted(per_kernel.items()):
        print("rows %-24s %-11s %-16s worst err/bound %.3f  deciding share %.3f" % (sr.case_id(case), opset, k, worst, share))
    if cap and opset == "plain":
        for nm, f in figures.items():
            assert f[0] <= CAP, (case, nm, f)


STAGE_CASES = [c for c in sr.all_cases() if c[0] in ("stage", "ln", "head")]


@pytest.mark.parametrize("case", STAGE_CASES, ids=sr.case_id)
def test_stage_kernels_row_by_row(case, nan_outputs):
    """ssilu_fwd / _bwd (both gradient layouts, T = 1 and 3, no bias, one bias row, bias blocks of 16 rows), update_mid,
    update_out, update_out_bwd, update_mid_bwd (nk = 0, N - 2, N; with and without the row mask; the three bias forms),
    layernorm_fwd / _bwd (with and without `add`; real widths that end inside a float4) and energy_head_fwd / _bwd through
    their nodeops wrappers, on both operand sets.
    Measured on the MI355X, worst err / bound over all cases and both sets: ssilu_fwd 0.11, ssilu_bwd 0.05,
    update_mid 0.09, update_out 0.13, update_out_bwd 0.03, update_mid_bwd 0.03, layernorm_fwd 0.09, layernorm_bwd 0.03,
    energy_head_fwd 0.06, energy_head_bwd 0.05; 8 x base decided on no row of the plain set but 1.5 % of update_mid's.
    Caught here: layernorm_fwd took the mean from one plain float32 sum, and on the adversarial row of 1e3 + unit noise at
    (rows, H, h_real) = (1, 1024, 1021) its n was 1.57e-5 off against a bound of 1.04e-5 (1.5 x); the kernel now corrects the
    mean by the sum of the shifted row, and that row stands at 0.08 of its bound."""
    dev = _dev()
    for opset in OPERAND_SETS:
        ref = sr.reference(case[0], *case[1:], opset)
        got = sr.FAMILIES[case[0]][1](nodeops, lambda v: v.to(dev), ref.t)
        _report(case, opset, sr.judge_all(got, ref, "%s %s" % (sr.case_id(case), opset)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("H", sr.TAIL_WIDTHS)
def test_scaled_silu_tail_rows(H, nan_outputs):
    """Saturated pre-activations through hermnet_ssilu_fwd / _bwd: rows in [-80, -20] within floor + 2 |h|max 2^-24 of the
    float64 restatement, rows at +-100 and +-1e6 finite, the negative ones below FLT_MIN.
    Measured on the MI355X: worst row error 1.2e-7 forward / 1.2e-7 backward at H = 4 and 7.6e-7 / 9.0e-7 at H = 128, against
    derived bounds of 1.15e-5 / 1.45e-5 (the chain kernels' sigmoid_ on the same rows, test_node_chain_kernels_on_adversarial_operands:
    6.3e-7 to 9.4e-7 against 1.25e-5).  The bound holds in both kernel families; the two sigmoid forms stay as they are."""
    dev = _dev()
    ref = sr.reference("tail", H)
    got = sr.tail_run(nodeops, lambda v: v.to(dev), ref.t)
    for nm, (err, bound) in sr.judge_tail(got, ref, "tail H=%d" % H).items():
        print("tail H=%d %-10s worst row err %.2e  derived bound %.2e" % (H, nm, err, bound))


# ---- the read-out: stage form, staged-weight form, matrix-pipe form --------------------------------------------------------
def _readout_forms(form, t, dev):
    c = lambda k: t[k].to(dev).contiguous()
    x, ge, w0, b0, w2, b2, m = (c(k) for k in ("x", "ge", "w0", "b0", "w2", "b2", "mask"))
    H, C = w0.size(1), w0.size(0)
    if form == "stage":
        h = torch.addmm(b0, x, w0.t())
        e = nodeops.energy_head_fwd(h, w2, b2, m)
        gx = torch.mm(nodeops.energy_head_bwd(ge, h, w2, m), w0)
    elif form == "fused":
        assert nodeops.head_fused_supported(H, C)
        h, e = nodeops.energy_head_fused_fwd(x, w0.t().contiguous(), b0, w2, b2, m)
        gx = nodeops.energy_head_fused_bwd(ge, h, w0, w2, m)
    else:
        assert nodeops.head16_supported(H, C)
        h, e = nodeops.energy_head16_fwd(x, nodeops.weight_fragments16(w0), b0, w2, b2, m)
        gx = nodeops.energy_head16_bwd(ge, h, nodeops.weight_fragments16(w0.t().contiguous()), w2, H, m)
    return h, e, gx


@pytest.mark.parametrize("rows", sr.READOUT_ROWS)
@pytest.mark.parametrize("H,C", list(sr.READOUT_SIZES), ids=lambda v: str(v))
def test_read_out_forms_row_by_row(H, C, rows, nan_outputs):
    """x -> h = W0 x + b0 -> e = w2 . ScaledSiLU(h) + b2 (times the row mask) and the gradient w.r.t. x, per row against ONE
    float64 reference: library GEMM + energy_head_fwd / _bwd ("stage"), energy_head_fused_* ("fused", weights staged in
    LDS), energy_head16_* ("head16", the product on the matrix pipe).  e is judged on the scale sum_c |ScaledSiLU(h_c) w2_c|
    + |b2| (tests/test_stage_reference.py); a masked row must be exactly zero.  No cap here: the outputs are dot products
    of 64 to 576 terms, on which 8 x base is the bound for about half of the rows of the fp32 restatement itself.
    Measured on the MI355X, worst err / bound: stage form h 0.20, e 0.10, gx 0.21; fused form h 0.61, e 0.12, gx 0.15; matrix-pipe form
    h 0.29, e 0.09, gx 0.10."""
    dev = _dev()
    for opset in OPERAND_SETS:
        ref = sr.reference("readout", rows, H, C, opset)
        A = ref.r64["readout_fwd:e"][:, 1]
        for form in sr.READOUT_SIZES[(H, C)]:
            h, e, gx = _readout_forms(form, ref.t, dev)
            got = {"readout_fwd:h": h, "readout_fwd:e": torch.stack([e.cpu().double(), A], 1), "readout_bwd:gx": gx}
            figures = sr.judge_all(got, ref, "read-out %s %dx%d rows=%d %s" % (form, H, C, rows, opset))
            for nm, f in sorted(figures.items()):
                print("rows read-out %-6s %3dx%-3d rows=%-3d %-11s %-15s worst err/bound %.3f  deciding share %.3f"
                      % (form, H, C, rows, opset, nm, f[1], f[0]))


# ---- HTNet's pair mean ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.PAIR_CASES, ids=sr.case_id)
def test_pair_mean_row_by_row(case, nan_outputs):
    """hermnet_pair_mean in its three modes (nodeops.pair_mean forward / backward, nodeops.pair_sum_accumulate) per row
    against float64: the [Te][P][B] index arithmetic, exactly zero rows behind Te B, the adjoint identity
    <mean(x), g> = <x, mean_bwd(g)> (float64 sums of the kernels' outputs, 1e-6 of the product of norms), and the `ranges`
    filter: two launches over complementary range lists, one of them with an empty entry, leave bit for bit what the
    unranged launch leaves; a launch over one list alone leaves the other rows untouched.
    Measured on the MI355X, worst err / bound: mean 0.07, its gradient 0.015, the accumulate 0.06."""
    dev = _dev()
    c = lambda v: v.to(dev)
    for opset in OPERAND_SETS:
        ref = sr.reference("pair", *case, opset)
        t = ref.t
        Te, P, B, rows_out = t["dims"]
        got = sr.pair_run(nodeops, c, t)
        _report(("pair",) + case, opset, sr.judge_all(got, ref, "pair %s %s" % (sr.case_id(case), opset)))
        for a, b, g, xin in (("pair_mean:x", "pair_mean_bwd:x", "gx", "x"), ("pair_mean:vec", "pair_mean_bwd:vec", "gvec", "vec")):
            ma, mb, tg, tx = got[a].cpu().double(), got[b].cpu().double(), t[g].double(), t[xin].double()
            assert abs(float((ma * tg).sum()) - float((tx * mb).sum())) <= 1e-6 * float(ma.norm() * tg.norm()), (a, opset)
        lists = sr.pair_ranges(Te, B)
        dev_ranges = [(torch.tensor(rg, dtype=torch.int32, device=dev).reshape(-1, 2), rg) for rg in lists]
        xa, va = c(t["x_acc"]).clone(), c(t["vec_acc"]).clone()
        nodeops.pair_sum_accumulate(c(t["x"]), c(t["vec"]), xa, va, Te, P, B, *sr.PAIR_SCALES, ranges=dev_ranges[0])
        part = ref_ops.pair_sum_accumulate
        xr, vr = t["x_acc"].double(), t["vec_acc"].double()
        part(t["x"].double(), t["vec"].double(), xr, vr, Te, P, B, *sr.PAIR_SCALES, ranges=dev_ranges[0])
        untouched = ~ref_ops._rows_of_ranges(lists[0], rows_out)
        assert torch.equal(xa.cpu()[untouched], t["x_acc"][untouched]) and torch.equal(va.cpu()[untouched], t["vec_acc"][untouched])
        judge_rows(xa, xr, ref.r32["pair_sum:x"].where(~untouched[:, None], t["x_acc"]), FWD, "pair_sum ranged x", tiny=FLT_MIN)
        nodeops.pair_sum_accumulate(c(t["x"]), c(t["vec"]), xa, va, Te, P, B, *sr.PAIR_SCALES, ranges=dev_ranges[1])
        assert torch.equal(xa, got["pair_sum:x"]) and torch.equal(va, got["pair_sum:vec"])
    torch.cuda.synchronize()


# ---- the layer of stage kernels as a layer, and against the chain layer ------------------------------------------------------
RC, R = 5.0, 16
ZS = [13, 28, 29]
LAYER_FLOORS = {"x_out": 1e-5, "vec_out": 1e-5, "gx": 2e-5, "gvec": 2e-5}      # the message rows' floors: they dominate a layer
LAYER_CASES = [(128, 128, ("gemm", "chain")), (320, 320, ("gemm", "chain")), (576, 576, ("gemm",)), (520, 576, ("gemm",))]
LAYER_GRAPHS = [(3, (70, 91, 45), None), (2, (33, 64), False)]


def _layer_setup(H, T, counts, uniform, dev):
    """Weights of T PaiNNModules (std 0.3 at width 128, 1 / sqrt(width) beyond) on the host and on the device, a graph of
    `counts[t]` atoms per element plus five of an unknown element with four random edges per atom (the last element without
    incoming edges: an inactive relation), as tests/test_host_logic._layer_weights_and_graph builds them, and its host view."""
    from hermnet_amd.layer import LayerWeights
    from hermnet_amd.relations import RelationalGraph
    from hermnet_amd.rmnet import PaiNNModule
    torch.manual_seed(H + T)
    mods = [PaiNNModule(hidden_channels=H, num_rbf=R) for _ in range(T)]
    for m in mods:
        for p in m.parameters():
            p.data.normal_(0, 0.3 * math.sqrt(128.0 / H))
    w = LayerWeights(mods).refresh()
    wd = LayerWeights([copy.deepcopy(m).to(dev) for m in mods]).refresh()
    gen = torch.Generator().manual_seed(T)
    z = torch.cat([torch.full((n,), ZS[t], dtype=torch.long) for t, n in enumerate(counts)] + [torch.full((5,), 1, dtype=torch.long)])
    z = z[torch.randperm(z.numel(), generator=gen)]
    n = z.numel()
    src, tgt = torch.randint(0, n, (4 * n,), generator=gen), torch.randint(0, n, (4 * n,), generator=gen)
    keep = z[tgt] != ZS[T - 1]
    graph = RelationalGraph.build(z.to(dev), torch.stack([src[keep], tgt[keep]]).to(dev), ZS[:T], uniform=uniform)
    view = mr.graph_view(graph)
    view.row_active = None if graph.row_active is None else graph.row_active.cpu()
    return w, wd, graph, view


def _layer_restatement(view, w, x, vec, edge, gxo, gvo, dt):
    """node_pre_fwd -> message_scatter_ref -> the update, and the gradients of <(gxo, gvo), outputs> w.r.t. x, vec and the
    edge (Cartesian), in `dt` on float32 inputs."""
    c = lambda v: v.to(dt)
    rbf = SimpleNamespace(offset=torch.linspace(0, 1, R).to(dt), inv_rc=1.0 / RC, env_kind=0, env_p=5)
    with torch.enable_grad():
        x_, v_, e_ = (c(v).clone().requires_grad_(True) for v in (x, vec, edge))
        xh = ref_ops.node_pre_fwd(x_, w, view.T)[1]
        x1, vec1 = ref_ops.message_scatter_ref(xh, v_, x_, e_, c(w.wt), c(w.brbf), view, rbf, factored=True, per_relation=True)
        xo, vo = ref_ops._node_update(x1, vec1, w, view)[:2]
        gx, gvec, ge = torch.autograd.grad([xo, vo], [x_, v_, e_], [c(gxo), c(gvo)])
    return dict(x_out=xo.detach(), vec_out=vo.detach(), gx=gx, gvec=gvec, gD=mr.cartesian(e_.detach(), ge))


@pytest.mark.parametrize("T,counts,uniform", LAYER_GRAPHS, ids=["T3", "T2-ragged"])
@pytest.mark.parametrize("H,Hp,forms", LAYER_CASES, ids=["128", "320", "576", "520-in-576"])
def test_stage_kernel_layer_row_by_row(H, Hp, forms, T, counts, uniform):
    """layer.GemmRelationalLayer (LayerNorm, library GEMMs joined by the stage kernels, the message kernels, the update
    stages) forward and backward against the float64 composition of ref_ops.node_pre_fwd, message_scatter_ref and the
    update, with the same composition in float32 as base: x_out and vec_out per row at 1e-5, gx and gvec per row at 2e-5;
    rows of the unknown element and padded channels exactly zero.  The edge gradient is judged by helpers.rel_err over the
    whole array at 2e-5: it is NOT judged per edge here (tests/test_message_rows.py does that for the message kernels).
    Width 576 and 520 padded to 576 (h_real): the path that widths above 512 take, the message kernels at nine column
    blocks, the LayerNorm kernel's third register chunk.  At 128 and 320 layer.FusedRelationalLayer runs on the same inputs
    and is held to the same rule against the same reference, so neither layer is the other's oracle.
    Measured on the MI355X, worst err / bound: stage-kernel layer x_out 0.22, vec_out 0.16, gx 0.19, gvec 0.13 (each at width 576);
    chain layer x_out 0.14, vec_out 0.12, gx 0.15, gvec 0.09; edge gradient rel_err at most 1.9e-6."""
    from hermnet_amd.layer import FusedRelationalLayer, GemmRelationalLayer, Route, StepState
    from hermnet_amd.ops import RbfDescriptor
    dev = _dev()
    w, wd, graph, view = _layer_setup(H, T, counts, uniform, dev)
    assert w.w1cat.size(1) == Hp and w.h_real == (H if H != Hp else 0) and wd.chain == (Hp <= 512)
    assert view.N > int(view.type_rowptr[view.T])                               # rows of the unknown element
    N = view.N
    gen = torch.Generator().manual_seed(Hp + T)
    chan = (torch.arange(Hp) < H).float()
    rnd = lambda *s: torch.randn(*s, generator=gen) * chan
    x, vec, gxo, gvo = rnd(N, Hp), rnd(N, 3, Hp), rnd(N, Hp), rnd(N, 3, Hp)
    rhat = torch.nn.functional.normalize(torch.randn(view.E, 3, generator=gen), dim=1)
    edge = torch.cat([rhat, RC * (0.05 + 1.05 * torch.rand(view.E, 1, generator=gen))], 1).contiguous()
    r64 = _layer_restatement(view, w, x, vec, edge, gxo, gvo, torch.float64)
    r32 = _layer_restatement(view, w, x, vec, edge, gxo, gvo, torch.float32)
    rbf = RbfDescriptor(torch.linspace(0, 1, R, device=dev), RC, 0, 5)
    filler = torch.tensor([[1.0, 0.0, 0.0, 1.0]]).expand(graph.E - view.E, 4)
    for form in forms:
        xd, vd, ed = (v.to(dev).requires_grad_(True) for v in (x, vec, torch.cat([edge, filler])))
        if form == "gemm":
            xo, vo = GemmRelationalLayer.apply(xd, vd, ed, graph, rbf, wd, StepState(graph=graph))
        else:
            xo, vo = FusedRelationalLayer.apply(xd, vd, ed, graph, rbf, wd, StepState(graph=graph), Route())
        gx, gvec, ge = torch.autograd.grad([xo, vo], [xd, vd, ed], [gxo.to(dev), gvo.to(dev)])
        got = dict(x_out=xo.detach(), vec_out=vo.detach(), gx=gx, gvec=gvec)
        for nm, a in got.items():
            f = judge_rows(a, r64[nm], r32[nm], LAYER_FLOORS[nm], "%s layer %d %s" % (form, H, nm), tiny=FLT_MIN)
            assert not bool(a.reshape(-1, Hp)[:, H:].any()), (form, nm)
            print("rows layer %-5s H=%d Hp=%d T=%d %-8s worst err/bound %.3f  deciding share %.3f" % (form, H, Hp, T, nm, f[1], f[0]))
        gD = ge[:view.E, :3].cpu().double()
        err = rel_err(gD, r64["gD"])
        print("rows layer %-5s H=%d Hp=%d T=%d gD       rel_err %.2e" % (form, H, Hp, T, err))
        assert err < 2e-5, (form, err)
    torch.cuda.synchronize()
