"""GPU: the kernels of the training step (csrc/train_kernels.hip, csrc/train_node_kernels.hip, csrc/band_product.hip)
behind hermnet_amd.trainops against float64 restatements: every row, edge and column on its own scale.

Inputs, references and rules are those of tests/test_train_reference.py, which checks them on the CPU: an output passes
at err <= max(floor, 8 x base) (floors 2e-6 for order-0 outputs, 5e-6 for first- and second-order ones; base = the error
of the fp32 restatement on that row), sums that can cancel on the scale of their terms' magnitudes, rows the contract
defines as zero exactly zero.  Every buffer a kernel writes is NaN-filled before its launch: the wrappers of
hermnet_amd.trainops allocate through `trainops._new`, which is replaced here (`kernels`); the same replacement records the
shapes, which is how the routes are asserted (kernel taken, row sums inside or behind the kernel).

The kernels are reached through trainops' plain launch functions where one exists (the three orders of the message algebra,
`_node_op` by name, `_edge_unit`, `_basis_window`, `_band_grads`), else through the static forward / backward of its autograd
functions, run as plain functions on a stand-in ctx: both hand a kernel the NULL operands the autograd engine would
materialise as zeros.

Measured on the MI355X: see each test's docstring and profiles/train_row_margin.md."""
import pytest
import torch

from hermnet_amd import switches, trainops
import test_train_reference as tr
from test_train_reference import CAP, OPERAND_SETS

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class _Ctx(object):
    """What the static methods of an autograd Function ask of their ctx."""
    needs_input_grad = (True,) * 16

    def __init__(self, saved=(), **attrs):
        self.saved_tensors = tuple(saved)
        self.__dict__.update(attrs)

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def set_materialize_grads(self, value):
        pass


class KernelOps(object):
    """tests/ref_ops.py's training restatements by name and signature, computed by the kernels."""

    def __init__(self, dev, log):
        self.dev, self.log, self.row_sums, self._keys = dev, log, None, {}

    def _since(self, mark):
        return self.log[mark:]

    # ---- the message algebra
    def edge_message_fwd(self, X, R, V, U):
        return trainops._message_fwd(X, R, V, U)

    def edge_message_bwd(self, GS, GM, X, R, V, U):
        return trainops._message_bwd(GS, GM, X, R, V, U)[1]

    def edge_message_bwd2(self, cX, cR, cV, cU, GS, GM, X, R, V, U):
        return trainops._message_bwd2(cX, cR, cV, cU, GS, GM, X, R, V, U)

    def keys(self, k):
        if id(k) not in self._keys:
            d = lambda v: None if v is None else v.to(self.dev)

            def key(idx, n, sort):
                perm = torch.argsort(idx, stable=True) if sort else None
                return trainops._RowKey(d(idx), d(perm), d(torch.bincount(idx, minlength=n)), n)

            assert bool((k.tgt[1:] >= k.tgt[:-1]).all())
            self._keys[id(k)] = (k, trainops.EdgeKeys(key(k.tgt, k.n_tgt, False), key(k.src, k.n_src, True),
                                                      key(k.xrow, k.T * k.n_src, True), d(k.r_rows), d(k.pad)))
        return self._keys[id(k)][1]

    def message_algebra_fwd(self, xh, vec, R, U, k):
        assert switches.train_row_sums == self.row_sums
        mark = len(self.log)
        out = trainops._message_fwd(xh, R, vec, U, self.keys(k))
        assert len(self._since(mark)) == (2 if self.row_sums else 4), self._since(mark)      # (dx, dv) | (S, M) + two row sums
        return out

    def message_algebra_bwd(self, g_dx, g_dv, xh, vec, R, U, k):
        mark = len(self.log)
        g_xh, gR, g_vec, gU = trainops._message_bwd(g_dx, g_dv, xh, R, vec, U, self.keys(k))[1]
        extra = 0 if vec is None else 1
        assert len(self._since(mark)) == (3 + extra if self.row_sums else 4 + 2 * extra), self._since(mark)
        return g_xh, g_vec, gR, gU

    def message_algebra_bwd2(self, c_xh, cR, c_vec, cU, g_dx, g_dv, xh, vec, R, U, k):
        d_gdx, d_gdv, d_xh, dR, d_vec, dU = trainops._message_bwd2(c_xh, cR, c_vec, cU, g_dx, g_dv, xh, R, vec, U, self.keys(k))
        return d_gdx, d_gdv, d_xh, d_vec, dR, dU

    # ---- sums
    def segment_sum(self, x, idx, n_rows):
        in_order = bool((idx[1:] >= idx[:-1]).all())
        perm = None if in_order else torch.argsort(idx, stable=True).to(self.dev)
        key = trainops._RowKey(idx.to(self.dev), perm, torch.bincount(idx, minlength=n_rows).to(self.dev), n_rows)
        mark = len(self.log)
        out = trainops.SumRows.apply(x, key)
        assert self._since(mark) == [(n_rows, x.size(1))], "hermnet_segment_sum not taken"
        return out

    def col_sum(self, g):
        T, K, O = g.shape
        mark = len(self.log)
        out = trainops._col_sum_over_rows(g)
        assert K >= 256 and self._since(mark) == [(T, (K + trainops._ColSum.ROWS - 1) // trainops._ColSum.ROWS, O)], "hermnet_col_sum not taken"
        return out

    def edge_unit(self, order, D, gU=None, gd=None, C=None):
        o0, o1, o2 = trainops._edge_unit(order, D, gU, gd, C)
        return (o0, o1) if order == 0 else (o0 if order == 1 else (o0, o1, o2))

    # ---- node stages
    def silu_bwd(self, gy, x):
        return trainops._SiLUBwd.forward(_Ctx(), gy, x)

    def silu_bwd2(self, u, gy, x):
        return trainops._SiLUBwd.backward(_Ctx((gy, x)), u)

    def ln_bwd(self, gy, x, eps):
        return trainops._LayerNormBwd.forward(_Ctx(), gy, x, eps)

    def ln_bwd2(self, v, gy, x, eps):
        return trainops._LayerNormBwd.backward(_Ctx((gy, x), eps=eps), v)[:2]

    def mid_fwd(self, vp, xt, c0, c1):
        return trainops.UpdateMid.forward(_Ctx(), vp, xt, c0, c1)

    def mid_bwd(self, g_vdot, g_xin, vp, c0, c1):
        return trainops._UpdateMidBwd.forward(_Ctx(), g_vdot, g_xin, vp, c0, c1)

    def mid_bwd2(self, u_vp, u_xt, g_vdot, g_xin, vp, c0, c1):
        return trainops._UpdateMidBwd.backward(_Ctx((g_vdot, g_xin, vp), c=c0, eps=c1), u_vp, u_xt)[:3]

    def out_fwd(self, q, vdot, vp, xt, vt, m, c0):
        return trainops.UpdateOut.forward(_Ctx(), q, vdot, vp, xt, vt, m, c0)

    def out_bwd(self, gx, gv, q, vdot, vp, m, c0, want_xt_vt=True):
        if want_xt_vt:
            return trainops._UpdateOutBwd.forward(_Ctx(), gx, gv, q, vdot, vp, m, c0)
        return trainops._node_op("out_bwd", [gx, gv, q, vdot, vp, m], [q.shape, vdot.shape, vp.shape, None, None], gx.size(0),
                                 gx.size(1), c0)[:3]

    def out_bwd2(self, c_gq, c_gvdot, c_gvp, c_gxt, c_gvt, gx, gv, q, vdot, vp, m, c0):
        return trainops._UpdateOutBwd.backward(_Ctx((gx, gv, q, vdot, vp, m), s=c0), c_gq, c_gvdot, c_gvp, c_gxt, c_gvt)[:5]

    def res_fwd(self, x, dx, v, dv, m, c0):
        return trainops.Residual.forward(_Ctx(), x, dx, v, dv, m, c0)

    def mask_scale(self, g1, gv1, m, c0, rows, H):
        return trainops._MaskScale.forward(_Ctx(), g1, gv1, m, c0)

    # ---- the band product
    def band_product(self, A, B, bias):
        assert trainops._band_kernels(A, B.size(2))
        return trainops.BandP.forward(_Ctx(), A, B, bias, None, None, None)[0]

    def band_grad_a(self, g1, g2, B):
        mark = len(self.log)
        out = trainops.BandQ.forward(_Ctx(), g1, g2, B)
        assert self._since(mark) == [tuple(g1.shape[:2]) + (32,)], "hermnet_band_product_grad_a not taken"
        return out

    def band_grad_b(self, A, g1, g2):
        mark = len(self.log)
        out = trainops.BandS.forward(_Ctx(), A, g1, g2)
        assert len(self._since(mark)) == 2, "hermnet_band_product_grad_b not taken"
        return out

    def band_grads(self, A, B, g1, g2):
        return trainops._band_grads(A, B, g1, g2)


@pytest.fixture
def kernels(monkeypatch):
    """KernelOps on buffers that start as NaN: every `trainops._new` is a NaN fill, and its shape is recorded."""
    log = []

    def new(like, *shape):
        log.append(tuple(int(s) for s in shape))
        return torch.full(shape, float("nan"), dtype=like.dtype, device=like.device)

    monkeypatch.setattr(trainops, "_new", new)
    return KernelOps(_dev(), log)


def _to(dev):
    return lambda v: v.to(dev).contiguous() if torch.is_tensor(v) and v.is_floating_point() else v


def _report(case, opset, figures, note=""):
    for k, (share, worst) in sorted(tr.worst_by_kernel(figures, {}).items()):
        print("train rows %-22s %-11s %-14s %s worst err/bound %.3f  deciding share %.3f" % (tr.case_id(case), opset, k, note, worst, share))
    if opset == "plain":
        for nm, f in figures.items():
            assert nm.split("/")[0] in tr.DOT_PRODUCTS or f[0] <= CAP, (case, nm, f)


def _run_case(case, ops, note=""):
    for opset in OPERAND_SETS:
        ref = tr.reference(*case, opset)
        got = tr.FAMILIES[case[0]].run(ops, _to(ops.dev), ref.t)
        _report(case, opset, tr.judge_all(got, ref, "%s %s %s" % (tr.case_id(case), opset, note)), note)
    torch.cuda.synchronize()


@pytest.mark.parametrize("H", tr.MSG_WIDTHS)
def test_message_algebra_kernels_row_by_row(H, kernels, monkeypatch):
    """hermnet_edge_message_{fwd, bwd, bwd2} per edge through trainops.EdgeMessage(Grad) (no index arrays) and, with the
    gathers inside and node-level outputs, through trainops.MessageAlgebra(Grad) with switches.train_row_sums on (the
    *_rows kernels) and off (per-edge kernels + hermnet_segment_sum): S, M, gX, gR, gV, gU, dGS, dGM, dX, dR, dV, dU and
    their row sums; with and without V; R in its own edge order and in a permuted order with padding rows (exactly zero in
    gR / dR); all four second-order cotangents, and each one absent in turn.  Graph: 23 source rows, one or three
    relations, 301 edges into rows of 0 .. 3 edges and a hub of 150 between a row of none and a row of one, an empty
    (relation, source) group, trailing rows without summed edges; and a graph of one edge.  Widths 4 .. 516: lane groups
    of 1, 16 (nine live), 32 and 64 lanes, two passes at 320 and three at 516 (gU / dU accumulated across the passes).
    Measured on the MI355X, worst err / bound over all widths, configurations and both operand sets: per edge forward 0.09,
    backward 0.05, backward of the backward 0.11; node level forward 0.13 (row sums inside and behind alike), backward 0.04,
    backward of the backward 0.11; 8 x base decided on no row of the plain set but 0.3 % of dGM's.  Nothing found: the `+=`
    of gU / dU across passes, the one-lane pass at 516 and the padding rows hold."""
    assert tr.msg_passes(H) == {4: 1, 36: 1, 128: 1, 256: 1, 320: 2, 516: 3}[H]
    for row_sums in (True, False):
        monkeypatch.setattr(switches, "train_row_sums", row_sums)
        kernels.row_sums = row_sums
        _run_case(("msg", H), kernels, "row sums %s" % ("inside" if row_sums else "behind"))


@pytest.mark.parametrize("case", [("node",) + s for s in tr.NODE_SHAPES], ids=tr.case_id)
def test_node_stage_kernels_row_by_row(case, kernels):
    """The twelve ops of hermnet_train_node_op behind trainops.{SiLU2, LayerNorm2, UpdateMid, UpdateOut, Residual,
    _MaskScale}: every operand and output that may be NULL absent once; rows whose mask is 0 exactly zero; LayerNorm on one
    and on five rows (four per workgroup), rows of 1e3 + unit noise, a constant row and a row at 1e-20; MID rows whose v2
    half is at 1e-6, exactly zero and at 1e12.
    Measured on the MI355X, worst err / bound over the five shapes and both sets: silu_bwd 0.06, silu_bwd2 0.12, ln_bwd 0.19,
    ln_bwd2 0.19 (both on the rows of 1e3 + unit noise at H = 576, where 8 x base is the bound: the plain float32 sum of the
    mean costs the kernel no more than it costs the restatement), mid_fwd 0.06, mid_bwd 0.03, mid_bwd2 0.09, out_fwd 0.05,
    out_bwd 0.02, out_bwd2 0.03, res_fwd 0.05, mask_scale 0.01.  Nothing found."""
    _run_case(case, kernels)


@pytest.mark.parametrize("H", tr.TAIL_WIDTHS)
def test_silu_tail_rows(H, kernels):
    """Saturated pre-activations through silu_bwd / silu_bwd2: rows in [-80, -20] and [20, 80] within the bounds derived in
    tests/test_train_reference.py from s = 1 / (1 + __expf(-x)) and 1 - s; rows at +-100 and +-1e6 finite.
    Measured on the MI355X, worst row error against a derived bound of 1.47e-5: gx 1.2e-7, c_gy 1.2e-7, c_x 1.8e-7 at H = 4;
    6.6e-7, 8.9e-7, 8.6e-7 at H = 128 (the fp32 restatement on the CPU: 1.2e-7, 1.3e-7, 0.9e-7)."""
    ref = tr.reference("tail", H)
    got = tr.tail_run(kernels, _to(kernels.dev), ref.t)
    for nm, (err, bound) in tr.judge_tail(got, ref, "silu tail H=%d" % H).items():
        print("train rows silu tail H=%d %-15s worst row err %.2e  derived bound %.2e" % (H, nm, err, bound))


@pytest.mark.parametrize("case", [("seg", w) for w in tr.SEG_WIDTHS] + [("col",) + s for s in tr.COL_CASES], ids=tr.case_id)
def test_segment_and_column_sums_row_by_row(case, kernels):
    """hermnet_segment_sum behind trainops.SumRows per output row -- 0, 1, 2, 3 and 200 members, sorted and permuted, widths
    of 1 .. 64 lanes per row, six column blocks, and 262,400 floats (beyond the clamp of blockIdx.y: the column stride) --
    and hermnet_col_sum behind trainops._col_sum_over_rows per column (the route is asserted), on the scale of the
    magnitudes summed.
    Measured on the MI355X, worst err / bound: segment sums 0.05 (width 1536, plain), column sums 0.07 (O = 1024, K = 300,
    adversarial).  The column stride beyond 262,144 floats is right."""
    _run_case(case, kernels)


@pytest.mark.parametrize("E", tr.UNIT_EDGES)
def test_edge_unit_kernel_edge_by_edge(E, kernels):
    """hermnet_edge_unit, orders 0, 1, 2, with and without gU and gd: the zero vector, an edge on the floor and one at 1.5e-6,
    lengths 1e-3 .. 1e4, gU nearly parallel to U; gD, c_gU, c_gd and c_D on the scale of their terms' magnitudes.
    Measured on the MI355X, worst err / bound: 0.07 (plain), 0.05 (adversarial)."""
    _run_case(("unit", E), kernels)


def test_basis_window_writes_every_row_of_its_outputs(kernels):
    """hermnet_basis_window, orders 0, 1, 2, on NaN-filled outputs (tests/ref_ops.py has no restatement of it, so no row rule):
    two chunks of 16 rows, one padding row (src == num_edges) and one distance beyond the cutoff -- rows the kernel must
    write as zeros, not skip.  Every output comes from `trainops._new` (the shapes in the log) and holds no NaN afterwards;
    the two dead rows are exactly zero in all of them."""
    dev, nc, C = kernels.dev, 2, 16
    gen = torch.Generator().manual_seed(11)
    rows = nc * C
    u = torch.sort(0.05 + 0.9 * torch.rand(rows, generator=gen)).values
    u[-1] = 1.25                                            # beyond the cutoff
    src = torch.arange(rows)
    src[5] = rows                                           # row 5 holds no edge (num_edges = rows)
    dead = torch.tensor([5, rows - 1])
    mu = (torch.linspace(0.0, 1.0, 32)[None, :] + torch.tensor([0.0, 0.02])[:, None]).contiguous()
    w = torch.ones(nc, 32)
    w[1, :3] = 0.0                                          # centres outside the basis
    g, cu = torch.randn(nc, C, 32, generator=gen), torch.randn(rows, generator=gen)
    u, src, mu, w, g, cu = (t.to(dev) for t in (u, src, mu, w, g, cu))
    consts = (rows, C, -50.0, 5)
    mark = len(kernels.log)
    phi = trainops._basis_window(0, u, src, mu, w, consts, None, None)[0]
    g_u = trainops._basis_window(1, u, src, mu, w, consts, g, None)[0]
    d_g, d_u = trainops._basis_window(2, u, src, mu, w, consts, g, cu)
    torch.cuda.synchronize()
    assert kernels.log[mark:] == [(nc, C, 32), (rows,), (nc, C, 32), (rows,)]
    for nm, out in (("phi", phi), ("g_u", g_u), ("d_g", d_g), ("d_u", d_u)):
        out = out.reshape(rows, -1).cpu()
        assert not bool(torch.isnan(out).any()), nm
        assert not bool(out[dead].any()), nm
    assert bool((phi.reshape(rows, 32).cpu()[4] > 0).all()) and not bool(phi.cpu()[1, :, :3].any())


@pytest.mark.parametrize("case", [("band",) + s for s in tr.BAND_CASES], ids=tr.case_id)
def test_band_product_kernels_row_by_row(case, kernels):
    """hermnet_band_product, _grad_a, _grad_b and _grads per (chunk, row) of out and gA, per (chunk, k) row of gB and per
    chunk row of gbias, with and without bias and the second addend; the staged gradient form (C % 64 == 0, N in 128, 256,
    384) and the unstaged one, one and three workgroups per chunk, chunks at 1e-6 / 1 / 1e6 next to each other; rows of
    zeros in A give the bias bit for bit.
    Measured on the MI355X, worst err / bound: out 0.28, gA 0.32 (both at (3, 96, 480), adversarial), gB / gbias 0.25 (at
    (2, 384, 160), plain); at the three staged shapes gA 0.15 and gB / gbias 0.11 from the single kernels and from the
    one-pass form alike.  No stale weight window, nothing found."""
    nc, C, N = case[1:]
    assert tr.band_staged(C, N) == {(32, 32): False, (64, 128): True, (128, 256): True, (64, 384): True, (96, 480): False,
                                    (256, 96): False, (384, 160): False}[(C, N)]
    _run_case(case, kernels)
