"""GPU: the message kernels (csrc/message_kernels.hip, csrc/message_bwd_cl.hip) against the dense fp64 restatement, every
target row, every (relation, source) row and every edge on its own scale.

Rules, references and inputs are those of tests/test_message_reference.py, which checks them on the CPU: a row passes at
err <= max(floor, 8 x base) (helpers.judge_rows; floors TOL = 1e-5 forward, 2 TOL backward; base = the error of the fp32
restatement on that row), an edge gradient at |gD_e - ref_e|_inf <= max(2 TOL x A_e, 8 x base_e) (helpers.judge_edges; A_e
= helpers.edge_grad_scale).  The graph is test_fwd_tap_table's (in-degrees 0, 1, 3, 5, 64, 65, 70, atoms of an unknown
element, NULL edges, the triadic variant); the distances are its list plus the placed ones (the geometry clamp's 1e-6, the
last float32 below rc, both float32 neighbours of 16 window decisions, the clamp of t beyond the cutoff); the operands are
unit normal ("plain") or spread over twelve decades per row with a cancelling 70-edge row ("adversarial").  The rows of
`wt` are at one common scale in both: the 12-tap band is a claim about such weights.

Forms: the forward with the taps evaluated in its edge loop and fed from the once-per-step records (bit-identical, one of
them judged); the backward channel-per-lane with the edge table, 16 lanes per edge (VW) where it applies, and the
gedge-only entry of a first layer.  Every output buffer is NaN-filled before the launch."""
from types import SimpleNamespace

import pytest
import torch

from hermnet_amd import _lib, ops
from hermnet_amd.ops import edge_radial_tables
from test_fwd_tap_table import _dev, _graph, _rbf, _fwd
from helpers import FLT_MIN
import test_message_reference as mr
from test_message_reference import CASES, OPERAND_SETS, FLOORS, CAP

pytestmark = pytest.mark.gpu
VW_MAX_RBF = 176          # the 16-lanes-per-edge backward holds the whole weight tile of num_rbf + 23 rows in the 160 KiB LDS


def _same_graph(view, host):
    return (view.N == host.N and view.T == host.T and view.E == host.E and view.num_src == host.num_src
            and torch.equal(view.csr_rowptr, host.csr_rowptr) and torch.equal(view.csr_src, host.csr_src)
            and torch.equal(view.type_rowptr, host.type_rowptr)
            and (view.res_row is None) == (host.res_row is None)
            and (view.res_row is None or torch.equal(view.res_row, host.res_row)))


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda:0")


def _record(case, opset, form, figures):
    for nm, f in figures.items():
        print("rows %-18s %-11s %-16s %-5s worst err/bound %.3f  deciding share %.3f%s"
              % (case, opset, form, nm, f[1], f[0], "  max base/A %.2e" % f[2] if nm == "gD" else ""))
        assert f[0] <= CAP, (case, opset, form, nm, f)


def _gedge_checked(gedge, graph, view, what):
    """[E,3] Cartesian edge gradients of the live edges (column blocks summed) after the slot contract of
    include/hermnet_hip.h: the NULL edges of a padded list and the edges into rows of unknown elements are in no segment --
    their slots keep what the caller put there (here NaN; the product hands in zeros); every other slot is written in
    every column block, finite, with a zero fourth word."""
    live = torch.zeros(graph.E, dtype=torch.bool, device=gedge.device)
    live[:mr.known_edges(view)] = True
    assert bool(torch.isnan(gedge[:, ~live]).all()), what
    assert bool(torch.isfinite(gedge[:, live]).all()), what
    assert not bool(gedge[:, live, 3].any()), what
    gD = torch.zeros(view.E, 3, device=gedge.device)
    gD[:mr.known_edges(view)] = gedge[:, live, :3].sum(0)
    return gD


def _bwd(graph, rbf, H, dev_ops, edge, cots, table, view):
    """One call of the backward wrapper into NaN-filled buffers; gD of the live edges, rows of gxh as (relation, source)."""
    xh, xb, vec, x, wt, brbf = dev_ops
    T, Ns = graph.T, graph.num_src or graph.N
    gedge = _nan(H // 64, graph.E, 4)
    part = None if (vec is None or T == 1 or table is None) else _nan(T, Ns, 3, H)
    out = (_nan(T, Ns, 3 * H), None if vec is None else _nan(Ns, 3, H), _nan(Ns, H), part)
    graph.edge_table = table
    try:
        gxh, gvec, gx = ops._msg_bwd(graph, rbf, H, xh, vec, SimpleNamespace(wt=wt, brbf=brbf, b2=xb), edge, cots[0], cots[1],
                                     gedge, xh_bias=True, out=out)
    finally:
        graph.edge_table = None
    got = dict(gxh=gxh.reshape(T * Ns, 3 * H), gx=gx, gD=_gedge_checked(gedge, graph, view, "gedge"))
    if vec is not None:
        got["gvec"] = gvec
    return got, gedge


RADIAL_LEAK = 1.5e-6


def _beyond_cutoff_is_transverse(gD, ref, what):
    """u >= 1: no radial gradient.  The envelope and its slope are zero there, so dE/dd is; the kernels emit the Cartesian
    gD = (g - (g . rhat) rhat) q summed over the channels, whose component along rhat is zero but for
      * the float32 unit vector: (1 - |rhat|^2) (g . rhat) q, |1 - |rhat|^2| <= 2^-22, at most 2.4e-7 A_e,
      * rounding: three roundings per channel term and seven levels of channel sums (64 lanes, two column blocks), ten
        half-ulps 2^-24 of terms whose absolute sum is A_e, seen through |rhat_x| + |rhat_y| + |rhat_z| <= sqrt(3): 1.0e-6 A_e,
    together below RADIAL_LEAK x A_e (gradients below FLT_MIN: the edge rule's floor, 2e-5 FLT_MIN).  The reference keeps
    only the first.  A spurious envelope value or slope beyond the cutoff would show here long before the edge rule sees it;
    what is left of gD is the bias-only message's pull on the direction, which the edge rule judges."""
    edge = ref.edge.double()
    out = edge[:, 3] * torch.tensor(ref.rbf.inv_rc, dtype=torch.float32).double() >= 1.0
    assert int(out.sum()) > 20
    radial = lambda g: (g.detach().cpu().double() * edge[:, :3]).sum(1).abs()[out]
    assert float((radial(ref.r64["gD"]) / ref.A[out].clamp(min=1e-300)).max()) < 2.0 ** -22 * 1.01
    bound = torch.maximum(RADIAL_LEAK * ref.A, torch.full_like(ref.A, FLOORS["gD"] * FLT_MIN))[out]
    leak = radial(gD)
    print("rows %-46s radial part beyond the cutoff / bound %.3f" % (what, float((leak / bound).max())))
    assert bool((leak <= bound).all()), (what, float((leak / bound).max()))
    assert float(ref.r64["gD"][out].abs().max()) > 0          # (and there is a transverse part to judge)


@pytest.mark.parametrize("case", list(CASES))
def test_message_kernels_row_by_row_and_edge_by_edge(case):
    """See the module docstring.  Measured on the MI355X (profiles/message_row_margin.md has every figure), worst err / bound
    over all cases: x1 0.42, vec1 0.45 (adversarial rows that 8 x base judges; 0.10 on the plain set), gxh 0.13, gx 0.004,
    gvec 0.13, gD 0.16 channel per lane, 0.20 with 16 lanes per edge, 0.11 through the gedge entry.
    The radial part of gD beyond the cutoff: at most 0.081 of RADIAL_LEAK x A_e.
    Before hn_envelope's `sval` (hermnet_math.h) the channel-per-lane gD of the adversarial set was out of bounds on 1 to 10
    edges at d = 0.9999 rc in every case with R >= 128 and vec rows, by up to 150 x: the slope of a tap took the envelope
    from `1 - u^p (...)`, which is an ulp of 1 where the envelope is 3.5e-11."""
    dev = _dev()
    H, R, env_kind, env_p, has_vec, kind = CASES[case]
    graph = _graph(kind, dev)
    view = mr.graph_view(graph)
    assert _same_graph(view, mr.host_view(kind)), "the device build orders rows or edges unlike the torch build"
    assert (graph.E > view.E) == (kind == "hvnet")                       # the padded list's NULL edges
    rbf = _rbf(R, dev, env_kind, env_p)
    unknown = slice(int(view.type_rowptr[view.T]), view.N)
    for opset in OPERAND_SETS:
        ref = mr.reference(case, opset)
        c = lambda t: None if t is None else t.to(dev).contiguous()
        dev_ops = tuple(c(t) for t in ref.ops)
        filler = torch.tensor([[1.0, 0.0, 0.0, 1.0]]).expand(graph.E - view.E, 4)
        edge = c(torch.cat([ref.edge, filler]))
        cots = tuple(c(t) for t in ref.cots)
        table, taps = edge_radial_tables(graph, rbf, edge)

        # ---- forward: the loop form and the table-fed form, the same bits; one of them judged
        x1, vec1 = _fwd(graph, rbf, H, dev_ops, edge, None, out=(_nan(view.N, H), _nan(view.N, 3, H)))
        y1, wec1 = _fwd(graph, rbf, H, dev_ops, edge, taps, out=(_nan(view.N, H), _nan(view.N, 3, H)))
        assert torch.equal(x1, y1) and torch.equal(vec1, wec1)
        assert not bool(x1[unknown].any()) and not bool(vec1[unknown].any())
        _record(case, opset, "forward", mr.judge_all(dict(x1=x1, vec1=vec1), ref, "%s %s forward" % (case, opset)))

        # ---- backward, channel per lane with the edge table
        got, _ = _bwd(graph, rbf, H, dev_ops, edge, cots, table, view)
        _record(case, opset, "channel-per-lane", mr.judge_all(got, ref, "%s %s channel-per-lane" % (case, opset)))
        _beyond_cutoff_is_transverse(got["gD"], ref, "%s %s channel-per-lane" % (case, opset))

        # ---- backward, 16 lanes per edge: where the library refuses it by contract, that is what is asserted
        with _lib.options(bwd_lanes16=1):
            if kind == "triadic":
                with pytest.raises(RuntimeError, match="HN_ERR_BAD_ARG"):
                    _bwd(graph, rbf, H, dev_ops, edge, cots, None, view)
            elif R > VW_MAX_RBF:
                with pytest.raises(RuntimeError, match="HN_ERR_LDS"):
                    _bwd(graph, rbf, H, dev_ops, edge, cots, None, view)
            else:
                got, _ = _bwd(graph, rbf, H, dev_ops, edge, cots, None, view)
                _record(case, opset, "16-lanes-per-edge", mr.judge_all(got, ref, "%s %s 16-lanes-per-edge" % (case, opset)))
                _beyond_cutoff_is_transverse(got["gD"], ref, "%s %s 16-lanes-per-edge" % (case, opset))

        # ---- the gedge-only entry of a first layer (HVNet rows, no vec rows): xh arrives with its bias added; bit for bit
        # what the full backward writes for the same operand and vec = NULL (include/hermnet_hip.h)
        if kind == "hvnet" and not has_vec:
            xh, xb, _, x, wt, brbf = dev_ops
            xh_b = (xh + xb[:, None, :]).contiguous()
            gedge = _nan(H // 64, graph.E, 4)
            graph.edge_table = table
            try:
                ops._msg_bwd_gedge(graph, rbf, H, xh_b, SimpleNamespace(wt=wt, brbf=brbf), edge, cots[0], cots[1], gedge)
            finally:
                graph.edge_table = None
            gD = _gedge_checked(gedge, graph, view, "gedge entry")
            _record(case, opset, "gedge entry", mr.judge_all(dict(gD=gD), ref, "%s %s gedge entry" % (case, opset)))
            _beyond_cutoff_is_transverse(gD, ref, "%s %s gedge entry" % (case, opset))
            _, gedge_full = _bwd(graph, rbf, H, (xh_b, torch.zeros_like(xb), None, x, wt, brbf), edge, cots, table, view)
            live = slice(0, mr.known_edges(view))
            assert torch.equal(gedge[:, live], gedge_full[:, live])
    torch.cuda.synchronize()
