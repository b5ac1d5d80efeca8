"""GPU: the edge stream of the channel-per-lane backward (csrc/message_bwd_cl.hip) on the smallest graph that walks every
path of it -- a row switch inside a group of four edges, the stream's partial last group, the 64-edge batch boundary, index
lanes past the batch's count, rows without edges behind the stream, and the two launches over tap-row windows.

37 source rows, three relations, H = 128 (two column blocks).  The CSC segment of every (relation, source row) has a length
drawn from {0, 0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 130}; the first twelve rows of relation 0 hold the set in order, the last
three rows of every relation are empty, relation 1 has no edge at all and 37 NULL edges sit behind the last segment.  The
library's default cuts the rows into chunks of 16 (three workgroups per relation and column block, a 130-edge row then a
wave's whole stream); `bwd_cl_rows = 64` makes one chunk, whose waves walk several rows each.

Every output is NaN-filled inside a NaN-filled guard band; rule, floors and references are those of
tests/test_message_reference.py (helpers.judge_rows / judge_edges against the dense fp64 restatement)."""
from types import SimpleNamespace

import pytest
import torch

from hermnet_amd import _lib, ops
from hermnet_amd.ops import edge_radial_tables
from hermnet_amd.relations import RelationalGraph
from test_fwd_tap_table import RC, Z_LIST, _dev, _edges, _inputs, _rbf
import test_message_reference as mr
from test_message_rows import _gedge_checked, _record

pytestmark = pytest.mark.gpu
H, NSRC, NULLS, GUARD = 128, 37, 37, 1024
LENGTHS = [0, 0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 130]
WIDTHS = {128: "whole tile", 200: "two tap-row windows"}
_CACHE = {}


def _segment_lengths():
    """[3, 37] edges per (relation, source row)."""
    gen = torch.Generator().manual_seed(23)
    L = torch.tensor(LENGTHS)[torch.randint(0, len(LENGTHS), (3, NSRC), generator=gen)]
    L[0, :len(LENGTHS)] = torch.tensor(LENGTHS)
    L[2, 16:20] = torch.tensor([3, 1, 2, 5])        # row switches inside the groups of four at the head of a chunk
    L[:, -3:] = 0
    L[1] = 0
    return L


def _built(dev):
    """(graph on the device, its host view): atoms sorted by element, so source row = atom id."""
    if "graph" not in _CACHE:
        z = torch.tensor([Z_LIST[0]] * 13 + [Z_LIST[1]] * 12 + [Z_LIST[2]] * 12)
        L = _segment_lengths()
        gen = torch.Generator().manual_seed(29)
        src, tgt = [], []
        for t in range(3):
            members = torch.nonzero(z == Z_LIST[t]).flatten()
            for s in range(NSRC):
                n = int(L[t, s])
                src.append(torch.full((n,), s))
                tgt.append(members[torch.randint(0, members.numel(), (n,), generator=gen)])
        src, tgt = torch.cat(src), torch.cat(tgt)
        perm = torch.randperm(src.numel(), generator=gen)
        ei = torch.stack([src[perm], tgt[perm]])
        if dev.type == "cuda":                          # (the NULL edges of a padded list: the device build files them last)
            ei = torch.cat([ei, torch.full((2, NULLS), -1)], 1)
        graph = RelationalGraph.build(z.to(dev), ei.to(dev), Z_LIST, uniform=False)   # (no padding rows: 37 rows)
        view = mr.graph_view(graph)
        assert graph.T == 3 and graph.N == NSRC and not graph.num_src and view.E == int(L.sum())
        assert graph.E == view.E + (NULLS if dev.type == "cuda" else 0)
        crp = graph.csc_rowptr.cpu().long()
        assert torch.equal((crp[1:] - crp[:-1])[:3 * NSRC].reshape(3, NSRC), L), "the segments are not the drawn ones"
        _CACHE["graph"] = (graph, view)
    return _CACHE["graph"]


def _reference(R, has_vec, dev):
    """Inputs and the fp64 / fp32 restatements of one (num_rbf, vec rows): computed once, shared, never modified."""
    key = (R, has_vec)
    if key not in _CACHE:
        _, view = _built(dev)
        cpu = torch.device("cpu")
        rbf = SimpleNamespace(offset=torch.linspace(0, 1, R), inv_rc=1.0 / RC, env_kind=0, env_p=5, num_rbf=R)
        ins = _inputs(view, H, R, has_vec, cpu)
        edge = _edges(view.E, R, 5, cpu)
        gen = torch.Generator().manual_seed(17)
        cots = (torch.randn(view.N, H, generator=gen), torch.randn(view.N, 3, H, generator=gen))
        r64, A = mr.restate(view, rbf, ins, edge, cots, torch.float64, scale=True)
        r32, _ = mr.restate(view, rbf, ins, edge, cots, torch.float32)
        _CACHE[key] = SimpleNamespace(view=view, rbf=rbf, ops=ins, edge=edge, cots=cots, r64=r64, r32=r32, A=A)
    return _CACHE[key]


def _guarded(*shape):
    """A NaN-filled tensor in the middle of a NaN-filled allocation: (tensor, whole allocation)."""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), float("nan"), device="cuda:0")
    return whole[GUARD:GUARD + n].view(*shape), whole


def _guards_intact(wholes, what):
    for nm, whole in wholes.items():
        assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all()), (what, nm)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(graph, rbf, dev_ops, edge, cots, table, view, what):
    """One call of hermnet_message_scatter_bwd through the wrapper into guarded, NaN-filled buffers:
    ({output: tensor} as the row rule reads them, {output: raw buffer})."""
    xh, xb, vec, x, wt, brbf = dev_ops
    T = graph.T
    bufs, wholes = {}, {}
    shapes = dict(gedge=(H // 64, graph.E, 4), gxh=(T, NSRC, 3 * H), gx=(NSRC, H))
    if vec is not None:
        shapes.update(gvec=(NSRC, 3, H), part=(T, NSRC, 3, H))
    for nm, shape in shapes.items():
        bufs[nm], wholes[nm] = _guarded(*shape)
    graph.edge_table = table
    try:
        ops._msg_bwd(graph, rbf, H, xh, vec, SimpleNamespace(wt=wt, brbf=brbf, b2=xb), edge, cots[0], cots[1], bufs["gedge"],
                     xh_bias=True, out=(bufs["gxh"], bufs.get("gvec"), bufs["gx"], bufs.get("part")))
    finally:
        graph.edge_table = None
    torch.cuda.synchronize()
    _guards_intact(wholes, what)
    got = dict(gxh=bufs["gxh"].reshape(T * NSRC, 3 * H), gx=bufs["gx"], gD=_gedge_checked(bufs["gedge"], graph, view, what))
    if vec is not None:
        got["gvec"] = bufs["gvec"]
        assert bool(torch.isfinite(bufs["part"]).all()), what
    for nm in ("gxh", "gx", "gvec"):
        assert nm not in got or bool(torch.isfinite(got[nm]).all()), (what, nm)
    return got, bufs


@pytest.mark.parametrize("rows", [0, 64], ids=["chunks_of_16", "one_chunk"])
@pytest.mark.parametrize("has_vec", [True, False], ids=["vec", "novec"])
@pytest.mark.parametrize("R", list(WIDTHS), ids=["r128", "r200_windows"])
def test_the_edge_stream_row_by_row(R, has_vec, rows):
    """Every path of the stream (module docstring) against the fp64 restatement, no NaN left, nothing written outside,
    the same bits from a second call; without vec rows also the gedge-only instance (NEED_GXH = false), bit for bit.
    Measured on the MI355X, worst err / bound over the eight cases: gxh 0.12, gx 0.003, gvec 0.014, gD 0.13 (the floors decide
    everywhere but on 4-5 % of the edges)."""
    dev = _dev()
    graph, view = _built(dev)
    ref = _reference(R, has_vec, dev)
    rbf = _rbf(R, dev)
    c = lambda t: None if t is None else t.to(dev).contiguous()
    dev_ops = tuple(c(t) for t in ref.ops)
    filler = torch.tensor([[1.0, 0.0, 0.0, 1.0]]).expand(graph.E - view.E, 4)
    edge = c(torch.cat([ref.edge, filler]))
    cots = tuple(c(t) for t in ref.cots)
    table, _ = edge_radial_tables(graph, rbf, edge)
    what = "stream R=%d %s rows=%d" % (R, "vec" if has_vec else "novec", rows)
    with _lib.options(bwd_cl_rows=rows):
        got, bufs = _run(graph, rbf, dev_ops, edge, cots, table, view, what)
        _record("stream_r%d" % R, "plain", what, mr.judge_all(got, ref, what))
        again, bufs2 = _run(graph, rbf, dev_ops, edge, cots, table, view, what + " again")
        live = slice(0, mr.known_edges(view))
        for nm in bufs:
            a, b = (bufs[nm], bufs2[nm]) if nm != "gedge" else (bufs[nm][:, live], bufs2[nm][:, live])
            assert torch.equal(_bits(a), _bits(b)), (what, nm, "two calls differ")
        if not has_vec:
            # the gedge-only entry of a first layer: xh arrives with its bias added; the general instance on the same
            # operand (zero bias, vec = NULL) writes the same bits
            xh, xb, _, x, wt, brbf = dev_ops
            xh_b = (xh + xb[:, None, :]).contiguous()
            gedge, whole = _guarded(H // 64, graph.E, 4)
            graph.edge_table = table
            try:
                ops._msg_bwd_gedge(graph, rbf, H, xh_b, SimpleNamespace(wt=wt, brbf=brbf), edge, cots[0], cots[1], gedge)
            finally:
                graph.edge_table = None
            torch.cuda.synchronize()
            _guards_intact(dict(gedge=whole), what + " gedge entry")
            gD = _gedge_checked(gedge, graph, view, what + " gedge entry")
            _record("stream_r%d" % R, "plain", what + " gedge entry", mr.judge_all(dict(gD=gD), ref, what + " gedge entry"))
            _, full = _run(graph, rbf, (xh_b, torch.zeros_like(xb), None, x, wt, brbf), edge, cots, table, view, what + " general")
            assert torch.equal(_bits(gedge[:, live]), _bits(full["gedge"][:, live])), (what, "gedge entry against the general instance")


def test_the_window_launches_against_the_whole_tile():
    """The pair of window launches bit for bit against the whole-tile launch needs a num_rbf that both forms run."""
    pytest.skip("hermnet_message_scatter_bwd takes the windows from num_rbf alone (whole tile up to 137, two windows above): "
                "no width runs both forms, and the entry point has no argument that forces a window")
