"""CPU: the references and the judging rules that tests/test_message_rows.py holds the message kernels to -- and the inputs
of that test, which are built here so that both files see the same ones.

The message kernels' accuracy used to be one number per tensor (helpers.rel_err: max |a - b| / max |b|), which a hub row of
70 edges or a source row at scale 1e+6 dominates.  Here every target row, every (relation, source) row and every edge is
judged on its own scale (helpers.judge_rows, helpers.judge_edges), against the dense fp64 restatement
(ref_ops.message_scatter_ref), with the fp32 restatement of the same expressions as the measure of what fp32 itself costs
on that row.  This file checks the references themselves: the envelope forms, what the kernels' 12-tap band may cost, that
the fp32 restatement leaves the floors in charge (the cap), and that the new rules see three perturbations the global rule
does not.

Weights: the rows of `wt` stay at one common scale (randn / sqrt(R)) in every input set.  Banding is a claim about such
weights -- a dropped tap is below exp(-18) of the largest tap VALUE (hermnet_math.h), which says nothing once one weight
row is 1e+6 times another."""
import math
from types import SimpleNamespace

import pytest
import torch

from helpers import rel_err, judge_rows, judge_edges, edge_grad_scale, FLT_MIN
import ref_ops
from test_fwd_tap_table import RC, Z_LIST, _edge_list, _edges, _inputs

TOL = 1e-5                          # the project's floors (test_gpu_parity.TOL), now per row: TOL forward, 2 TOL backward
FLOORS = {"x1": TOL, "vec1": TOL, "gxh": 2 * TOL, "gx": 2 * TOL, "gvec": 2 * TOL, "gD": 2 * TOL}
CAP = 0.10                          # 8 x base may decide on at most this share of the live rows / edges of any output

# name: (H, R, envelope kind, envelope p, vec rows, graph)
CASES = {
    "h64_r128": (64, 128, 0, 5, True, "hvnet"),
    "h128_r128_layer0": (128, 128, 0, 5, False, "hvnet"),
    "h64_r2": (64, 2, 0, 5, True, "hvnet"),
    "h64_r13": (64, 13, 0, 5, True, "hvnet"),
    "h64_r20_exp": (64, 20, 1, 0, True, "hvnet"),
    "h64_r176": (64, 176, 0, 5, True, "hvnet"),          # the last width of the forward's one-tile form
    "h64_r177": (64, 177, 0, 5, True, "hvnet"),          # ... and the first of its two tap-row windows
    "h128_r200_exp": (128, 200, 1, 0, True, "hvnet"),
    "triadic_h64_r128": (64, 128, 0, 5, True, "triadic"),
}
OPERAND_SETS = ("plain", "adversarial")
_VIEWS, _REFS = {}, {}


def graph_view(graph):
    """What the restatements read of a RelationalGraph, on the host.  E counts the edges of the CSR segments: the NULL
    edges of a padded list are in none (the device build files them behind the last row; the torch build is not handed any)."""
    cpu = lambda t: None if t is None else t.detach().cpu()
    N = graph.N
    rowptr = cpu(graph.csr_rowptr)
    E = int(rowptr[N])
    return SimpleNamespace(N=N, T=graph.T, E=E, num_src=graph.num_src, res_row=cpu(graph.res_row), csr_rowptr=rowptr,
                           csr_src=cpu(graph.csr_src)[:E], type_rowptr=cpu(graph.type_rowptr),
                           type_rowptr_host=list(graph.type_rowptr_host))


def host_view(kind):
    """test_fwd_tap_table's graphs from the torch build: 200 atoms, in-degrees 0, 1, 3, 5, 64, 65, 70, ten atoms of an
    unknown element; "triadic": two elements, num_src != N, res_row."""
    from hermnet_amd.relations import RelationalGraph
    if kind not in _VIEWS:
        z, ei = _edge_list(11)
        ei = ei[:, ei[0] >= 0]
        if kind == "triadic":
            z = torch.where(z != 29, z, torch.ones_like(z))
            g = RelationalGraph.build_triadic(z, ei, Z_LIST[:2])
        else:
            g = RelationalGraph.build(z, ei, Z_LIST)
        _VIEWS[kind] = graph_view(g)
    return _VIEWS[kind]


def rbf_of(case, dt=torch.float32):
    H, R, kind, p, _, _ = CASES[case]
    return SimpleNamespace(offset=torch.linspace(0, 1, R).to(dt), inv_rc=1.0 / RC, env_kind=kind, env_p=p, num_rbf=R)


def known_edges(view):
    """Edges into rows of known elements are the first csr_rowptr[type_rowptr[T]] of the CSR order."""
    return int(view.csr_rowptr[int(view.type_rowptr[view.T])])


def placed_distances(R):
    """The distances at which the kernels take another path, as float32:
    the geometry clamp's value; the last float32 below rc; for 16 taps k spread over [0, R) the distance rc k / (R - 1) and
    its two float32 neighbours (hn_window_lo's floor decides there which window is taken; the result must not depend on
    it); and three distances from rc (R + 5) / (R - 1) on, where hn_window_lo's clamp of t acts."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    inf = f32(float("inf"))
    vals = [f32(1e-6), f32(RC * (1 - 2.0 ** -24))]
    for k in sorted(set(round(i * (R - 1) / 15) for i in range(16))):
        d = f32(RC * k / (R - 1))
        vals += [torch.nextafter(d, -inf), d, torch.nextafter(d, inf)]
    vals += [f32(RC * (R + 5) / (R - 1)), f32(RC * (R + 6) / (R - 1)), f32(RC * (R + 40) / (R - 1))]
    return torch.stack(vals).clamp(min=1e-6)


def edges_of(view, R, seed=5):
    """[E,4] (rhat, d): test_fwd_tap_table._edges' list, the placed distances on edges into known rows at even strides."""
    edge = _edges(view.E, R, seed, torch.device("cpu"))
    edge[:, 3] = edge[:, 3].abs().clamp(min=1e-6)          # (num_rbf = 2: one distance of that list is negative)
    placed = placed_distances(R)
    pos = torch.linspace(0, known_edges(view) - 1, placed.numel()).long()
    assert pos.unique().numel() == placed.numel()
    edge[pos, 3] = placed
    return edge.contiguous()


def _largest_row(view):
    deg = (view.csr_rowptr[1:] - view.csr_rowptr[:-1])[:int(view.type_rowptr[view.T])]
    return int(deg.argmax())


def inputs_of(case, opset):
    """(operands (xh, xb, vec, x, wt, brbf), edge, cotangents (gx1, gvec1)) as float32 host tensors.
    "plain": unit normal operands (test_fwd_tap_table._inputs).
    "adversarial": source rows of xh, vec and x at scales 10^U(-6, 6) each, target rows of the cotangents likewise, every
    ninth cotangent row at 1e-30, and the target row with the most edges made to cancel: its sources come in pairs (u, v)
    with xh[., v] = -(n_u / n_v) xh[., u] and vec[v] = vec[u] (n: how many of the row's edges leave the source), every edge
    of a pair at one (rhat, d), its own residual rows zero -- so the row's sums are noise and 8 x base judges them."""
    H, R, _, _, has_vec, kind = CASES[case]
    view = host_view(kind)
    cpu = torch.device("cpu")
    ops = list(_inputs(view, H, R, has_vec, cpu))
    edge = edges_of(view, R)
    gen = torch.Generator().manual_seed(17)
    N, Ns = view.N, view.num_src or view.N
    gx1, gvec1 = torch.randn(N, H, generator=gen), torch.randn(N, 3, H, generator=gen)
    if opset == "adversarial":
        xh, xb, vec, x, wt, brbf = ops
        scale = lambda n: 10.0 ** (-6 + 12 * torch.rand(n, generator=gen))
        s_src, s_tgt = scale(Ns), scale(N)
        xh = xh * s_src[None, :, None]
        xb = torch.zeros_like(xb)               # (a common bias row would drown every source row below its scale)
        x = x * s_src[:, None]
        vec = None if vec is None else vec * s_src[:, None, None]
        gx1, gvec1 = gx1 * s_tgt[:, None], gvec1 * s_tgt[:, None, None]
        ninth = torch.arange(0, N, 9)
        gx1[ninth] = 1e-30 * torch.randn(ninth.numel(), H, generator=gen)
        gvec1[ninth] = 1e-30 * torch.randn(ninth.numel(), 3, H, generator=gen)
        r = _largest_row(view)
        lo, hi = int(view.csr_rowptr[r]), int(view.csr_rowptr[r + 1])
        srcs = view.csr_src[lo:hi].long()
        uniq, count = srcs.unique(return_counts=True)
        res = r if view.res_row is None else int(view.res_row[r])
        x[res] = 0
        if vec is not None:
            vec[res] = 0
        for k in range(0, uniq.numel() - 1, 2):
            u, v = int(uniq[k]), int(uniq[k + 1])
            xh[:, v] = -(float(count[k]) / float(count[k + 1])) * xh[:, u]
            if vec is not None:
                vec[v] = vec[u]
            pair = torch.nonzero((srcs == u) | (srcs == v)).flatten() + lo
            edge[pair] = edge[pair[0]].clone()
        if uniq.numel() % 2:                    # an odd source out: no partner, no message
            xh[:, int(uniq[-1])] = 0
        ops = [xh.contiguous(), xb, vec, x, wt, brbf]
    return tuple(ops), edge, (gx1, gvec1)


def cartesian(edge, g):
    """The wrappers' edge gradient: (dE/drhat, dE/dd) [E,4] of the independent inputs (rhat, d) as the gradient w.r.t. the
    edge vector D = rhat d (ops.TrueEdgeGradient): gD = gd rhat + (gr - (gr . rhat) rhat) / d."""
    rh, d = edge[:, :3], edge[:, 3:4]
    gr, gd = g[:, :3], g[:, 3:4]
    return gd * rh + (gr - (gr * rh).sum(1, keepdim=True) * rh) / d


def restate(view, rbf, ops, edge, cots, dt, factored=True, band=None, scale=False):
    """The restatement of forward and backward in `dt` on float32 inputs: outputs, and the gradients of <cots, outputs>
    w.r.t. xh (with its bias added: the kernels add it on load), x, vec and the edge -- Cartesian, as the wrappers return
    it.  (rhat, d) enter exactly as the kernels read them, d as it stands and not as |rhat d|: a float32 unit vector is
    6e-8 off unit length, and (R - 1) times that is what the window decisions and the tap derivatives would see.)  The
    kernels' contract with virtual target rows (res_row) has no residual term in gx / gvec (the residual's operands enter
    detached): x feeds the residual only, so gx is zero there.  `scale`: also helpers.edge_grad_scale."""
    xh, xb, vec, x, wt, brbf = ops
    c = lambda t: None if t is None else t.to(dt)
    with torch.enable_grad():
        xh_ = (c(xh) + c(xb)[:, None, :]).detach().requires_grad_(True)
        x_ = c(x).clone().requires_grad_(True)
        v_ = None if vec is None else c(vec).clone().requires_grad_(True)
        e_ = c(edge).clone().requires_grad_(True)
        r_ = SimpleNamespace(offset=rbf.offset.to(dt), inv_rc=rbf.inv_rc, env_kind=rbf.env_kind, env_p=rbf.env_p)
        residual = None
        if view.res_row is not None:
            res = view.res_row.long()
            residual = (x_.detach()[res], None if v_ is None else v_.detach()[res])
        x1, vec1 = ref_ops.message_scatter_ref(xh_, v_, x_, e_, c(wt), c(brbf), view, r_, factored=factored, band=band,
                                               per_relation=True, residual=residual)
        ins = [xh_, x_, e_] + ([v_] if vec is not None else [])
        g = [c(t) for t in cots]
        gr = torch.autograd.grad([x1, vec1], ins, g, retain_graph=scale, allow_unused=True)
        A = edge_grad_scale([x1, vec1], e_, g, lambda ge: cartesian(e_.detach(), ge)) if scale else None
    gxh, gD, gvec = gr[0], cartesian(e_.detach(), gr[2]), (gr[3] if vec is not None else None)
    gx = torch.zeros_like(x_) if gr[1] is None else gr[1]
    out = dict(x1=x1.detach(), vec1=vec1.detach(), gxh=gxh.reshape(-1, gxh.shape[-1]), gx=gx, gD=gD)
    if gvec is not None:
        out["gvec"] = gvec
    return out, A


def reference(case, opset):
    """(inputs, fp64 dense restatement, fp32 restatement with the factored envelope, A_e) of a case: computed once, shared
    by every test of this file and of tests/test_message_rows.py, never modified."""
    key = (case, opset)
    if key not in _REFS:
        view, rbf = host_view(CASES[case][5]), rbf_of(case)
        ops, edge, cots = inputs_of(case, opset)
        r64, A = restate(view, rbf, ops, edge, cots, torch.float64, scale=True)
        r32, _ = restate(view, rbf, ops, edge, cots, torch.float32)
        _REFS[key] = SimpleNamespace(view=view, rbf=rbf, ops=ops, edge=edge, cots=cots, r64=r64, r32=r32, A=A)
    return _REFS[key]


def judge_all(got, ref, what, outputs=None):
    """Every output of `got` by its rule; {output: (deciding share, worst err / bound[, max base_e / A_e])}."""
    figures = {}
    for nm in outputs or [k for k in FLOORS if k in got]:
        if nm == "gD":
            figures[nm] = judge_edges(got[nm], ref.r64[nm], ref.r32[nm], ref.A, FLOORS[nm], "%s %s" % (what, nm))
        else:
            figures[nm] = judge_rows(got[nm], ref.r64[nm], ref.r32[nm], FLOORS[nm], "%s %s" % (what, nm), tiny=FLT_MIN)
    return figures


# ---- the envelope forms -------------------------------------------------------------------------------------------
def test_envelope_forms_agree_and_have_no_gradient_beyond_the_cutoff():
    one = torch.tensor(1.0, dtype=torch.float32)
    pts = [0.0, 1e-7, 0.5, 1 - 2.0 ** -24, 1.0, float(torch.nextafter(one, one * 2)), 1.3, 2000.0]
    u = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
    for p in (5, 6):
        a, b = ref_ops.envelope_ref(u, 0, p), ref_ops.envelope_ref(u, 0, p, factored=True)
        assert float((a - b).detach().abs().max()) <= 1e-13
        assert float(a[0].detach()) == 1.0 and not bool(a[4:].any()) and not bool(b[4:].any())
    for kind, p, factored in [(0, 5, False), (0, 5, True), (1, 0, False)]:
        env = ref_ops.envelope_ref(u, kind, p, factored)
        (g,) = torch.autograd.grad(env.sum(), u)
        assert bool(torch.isfinite(env).all()) and bool(torch.isfinite(g).all())
        assert not bool(g[4:].any()) and not bool(env[4:].any())          # u >= 1: exactly zero, value and gradient
        assert float(g[2]) < 0
    # float32, as the fp32 restatement runs it: the factored form is good to two ulps of 1, the left-to-right sum of terms of
    # size ~p^2 is not (hermnet_math.h) -- the reason `base` is taken with the factored form
    u32 = torch.linspace(0.5, 0.999, 500, dtype=torch.float32)
    exact = ref_ops.envelope_ref(u32.double(), 0, 5)
    err = lambda v: float((v.double() - exact).abs().max())
    assert err(ref_ops.envelope_ref(u32, 0, 5, factored=True)) <= 2.0 ** -22 < 1e-6 < err(ref_ops.envelope_ref(u32, 0, 5))


def test_window_restatement_matches_the_host_twin_of_the_kernels():
    """ref_ops.window_lo_ref against the definition in hermnet_math.h at the placed distances: floor(t) - 5 with t clamped to
    [0, R + 5], t evaluated in float32."""
    import numpy as np
    for R in (2, 13, 128, 200):
        d = placed_distances(R)
        lo = ref_ops.window_lo_ref(d, 1.0 / RC, R)
        u = d.numpy() * np.float32(1.0 / RC)
        t = np.minimum(np.maximum(u * np.float32(R - 1), np.float32(0)), np.float32(R + 5))
        assert t.dtype == np.float32
        assert lo.tolist() == (t.astype(np.int64) - 5).tolist()
        assert int(lo.min()) == -5 and int(lo.max()) == R           # both clamps are reached


# ---- what the 12-tap band may cost -------------------------------------------------------------------------------------
BAND_TOL = 1e-7


def _banded(ref, R, taps=12, shift=0):
    lo = ref_ops.window_lo_ref(ref.edge[:, 3], ref.rbf.inv_rc, R) + shift
    return restate(ref.view, ref.rbf, ref.ops, ref.edge, ref.cots, torch.float64, band=(lo, taps))[0]


def _band_errors(got, ref, exempt=()):
    """Per row: max |banded - dense| over the row / max |dense| over the row; per edge: |banded - dense|_inf / A_e.  Rows and
    edges whose dense value is identically zero must be zero.  `exempt`: (output, row) pairs left out by name."""
    worst = {}
    for nm in got:
        a, b = got[nm], ref.r64[nm]
        diff = (a - b).reshape(a.shape[0], -1).abs().amax(1)
        size = ref.A if nm == "gD" else b.reshape(b.shape[0], -1).abs().amax(1)
        keep = torch.ones_like(size, dtype=torch.bool)
        for out, row in exempt:
            if out == nm:
                keep[row] = False
        live = (size > 0) & keep
        assert not bool(diff[(size == 0) & keep].any()), nm
        worst[nm] = float((diff[live] / size[live]).max()) if bool(live.any()) else 0.0
    return worst


@pytest.mark.parametrize("opset", OPERAND_SETS)
@pytest.mark.parametrize("R", [2, 3, 12, 13, 20, 128, 200])
def test_banded_restatement_agrees_with_the_dense_one(R, opset, monkeypatch):
    """The kernels keep the taps floor(t) - 5 .. floor(t) + 6 of an edge (hermnet_math.h).  In fp64, on the inputs of
    tests/test_message_rows.py, that band costs less than 1e-7 of every row's own largest entry and of every edge's A_e: a
    dropped tap is more than 6 spacings from t, below exp(-18) = 1.5e-8 of a tap at the centre, and it enters a sum of kept
    taps times weights of one common scale.  R <= 6: the band holds every tap inside the cutoff, and the two restatements
    are the same bits.
    One row is left out, by name: the target row of the adversarial set that is made to cancel, in x1 and vec1 -- its
    entries are the rounding noise of sums 1e+16 times their size, so "its own largest entry" is no scale for anything."""
    case = "h64_r%d_band" % R
    monkeypatch.setitem(CASES, case, (64, R, 0, 5, True, "hvnet"))
    ref = reference(case, opset)
    got = _banded(ref, R)
    if R <= 6:
        assert all(torch.equal(got[nm], ref.r64[nm]) for nm in got)
    row = _largest_row(ref.view)
    worst = _band_errors(got, ref, exempt=[("x1", row), ("vec1", row)] if opset == "adversarial" else ())
    print("band R=%d %s, worst |banded - dense| / scale: %s" % (R, opset, " ".join("%s %.1e" % kv for kv in worst.items())))
    for nm, e in worst.items():
        assert e <= BAND_TOL, (nm, e)


# ---- the cap: under the fp32 restatement alone the floors decide ---------------------------------------------------------
@pytest.mark.parametrize("opset", OPERAND_SETS)
@pytest.mark.parametrize("case", list(CASES))
def test_the_floors_decide_under_the_fp32_restatement(case, opset):
    """A condition on the INPUTS of tests/test_message_rows.py, not a measurement of any kernel: judged like a kernel, the
    fp32 restatement passes (it is its own base), and on at least 90 % of the live rows / edges of every output the floor,
    not 8 x base, is the bound -- so the kernels are held to the project's 1e-5 / 2e-5 almost everywhere and `8 x base`
    only excuses the rows where fp32 itself has lost digits."""
    ref = reference(case, opset)
    figures = judge_all(ref.r32, ref, "%s %s fp32" % (case, opset))
    for nm, f in figures.items():
        worst_floor = _worst_over_floor(ref.r32[nm], ref, nm)
        print("%-18s %-11s %-5s fp32 restatement: err/floor %.2e  deciding share %.3f%s"
              % (case, opset, nm, worst_floor, f[0], "  max base/A %.2e" % f[2] if nm == "gD" else ""))
        assert f[0] <= CAP, (nm, f)


def _worst_over_floor(got, ref, nm):
    """Worst err / floor of `got` over the live rows / edges (the figure profiles/message_row_margin.md lists)."""
    a, b = got.detach().cpu().double(), ref.r64[nm]
    if nm == "gD":
        live = ref.A > 0
        return float(((a - b).abs().amax(1)[live] / (FLOORS[nm] * ref.A[live])).max())
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    live = b.abs().amax(1) > 0
    if not bool(live.any()):
        return 0.0
    return float(((a - b).abs().amax(1)[live] / b.abs().amax(1)[live]).max() / FLOORS[nm])


# ---- sensitivity: three perturbations of the RESTATEMENT (never of a kernel) ----------------------------------------------
class _ScaledSlope(torch.autograd.Function):
    """env with d env / d u scaled by 1 + 1e-3 for u > 0.98: a force that is not the derivative of the energy any more."""

    @staticmethod
    def forward(ctx, env, u):
        ctx.save_for_backward(u)
        return env.clone()

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        return g * torch.where(u > 0.98, 1.0 + 1e-3, 1.0).to(g.dtype), None


def _global_rule_passes(got, ref):
    return all(rel_err(got[nm], ref.r64[nm]) < (TOL if nm in ("x1", "vec1") else 2 * TOL) for nm in got)


def _perturbed(ref, ops=None, **kw):
    return restate(ref.view, ref.rbf, ref.ops if ops is None else ops, ref.edge, ref.cots, torch.float64, **kw)[0]


def _failing_outputs(got, ref, what):
    """The outputs of `got` that miss their row / edge rule (all of them finite)."""
    failing = set()
    for nm in got:
        assert bool(torch.isfinite(got[nm]).all()), nm
        try:
            judge_all(got, ref, what, [nm])
        except AssertionError:
            failing.add(nm)
    return failing


@pytest.mark.parametrize("what", ["11-tap band", "envelope slope", "bf16 row"])
def test_the_row_and_edge_rules_see_what_the_global_rule_does_not(what, monkeypatch):
    """Each perturbed fp64 restatement passes the old rule (rel_err over the whole tensor below TOL forward, 2 TOL backward, as
    test_message_scatter_op applies it) and fails the new one, on the output where the perturbation acts.
    The envelope slope and the bf16 row run on the adversarial operands, where the rows differ in scale and the global
    norm sees only the largest: the slope must fail the edge rule of gD (and no forward output), the bf16 row the row rule
    of x1 and vec1.
    THE MARGIN OF THE 11-TAP BAND IS THIN.  It runs on the plain operands and fails the edge rule of gD alone, on one edge,
    at 2.1e-5 A_e against the floor of 2e-5: with weights of one common scale the dropped tap (5 spacings below t at a
    placed window decision) is exp(-12.5) = 3.7e-6 of the centre tap and its slope 5 x that, 1.9e-5 -- the effect of an
    11-tap band IS the floor.  Inputs that make it plainer (weights smooth over the taps, cotangents in one channel) also
    push the 12-tap band itself past 1e-7, so they would say nothing about the band the kernels keep; a different
    summation order in torch could move this one edge to the other side of its bound."""
    ref = reference(*SENSITIVITY[what])
    view = ref.view
    if what == "11-tap band":       # the window without its lowest tap: floor(t) - 4 .. floor(t) + 6
        R = ref.rbf.num_rbf
        got = _perturbed(ref, band=(ref_ops.window_lo_ref(ref.edge[:, 3], ref.rbf.inv_rc, R) + 1, 11))
        expect = lambda failing: failing == {"gD"}
    elif what == "envelope slope":
        plain = ref_ops.envelope_ref
        monkeypatch.setattr(ref_ops, "envelope_ref", lambda u, *a, **k: _ScaledSlope.apply(plain(u, *a, **k), u))
        got = _perturbed(ref)
        monkeypatch.undo()
        expect = lambda failing: "gD" in failing and not failing & {"x1", "vec1"}
    else:
        # the sources of one low-degree target row, bf16-rounded in xh of that row's relation (the few other targets of
        # those sources in that relation see them too): the smallest such row that is not all residual
        deg = (view.csr_rowptr[1:] - view.csr_rowptr[:-1])[:int(view.type_rowptr[view.T])]
        x1, x = ref.r64["x1"], ref.ops[3].double()
        message = (x1[:deg.numel()] - x[:deg.numel()] / math.sqrt(2.0)).abs().amax(1)
        size = x1[:deg.numel()].abs().amax(1)
        ok = (deg >= 1) & (deg <= 5) & (message >= 0.1 * size)
        row = int(torch.where(ok, size, torch.full_like(size, float("inf"))).argmin())
        assert bool(ok[row]) and float(size[row]) < 1e-3 * float(x1.abs().max())
        t = int(torch.bucketize(torch.tensor(row), view.type_rowptr.long()[1:], right=True))
        srcs = view.csr_src[int(view.csr_rowptr[row]):int(view.csr_rowptr[row + 1])].long()
        ops = list(ref.ops)
        ops[0] = ops[0].clone()
        ops[0][t, srcs] = ops[0][t, srcs].bfloat16().float()
        got = _perturbed(ref, ops=ops)
        expect = lambda failing: {"x1", "vec1"} <= failing
    assert _global_rule_passes(got, ref), {nm: rel_err(got[nm], ref.r64[nm]) for nm in got}
    failing = _failing_outputs(got, ref, what)
    print("%s: misses the rule of %s" % (what, sorted(failing)))
    assert expect(failing), failing


SENSITIVITY = {"11-tap band": ("h64_r128", "plain"), "envelope slope": ("h64_r128", "adversarial"),
               "bf16 row": ("h64_r128", "adversarial")}


# ---- the tap slope just below the cutoff (what the row-by-row test found) -------------------------------------------------
@pytest.mark.parametrize("R", [20, 128, 200])
def test_the_host_twin_keeps_the_tap_slope_relative_up_to_the_cutoff(R):
    """hermnet_host_rbf_row (csrc/host_api.cpp: the kernels' per-edge arithmetic from hermnet_math.h on the host) against
    fp64 at w = 1 - u from 1e-1 down to 1e-4.  The slope of a tap is env' g + env g'; `1 - u^p (...)` gives env to an ulp of 1,
    which at w = 1e-4 is 300 x env itself, and g' carries (R - 1)^2 |u - mu|: with that value the slope was off by its own
    size (0.7 at R = 128, w = 1e-4).  hn_envelope's `sval` keeps it relative.  Bound: u is a float32, so w carries u's
    rounding, 2^-24 / w relative; the slope goes as w^2 and env as w^3: 5 x 2^-24 / w, plus 1e-5 for the taps themselves."""
    import numpy as np
    from hermnet_amd import _lib
    lib, P = _lib.load(), _lib.ptr
    C = 8
    off = torch.linspace(0, 1, R)
    coeff = -0.5 / float(off[1] - off[0]) ** 2
    gen = torch.Generator().manual_seed(R)
    wt = (torch.randn(R, C, generator=gen) / math.sqrt(R)).contiguous()
    b = torch.zeros(C)
    inv_rc = float(np.float32(1.0 / RC))
    for w in (1e-1, 3e-2, 1e-2, 1e-3, 1e-4):
        d = float(np.float32(RC * (1.0 - w)))
        rb, drb = torch.zeros(C), torch.zeros(C)
        assert lib.hermnet_host_rbf_row(P(off), R, inv_rc, coeff, 0, 5, P(wt), P(b), C, d, P(rb), P(drb)) == 0
        dd = torch.tensor(d, dtype=torch.float64, requires_grad=True)
        u = dd * inv_rc
        slope = torch.autograd.functional.jacobian(lambda x: (ref_ops.envelope_ref(x * inv_rc, 0, 5)
                                                             * torch.exp(coeff * (x * inv_rc - off.double()) ** 2)) @ wt.double(), dd)
        err = float((drb.double() - slope).abs().max() / slope.abs().max())
        w_true = 1.0 - float(u.detach())
        print("R=%d w=%.0e: slope err %.2e (bound %.2e)" % (R, w, err, 5 * 2.0 ** -24 / w_true + 1e-5))
        assert err <= 5 * 2.0 ** -24 / w_true + 1e-5, (R, w, err)
