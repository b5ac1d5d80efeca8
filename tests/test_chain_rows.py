"""GPU: every compiled instance of the node chain kernels (csrc/node_chain.hip, node_chain_wide.hip, node_chain16.hip) against
float64 restatements, every row on its own scale, on row layouts cut for the instance's own tile height.

The ledger, the cases, the references and the rules are those of tests/test_chain_reference.py, which checks them on the CPU:
a row passes at err <= max(floor, 8 x base) (helpers.judge_rows; floors 2e-6 projection forward, 3e-6 update forward and saved
tensors, 5e-6 both backwards; base = the error of the fp32 restatement on that row); rows of unknown elements and inactive rows
exactly zero; padded channels exactly zero in what is handed on.  The share of rows on which 8 x base decides depends on the
restatements alone and is settled there; it is printed here with the worst err / bound of every case.  The C entry points are
called directly, so the test and not nodeops.update_tile_rows chooses the tile form: tile_rows = 16 / 0,
_lib.options(update_tile64_max=...) for the 64-row instance at width 128, _lib.options(node_chain_wide=1) for the panelled
kernels at 128 / 256 -- options through the context manager only, their defaults asserted behind the block.  Every output buffer and every handed-down buffer starts as NaN.

Each kernel is judged on its own.  A backward reads the saved tensors of the device's forward of the same form.  The
projection backward's reference reads the float64 ones; the update backward's reads the device's own, and off the scaled set
the float64 ones as well (`_judge_upd_bwd` says why, with the figures).  The fused forward's projection (the next layer's, on
the x_out the launch has just produced) is referred to the restatement of that projection on the device's own x_out; the pending backwards (held: gn_parts; fused: gxh
through the projection's backward of the layer above) are judged in two stages -- the gx_out / gvec_out they form against float64,
then gx1 / gvec1 against the restatement of the update backward on the device's own gx_out.

test_the_intended_instance_runs puts every ledger route under torch.profiler once, in one session, and asserts, by the kernel
names normalised to the CHAIN_KERNEL_BUDGETS key form, that the intended instance ran and no other chain kernel did.

Measured on the MI355X: see each test's docstring."""
import copy
import ctypes
import re
from contextlib import contextmanager
from types import SimpleNamespace

import pytest
import torch

from hermnet_amd import _lib
from hermnet_amd.ops import _stream
from helpers import row_err
import ref_ops
import test_chain_reference as cr
from test_cabi_cpu import CHAIN_KERNEL_BUDGETS, _chain_kernel_key

pytestmark = pytest.mark.gpu
P = _lib.ptr
_DEV = {}
ALL_KEYS = {k for unit in CHAIN_KERNEL_BUDGETS.values() for k in unit}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _weights_on(w, dev):
    """The device copy of a LayerWeights (once per width)."""
    if id(w) not in _DEV:
        wd = copy.copy(w)
        for k, v in vars(w).items():
            if torch.is_tensor(v):
                setattr(wd, k, v.to(dev))
        _DEV[id(w)] = (w, wd)
    return _DEV[id(w)][1]


def _graph_on(g, dev):
    if id(g) not in _DEV:
        rp = list(g.type_rowptr_host)
        _DEV[id(g)] = (g, SimpleNamespace(N=g.N, T=g.T, rowptr_c=(ctypes.c_int * len(rp))(*rp), type_rowptr=g.type_rowptr.to(dev),
                                         row_active=g.row_active.to(dev)))
    return _DEV[id(g)][1]


@contextmanager
def _options(route):
    with _lib.options(**route.options):
        yield
    for name in route.options:
        assert _lib.get_option(name) == 0, name
    assert _lib.get_option("update_tile64_max") == 0 and _lib.get_option("node_chain_wide") == 0


def _ok(rc):
    assert rc == 0, rc


# ---- the projection chain -----------------------------------------------------------------------------------------------------------
def _pre_fwd(route, t, dev):
    wd, x = _weights_on(t["w"], dev), t["x"].to(dev)
    N, T, H = t["N"], t["T"], t["H"]
    hb, xh, mean, rstd = _nan(dev, T, N, H), _nan(dev, T, N, 3 * H), _nan(dev, N), _nan(dev, N)
    lib = _lib.load()
    if route.tr == 16:
        _ok(lib.hermnet_node_pre_fwd16(P(x), P(wd.w1f16), P(wd.b1cat), P(wd.w2f16), P(wd.b2), P(hb), P(xh), P(mean), P(rstd), N, T, H,
                                       wd.h_real, 1e-5, _stream()))
    else:
        _ok(lib.hermnet_node_pre_fwd(P(x), P(wd.w1f), P(wd.b1cat), P(wd.w2f), P(wd.b2), P(hb), P(xh), P(mean), P(rstd), None, N, T, H,
                                     wd.h_real, 1e-5, None, 0, 0, _stream()))
    return hb, xh, mean, rstd


def _pre_bwd(route, t, dev, saved):
    wd, x, gxh, add = _weights_on(t["w"], dev), t["x"].to(dev), t["gxh"].to(dev), t["add"].to(dev)
    N, T, H = t["N"], t["T"], t["H"]
    hb, _, mean, rstd = saved
    parts = _nan(dev, T, N, H)
    lib = _lib.load()
    if route.tr == 16:
        _ok(lib.hermnet_node_pre_bwd16(P(gxh), P(hb), P(wd.w2tf16), P(wd.w1tf16), P(parts), N, T, H, _stream()))
        return {"pre_bwd:parts": parts.reshape(T * N, -1)}
    gx = _nan(dev, N, H)
    _ok(lib.hermnet_node_pre_bwd(P(gxh), P(hb), P(wd.w2tf), P(wd.w1tf), P(parts), P(x), P(mean), P(rstd), P(add), P(gx), None, N, T, H,
                                 wd.h_real, None, 0, 0, _stream()))
    return {"pre_bwd:parts": parts.reshape(T * N, -1), "pre_bwd:gx": gx}


# ---- the update chain ------------------------------------------------------------------------------------------------------------------
def _upd_fwd(route, t, dev, form=None):
    """-> the forward's buffers by name (xo, vo, vp, h2b, q23, nrm; "next": the fused form's projection outputs)."""
    form = form or route.form
    wd, g = _weights_on(t["w"], dev), _graph_on(t["graph"], dev)
    N, T, H = t["N"], t["T"], t["H"]
    x1, vec1 = t["x1"].to(dev), t["vec1"].to(dev)
    o = dict(vp=_nan(dev, N, 3, 2 * H), h2b=_nan(dev, N, H), q23=_nan(dev, N, 2 * H), nrm=_nan(dev, N, H), xo=_nan(dev, N, H),
             vo=_nan(dev, N, 3, H))
    tile = 16 if route.tr == 16 else 0
    ws = (wd.wvf16, wd.wx0f16, wd.wx2f16) if tile == 16 else (wd.wvf, wd.wx0f, wd.wx2f)
    head = (P(x1), P(vec1), P(ws[0]), P(ws[1]), P(wd.bx0_s), P(ws[2]), P(wd.bx2_s), P(g.row_active), P(g.type_rowptr), g.rowptr_c,
            P(o["vp"]), P(o["h2b"]), P(o["q23"]), P(o["nrm"]), P(o["xo"]))
    lib = _lib.load()
    if form == "last":
        _ok(lib.hermnet_node_update_fwd_last(*head, N, T, H, _stream()))
        assert bool(torch.isnan(o["vo"]).all())
    elif form == "fused" and route.direction == "fwd":
        wn = _weights_on(t["w_other"], dev)
        o["next"] = (_nan(dev, T, N, H), _nan(dev, T, N, 3 * H), _nan(dev, N), _nan(dev, N))
        _ok(lib.hermnet_node_update_pre_fwd(*head, P(o["vo"]), N, T, H, P(wn.w1f16), P(wn.b1cat), P(wn.w2f16), P(wn.b2),
                                            *[P(v) for v in o["next"]], T, wn.h_real, 1e-5, _stream()))
    else:
        _ok(lib.hermnet_node_update_fwd(*head, P(o["vo"]), N, T, H, tile, _stream()))
    return o


def _pending(t, dev, fused):
    """(the hn_pending_grads record, the tensors it points to) of the layer above: its gn_parts, or -- fused -- its gxh, hb and
    frag16 weights."""
    wa = _weights_on(t["w_other"], dev)
    keep = {k: t[k].to(dev) for k in ("gn_parts", "gv_parts", "xa", "mean_a", "rstd_a", "gx1_a", "gvec1_a", "gxh_a", "hb_a")}
    f = [None if fused else P(keep["gn_parts"])] + [P(keep[k]) for k in ("gv_parts", "xa", "mean_a", "rstd_a", "gx1_a", "gvec1_a")]
    chain = [P(keep["gxh_a"]), P(keep["hb_a"]), P(wa.w2tf16), P(wa.w1tf16)] if fused else [None] * 4
    return _lib.PendingGrads(*f, t["T"], t["hr"], *chain), keep


def _upd_bwd(route, t, dev, s):
    """-> {name: tensor} of what the backward of this form writes, on the saved tensors `s` of the device's forward."""
    wd, g = _weights_on(t["w"], dev), _graph_on(t["graph"], dev)
    N, T, H = t["N"], t["T"], t["H"]
    gx1, gvec1 = _nan(dev, N, H), _nan(dev, N, 3, H)
    gxo, gvo = t["gxo"].to(dev), t["gvo"].to(dev)       # (held in names until the launch is enqueued)
    tile = 16 if route.tr == 16 else 0
    ws = (wd.wx2tf16, wd.wx0tf16, wd.wvtf16) if tile == 16 else (wd.wx2tf, wd.wx0tf, wd.wvtf)
    tail = (P(s["vp"]), P(s["h2b"]), P(s["q23"]), P(s["nrm"]), P(ws[0]), P(ws[1]), P(ws[2]), P(g.row_active), P(g.type_rowptr),
            g.rowptr_c, P(gx1), P(gvec1), N, T, H)
    lib = _lib.load()
    out = {"gx1": gx1, "gvec1": gvec1}
    if route.form == "last":
        _ok(lib.hermnet_node_update_bwd_last(P(gxo), *tail, None, _stream()))
    elif route.form in ("held", "fused"):
        pend, keep = _pending(t, dev, route.form == "fused")
        out["gxo"], out["gvo"] = _nan(dev, N, H), _nan(dev, N, 3, H)
        _ok(getattr(lib, route.entry)(P(out["gxo"]), P(out["gvo"]), *tail, 16, ctypes.byref(pend), _stream()))
        torch.cuda.synchronize()
        del keep
    else:
        _ok(lib.hermnet_node_update_bwd(P(gxo), P(gvo), *tail, tile, None, _stream()))
    return out


# ---- one case of one instance -----------------------------------------------------------------------------------------------------------
def _run_case(route, ref, what, profile_only=False):
    """The instance's launch on one case, judged -> {output: (deciding share, worst err / bound)}.  `profile_only`: the launch
    alone (its forward, where a backward needs one, in front of it), as a callable for the profiler."""
    dev, t = _dev(), ref.t
    with _options(route):
        if route.family == "pre":
            if route.direction == "fwd":
                if profile_only:
                    return lambda: _pre_fwd(route, t, dev)
                got = cr.pre_fwd_outputs(*_pre_fwd(route, t, dev), t["x"])
            else:
                saved = _pre_fwd(route, t, dev)
                if profile_only:
                    return lambda: _pre_bwd(route, t, dev, saved)
                got = _pre_bwd(route, t, dev, saved)
            torch.cuda.synchronize()
            return cr.judge_outputs(got, ref, what)
        if route.direction == "fwd":
            if profile_only:
                return lambda: _upd_fwd(route, t, dev)
            o = _upd_fwd(route, t, dev)
            torch.cuda.synchronize()
            return _judge_upd_fwd(route, ref, o, what)
        s = _upd_fwd(route, t, dev, form="last" if route.form == "last" else "plain")
        if profile_only:
            return lambda: _upd_bwd(route, t, dev, s)
        o = _upd_bwd(route, t, dev, s)
        torch.cuda.synchronize()
    return _judge_upd_bwd(route, ref, o, s, what)


def _judge_upd_fwd(route, ref, o, what):
    t, H = ref.t, ref.t["H"]
    names = ["xo", "vo", "vp", "h2b", "q23", "nrm"]
    r64, r32 = ref.r64, ref.r32
    if route.form == "last":        # no vec_out; of q23 only the q half is written
        names.remove("vo")
        o = dict(o, q23=o["q23"][:, :H])
        r64, r32 = (dict(r, **{"upd_fwd:q23": r["upd_fwd:q23"][:, :H]}) for r in (r64, r32))
    figures = cr.judge_outputs({"upd_fwd:" + n: o[n] for n in names}, ref, what, r64, r32)
    if "next" in o:                 # the next layer's projection of the x_out this launch produced
        xo = o["xo"].cpu()
        nxt = [cr.pre_fwd_outputs(*ref_ops.node_pre_fwd(c(xo), t["w_other"], t["T"]), xo) for c in (lambda v: v.double(), lambda v: v.clone())]
        got = cr.pre_fwd_outputs(*o["next"], xo)
        rename = lambda d: {k.replace("pre_fwd", "next_fwd"): v for k, v in d.items()}
        figures.update(cr.judge_outputs(rename(got), ref, what, rename(nxt[0]), rename(nxt[1])))
    return figures


def _own_saved(t, s, gvo_zero):
    """The update backward's restatements in float64 and float32 on the DEVICE's saved tensors `s` (what the contract leaves
    unwritten -- rows of unknown elements, the r half of the last-layer form's q23 -- as zeros: it is not read)."""
    saved = [torch.nan_to_num(s[n].cpu()) for n in ("vp", "h2b", "q23", "nrm")]
    out = []
    for c in (lambda v: v.double(), lambda v: v.clone()):
        gvo = c(t["gvo"])
        out.append(cr.upd_bwd_ref(t, c(t["gxo"]), torch.zeros_like(gvo) if gvo_zero else gvo, tuple(c(v) for v in saved)))
    return out


def _judge_upd_bwd(route, ref, o, s, what):
    """gx1 / gvec1 of a backward.  Asserted in every case: the row rule against the restatements on the device's own saved
    tensors `s` -- the backward kernel alone.  Asserted on the plain and hostile sets as well: the row rule against the
    restatements that read their own (float64, float32) saved tensors.  On the scaled set that second form is printed, not
    asserted: there it measures the FORWARD.  Measured on the MI355X, node_update_bwd_wide_kernel<512>, n333 scaled, gx1 of row
    70: 1.48e-04 off the float64 backward on float64 saved tensors (bound 2.1e-05), 7.6e-07 off the float64 backward on the
    device's saved tensors (bound 5e-06) -- and the float64 backward itself moves by 1.48e-04 when it reads the device's saved
    tensors instead: the forward's rounding of vp, inside its own row bound, through the cancelling vec_dot of that row.  Three
    rows at 512 and one at 448 are over that way (6.9 x and 1.4 x), none in the form asserted (worst 0.34)."""
    t = ref.t
    if route.form in ("plain", "last"):
        tag = "upd_bwd" if route.form == "plain" else "last_bwd"
        got = {"upd_bwd:gx1": o["gx1"], "upd_bwd:gvec1": o["gvec1"]}
        own64, own32 = _own_saved(t, s, route.form == "last")
        figures = cr.judge_outputs(got, ref, what + " (device's saved tensors)", own64, own32)
        both = [{k: r[k.replace("upd_bwd", tag)] for k in got} for r in (ref.r64, ref.r32)]
        if ref.key[-1] != "scaled":
            cr.judge_outputs(got, ref, what + " (float64 saved tensors)", *both)
        else:
            for nm, a in got.items():
                e = row_err(a, both[0][nm]) / torch.maximum(torch.full((a.shape[0],), cr.BWD, dtype=torch.float64), 8.0 * row_err(both[1][nm], both[0][nm]))
                print("rows %s %s against float64 saved tensors (not asserted): worst err/bound %.3f, %d rows over" % (what, nm, float(e.max()), int((e > 1).sum())))
        return figures
    # held / fused: the sums the launch forms, then the update backward on the device's own gx_out
    tag, nk = route.form, t["nk"]
    got = {tag + ":gxo": o["gxo"]}
    if route.form == "held":
        assert bool(torch.isnan(o["gvo"]).all())                  # gvec_out is left alone
    else:
        got[tag + ":gvo"] = o["gvo"]
    figures = cr.judge_outputs(got, ref, what)
    gxo = o["gxo"].cpu()
    gxo[nk:] = 0.0                                                # (rows of unknown elements: not filled, not read)
    gvo = {torch.float64: ref.r64[tag + ":gvo"], torch.float32: ref.r32[tag + ":gvo"]}
    if route.form == "fused":
        dgvo = o["gvo"].cpu()
        dgvo[nk:] = 0.0
        gvo = {torch.float64: dgvo.double(), torch.float32: dgvo}
    second = []
    for dt, r in ((torch.float64, ref.r64), (torch.float32, ref.r32)):
        saved = tuple(r["upd_fwd:" + n] for n in ("vp", "h2b", "q23", "nrm"))
        second.append(cr.upd_bwd_ref(t, gxo.to(dt), gvo[dt], saved))
    figures.update(cr.judge_outputs({"upd_bwd:gx1": o["gx1"], "upd_bwd:gvec1": o["gvec1"]}, ref, what, second[0], second[1]))
    return figures


def _report(key, case, figures, ref):
    for k, (share, worst) in sorted(cr.worst_by_kernel(figures, {}).items()):
        print("rows %-36s %-9s %-8s hr=%-3d %-9s worst err/bound %.3f  deciding share %.3f" % ((key,) + case + (k, worst, share)))


def _case_id(case):
    return "%s-%s-%d" % case


CASES = [pytest.param(key, case, id="%s-%s" % (key, _case_id(case))) for key in cr.NODE_KEYS for case in cr.cases(cr.ROUTES[key])]
TILE64_KEYS = ("node_update_fwd_kernel128,64,1", "node_update_bwd_kernel128,64,1")


@pytest.mark.parametrize("key,case", CASES)
def test_chain_kernels_row_by_row(key, case):
    """Every node_* instance of the ledger on every layout of its tile height with the plain and the hostile operands, on n333 /
    N = 333 with the scaled ones, and on its padded widths.
    Measured on the MI355X, worst err / bound over all cases of a family, by width 64 / 128 / 192 / 256 / 320 / 384 / 448 / 512:
      node_pre_fwd 0.30 / 0.39 / - / 0.54, its wide form - / 0.25 / 0.24 / 0.39 / 0.39 / 0.36 / 0.44 / 0.50, 16-row form 0.37;
      node_pre_bwd (parts and gx) 0.17 / 0.23 / - / 0.33, wide - / 0.28 / 0.24 / 0.33 / 0.30 / 0.34 / 0.34 / 0.36, 16-row 0.21;
      node_update_fwd 0.29 / 0.35 (both tile heights) / - / 0.37, wide - / 0.35 / 0.35 / 0.37 / 0.49 / 0.48 / 0.85 / 0.60,
        16-row forms 0.32, the fused form's projection 0.51;
      node_update_bwd 0.15 / 0.21 / - / 0.26, wide - / 0.18 / 0.24 / 0.26 / 0.27 / 0.33 / 0.33 / 0.37, 16-row forms 0.89 (plain,
        last layer, and the second stage of the fused form), the sums the fused form builds 0.17.
    The 64-row instances at width 128, which no test had run: forward 0.35, backward 0.21.  Deciding shares (printed per case):
    0.2 .. 1.0 on the forward outputs, up to 0.16 on the update backward's, as tests/test_chain_reference.py derives."""
    route = cr.ROUTES[key]
    ref = cr.case_reference(route, case)
    _report(key, case, _run_case(route, ref, "%s %s" % (key, _case_id(case))), ref)


@pytest.mark.parametrize("case", cr.cases(cr.HELD), ids=_case_id)
def test_held_form_row_by_row(case):
    """hermnet_node_update_bwd_held: the second route to node_update_bwd16_kernel<128, false, false> -- `pending` in its gn_parts
    form, gvec_out neither read nor written (it stays NaN).
    Measured on the MI355X, worst err / bound: the gx_out it forms 0.05, gx1 / gvec1 0.61."""
    ref = cr.case_reference(cr.HELD, case)
    _report("held", case, _run_case(cr.HELD, ref, "held %s" % _case_id(case)), ref)


# ---- which kernel ran -------------------------------------------------------------------------------------------------------------------
def _key_of(name):
    """The CHAIN_KERNEL_BUDGETS key of a device kernel name as the profiler reports it (mangled, or demangled with or without
    its argument list), None for anything that is not a chain kernel."""
    if name.startswith("_Z"):
        m = re.match(r"_ZN12_GLOBAL__N_1\d+(\w+?_kernel)", name)
        return _chain_kernel_key(name) if m else None
    m = re.search(r"(\w+_kernel)(?:<([^>]*)>)?", name)
    if not m:
        return None
    base, targs = m.group(1), [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    bools = {"false": "b0", "true": "b1", "(bool)0": "b0", "(bool)1": "b1"}
    if re.match(r"node_update_(fwd|bwd)16_kernel", base):
        targs = targs[:1] + [bools.get(a, "b" + a) for a in targs[1:]] + ["b0"] * (3 - len(targs))
    return base + ",".join(bools.get(a, a) for a in targs)


def test_kernel_names_normalise_to_the_budget_keys():
    for name, key in (("void (anonymous namespace)::node_update_fwd_kernel<128, 64, 1>(hn_chain::UpdFwdArgs)", "node_update_fwd_kernel128,64,1"),
                      ("(anonymous namespace)::node_update_bwd16_kernel<128, true, false>(hn_chain::UpdBwdArgs)", "node_update_bwd16_kernel128,b1,b0"),
                      ("void (anonymous namespace)::node_update_fwd16_kernel<128, (bool)0, (bool)1>(...)", "node_update_fwd16_kernel128,b0,b1"),
                      ("(anonymous namespace)::layernorm_bwd_parts_kernel(float const*, int)", "layernorm_bwd_parts_kernel"),
                      ("_ZN12_GLOBAL__N_124node_update_fwd16_kernelILi128ELb0ELb1EEEvN8hn_chain10UpdFwdArgsENS1_10PreFwdArgsE", "node_update_fwd16_kernel128,b0,b1"),
                      ("void (anonymous namespace)::node_pre_fwd_wide_kernel<320>(hn_chain::PreFwdArgs)", "node_pre_fwd_wide_kernel320")):
        assert _key_of(name) == key and key in ALL_KEYS, (name, _key_of(name))
    assert _key_of("void at::native::vectorized_elementwise_kernel<4, ...>") not in ALL_KEYS


def test_the_intended_instance_runs():
    """Every ledger route once, one after the other, in ONE torch.profiler session (as tests/test_pimd_device.py takes its
    device activity): the chain kernels among the device events, in the order they started, are exactly the intended instances in
    the order of the routes (behind a hermnet_node_pre_bwd with a gx also layernorm_bwd_parts_kernel) -- each instance ran where
    it was meant to and no other chain kernel did.  A dispatch change that turns the row cases into a test of another kernel
    fails here."""
    from torch.profiler import ProfilerActivity, profile
    keys = sorted(cr.ROUTES) + ["held"]
    launches, expect = [], []
    for key in keys:
        route = cr.HELD if key == "held" else cr.ROUTES[key]
        want = "node_update_bwd16_kernel128,b0,b0" if key == "held" else key
        ref = cr.case_reference(route, cr.cases(route)[0])
        launch = _run_case(route, ref, key, profile_only=True)
        with _options(route):
            launch()                                # (a kernel's first launch opts in to its LDS size: outside the profile)
        launches.append((route, launch))
        if route.entry == "hermnet_node_pre_bwd":   # (the ledger reaches the LayerNorm backward behind the base kernel of width 128)
            expect.append(["node_pre_bwd_kernel128,64" if key == "layernorm_bwd_parts_kernel" else want, "layernorm_bwd_parts_kernel"])
        else:
            expect.append([want])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for route, launch in launches:
            with _options(route):
                launch()
            torch.cuda.synchronize()
    device = sorted((ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA), key=lambda ev: ev.time_range.start)
    assert device, "the profiler recorded no device activity"
    ran = [k for k in (_key_of(ev.name) for ev in device) if k in ALL_KEYS]
    at = 0
    for key, want in zip(keys, expect):
        got = ran[at:at + len(want)]
        print("instance %-40s ran: %s" % (key, ", ".join(got)))
        assert got == want, (key, got, want)
        at += len(want)
    assert at == len(ran), ran[at:]
    assert {k for k in ran if k.startswith("node_")} == set(cr.NODE_KEYS)
