"""CPU: the instance ledger, the cases, the references and the judging rules that tests/test_chain_rows.py holds the node chain
kernels (csrc/node_chain.hip, node_chain_wide.hip, node_chain16.hip) to, built here so that both files see the same ones --
and the checks of those rules themselves.

Ledger.  LEDGER maps every key of test_cabi_cpu.CHAIN_KERNEL_BUDGETS (53 kernels in three units) to a Route -- the C entry
point, the width, the `tile_rows` argument, the library options and the form (plain; fused boundary; last layer; held) through
which tests/test_chain_rows.py reaches that instance -- or, for the two energy_head16 kernels, to the node id of the test that
already judges them row by row against float64.  50 of the 53 are node_* kernels; layernorm_bwd_parts_kernel runs behind
every hermnet_node_pre_bwd with a gx and is judged here through it (the output "pre_bwd:gx").

Row layouts are a function of the instance's tile height TR (T = 3 but for "t1"); every one asserts what it is meant to be.
  update kernels (tiles cut per relation block):  ragged (TR + 1, TR, 1 rows + 5 of an unknown element), empty (TR + 4, 0, 9),
      inactive (2 TR + 8 rows in relation 0: one row off in its first tile, one in its last, its middle tile entirely off),
      uniform (equal blocks of TR + 4 with inert padding rows), n333 (333 random species incl. an unknown one), t1 (T = 1, 2 TR + 1).
  pre kernels (tiles cut over all rows): N = 1, TR, TR + 1, 333.
Operand sets.  "plain": unit normal.  "hostile": unit normal with up to three rows replaced -- 1e3 + noise on the first row of a
tile, 1e-20 x noise on row TR - 1 of a tile, a constant on the first row of the ragged last tile -- in every operand; a case
takes as many of the three as CAP of its live rows allows, the ragged row first (`_hostile_positions`).  "scaled": on n333 /
N = 333 only, the per-row scales of test_node_chain_kernels_on_adversarial_operands, rows at 1e-30 in the linear backward chain
included.  Padded widths: hidden_real = H - 28 at every H >= 128 (cuts the last 32-channel block), H - 36 at 192 / 320 / 448
(leaves it entirely padded), 50 at 64; weights through LayerWeights.refresh(); operands zero in the padded channels.

Judging.  Every output row by row (helpers.judge_rows) against the restatements of tests/ref_ops.py in float64, the same in
float32 as base: err <= max(floor, 8 x base).  Floors: 2e-6 projection forward, 3e-6 update forward and saved tensors, 5e-6 both
backwards.  [T, N, .] arrays per (t, row); saved tensors on the active rows of known elements; rows of unknown elements and
inactive rows exactly zero (their float64 rows are zero); padded channels exactly zero in everything handed on (nrm, which is
1e-4 there, and the per-relation partial sums excepted).  The LayerNorm mean is judged as [mean, max |x|] (a number has no
scale but itself: tests/test_stage_reference.py).  Every kernel is judged on its own: a backward reads the device's saved
tensors while its reference reads the float64 ones; the second stage of a fused launch is referred to the restatement of that
stage on the device's own first-stage result (test_chain_rows).

Checks here.  (a) Cap (test_message_reference.CAP = 0.10, not raised).  The share of live rows on which 8 x base, not the floor,
is the bound depends on the two restatements alone.  For the LayerNorm statistics it is at most CAP on the plain and on the
hostile set.  For every other output here -- each is a matrix product over K = 64 .. 1536 terms -- it is NOT, and no choice of
rows makes it so: a float32 dot product of K unit-normal terms is by itself about sqrt(K) 2^-24 of the row's scale off, 8 x that
is 4e-7 .. 2e-6 against floors of 2e-6 .. 5e-6, and on the PLAIN set the share measured here is 0.2 .. 1.0 forward and
0.07 .. 1.0 backward (tests/test_stage_reference.py exempts its read-out, x W0^T, for the same reason).  What the cap is for
still holds and is asserted: the hostile set is the plain set of the same case with at most CAP of its live rows replaced,
so its share may exceed the plain set's by at most CAP -- enlarging the hostile rows past that fails here.  Outputs of fewer
than ten live rows are left out.  The scaled set is exempt: a seventh of its rows are 1e3 + noise on purpose; all shares are
printed.  (b) Sensitivity: four mutants of the fp32 restatement, per family (pre_fwd, pre_bwd, upd_fwd, upd_bwd).
Measured here (err / bound of the worst row of the mutant; > 1 fails):
  rows TR - 1 and TR swapped: fails in every family (1e5 and more);
  one 32-channel block of the ragged row zeroed: fails in every family (1e5 and more);
  LayerNorm statistics over `hidden` on a padded width (the families with a LayerNorm: pre_fwd, pre_bwd): fails, 2e4 and more;
  smallest bf16 plane of one weight dropped, scaled set: see test_the_two_plane_mutant_on_the_scaled_set's docstring."""
import copy
import hashlib
import math
from collections import namedtuple
from types import SimpleNamespace

import pytest
import torch

from helpers import judge_rows, FLT_MIN
import ref_ops
from test_cabi_cpu import CHAIN_KERNEL_BUDGETS
from test_message_reference import CAP

PRE_FWD, UPD_FWD, BWD = 2e-6, 3e-6, 5e-6
Z_LIST = [13, 28, 29]
WIDE_WIDTHS = (128, 192, 256, 320, 384, 448, 512)
_CACHE = {}

# entry: the C entry point; tile_rows: its argument (None: it has none); options: _lib.options(**options) around the call;
# form: plain | fused | last | held; family / direction: which outputs the instance writes; tr: rows per tile (the layouts)
Route = namedtuple("Route", "entry width tile_rows options form family direction tr")
HEAD_TEST = "tests/test_stage_rows.py::test_read_out_forms_row_by_row"
TILE64, WIDE = dict(update_tile64_max=10 ** 6), dict(node_chain_wide=1)


def _ledger():
    led = {"node_chain.hip": {}, "node_chain16.hip": {}, "node_chain_wide.hip": {}}
    base = led["node_chain.hip"]
    for H, tr in ((64, 64), (128, 64), (256, 32)):
        base["node_pre_fwd_kernel%d,%d" % (H, tr)] = Route("hermnet_node_pre_fwd", H, None, {}, "plain", "pre", "fwd", tr)
        base["node_pre_bwd_kernel%d,%d" % (H, tr)] = Route("hermnet_node_pre_bwd", H, None, {}, "plain", "pre", "bwd", tr)
    for H, tr, minw, opts in ((64, 64, 2, {}), (128, 32, 2, {}), (128, 64, 1, TILE64), (256, 32, 1, {})):
        base["node_update_fwd_kernel%d,%d,%d" % (H, tr, minw)] = Route("hermnet_node_update_fwd", H, 0, opts, "plain", "upd", "fwd", tr)
        base["node_update_bwd_kernel%d,%d,%d" % (H, tr, minw)] = Route("hermnet_node_update_bwd", H, 0, opts, "plain", "upd", "bwd", tr)
    # behind every hermnet_node_pre_bwd with a gx: judged through "pre_bwd:gx" of the base kernel's cases at width 128
    base["layernorm_bwd_parts_kernel"] = Route("hermnet_node_pre_bwd", 128, None, {}, "plain", "pre", "bwd", 64)
    k16 = led["node_chain16.hip"]
    k16["node_pre_fwd16_kernel128"] = Route("hermnet_node_pre_fwd16", 128, None, {}, "plain", "pre", "fwd", 16)
    k16["node_pre_bwd16_kernel128"] = Route("hermnet_node_pre_bwd16", 128, None, {}, "plain", "pre", "bwd", 16)
    k16["node_update_fwd16_kernel128,b0,b0"] = Route("hermnet_node_update_fwd", 128, 16, {}, "plain", "upd", "fwd", 16)
    k16["node_update_fwd16_kernel128,b0,b1"] = Route("hermnet_node_update_fwd_last", 128, None, {}, "last", "upd", "fwd", 16)
    k16["node_update_fwd16_kernel128,b1,b0"] = Route("hermnet_node_update_pre_fwd", 128, None, {}, "fused", "upd", "fwd", 16)
    k16["node_update_bwd16_kernel128,b0,b0"] = Route("hermnet_node_update_bwd", 128, 16, {}, "plain", "upd", "bwd", 16)
    k16["node_update_bwd16_kernel128,b0,b1"] = Route("hermnet_node_update_bwd_last", 128, None, {}, "last", "upd", "bwd", 16)
    k16["node_update_bwd16_kernel128,b1,b0"] = Route("hermnet_node_update_bwd", 128, 16, {}, "fused", "upd", "bwd", 16)
    k16["energy_head16_fwd_kernel128,64"] = k16["energy_head16_bwd_kernel128,64"] = HEAD_TEST
    wide = led["node_chain_wide.hip"]
    for H in WIDE_WIDTHS:
        opts = WIDE if H in (128, 256) else {}
        wide["node_pre_fwd_wide_kernel%d" % H] = Route("hermnet_node_pre_fwd", H, None, opts, "plain", "pre", "fwd", 32)
        wide["node_pre_bwd_wide_kernel%d" % H] = Route("hermnet_node_pre_bwd", H, None, opts, "plain", "pre", "bwd", 32)
        wide["node_update_fwd_wide_kernel%d" % H] = Route("hermnet_node_update_fwd", H, 0, opts, "plain", "upd", "fwd", 32)
        wide["node_update_bwd_wide_kernel%d" % H] = Route("hermnet_node_update_bwd", H, 0, opts, "plain", "upd", "bwd", 32)
    return led


LEDGER = _ledger()
# The 16-row update backward in its plain instance also serves hermnet_node_update_bwd_held (`pending` in its gn_parts form,
# gvec_out kept on chip): a second route to the same kernel, with cases of its own in tests/test_chain_rows.py
HELD = Route("hermnet_node_update_bwd_held", 128, 16, {}, "held", "upd", "bwd", 16)
ROUTES = {key: r for unit in LEDGER.values() for key, r in unit.items() if isinstance(r, Route)}
NODE_KEYS = sorted(k for k in ROUTES if k.startswith("node_"))


def _gen(*key):
    return torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:4], "little"))


def padded_widths(H):
    """The hidden_real values a width is run at besides 0 (= no padding)."""
    if H == 64:
        return (50,)
    return (H - 28, H - 36) if H in (192, 320, 448) else (H - 28,)


# ---- weights ----------------------------------------------------------------------------------------------------------------
def weights(H, hr, T=3, seed=0):
    """LayerWeights of T randomly initialised PaiNNModules of hidden_channels = hr or H (std 0.3 up to width 128,
    0.3 sqrt(128 / H) beyond: pre-activations of order one at every width), padded to H by refresh()."""
    key = ("w", H, hr, T, seed)
    if key not in _CACHE:
        from hermnet_amd.layer import LayerWeights
        from hermnet_amd.rmnet import PaiNNModule
        torch.manual_seed(1000 * seed + H + (hr or 0))
        mods = [PaiNNModule(hidden_channels=hr or H, num_rbf=16) for _ in range(3)][:T]
        for m in mods:
            for p in m.parameters():
                p.data.normal_(0, 0.3 * min(1.0, math.sqrt(128.0 / H)))
        w = LayerWeights(mods).refresh()
        assert w.h_real == (hr or 0) and w.w1cat.size(1) == H and w.chain
        _CACHE[key] = w
    return _CACHE[key]


# ---- row layouts --------------------------------------------------------------------------------------------------------------
UPD_LAYOUTS = ("ragged", "empty", "inactive", "uniform", "n333", "t1")
PRE_LAYOUTS = ("N1", "NTR", "NTR+1", "N333")


def pre_rows(kind, TR):
    return {"N1": 1, "NTR": TR, "NTR+1": TR + 1, "N333": 333}[kind]


def layout(kind, TR):
    """The CPU RelationalGraph of an update layout (every atom has an incoming edge: every non-empty relation runs)."""
    key = ("layout", kind, TR)
    if key in _CACHE:
        return _CACHE[key]
    from hermnet_amd.relations import RelationalGraph
    gen = _gen(*key)
    T = 1 if kind == "t1" else 3
    if kind == "n333":
        z, uniform = torch.tensor(Z_LIST + [1])[torch.randint(0, T + 1, (333,), generator=gen)], None
    else:
        counts, unknown, uniform = {"ragged": ((TR + 1, TR, 1), 5, False), "empty": ((TR + 4, 0, 9), 0, False),
                                    "inactive": ((2 * TR + 8, 20, 7), 2, False), "uniform": ((TR + 4, TR - 3, 9), 3, True),
                                    "t1": ((2 * TR + 1,), 2, None)}[kind]
        z = torch.cat([torch.full((c,), Z_LIST[t]) for t, c in enumerate(counts)] + [torch.full((unknown,), 1)])
        z = z[torch.randperm(z.numel(), generator=gen)]
    n = z.numel()
    ei = torch.stack([torch.randint(0, n, (4 * n,), generator=gen), torch.cat([torch.arange(n), torch.randint(0, n, (3 * n,), generator=gen)])])
    g = RelationalGraph.build(z, ei, Z_LIST[:T], uniform=uniform)
    rp = list(g.type_rowptr_host)
    blocks = [rp[t + 1] - rp[t] for t in range(T)]
    if kind == "ragged":        # a full tile and a one-row tile in relation 0, an exactly full tile, a one-row relation, zero tiles
        assert blocks == [TR + 1, TR, 1] and g.N - rp[T] == 5 and not g.uniform and bool((g.row_active[:rp[T]] == 1).all())
    if kind == "empty":
        assert blocks == [TR + 4, 0, 9] and g.N == rp[T]
    if kind == "inactive":      # zeros inside the first and the last tile of relation 0, its middle tile entirely off
        assert blocks[0] == 2 * TR + 8 and not g.uniform
        g.row_active[[3, 2 * TR + 1]] = 0.0
        g.row_active[TR:2 * TR] = 0.0
    if kind == "uniform":       # equal blocks that no tile height divides, their tails inert
        assert g.uniform and g.block == TR + 4 and blocks == [TR + 4] * 3 and int((g.row_active[:rp[T]] == 0).sum()) == TR + 2
    if kind == "n333":
        assert g.N >= 333 and g.N - rp[T] > 0 and min(blocks) > TR
    if kind == "t1":
        assert g.T == 1 and blocks == [2 * TR + 1] and g.N - rp[1] == 2
    _CACHE[key] = g
    return g


def _hostile_positions(blocks, TR, live):
    """[(row, kind)] of the hostile rows: in the first block of more than TR rows with a ragged last tile, the first row of that
    tile ("const"), row TR - 1 of the first tile ("tiny") and the block's first row ("big") -- as many of them, in this order,
    as CAP of the `live` rows allows (an output of fewer than ten rows takes none)."""
    for lo, n in blocks:
        if n > TR and n % TR:
            want = [(lo + n // TR * TR, "const"), (lo + TR - 1, "tiny"), (lo, "big")]
            return want[:int(CAP * live)]
    for lo, n in blocks:
        if n >= TR:
            return [(lo + TR - 1, "tiny"), (lo, "big")][:int(CAP * live)]
    return []


def _hostile(t, positions, gen, chan):
    for row, kind in positions:
        if kind == "big":
            t[row] = (1.0e3 + torch.randn(t[row].shape, generator=gen)) * chan
        elif kind == "tiny":
            t[row] = 1.0e-20 * torch.randn(t[row].shape, generator=gen) * chan
        else:
            t[row] = 0.37 * chan
    return t


def _scales(n, lo, hi, gen):
    return 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen))


def _chan(H, hr):
    return (torch.arange(H) < (hr or H)).float()


# ---- the projection chain: LayerNorm + x_proj, and its backward ----------------------------------------------------------------
def pre_inputs(H, hr, TR, kind, opset):
    gen = _gen("pre", H, hr, TR, kind)                 # (the hostile set IS the plain one but for its replaced rows)
    N, T, chan = pre_rows(kind, TR), 3, _chan(H, hr)
    rnd = lambda *s: torch.randn(*s, generator=gen) * chan.repeat(s[-1] // H)
    x, gxh, add = rnd(N, H), rnd(T, N, 3 * H) * 0.3, rnd(N, H)
    gen = _gen("pre", H, hr, TR, kind, opset)
    pos = []
    if opset == "hostile":
        pos = _hostile_positions([(0, N)], TR, N)
        x, add = _hostile(x, pos, gen, chan), _hostile(add, pos, gen, chan)
        gxh = _hostile(gxh.transpose(0, 1).contiguous(), pos, gen, chan.repeat(3)).transpose(0, 1).contiguous()
    if opset == "scaled":
        sx, sg = _scales(N, -12, 12, gen), _scales(N, -12, 12, gen)
        x = x * sx[:, None]
        x[::7] = (1.0e3 + torch.randn(x[::7].shape, generator=gen)) * chan
        gxh = gxh * sg[None, :, None]
        gxh[:, ::9] = rnd(T, gxh[:, ::9].shape[1], 3 * H) * 1.0e-30
        sg[::9] = 1.0e-30
        rstd = 1.0 / torch.sqrt(x[:, :hr or H].double().var(1, unbiased=False) + 1e-5)
        add = add * (sg.double() * rstd).float()[:, None]            # at the scale of the gradient it joins
    return dict(H=H, hr=hr, TR=TR, N=N, T=T, x=x, gxh=gxh, add=add, hostile=pos, w=weights(H, hr))


def pre_fwd_outputs(hb, xh, mean, rstd, x):
    T, N = hb.shape[:2]
    return {"pre_fwd:hb": hb.reshape(T * N, -1), "pre_fwd:xh": xh.reshape(T * N, -1),
            "pre_fwd:mean": torch.stack([mean.detach().cpu().double(), x.detach().cpu().double().abs().amax(1)], 1),
            "pre_fwd:rstd": rstd[:, None]}


def pre_run(c, t, w=None):
    """The projection and its backward through ref_ops on the inputs `t` converted by `c`; the backward reads this run's hb."""
    w = w or t["w"]
    x, gxh, add, T = c(t["x"]), c(t["gxh"]), c(t["add"]), t["T"]
    hb, xh, mean, rstd = ref_ops.node_pre_fwd(x, w, T)
    out = pre_fwd_outputs(hb, xh, mean, rstd, t["x"])
    parts = ref_ops.node_pre_bwd(gxh, hb, x, mean, rstd, w, parts_only=True)
    out["pre_bwd:parts"] = parts.reshape(T * t["N"], -1)
    out["pre_bwd:gx"] = ref_ops.layernorm_bwd(parts.sum(0), x, mean, rstd, add=add, h_real=w.h_real)
    return out


# ---- the update chain ---------------------------------------------------------------------------------------------------------
def upd_inputs(H, hr, TR, kind, opset):
    gen = _gen("upd", H, hr, TR, kind)                 # (the hostile set IS the plain one but for its replaced rows)
    g, chan = layout(kind, TR), _chan(H, hr)
    N, T, rp = g.N, g.T, list(g.type_rowptr_host)
    rnd = lambda *s: torch.randn(*s, generator=gen) * chan.repeat(s[-1] // H)
    x1, vec1, gxo, gvo = rnd(N, H), rnd(N, 3, H), rnd(N, H), rnd(N, 3, H)
    gen = _gen("upd", H, hr, TR, kind, opset)
    live = torch.zeros(N, dtype=torch.bool)
    live[:rp[T]] = g.row_active[:rp[T]] != 0
    pos = []
    if opset == "hostile":
        pos = _hostile_positions([(rp[t], rp[t + 1] - rp[t]) for t in range(T)], TR, int(live.sum()))
        assert all(bool(live[r]) for r, _ in pos)
        x1, vec1, gxo, gvo = (_hostile(v, pos, gen, chan) for v in (x1, vec1, gxo, gvo))
    if opset == "scaled":
        x1 = x1 * _scales(N, -6, 6, gen)[:, None]
        alt = torch.tensor([1.0, -1.0]).repeat(H // 2) * chan
        vec1 = vec1 * _scales(N, -6, 6, gen)[:, None, None]
        k = vec1[::5].shape[0]
        vec1[::5] = (alt[None, None, :] + 1e-3 * rnd(k, 3, H)) * _scales(k, -3, 3, gen)[:, None, None]
        gxo, gvo = gxo * _scales(N, -6, 6, gen)[:, None], gvo * _scales(N, -6, 6, gen)[:, None, None]
    t = dict(H=H, hr=hr, TR=TR, N=N, T=T, nk=rp[T], graph=g, live=live, x1=x1, vec1=vec1, gxo=gxo, gvo=gvo, hostile=pos,
             w=weights(H, hr, T))
    if H == 128 and TR == 16 and T == 3:
        # the layer above, for the forms of the 16-row kernels that take its gradients as partial sums (held: gn_parts;
        # fused: gxh, hb and its weights) and the layer below for the fused forward
        xa = _hostile(rnd(N, H), pos, gen, chan)
        _, mean, rstd = ref_ops.layernorm_fwd(xa.double(), 1e-5, h_real=hr)
        t.update(w_other=weights(H, hr, T, seed=1), xa=xa, mean_a=mean.float(), rstd_a=rstd.float(), hb_a=rnd(T, N, H),
                 gxh_a=rnd(T, N, 3 * H) * 0.3, gn_parts=rnd(T, N, H), gv_parts=rnd(T, N, 3, H),
                 gx1_a=_hostile(rnd(N, H), pos, gen, chan), gvec1_a=_hostile(rnd(N, 3, H), pos, gen, chan))
    return t


def pending_sums(c, t, gn):
    """What a pending update backward forms first: gx_out = LayerNorm'(x)^T (sum_t gn[t]) + gx1 / sqrt(2), gvec_out = sum_t
    gv[t] + gvec1 (the residual's identity terms on the rows of known elements only) -> (gxo, gvo) [N, ...]."""
    ident = c((torch.arange(t["N"]) < t["nk"]).float())
    gxo = ref_ops.layernorm_bwd(gn.sum(0), c(t["xa"]), c(t["mean_a"]), c(t["rstd_a"]),
                                add=c(t["gx1_a"]) * ident[:, None] / math.sqrt(2.0), h_real=t["hr"])
    return gxo, c(t["gv_parts"]).sum(0) + c(t["gvec1_a"]) * ident[:, None, None]


def upd_bwd_ref(t, gxo, gvo, saved, w=None):
    """ref_ops.node_update_bwd in the dtype of gxo on the saved tensors `saved` = (vp, h2b, q23, nrm)."""
    gx1, gvec1 = ref_ops.node_update_bwd(gxo, gvo, *saved, w or t["w"], t["graph"])
    return {"upd_bwd:gx1": gx1, "upd_bwd:gvec1": gvec1}


def upd_run(c, t, w=None):
    """The update and its backward through ref_ops on the inputs `t` converted by `c`; the backward reads this run's saved
    tensors.  At (H, TR) = (128, 16), T = 3 also what the 16-row forms add: the last-layer backward (gvec_out = 0) and the sums
    the pending forms hand to the update backward ("held:" from gn_parts, "fused:" through the projection's backward)."""
    w = w or t["w"]
    x1, vec1, gxo, gvo = c(t["x1"]), c(t["vec1"]), c(t["gxo"]), c(t["gvo"])
    xo, vo, vp, h2b, q23, nrm = ref_ops.node_update_fwd(x1, vec1, w, t["graph"])
    out = {"upd_fwd:xo": xo, "upd_fwd:vo": vo, "upd_fwd:vp": vp, "upd_fwd:h2b": h2b, "upd_fwd:q23": q23, "upd_fwd:nrm": nrm}
    out.update(upd_bwd_ref(t, gxo, gvo, (vp, h2b, q23, nrm), w))
    if t["H"] == 128 and t["TR"] == 16:
        last = upd_bwd_ref(t, gxo, torch.zeros_like(gvo), (vp, h2b, q23, nrm), w)
        out["last_bwd:gx1"], out["last_bwd:gvec1"] = last["upd_bwd:gx1"], last["upd_bwd:gvec1"]
    if "w_other" in t:
        out["held:gxo"], out["held:gvo"] = pending_sums(c, t, c(t["gn_parts"]))
        out["fused:gxo"], out["fused:gvo"] = pending_sums(c, t, ref_ops.node_pre_bwd16(c(t["gxh_a"]), c(t["hb_a"]), t["w_other"]))
    return out


FAMILIES = {"pre": (pre_inputs, pre_run), "upd": (upd_inputs, upd_run)}


def reference(family, H, hr, TR, kind, opset):
    """SimpleNamespace(t = inputs, r64, r32) of one case: computed once, shared by both files, never modified."""
    key = (family, H, hr, TR, kind, opset)
    if key not in _CACHE:
        inputs, run = FAMILIES[family]
        t = inputs(H, hr, TR, kind, opset)
        _CACHE[key] = SimpleNamespace(t=t, r64=run(lambda v: v.double(), t), r32=run(lambda v: v.clone(), t), key=key)
    return _CACHE[key]


def cases(route):
    """(layout, operand set, hidden_real) of every case of an instance: every layout of its tile height with both operand
    sets, the scaled set once, the padded widths on the layout with a ragged tile."""
    layouts = PRE_LAYOUTS if route.family == "pre" else UPD_LAYOUTS
    if route.form in ("fused", "held"):          # (the layer above / below is built for T = 3)
        layouts = tuple(k for k in layouts if k != "t1")
    out = [(kind, opset, 0) for kind in layouts for opset in ("plain", "hostile")]
    out.append((layouts[-1] if route.family == "pre" else "n333", "scaled", 0))
    edge = "NTR+1" if route.family == "pre" else "ragged"
    out += [(edge, opset, hr) for hr in padded_widths(route.width) for opset in ("plain", "hostile")]
    return out


def case_reference(route, case):
    kind, opset, hr = case
    return reference(route.family, route.width, hr, route.tr, kind, opset)


def all_references():
    """The distinct (family, H, hr, TR, layout, operand set) of every instance's cases."""
    keys = []
    for route in list(ROUTES.values()) + [HELD]:
        for kind, opset, hr in cases(route):
            k = (route.family, route.width, hr, route.tr, kind, opset)
            if k not in keys:
                keys.append(k)
    return keys


def ref_id(key):
    return "-".join(str(v) for v in key)


# ---- judging ----------------------------------------------------------------------------------------------------------------------
def floor_of(name):
    head = name.split(":")[0]
    return PRE_FWD if head in ("pre_fwd", "next_fwd") else UPD_FWD if head == "upd_fwd" else BWD


SAVED = ("upd_fwd:vp", "upd_fwd:h2b", "upd_fwd:q23", "upd_fwd:nrm")
KNOWN_ROWS = ("held:gxo", "held:gvo", "fused:gxo", "fused:gvo")       # filled on the rows below type_rowptr[T]
NOT_ZERO_PADDED = ("upd_fwd:nrm", "pre_bwd:parts", "pre_fwd:mean", "pre_fwd:rstd", "next_fwd:mean", "next_fwd:rstd")


def _rows(name, a, t):
    """The rows of output `name` that the contract defines."""
    if name in SAVED:
        return a[t["live"].to(a.device)]
    return a[:t["nk"]] if name in KNOWN_ROWS else a


def judge_outputs(got, ref, what, r64=None, r32=None):
    """Every output of `got` (a subset of the reference's names -> tensors) by the row rule -> {name: (deciding share, worst
    err / bound)}; on a padded width the padded channels of what is handed on must be exactly zero."""
    t, figures = ref.t, {}
    r64, r32 = r64 or ref.r64, r32 or ref.r32
    for nm, a in got.items():
        a, b64, b32 = (_rows(nm, v, t) for v in (a, r64[nm], r32[nm]))
        if a.shape[0] == 0:
            continue
        figures[nm] = judge_rows(a, b64, b32, floor_of(nm), "%s %s" % (what, nm), tiny=FLT_MIN)
        if t["hr"] and nm not in NOT_ZERO_PADDED:
            assert not bool(a.reshape(-1, t["H"])[:, t["hr"]:].any()), (what, nm, "padded channels")
    return figures


def live_rows(nm, ref):
    b = _rows(nm, ref.r64[nm], ref.t)
    return int((b.reshape(b.shape[0], -1).abs().amax(1) > 0).sum()) if b.shape[0] else 0


STATISTICS = ("pre_fwd:mean", "pre_fwd:rstd")      # the outputs that are no matrix product


def fp32_figures(key):
    """{output: (deciding share, worst err / bound)} of the fp32 restatement of a case, judged like a kernel."""
    k = ("fp32",) + tuple(key)
    if k not in _CACHE:
        ref = reference(*key)
        _CACHE[k] = judge_outputs(ref.r32, ref, "%s fp32" % ref_id(key))
    return _CACHE[k]


def check_cap(key):
    """(a), see the module docstring: the statistics by the absolute cap on both sets; every product output of the hostile set
    by its share on the plain set of the same case + CAP.  Outputs of fewer than ten live rows cannot tell 10 % from nothing
    and are left out."""
    opset, ref = key[-1], reference(*key)
    if opset == "scaled":
        return
    figures = fp32_figures(key)
    plain = fp32_figures(tuple(key[:-1]) + ("plain",))
    for nm, (share, _) in figures.items():
        if live_rows(nm, ref) < 10:
            continue
        if nm in STATISTICS:
            assert share <= CAP, (ref_id(key), nm, share)
        assert share <= plain[nm][0] + CAP, (ref_id(key), nm, share, plain[nm][0])


def worst_by_kernel(figures, into):
    """Fold {output: (share, worst)} into {kernel family: (largest share, largest worst)}: the name up to the ':'."""
    for nm, (share, worst) in figures.items():
        k = nm.split(":")[0]
        s, w = into.get(k, (0.0, 0.0))
        into[k] = (max(s, share), max(w, worst))
    return into


# ---- the ledger -------------------------------------------------------------------------------------------------------------------
def test_the_ledger_names_every_compiled_chain_kernel():
    """Unit by unit the ledger's keys are exactly CHAIN_KERNEL_BUDGETS' keys: a kernel instance added or renamed without a row
    case fails here.  53 kernels, 50 of them node_* kernels with a route of their own."""
    assert sorted(LEDGER) == sorted(CHAIN_KERNEL_BUDGETS)
    for unit, table in CHAIN_KERNEL_BUDGETS.items():
        assert sorted(LEDGER[unit]) == sorted(table), (unit, sorted(set(LEDGER[unit]) ^ set(table)))
    assert sum(len(u) for u in LEDGER.values()) == 53 and len(NODE_KEYS) == 50
    for unit in LEDGER.values():
        for key, r in unit.items():
            assert isinstance(r, Route) == (not key.startswith("energy_head16")), key


def test_routes_are_well_formed_and_existing_tests_exist():
    """Every route names an entry point of the C header, a supported width, a tile height its layouts are cut for and options the
    library knows; a kernel that points at an existing test names a test function that exists."""
    import importlib
    from hermnet_amd import _lib
    for key, r in list(ROUTES.items()) + [("held", HELD)]:
        assert r.entry in _lib.SIGNATURES, key
        assert r.width % 64 == 0 and 64 <= r.width <= 512 and r.tr in (16, 32, 64) and r.tile_rows in (None, 0, 16), key
        assert set(r.options) <= set(_lib.OPTIONS), key
        assert r.form in ("plain", "fused", "last", "held") and r.family in ("pre", "upd") and r.direction in ("fwd", "bwd"), key
        assert str(r.width) in key or key == "layernorm_bwd_parts_kernel" or key == "held", key
        assert len(cases(r)) >= 11
    for unit in LEDGER.values():
        for key, r in unit.items():
            if not isinstance(r, Route):
                path, name = r.split("::")
                mod = importlib.import_module(path[len("tests/"):-len(".py")])
                assert callable(getattr(mod, name)), r


def test_hostile_rows_meet_the_tile_edges():
    """Where the cap leaves room for all three, the hostile rows are the first row of a tile, row TR - 1 of it and the first row
    of the ragged last tile of the same block; a layout too small for three takes the ragged row first and never more than CAP
    of its live rows."""
    for TR in (16, 32, 64):
        t = reference("upd", 128 if TR != 64 else 64, 0, TR, "ragged", "hostile").t
        assert t["hostile"] == [(TR, "const"), (TR - 1, "tiny"), (0, "big")][:int(CAP * int(t["live"].sum()))]
        assert float(t["x1"][TR].min()) == float(t["x1"][TR].max()) == pytest.approx(0.37)
        for kind in UPD_LAYOUTS:
            t = reference("upd", 128 if TR != 64 else 64, 0, TR, kind, "hostile").t
            assert 1 <= len(t["hostile"]) <= CAP * int(t["live"].sum()), (TR, kind)
        assert pre_inputs(64, 0, TR, "N1", "hostile")["hostile"] == []
        assert pre_inputs(64, 0, TR, "NTR+1", "hostile")["hostile"][0] == (TR, "const")
    t = reference("upd", 128, 0, 32, "ragged", "hostile").t
    assert len(t["hostile"]) == 3 and float(t["vec1"][0].mean()) > 900.0 and float(t["gvo"][31].abs().max()) < 1e-18


# ---- (a) the cap ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", all_references(), ids=ref_id)
def test_the_floors_decide_under_the_fp32_restatement(key):
    """A condition on the INPUTS of tests/test_chain_rows.py: judged like a kernel, the fp32 restatement passes every case, and
    the hostile rows add at most CAP to the share of live rows on which 8 x base, not the floor, is the bound (`check_cap`;
    the module docstring says why the share itself cannot be capped for a matrix product)."""
    for k, (share, worst) in sorted(worst_by_kernel(fp32_figures(key), {}).items()):
        print("%s %-9s fp32 restatement: worst err/bound %.3f  deciding share %.3f" % (ref_id(key), k, worst, share))
    check_cap(key)


# ---- (b) sensitivity: mutants of the fp32 RESTATEMENT (never of a kernel) -------------------------------------------------------
MUTANT_FAMILIES = {"pre_fwd": ("pre", "pre_fwd:xh"), "pre_bwd": ("pre", "pre_bwd:gx"), "upd_fwd": ("upd", "upd_fwd:vo"),
                   "upd_bwd": ("upd", "upd_bwd:gvec1")}


def _verdict(got, ref, nm):
    """(fails, err / bound of the worst row) of one output under the row rule, unrestricted rows."""
    from helpers import row_err
    assert bool(torch.isfinite(got).all())
    a, b64, b32 = (_rows(nm, v, ref.t) for v in (got, ref.r64[nm], ref.r32[nm]))
    err, base = row_err(a, b64), row_err(b32, b64)
    ratio = float((err / torch.maximum(torch.full_like(err, floor_of(nm)), 8.0 * base)).max())
    try:
        judge_rows(a, b64, b32, floor_of(nm), nm, tiny=FLT_MIN)
    except AssertionError:
        return True, ratio
    return False, ratio


def _edge_case(fam, TR, hr=0):
    family, nm = MUTANT_FAMILIES[fam]
    # (the plain set: on the hostile one rows TR - 1 and TR of the projection are a tiny and a constant row, both of which
    # LayerNorm maps to n = 0 -- the same xh)
    return reference(family, 128, hr, TR, "NTR+1" if family == "pre" else "ragged", "plain"), nm


@pytest.mark.parametrize("TR", [16, 32, 64])
@pytest.mark.parametrize("fam", sorted(MUTANT_FAMILIES))
def test_mutants_at_the_tile_edge_fail(fam, TR):
    """Rows TR - 1 and TR swapped, and one 32-channel block of row TR (the ragged last tile's) zeroed: each fails the row rule on
    the ragged case of every family at every tile height; unmutated, the fp32 restatement passes."""
    ref, nm = _edge_case(fam, TR)
    per_t = ref.r32[nm].shape[0] // ref.t["N"] if ref.t["N"] else 1          # ([T, N, .] outputs: the rows of t = 0)
    assert per_t in (1, 3) and not _verdict(ref.r32[nm], ref, nm)[0]
    swapped = ref.r32[nm].clone()
    swapped[[TR - 1, TR]] = swapped[[TR, TR - 1]]
    block = ref.r32[nm].clone()
    block.reshape(block.shape[0], -1)[TR, 32:64] = 0.0
    for what, got in (("swapped", swapped), ("block", block)):
        fails, ratio = _verdict(got, ref, nm)
        print("mutant %-8s %-8s TR=%d: err/bound %.3g" % (what, fam, TR, ratio))
        assert fails, (what, fam, TR, ratio)


@pytest.mark.parametrize("H,hr", [(64, 50), (128, 100), (320, 284), (512, 484)])
@pytest.mark.parametrize("fam", ["pre_fwd", "pre_bwd"])
def test_layernorm_over_the_padded_width_fails(fam, H, hr):
    """The families with a LayerNorm: statistics over `hidden` instead of `hidden_real` (the restatement with h_real = 0 on the
    padded weights and operands) fail the row rule on a padded width."""
    TR = {64: 64, 128: 64}.get(H, 32)
    ref = reference("pre", H, hr, TR, "NTR+1", "plain")
    nm = MUTANT_FAMILIES[fam][1]
    w = copy.copy(ref.t["w"])
    w.h_real = 0
    fails, ratio = _verdict(pre_run(lambda v: v.clone(), ref.t, w)[nm], ref, nm)
    print("mutant statistics over H %-8s H=%d hr=%d: err/bound %.3g" % (fam, H, hr, ratio))
    assert fails, (fam, H, hr, ratio)


def two_planes(wt):
    """`wt` rounded to its two largest bf16 planes (nodeops._bf16_planes without the smallest)."""
    p0 = wt.float().to(torch.bfloat16).float()
    return p0 + (wt.float() - p0).to(torch.bfloat16).float()


TWO_PLANE_WEIGHT = {"pre_fwd": "w2t", "pre_bwd": "w2", "upd_fwd": "wv", "upd_bwd": "wv"}


@pytest.mark.parametrize("H", [128, 512])
@pytest.mark.parametrize("fam", sorted(MUTANT_FAMILIES))
def test_the_two_plane_mutant_on_the_scaled_set(fam, H):
    """The smallest bf16 plane of one weight matrix dropped (x_proj[2] in the projection chain, vec_proj in the update chain),
    on the scaled set: the restatement in fp32 with that weight rounded to two planes, 16 significant bits.  A weight is then
    up to 2^-17 = 7.6e-6 of itself off; over a row of K random-sign terms that is about 2^-17 / sqrt(3) = 4e-6 of the row's
    scale at the worst of a few hundred rows.
    Measured here, err / bound of the worst row (H = 128 / 512): pre_fwd 1.83 / 1.13, upd_fwd 1.62 / 1.12, upd_bwd 16.6 / 2.25:
    the mutant fails.  pre_bwd 0.93 / 0.77: it does NOT fail -- the backward floor (5e-6) is wider than a dropped third plane of
    x_proj[2] on these rows, and it stays where it is.  Asserted: what is measured, so that a loosened floor shows here."""
    family, nm = MUTANT_FAMILIES[fam]
    TR = 32 if family == "upd" or H == 512 else 64
    ref = reference(family, H, 0, TR, "N333" if family == "pre" else "n333", "scaled")
    w, name = copy.copy(ref.t["w"]), TWO_PLANE_WEIGHT[fam]
    full = getattr(w, name)
    setattr(w, name, [two_planes(v) for v in full] if isinstance(full, list) else two_planes(full))
    fails, ratio = _verdict(FAMILIES[family][1](lambda v: v.clone(), ref.t, w)[nm], ref, nm)
    print("mutant two planes %-8s H=%d: err/bound %.3g %s" % (fam, H, ratio, "fails" if fails else "passes"))
    assert ratio > 0.5, (fam, H, ratio)
    assert fails == (fam != "pre_bwd"), (fam, H, ratio)
