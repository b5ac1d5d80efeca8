"""Writes tests/golden/chain_dispatch.json: what the host side of the node chain kernels (csrc/node_chain*.hip) answers WITHOUT
launching anything -- per entry point and width the return code of every call it must refuse (or finish as "no rows") in front
of its launch, the widths each family supports, and the tile height hermnet_node_update_tile_rows picks for four row layouts
under every setting of the two options it reads (update_tile16, node_chain_wide; it does not read update_tile64_max, which
only hermnet_node_update_fwd / _bwd consult at tile_rows = 0, so that option is not varied here).  Recorded from the library as it stood before the host dispatch was
rearranged; tests/test_cabi_cpu.py holds the library to it entry for entry.  `table(lib)` is shared with that test.
No call recorded here may reach a launch (its pointers are host memory): every one with rows must come back HN_ERR_BAD_ARG,
which `table` itself asserts.  Run from the repository root: python tests/golden/gen_chain_dispatch.py"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from hermnet_amd import _lib  # noqa: E402

WIDTHS = (0, 32, 64, 100, 128, 192, 256, 512, 576)
HN_OK, HN_ERR_BAD_ARG = 0, 1
ROWS, REL = 5, 1

# (name, kind) in the order of include/hermnet_hip.h.  Kinds: "req" a pointer the entry point requires, "opt" one that may be
# NULL (passed as NULL), "set" one that may be NULL and is passed set (NULL would launch), "rph" the host copy of type_rowptr,
# "pend" the hn_pending_grads pointer (NULL), "stream" (NULL);
# integers and floats by the role the cases vary: "rows", "rel", "hidden", "real" (hidden_real), "nwin", "wmode", "tile", "cols".
PRE9 = [(n, "req") for n in ("x", "w1", "b1", "w2", "b2", "hb", "xh", "mean", "rstd")]
UPD_FWD = ([(n, "req") for n in ("x1", "vec1", "wv", "wx0", "bx0", "wx2", "bx2")] + [("row_active", "opt"), ("type_rowptr", "req"),
           ("type_rowptr_host", "rph")] + [(n, "req") for n in ("vp", "h2b", "q23", "nrm", "x_out")])
UPD_BWD_TAIL = ([(n, "req") for n in ("vp", "h2b", "q23", "nrm", "wx2t", "wx0t", "wvt")] + [("row_active", "opt"),
                ("type_rowptr", "req"), ("type_rowptr_host", "rph"), ("gx1", "req"), ("gvec1", "req"), ("rows", "rows"),
                ("rel", "rel"), ("hidden", "hidden")])
ENTRY_POINTS = {
    "hermnet_node_pre_fwd": PRE9 + [("src_ranges", "opt"), ("rows", "rows"), ("rel", "rel"), ("hidden", "hidden"), ("real", "real"),
                                    ("eps", "eps"), ("row_windows", "opt"), ("nwin", "nwin"), ("wmode", "wmode"), ("stream", "stream")],
    "hermnet_node_pre_bwd": [(n, "req") for n in ("gxh", "hb", "w2t", "w1t", "gn_parts", "x", "mean", "rstd")] +
                            [("add", "opt"), ("gx", "set"), ("src_ranges", "opt"), ("rows", "rows"), ("rel", "rel"),
                             ("hidden", "hidden"), ("real", "real"), ("row_windows", "opt"), ("nwin", "nwin"), ("wmode", "wmode"),
                             ("stream", "stream")],
    "hermnet_node_update_fwd": UPD_FWD + [("vec_out", "req"), ("rows", "rows"), ("rel", "rel"), ("hidden", "hidden"), ("tile", "tile"),
                                          ("stream", "stream")],
    "hermnet_node_update_bwd": [("gx_out", "req"), ("gvec_out", "req")] + UPD_BWD_TAIL + [("tile", "tile"), ("pending", "pend"),
                                                                                         ("stream", "stream")],
    "hermnet_node_update_fwd_last": UPD_FWD + [("rows", "rows"), ("rel", "rel"), ("hidden", "hidden"), ("stream", "stream")],
    "hermnet_node_update_bwd_last": [("gx_out", "req")] + UPD_BWD_TAIL + [("pending", "pend"), ("stream", "stream")],
    "hermnet_node_update_pre_fwd": UPD_FWD + [("vec_out", "req"), ("rows", "rows"), ("rel", "rel"), ("hidden", "hidden")] +
                                   [(n, "req") for n in ("w1", "b1", "w2", "b2", "hb", "xh", "mean", "rstd")] +
                                   [("next_rel", "rel2"), ("real", "real"), ("eps", "eps"), ("stream", "stream")],
    "hermnet_node_pre_fwd16": PRE9 + [("rows", "rows"), ("rel", "rel"), ("hidden", "hidden"), ("real", "real"), ("eps", "eps"),
                                      ("stream", "stream")],
    "hermnet_node_pre_bwd16": [(n, "req") for n in ("gxh", "hb", "w2t", "w1t", "gn_parts")] +
                              [("rows", "rows"), ("rel", "rel"), ("hidden", "hidden"), ("stream", "stream")],
    "hermnet_energy_head16_fwd": [("x", "req"), ("w0", "req"), ("b0", "req"), ("w2", "req"), ("b2", "opt"), ("row_mask", "opt"),
                                  ("h", "req"), ("e", "req"), ("rows", "rows"), ("hidden", "hidden"), ("cols", "cols"),
                                  ("stream", "stream")],
    "hermnet_energy_head16_bwd": [("ge", "req"), ("h", "req"), ("w0t", "req"), ("w2", "req"), ("row_mask", "opt"), ("gx", "req"),
                                  ("rows", "rows"), ("hidden", "hidden"), ("cols", "cols"), ("stream", "stream")],
}


def table(lib):
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    rph = (ctypes.c_int * 2)(0, ROWS)
    rph_long = (ctypes.c_int * 2)(0, ROWS + 1)
    out = {"entry_points": {}, "supported": {}, "update_tile_rows": {}}

    def call(name, hidden, null=(), all_null=False, **over):
        """The entry point with every required pointer set (NULL: those named in `null`; all of them with all_null)."""
        val = dict(rows=ROWS, rel=REL, rel2=REL, hidden=hidden, real=0, eps=1e-5, nwin=0, wmode=0, tile=0, cols=64)
        val.update({k: v for k, v in over.items() if k in val})
        args = []
        for arg, kind in ENTRY_POINTS[name]:
            if arg in over and arg not in val:
                args.append(over[arg])
            elif kind == "req":
                args.append(None if all_null or arg in null else ptr)
            elif kind == "set":
                args.append(None if arg in null else ptr)
            elif kind == "rph":
                args.append(None if all_null or arg in null else over.get("rph", rph))
            elif kind in ("opt", "pend", "stream"):
                args.append(None)
            elif kind == "eps":
                args.append(ctypes.c_float(val["eps"]))
            else:
                args.append(val[kind])
        return int(getattr(lib, name)(*args))

    def pending(**over):
        f = dict(gn_parts=ptr, gvec_parts=ptr, x=ptr, mean=ptr, rstd=ptr, gx1=ptr, gvec1=ptr, num_parts=1, hidden_real=0, gxh=None,
                 hb=None, w2t_frag16=None, w1t_frag16=None)
        f.update(over)
        return ctypes.byref(_lib.PendingGrads(*[f[n] for n, _ in _lib.PendingGrads._fields_]))

    for name, spec in ENTRY_POINTS.items():
        kinds = {kind for _, kind in spec}
        rows = out["entry_points"][name] = {}
        for h in WIDTHS:
            rec = rows[str(h)] = {}
            refused = {}
            rec["no_rows_null_pointers"] = call(name, h, all_null=True, rows=0)
            for arg, kind in spec:
                if kind in ("req", "rph"):
                    refused["null:" + arg] = call(name, h, null=(arg,))
            refused["rows<0"] = call(name, h, rows=-1)
            if "rel" in kinds:
                refused["rel=0"] = call(name, h, rel=0)
                refused["rel<0"] = call(name, h, rel=-1)
            if "rel2" in kinds:
                refused["next_rel=0"] = call(name, h, rel2=0)
            if "real" in kinds:
                refused["hidden_real>hidden"] = call(name, h, real=h + 1)
            if "rph" in kinds:
                refused["rowptr_host[T]>rows"] = call(name, h, rph=rph_long)
            if "wmode" in kinds:
                refused["wmode=3"] = call(name, h, wmode=3, row_windows=ptr, nwin=1)
                refused["wmode<0"] = call(name, h, wmode=-1, row_windows=ptr, nwin=1)
                refused["wmode=1,no_windows"] = call(name, h, wmode=1)
                refused["wmode=1,nwin<0"] = call(name, h, wmode=1, row_windows=ptr, nwin=-1)
                if name == "hermnet_node_pre_bwd":
                    refused["wmode=1,gx_null"] = call(name, h, null=("gx",), wmode=1, row_windows=ptr, nwin=1)
            if "tile" in kinds and h != 128:            # (at 128 the 16-row kernels exist: the call would launch)
                refused["tile_rows=16"] = call(name, h, tile=16)
            if name == "hermnet_node_update_bwd_last":
                refused["pending"] = call(name, h, pending=pending())
            if name == "hermnet_node_update_bwd":
                fused = dict(gn_parts=None, gxh=ptr, hb=ptr, w2t_frag16=ptr, w1t_frag16=ptr)
                refused["fused_pending,tile_rows=0"] = call(name, h, pending=pending(**fused))
                refused["fused_pending,tile_rows=32"] = call(name, h, tile=32, pending=pending(**fused))
                for f in ("hb", "w2t_frag16", "w1t_frag16"):
                    refused["fused_pending,tile_rows=16,null:" + f] = call(name, h, tile=16, pending=pending(**dict(fused, **{f: None})))
                for tile in (0, 16):
                    for f in ("gvec_parts", "x", "mean", "rstd", "gx1", "gvec1"):
                        refused["pending,tile_rows=%d,null:%s" % (tile, f)] = call(name, h, tile=tile, pending=pending(**{f: None}))
                    refused["pending,tile_rows=%d,null:gn_parts+gxh" % tile] = call(name, h, tile=tile, pending=pending(gn_parts=None))
                    refused["pending,tile_rows=%d,num_parts=0" % tile] = call(name, h, tile=tile, pending=pending(num_parts=0))
                    refused["pending,tile_rows=%d,hidden_real>hidden" % tile] = call(name, h, tile=tile,
                                                                                    pending=pending(hidden_real=h + 1))
            if "cols" in kinds:
                refused["cols=32"] = call(name, h, cols=32)
                refused["cols=128"] = call(name, h, cols=128)
            bad = {k: v for k, v in refused.items() if v != HN_ERR_BAD_ARG}
            assert not bad, (name, h, bad)                # anything else has been launched (or has tried to)
            assert rec["no_rows_null_pointers"] in (HN_OK, HN_ERR_BAD_ARG), (name, h, rec)
            rec.update(refused)

    layouts = {"configs[1]": ((0, 3347, 6694, 10041), 10041, 3), "configs[3]": ((0, 33800, 67600, 101397), 101397, 3),
               "one_relation": ((0, 10041), 10041, 1), "empty": ((0, 0), 0, 1)}
    for wide in (0, 1):
        with _lib.options(node_chain_wide=wide):
            sup = out["supported"]["node_chain_wide=%d" % wide] = {}
            for h in WIDTHS:
                sup[str(h)] = {"chain_supported": int(lib.hermnet_node_chain_supported(h)),
                               "chain_tile_rows(update=0)": int(lib.hermnet_node_chain_tile_rows(h, 0)),
                               "chain_tile_rows(update=1)": int(lib.hermnet_node_chain_tile_rows(h, 1)),
                               "fused_supported": int(lib.hermnet_node_fused_supported(h)),
                               "energy_head16_supported": {str(c): int(lib.hermnet_energy_head16_supported(h, c))
                                                           for c in (0, 32, 64, 128)}}
            for t16 in (0, 1, 2):
                with _lib.options(update_tile16=t16):
                    rec = out["update_tile_rows"]["update_tile16=%d,node_chain_wide=%d" % (t16, wide)] = {}
                    for label, (rp, n, t) in layouts.items():
                        arr = (ctypes.c_int * len(rp))(*rp)
                        rec[label] = {str(h): int(lib.hermnet_node_update_tile_rows(arr, n, t, h)) for h in WIDTHS}
                    rec["null_rowptr"] = {str(h): int(lib.hermnet_node_update_tile_rows(None, 5, 1, h)) for h in WIDTHS}
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "chain_dispatch.json"), "w") as fh:
        json.dump(table(_lib.load()), fh, indent=1, sort_keys=True)
        fh.write("\n")
