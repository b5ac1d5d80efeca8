"""CPU: the C-ABI library loads without a GPU, exports every symbol include/hermnet_hip.h
declares, the binding `hermnet_amd._lib` reads from that header equals the recorded ABI v13, and its
banded radial contraction (the formulation the kernels use) agrees with the
dense reference formula (rmnet.py:55,168-172) and with finite differences."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from hermnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "hermnet_hip.h")) as fh:
        return fh.read()


def _declared_parameters(hdr):
    """name -> number of parameters of every hermnet_* declaration, counted on the header text by itself (commas between the
    parentheses; `(void)` is none) -- not through `_lib.read_header`."""
    text = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return {name: 0 if params.strip() == "void" else params.count(",") + 1
            for name, params in re.findall(r"\b(hermnet_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}


def test_library_exports_every_declared_symbol():
    hdr = _header()
    declared = set(re.findall(r"\b(hermnet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES.keys()), declared ^ set(_lib.SIGNATURES.keys())
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.hermnet_abi_version() == _lib.ABI_VERSION == 13
    assert b"gfx950" in lib.hermnet_build_info()
    # every bound function takes as many arguments as the header's parameter list has
    counts = _declared_parameters(hdr)
    assert set(counts) == declared
    for name in declared:
        assert len(getattr(lib, name).argtypes) == counts[name], (name, len(getattr(lib, name).argtypes), counts[name])


def test_binding_read_from_the_header_equals_the_recorded_abi_v13():
    """tests/golden/cabi_v13.json (gen_cabi_fixture.py) is the binding as `_lib` held it in hand-written tables; what `_lib` now
    reads from include/hermnet_hip.h must equal it entry for entry: restype and every argtype of every recorded entry point, every
    struct's fields in order with their types and its size, the option ids, the envelope kinds, the version and the error
    codes.  The header may declare MORE entry points (the ABI is additive), never other ones: "STABLE from v11 on" as a test.
    Where the derived type may differ, and only there: the tables wrote three pointers otherwise than the header does --
    hermnet_get_option's `int* value` as POINTER(c_int), which the reader's uniform rule makes c_void_p, and the `const
    hn_pending_grads* pending` of hermnet_node_update_bwd / _bwd_last as c_void_p, which the rule for pointers to the
    header's structs makes POINTER(PendingGrads).  All are pointers; `ctypes.byref`, which every caller uses, serves both."""
    with open(os.path.join(ROOT, "tests", "golden", "cabi_v13.json")) as fh:
        want = json.load(fh)
    allowed = {("hermnet_get_option", 1): ("LP_c_int", "c_void_p"),
               ("hermnet_node_update_bwd", 18): ("c_void_p", "LP_PendingGrads"),
               ("hermnet_node_update_bwd_last", 16): ("c_void_p", "LP_PendingGrads")}
    assert len(want["functions"]) == 98 and set(want["functions"]) <= set(_lib.SIGNATURES)
    used = set()
    for name, rec in want["functions"].items():
        res, args = _lib.SIGNATURES[name]
        assert res.__name__ == rec["restype"], name
        assert len(args) == len(rec["argtypes"]), name
        for i, (got, old) in enumerate(zip((a.__name__ for a in args), rec["argtypes"])):
            if got != old:
                assert allowed.get((name, i)) == (old, got), (name, i, old, got)
                used.add((name, i))
    assert used == set(allowed)
    assert sorted(want["structs"]) == ["Graph", "PendingGrads", "RbfDesc", "RelationsOut"]
    for name, rec in want["structs"].items():
        cls = getattr(_lib, name)
        assert issubclass(cls, ctypes.Structure)
        assert [[n, t.__name__] for n, t in cls._fields_] == rec["fields"], name
        assert ctypes.sizeof(cls) == rec["sizeof"], name
    assert _lib.OPTIONS == want["options"] and _lib.HN_ENV == want["env"]
    assert _lib.ABI_VERSION == want["abi_version"] == 13 and sorted(_lib._ERR) == want["error_codes"] == [1, 2, 3]
    # the loaded library carries exactly these types
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES.items():
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args), name


_MINI = """
#define HN_OK 0
#define HN_ERR_BAD_ARG 1  /* bad */
#define HN_ABI_VERSION 13
typedef struct hn_box { const float* p; int n; } hn_box;
/* a comment that mentions hermnet_foo( and hermnet_bar (int) must not count */
int hermnet_a(void);
const char* hermnet_b(const hn_box* box, unsigned long seed, const float* const* in, size_t bytes, void* stream);
"""


def test_header_reader_is_strict():
    """`_lib.read_header` on small header strings: what it reads, and that it raises -- naming the culprit -- on a scalar type
    it does not know, on a declaration its pattern cannot read (through the count of `hermnet_*(` occurrences), and on a
    struct field of unknown type; a comment that contains `hermnet_foo(` is not a declaration."""
    defines, structs, sigs, notes = _lib.read_header(_MINI)
    assert defines == {"HN_OK": 0, "HN_ERR_BAD_ARG": 1, "HN_ABI_VERSION": 13} and notes == {"HN_ERR_BAD_ARG": "bad"}
    box = structs["hn_box"]
    assert box.__name__ == "Box" and [(n, t) for n, t in box._fields_] == [("p", ctypes.c_void_p), ("n", ctypes.c_int)]
    assert sorted(sigs) == ["hermnet_a", "hermnet_b"] and sigs["hermnet_a"] == (ctypes.c_int, [])
    res, args = sigs["hermnet_b"]
    assert res is ctypes.c_char_p
    assert args == [ctypes.POINTER(box), ctypes.c_ulong, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    with pytest.raises(ValueError, match=r"unknown type `short flag` in hermnet_c"):
        _lib.read_header(_MINI + "int hermnet_c(int n, short flag);\n")
    with pytest.raises(ValueError, match=r"unknown type `bool` in hermnet_c's return type"):
        _lib.read_header(_MINI + "bool hermnet_c(int n);\n")
    with pytest.raises(ValueError, match=r"2 declarations read, 3 .* not read: \['hermnet_c'\]"):
        _lib.read_header(_MINI + "int hermnet_c(int (*callback)(int), void* stream);\n")
    with pytest.raises(ValueError, match=r"unknown type `uint8_t kind` in struct hn_box"):
        _lib.read_header(_MINI.replace("int n; }", "int n; uint8_t kind; }"))
    with pytest.raises(ValueError, match=r"2 declarations read, 3"):           # one name declared twice
        _lib.read_header(_MINI + "int hermnet_a(int n);\n")


def test_missing_header_is_named_by_load(monkeypatch, tmp_path):
    """The binding is read from the header on first use: without it `load()` raises a RuntimeError that names the path, as it
    does for a missing library.  (A fresh copy of the module: the test process has long read the header.)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("hermnet_amd._lib_without_header", _lib.__file__)
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    fresh.HEADER_PATH = str(tmp_path / "hermnet_hip.h")
    with pytest.raises(RuntimeError, match="hermnet_hip.h not found"):
        fresh.load()
    with pytest.raises(RuntimeError, match=re.escape(fresh.HEADER_PATH)):
        fresh.ABI_VERSION


def test_call_raises_under_the_entry_points_name():
    """`_lib.call`: HN_OK returns None, any other code raises RuntimeError with the entry point's name and the HN_ERR_* text."""
    assert _lib.call("hermnet_set_option", _lib.OPTIONS["fwd_rows"], _lib.get_option("fwd_rows")) is None
    with pytest.raises(RuntimeError, match=r"hermnet_set_option failed: HN_ERR_BAD_ARG \(unsupported shape / null pointer\)"):
        _lib.call("hermnet_set_option", 99, 1)
    with pytest.raises(AttributeError):
        _lib.call("hermnet_no_such_entry_point")


def _dense(offset, inv_rc, coeff, env_kind, p, wt, b, d):
    """float64 dense evaluation of rbf_proj(env * gaussians) and its d-derivative."""
    u = d * inv_rc
    off = offset.astype(np.float64)
    if env_kind == 0:
        a_, b_, c_ = -(p + 1) * (p + 2) / 2, p * (p + 2), -p * (p + 1) / 2
        env = 1 + a_ * u ** p + b_ * u ** (p + 1) + c_ * u ** (p + 2)
        denv = a_ * p * u ** (p - 1) + b_ * (p + 1) * u ** p + c_ * (p + 2) * u ** (p + 1)
    else:
        q = -(u * u) / ((1 - u) * (1 + u))
        env = np.exp(q)
        denv = -2 * u / ((1 - u) * (1 + u)) ** 2 * env
    if u >= 1:
        env = denv = 0.0
    gk = np.exp(coeff * (u - off) ** 2)
    dgk = gk * 2 * coeff * (u - off)
    rb = b + env * (gk @ wt)
    drb = inv_rc * (denv * (gk @ wt) + env * (dgk @ wt))
    return rb, drb


def ref_env(u, env_kind, p):
    u = float(u)
    if env_kind == 0:
        return 1 - (p + 1) * (p + 2) / 2 * u ** p + p * (p + 2) * u ** (p + 1) - p * (p + 1) / 2 * u ** (p + 2)
    return np.exp(-(u * u) / ((1 - u) * (1 + u)))


@pytest.mark.parametrize("R,env_kind,p", [(128, 0, 5), (32, 0, 5), (64, 1, 0), (16, 0, 3)])
def test_banded_rbf_row_matches_dense(R, env_kind, p):
    lib = _lib.load()
    rs = np.random.RandomState(R)
    C, rc = 24, 5.0
    offset = torch.linspace(0, 1, R).numpy().copy()
    coeff = -0.5 / float(offset[1] - offset[0]) ** 2
    wt = (rs.uniform(-1, 1, size=(R, C)) / np.sqrt(R)).astype(np.float32)
    b = rs.uniform(-0.1, 0.1, size=C).astype(np.float32)
    rb = np.zeros(C, np.float32)
    drb = np.zeros(C, np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    worst = worst_d = worst32 = 0.0
    for d in list(rs.uniform(0.05, rc * 0.999, size=200)) + [1e-6, 0.01, rc * 0.9999, rc, rc * 1.5, 33.7, 1e4]:
        rcode = lib.hermnet_host_rbf_row(P(offset), R, 1.0 / rc, coeff, env_kind, p, P(wt), P(b), C,
                                         float(np.float32(d)), P(rb), P(drb))
        assert rcode == 0
        ref, dref = _dense(offset, np.float32(1.0 / rc), coeff, env_kind, p, wt.astype(np.float64), b.astype(np.float64),
                           float(np.float32(d)))
        assert np.all(np.isfinite(rb)) and np.all(np.isfinite(drb))
        scale = np.abs(ref).max()
        worst = max(worst, np.abs(rb - ref).max() / scale)
        # same dense sum in fp32 with the reference's operation order isolates the band truncation
        u32 = np.float32(d) * np.float32(1.0 / rc)
        if u32 < 1:
            g32 = np.exp(np.float32(coeff) * (u32 - offset) ** 2, dtype=np.float32)
            ref32 = b.astype(np.float64) + float(np.float32(ref_env(u32, env_kind, p))) * (g32.astype(np.float64) @ wt.astype(np.float64))
            worst32 = max(worst32, np.abs(rb - ref32).max() / scale)
        worst_d = max(worst_d, np.abs(drb - dref).max() / max(np.abs(dref).max(), 0.1))   # abs error floor: derivative -> 0 at the cutoff
        if d >= rc:   # beyond the cutoff only the bias is left
            assert np.array_equal(rb, b) and not drb.any()
    # dropped taps are < exp(-18) of the largest; the rest is fp32 rounding of u - offset[k]
    assert worst32 < 1e-6, worst32    # band truncation + summation order only
    assert worst < 2e-5, worst        # + fp32 rounding of (u - offset[k]) * (R-1), shared with the reference
    assert worst_d < 2e-4, worst_d


def test_banded_rbf_derivative_vs_finite_difference():
    lib = _lib.load()
    R, C, rc = 128, 8, 5.0
    rs = np.random.RandomState(0)
    offset = torch.linspace(0, 1, R).numpy().copy()
    coeff = -0.5 / float(offset[1] - offset[0]) ** 2
    wt = (rs.uniform(-1, 1, size=(R, C)) / np.sqrt(R)).astype(np.float64)
    b = np.zeros(C)
    for d in [0.7, 2.345, 4.2]:
        h = 1e-6
        rp, _ = _dense(offset, 1 / rc, coeff, 0, 5, wt, b, d + h)
        rm, _ = _dense(offset, 1 / rc, coeff, 0, 5, wt, b, d - h)
        _, dr = _dense(offset, 1 / rc, coeff, 0, 5, wt, b, d)
        assert np.allclose((rp - rm) / (2 * h), dr, rtol=1e-5, atol=1e-7)


def _geometry_f64(cell, lo, hi, rc, n):
    """The cell-list geometry of the neighbour search (csrc/neighbor_kernels.hip, nbr_make_geom) restated in scalar
    np.float64 operations, one rounding each, in the routine's order: (22 doubles, 7 ints), or None for a geometry it
    refuses."""
    f = np.float64
    rc = f(rc)
    inv = [f(0.0)] * 9
    with np.errstate(all="ignore"):
        if cell is not None:
            c = [f(v) for v in cell]
            out_cell = list(c)
            det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6])
            if not (abs(det) >= 1e-12) or not (abs(det) <= 1.0e300):
                return None
            inv = [(c[4] * c[8] - c[5] * c[7]) / det, (c[2] * c[7] - c[1] * c[8]) / det, (c[1] * c[5] - c[2] * c[4]) / det,
                   (c[5] * c[6] - c[3] * c[8]) / det, (c[0] * c[8] - c[2] * c[6]) / det, (c[2] * c[3] - c[0] * c[5]) / det,
                   (c[3] * c[7] - c[4] * c[6]) / det, (c[1] * c[6] - c[0] * c[7]) / det, (c[0] * c[4] - c[1] * c[3]) / det]
        else:
            out_cell = [f(1.0) if k % 4 == 0 else f(0.0) for k in range(9)]
        nbins, reach, out_lo = [0] * 3, [0] * 3, [f(0.0)] * 3
        for k in range(3):
            if cell is not None:
                h = f(1.0) / np.sqrt(inv[k] * inv[k] + inv[3 + k] * inv[3 + k] + inv[6 + k] * inv[6 + k])
            else:
                h = f(hi[k]) - f(lo[k]) + f(2e-6)
            if not (h > 0.0) or not (h <= 1.0e300):
                return None
            q = np.floor(h / rc)
            nbins[k] = max(1, 1024 if q > 1024.0 else int(q))
            if cell is not None:
                r = np.ceil(rc / (h / f(nbins[k])) - f(1e-12))
                reach[k] = max(1, 9 if r > 9.0 else int(r))
                if reach[k] > 8:
                    return None
            else:
                out_lo[k] = f(lo[k]) - f(1e-6)
                inv[4 * k] = f(nbins[k]) / h
                reach[k] = 1
        while nbins[0] * nbins[1] * nbins[2] > 8 * n + 64:
            kmax = 0
            for k in (1, 2):
                if nbins[k] > nbins[kmax]:
                    kmax = k
            if nbins[kmax] <= 1:
                break
            nb = (nbins[kmax] + 1) // 2
            if cell is None:
                inv[4 * kmax] = inv[4 * kmax] * (f(nb) / f(nbins[kmax]))
            nbins[kmax] = nb
        return np.array(out_cell + inv + out_lo + [rc * rc], dtype=np.float64), nbins + reach + [0 if cell is None else 1]


def _cube(a):
    return [a, 0, 0, 0, a, 0, 0, 0, a]


_GEOMETRY_CASES = {       # name: (cell or None, lo, hi, rc, atoms)
    "cubic 10.86 A": (_cube(10.86), None, None, 5.0, 64),
    "triclinic": ([9.3, 0.4, -0.7, 2.1, 11.2, 0.3, -1.6, 3.3, 14.9], None, None, 5.0, 96),
    "cell smaller than the cutoff (reach 2)": (_cube(3.6), None, None, 5.0, 4),
    "sheared cell smaller than the cutoff (reach above 2)": ([1.3, 0.2, 0, 0, 2.2, 0.1, 0.3, 0, 3.1], None, None, 5.0, 2),
    "one atom in a 100 A cube, periodic": (_cube(100.0), None, None, 5.0, 1),
    "one atom in a 100 A cube, open": (None, [0.0, 0.0, 0.0], [100.0, 100.0, 100.0], 5.0, 1),
    "open box of a single atom": (None, [1.25, -3.5, 0.75], [1.25, -3.5, 0.75], 5.0, 1),
}
_GEOMETRY_REFUSED = {
    "singular cell": ([4.0, 0, 0, 0, 4.0, 4.0, 0, 4.0, 4.0], None, None, 5.0, 8),
    "reach 9": (_cube(0.6), None, None, 5.0, 8),
    "NaN entry": ([10.0, 0, 0, 0, float("nan"), 0, 0, 0, 10.0], None, None, 5.0, 8),
    "open box with an infinite corner": (None, [0.0, 0.0, 0.0], [3.0, float("inf"), 3.0], 5.0, 8),
}


def _host_geometry(lib, cell, lo, hi, rc, n):
    arr = lambda v, k: None if v is None else (ctypes.c_double * k)(*v)
    geom, grid = np.full(22, -7.0), np.full(7, -7, dtype=np.int32)
    rcode = lib.hermnet_host_neighbor_geometry(arr(cell, 9), arr(lo, 3), arr(hi, 3), rc, n, geom.ctypes.data, grid.ctypes.data)
    return rcode, geom, grid


@pytest.mark.parametrize("name", sorted(_GEOMETRY_CASES))
def test_neighbour_geometry_equals_its_float64_restatement_bit_for_bit(name):
    """hermnet_host_neighbor_geometry runs the ONE geometry routine of the search on the host: all 29 values equal the
    scalar float64 restatement above, bit for bit (no tolerance: every form of the search must bin alike)."""
    cell, lo, hi, rc, n = _GEOMETRY_CASES[name]
    rcode, geom, grid = _host_geometry(_lib.load(), cell, lo, hi, rc, n)
    want_geom, want_grid = _geometry_f64(cell, lo, hi, rc, n)
    assert rcode == 0
    assert np.array_equal(geom.view(np.uint64), want_geom.view(np.uint64)), (geom, want_geom)
    assert grid.tolist() == want_grid, (grid.tolist(), want_grid)
    nb, reach = grid[:3], grid[3:6]
    assert int(nb[0]) * int(nb[1]) * int(nb[2]) <= 8 * n + 64 and grid[6] == (cell is not None)
    if "reach" in name:
        assert 2 <= reach.max() <= 8
    if "100 A" in name:       # 20 bins per axis, 72 allowed: eight rounds of the coarsening loop, the first largest axis first
        assert nb.tolist() == [3, 3, 5]
    if name == "open box of a single atom":
        assert nb.tolist() == [1, 1, 1] and np.all(geom[[9, 13, 17]] == 1.0 / 2e-6)


@pytest.mark.parametrize("name", sorted(_GEOMETRY_REFUSED))
def test_neighbour_geometry_refuses_degenerate_cells_and_boxes(name):
    cell, lo, hi, rc, n = _GEOMETRY_REFUSED[name]
    assert _geometry_f64(cell, lo, hi, rc, n) is None
    assert _host_geometry(_lib.load(), cell, lo, hi, rc, n)[0] == 1                  # HN_ERR_BAD_ARG
    # ... as it does a call without its pointers, a cutoff that is not positive, and no atom
    lib, good = _lib.load(), _GEOMETRY_CASES["cubic 10.86 A"]
    assert _host_geometry(lib, None, None, None, 5.0, 8)[0] == 1 and _host_geometry(lib, None, [0.0] * 3, None, 5.0, 8)[0] == 1
    assert _host_geometry(lib, good[0], None, None, 0.0, 8)[0] == 1 and _host_geometry(lib, good[0], None, None, float("nan"), 8)[0] == 1
    assert _host_geometry(lib, good[0], None, None, 5.0, 0)[0] == 1
    assert lib.hermnet_host_neighbor_geometry((ctypes.c_double * 9)(*good[0]), None, None, 5.0, 8, None, None) == 1


def test_default_message_kernels_fit_their_register_budget(tmp_path):
    """The channel-per-lane backward must stay at 4 waves per SIMD (<= 128 VGPRs at 1024 threads) without scratch:
    a spill or a fifth-wave-less build is a silent 2x.  Checked on the code hipcc generates for gfx950 (no GPU)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    src = os.path.join(ROOT, "hermnet_amd", "csrc", "message_bwd_cl.hip")
    out = str(tmp_path / "cl.s")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-S", "--cuda-device-only",
                    src, "-o", out], check=True, capture_output=True, timeout=600)
    text = open(out).read()
    kernels = re.findall(r"\.name:\s+(\S*message_scatter_bwd_cl_kernel\S*)(.*?)\.wavefront_size", text, flags=re.S)
    assert len(kernels) == 4        # {with, without vec rows} x {whole tile, tap-row windows (num_rbf > 137)}
    for name, meta in kernels:
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))
        assert get("vgpr_count") <= 128, (name, get("vgpr_count"))
        assert get("vgpr_spill_count") == 0, name
        if "ELb0EEE" in name:       # the whole-tile instances (the ones every default-sized model runs)
            assert get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name


# The node chain kernels as hipcc compiled them for gfx950 before the knobs of their experiments were taken out of the sources:
# (registers, VGPR spills, SGPR spills, scratch bytes) per kernel, by template arguments (b0 / b1: bool).  The same commit compiled
# layernorm_bwd_parts_kernel into all three units, out of the shared header; only node_chain.hip launches it and now holds it.
CHAIN_KERNEL_BUDGETS = {
    "node_chain.hip": {
        "node_pre_bwd_kernel128,64": (206, 0, 0, 0),
        "node_pre_bwd_kernel256,32": (172, 0, 0, 0),
        "node_pre_bwd_kernel64,64": (118, 0, 0, 0),
        "node_pre_fwd_kernel128,64": (174, 0, 0, 0),
        "node_pre_fwd_kernel256,32": (204, 0, 0, 0),
        "node_pre_fwd_kernel64,64": (114, 0, 0, 0),
        "node_update_bwd_kernel128,32,2": (246, 0, 0, 0),
        "node_update_bwd_kernel128,64,1": (450, 0, 20, 0),
        "node_update_bwd_kernel256,32,1": (456, 0, 14, 0),
        "node_update_bwd_kernel64,64,2": (246, 0, 0, 0),
        "node_update_fwd_kernel128,32,2": (249, 0, 0, 0),
        "node_update_fwd_kernel128,64,1": (506, 0, 0, 0),
        "node_update_fwd_kernel256,32,1": (512, 28, 0, 116),
        "node_update_fwd_kernel64,64,2": (249, 0, 0, 0),
        "layernorm_bwd_parts_kernel": (56, 0, 0, 0),
    },
    "node_chain16.hip": {
        "node_pre_bwd16_kernel128": (164, 0, 0, 0),
        "node_pre_fwd16_kernel128": (212, 0, 0, 0),
        "energy_head16_bwd_kernel128,64": (84, 0, 0, 0),
        "energy_head16_fwd_kernel128,64": (76, 0, 0, 0),
        "node_update_bwd16_kernel128,b0,b0": (168, 1, 0, 8),
        "node_update_bwd16_kernel128,b0,b1": (166, 0, 0, 0),
        "node_update_bwd16_kernel128,b1,b0": (168, 6, 0, 20),
        "node_update_fwd16_kernel128,b0,b0": (200, 0, 0, 0),
        "node_update_fwd16_kernel128,b0,b1": (196, 0, 0, 0),
        "node_update_fwd16_kernel128,b1,b0": (215, 0, 1, 0),
    },
    "node_chain_wide.hip": {
        "node_pre_bwd_wide_kernel128": (136, 0, 0, 0),
        "node_pre_bwd_wide_kernel192": (176, 0, 0, 0),
        "node_pre_bwd_wide_kernel256": (180, 0, 0, 0),
        "node_pre_bwd_wide_kernel320": (244, 0, 0, 0),
        "node_pre_bwd_wide_kernel384": (240, 0, 0, 0),
        "node_pre_bwd_wide_kernel448": (296, 0, 0, 0),
        "node_pre_bwd_wide_kernel512": (288, 0, 0, 0),
        "node_pre_fwd_wide_kernel128": (192, 0, 0, 0),
        "node_pre_fwd_wide_kernel192": (200, 0, 0, 0),
        "node_pre_fwd_wide_kernel256": (200, 0, 3, 0),
        "node_pre_fwd_wide_kernel320": (208, 0, 24, 0),
        "node_pre_fwd_wide_kernel384": (204, 0, 45, 0),
        "node_pre_fwd_wide_kernel448": (308, 0, 93, 0),
        "node_pre_fwd_wide_kernel512": (324, 0, 113, 0),
        "node_update_bwd_wide_kernel128": (232, 0, 0, 0),
        "node_update_bwd_wide_kernel192": (307, 0, 11, 0),
        "node_update_bwd_wide_kernel256": (304, 0, 15, 0),
        "node_update_bwd_wide_kernel320": (407, 0, 44, 0),
        "node_update_bwd_wide_kernel384": (407, 0, 56, 0),
        "node_update_bwd_wide_kernel448": (504, 0, 68, 0),
        "node_update_bwd_wide_kernel512": (492, 0, 74, 0),
        "node_update_fwd_wide_kernel128": (348, 0, 0, 0),
        "node_update_fwd_wide_kernel192": (371, 0, 0, 0),
        "node_update_fwd_wide_kernel256": (370, 0, 0, 0),
        "node_update_fwd_wide_kernel320": (371, 0, 0, 0),
        "node_update_fwd_wide_kernel384": (386, 0, 0, 0),
        "node_update_fwd_wide_kernel448": (442, 0, 0, 0),
        "node_update_fwd_wide_kernel512": (396, 0, 0, 0),
    },
}


def _chain_kernel_key(mangled):
    """`node_update_fwd16_kernel128,b0,b1` for `_ZN12_GLOBAL__N_124node_update_fwd16_kernelILi128ELb0ELb1EEEvN8hn_chain...`"""
    name, targs = re.match(r"_ZN12_GLOBAL__N_1\d+(\w+?_kernel)(?:I((?:L[ib]\d+E)+)E)?", mangled).groups()
    return name + ",".join(("b" if kind == "b" else "") + value for kind, value in re.findall(r"L([ib])(\d+)", targs or ""))


def test_node_chain_kernels_keep_their_register_budgets(tmp_path):
    """Per chain kernel, as hipcc compiles the three units for gfx950 (no GPU): no more spilled registers and no more scratch
    than CHAIN_KERNEL_BUDGETS records, and no fewer waves per SIMD than its registers allowed there (512 registers per lane and
    SIMD, allocated in eights, at most 8 waves).  The kernels are exactly the recorded ones: 53, none compiled twice."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    waves = lambda regs: min(8, 512 // (-(-regs // 8) * 8))
    jobs = {unit: subprocess.Popen([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                                    os.path.join(ROOT, "hermnet_amd", "csrc", unit), "-o", str(tmp_path / (unit + ".s"))],
                                   stdout=subprocess.DEVNULL, stderr=subprocess.PIPE) for unit in CHAIN_KERNEL_BUDGETS}
    for unit, job in jobs.items():
        _, err = job.communicate(timeout=900)
        assert job.returncode == 0, (unit, err.decode()[-2000:])
    assert sum(len(t) for t in CHAIN_KERNEL_BUDGETS.values()) == 53
    for unit, table in CHAIN_KERNEL_BUDGETS.items():
        text = open(str(tmp_path / (unit + ".s"))).read()
        found = {_chain_kernel_key(name): meta for name, meta in
                 re.findall(r"^    \.name:\s+(\S+)\n(.*?)\.wavefront_size", text, flags=re.S | re.M)}
        assert sorted(found) == sorted(table), (unit, sorted(set(found) ^ set(table)))
        for key, (regs, vspill, sspill, scratch) in table.items():
            get = lambda field: int(re.search(r"\.%s:\s+(\d+)" % field, found[key]).group(1))
            print(unit, key, get("vgpr_count"), get("vgpr_spill_count"), get("sgpr_spill_count"), get("private_segment_fixed_size"))
            assert get("vgpr_spill_count") <= vspill and get("sgpr_spill_count") <= sspill, (unit, key)
            assert get("private_segment_fixed_size") <= scratch, (unit, key, get("private_segment_fixed_size"))
            assert waves(get("vgpr_count")) >= waves(regs), (unit, key, get("vgpr_count"), regs)


def test_node_chain_entry_points_refuse_and_choose_as_recorded():
    """tests/golden/chain_dispatch.json (gen_chain_dispatch.py, recorded before the chain kernels' host dispatch was rearranged):
    every refusal in front of a launch, the supported widths and the tile heights, entry for entry.  `table` asserts by itself
    that no call with rows came back as anything but HN_ERR_BAD_ARG, i.e. that none reached a launch."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_chain_dispatch", os.path.join(ROOT, "tests", "golden", "gen_chain_dispatch.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(ROOT, "tests", "golden", "chain_dispatch.json")) as fh:
        want = json.load(fh)
    got = json.loads(json.dumps(gen.table(_lib.load())))
    assert sorted(got["entry_points"]) == sorted(want["entry_points"]) and len(want["entry_points"]) == 11
    for name, widths in want["entry_points"].items():
        assert sorted(widths) == sorted(str(h) for h in gen.WIDTHS), name
        for h, cases in widths.items():
            assert got["entry_points"][name][h] == cases, (name, h, {k: (v, got["entry_points"][name][h].get(k))
                                                                     for k, v in cases.items() if got["entry_points"][name][h].get(k) != v})
    assert got["supported"] == want["supported"]
    assert got["update_tile_rows"] == want["update_tile_rows"]
    assert len(want["update_tile_rows"]) == 6 and want["update_tile_rows"]["update_tile16=2,node_chain_wide=0"]["configs[1]"]["128"] == 16


def test_argument_checks_of_the_round_4_entry_points_need_no_gpu():
    """The entry points added with ABI v8 refuse malformed calls before anything is launched (and treat empty inputs as
    done), so their argument contracts can be checked here: hermnet_train_node_op (operand counts per op), the *_rows edge
    kernels, hn_pending_grads of hermnet_node_update_bwd."""
    lib = _lib.load()
    HN_OK, BAD = 0, lib.hermnet_train_node_op(0, None, 0, None, 0, 0, 4, 0.0, 0.0, None)
    assert BAD != HN_OK
    buf = np.zeros(64, dtype=np.float32)
    ptr = buf.ctypes.data
    arr = lambda n: (ctypes.c_void_p * max(n, 1))(*([ptr] * n))
    need_in = {1: 2, 2: 3, 3: 2, 4: 3, 5: 5, 6: 6, 7: 6, 8: 11, 9: 2, 10: 3, 11: 5, 12: 3}
    need_out = {1: 1, 2: 2, 3: 2, 4: 2, 5: 3, 6: 2, 7: 5, 8: 5, 9: 1, 10: 2, 11: 2, 12: 2}
    for op in need_in:
        ni, no = need_in[op], need_out[op]
        assert lib.hermnet_train_node_op(op, arr(ni), ni, arr(no), no, 0, 128, 0.0, 0.0, None) == HN_OK        # no rows: done
        assert lib.hermnet_train_node_op(op, arr(ni), ni + 1, arr(no), no, 0, 128, 0.0, 0.0, None) == BAD     # operand count
        assert lib.hermnet_train_node_op(op, arr(ni), ni, arr(no), no, 0, 130, 0.0, 0.0, None) == BAD         # width % 4
    assert lib.hermnet_train_node_op(13, arr(2), 2, arr(1), 1, 0, 128, 0.0, 0.0, None) == BAD
    # the row-sum edge kernels: a negative group count is refused, no groups = nothing to do
    assert lib.hermnet_edge_message_fwd_rows(ptr, ptr, None, ptr, 0, 128, None, None, None, ptr, None, -1, ptr, ptr, None) == BAD
    assert lib.hermnet_edge_message_fwd_rows(ptr, ptr, None, ptr, 0, 128, None, None, None, ptr, None, 0, ptr, ptr, None) == HN_OK
    assert lib.hermnet_edge_message_fwd_rows(ptr, ptr, None, ptr, 0, 130, None, None, None, ptr, None, 0, ptr, ptr, None) == BAD
    # hn_pending_grads: every pointer of the record is required
    rp = (ctypes.c_int * 2)(0, 5)
    pend = _lib.PendingGrads(ptr, None, ptr, ptr, ptr, ptr, ptr, 1, 0)
    assert lib.hermnet_node_update_bwd(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None, ptr, rp, ptr, ptr, 5, 1, 128, 0,
                                       ctypes.byref(pend), None) == BAD
    assert lib.hermnet_node_update_bwd(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None, ptr, rp, ptr, ptr, 0, 1, 128, 0,
                                       None, None) == HN_OK                                                 # no rows


def test_node_op_table_of_the_package_equals_the_operand_counts_the_library_checks():
    """trainops.NODE_OPS (name -> code, inputs, outputs) against hermnet_train_node_op itself, which checks the counts before
    any launch: with no rows the table's counts are accepted for every op, one input more or one output more is refused.
    Exactly the codes 1 .. 12, under the kernel names of csrc/train_node_kernels.hip."""
    from hermnet_amd import trainops
    lib = _lib.load()
    HN_OK, HN_ERR_BAD_ARG = 0, 1
    ptr = np.zeros(64, dtype=np.float32).ctypes.data
    arr = lambda n: (ctypes.c_void_p * n)(*([ptr] * n))
    table = trainops.NODE_OPS
    assert sorted(code for code, _, _ in table.values()) == list(range(1, 13))
    assert list(table) == ["silu_bwd", "silu_bwd2", "mid_fwd", "mid_bwd", "mid_bwd2", "out_fwd", "out_bwd", "out_bwd2", "ln_bwd",
                           "ln_bwd2", "res_fwd", "mask_scale"]
    src = open(os.path.join(ROOT, "hermnet_amd", "csrc", "train_node_kernels.hip")).read()
    for name, (code, ni, no) in table.items():
        assert re.search(r"case %d: hipLaunchKernelGGL\(%s_kernel," % (code, name), src) or (code == 10 and "default: hipLaunchKernelGGL(ln_bwd2_kernel," in src), name
        call = lambda n_in, n_out: lib.hermnet_train_node_op(code, arr(n_in + 1), n_in, arr(n_out + 1), n_out, 0, 128, 0.0, 0.0, None)
        assert call(ni, no) == HN_OK, name
        assert call(ni + 1, no) == HN_ERR_BAD_ARG and call(ni, no + 1) == HN_ERR_BAD_ARG, name


def test_argument_checks_of_the_projected_halo_entry_points_need_no_gpu():
    """hermnet_halo_proj_rows / hermnet_halo_proj_accumulate (ABI v12): malformed calls are refused before a launch, an empty
    row list is done."""
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    ptr = buf.ctypes.data
    HN_OK, BAD = 0, 1
    rows = lambda mode, nseg, nsum, n, width, a=ptr: lib.hermnet_halo_proj_rows(mode, a, 0, nseg, ptr, 0, nsum, ptr, n, width, ptr, None)
    assert rows(0, 3, 1, 0, 384) == HN_OK                       # no rows: done (whatever the pointers)
    assert rows(0, 3, 1, 0, 384, a=None) == HN_OK
    assert rows(0, 3, 1, -1, 384) == BAD                        # negative count
    assert rows(0, 3, 1, 0, 386) == BAD and rows(0, 3, 1, 0, 0) == BAD          # width % 4, width <= 0
    assert rows(0, 0, 1, 0, 384) == BAD and rows(1, 3, 0, 0, 384) == BAD        # at least one block and one slice
    assert rows(2, 3, 3, 0, 384) == BAD                         # unpack takes b without a slice axis
    assert rows(3, 3, 1, 4, 384) == BAD                         # unknown mode (checked after the pointers, before a launch)
    assert rows(0, 3, 1, 4, 384, a=None) == BAD                 # rows but no source
    acc = lambda nseg, nu, width, a=ptr: lib.hermnet_halo_proj_accumulate(a, 0, nseg, ptr, ptr, ptr, ptr, nu, width, ptr, None)
    assert acc(3, 0, 384) == HN_OK and acc(3, 0, 384, a=None) == HN_OK
    assert acc(3, -1, 384) == BAD and acc(0, 0, 384) == BAD and acc(3, 0, 382) == BAD
    assert acc(3, 2, 384, a=None) == BAD


def test_argument_checks_of_the_training_entry_points_of_abi_13_need_no_gpu():
    """hermnet_band_product / _grad_a / _grad_b / _grads, hermnet_basis_window, hermnet_edge_unit: malformed calls are refused
    before a launch; nothing to do (no chunks, no edges) is done."""
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    ptr = buf.ctypes.data
    OK, BAD = 0, 1
    assert lib.hermnet_band_product_supported(1024, 384) == 1 and lib.hermnet_band_product_supported(64, 96) == 1
    assert lib.hermnet_band_product_supported(1000, 384) == 0 and lib.hermnet_band_product_supported(1024, 100) == 0
    assert lib.hermnet_band_product_supported(1024, 512) == 0                     # wider than the weight window's LDS image
    prod = lambda nc, C, N, a=ptr: lib.hermnet_band_product(a, ptr, None, nc, C, N, ptr, None)
    assert prod(0, 1024, 384) == OK and prod(0, 1024, 384, a=None) == OK
    assert prod(-1, 1024, 384) == BAD and prod(0, 1000, 384) == BAD and prod(0, 1024, 100) == BAD and prod(2, 1024, 384, a=None) == BAD
    ga = lambda nc, C, N, g=ptr: lib.hermnet_band_product_grad_a(g, None, ptr, nc, C, N, ptr, None)
    assert ga(0, 64, 96) == OK and ga(0, 60, 96) == BAD and ga(3, 64, 96, g=None) == BAD
    gb = lambda nc, C, N, a=ptr: lib.hermnet_band_product_grad_b(a, ptr, None, nc, C, N, ptr, None, None)
    assert gb(0, 64, 96) == OK and gb(0, 64, 98) == BAD and gb(3, 64, 96, a=None) == BAD
    gs = lambda nc, C, N, a=ptr: lib.hermnet_band_product_grads(a, ptr, ptr, None, nc, C, N, ptr, ptr, None, None)
    assert gs(0, 1024, 384) == OK and gs(0, 1024, 385) == BAD and gs(1, 1024, 384, a=None) == BAD
    bw = lambda order, nc, p, u=ptr: lib.hermnet_basis_window(order, u, ptr, 5, ptr, ptr, nc, 1024, -1.0, p, ptr, ptr, ptr, ptr, None)
    assert bw(0, 0, 5) == OK and bw(3, 0, 5) == BAD and bw(0, 0, 0) == BAD and bw(0, -1, 5) == BAD and bw(1, 2, 5, u=None) == BAD
    eu = lambda order, E, D=ptr: lib.hermnet_edge_unit(order, D, None, None, ptr, E, ptr, ptr, ptr, None)
    assert eu(0, 0) == OK and eu(3, 0) == BAD and eu(0, -1) == BAD and eu(0, 4, D=None) == BAD


@pytest.mark.parametrize("out_f,in_f", [(128, 128), (384, 128), (128, 256), (64, 64), (32, 96)])
def test_weight_fragments_through_the_c_abi_equal_the_host_codes(out_f, in_f):
    """a binder of the C seam must not re-implement the three-plane weight stream.  `hermnet_weight_fragments`
    (host pointers in and out) gives frag(W) (tile_rows 32) and frag16(W) (16) bit for bit as `nodeops.weight_fragments` /
    `weight_fragments16` build them in torch ops -- values that are bf16 ties, denormals, huge, tiny and negative zeros
    included -- and the planes sum back to the weight exactly."""
    from hermnet_amd import nodeops
    lib = _lib.load()
    gen = torch.Generator().manual_seed(out_f * 1000 + in_f)
    w = torch.randn(out_f, in_f, generator=gen) * (10.0 ** torch.randint(-6, 7, (out_f, 1), generator=gen).float())
    w[0, :8] = torch.tensor([1.00390625, -1.00390625, 1.01171875, 3.0e38, -3.0e38, 1.0e-38, 1.0e-41, -0.0])   # ties, extremes, a denormal
    w = w.contiguous()
    for tile_rows, ref_fn in ((32, nodeops.weight_fragments), (16, nodeops.weight_fragments16)):
        if out_f % tile_rows or in_f % (16 if tile_rows == 32 else 32):
            out = np.zeros(out_f * in_f * 3, dtype=np.uint16)
            assert lib.hermnet_weight_fragments(w.data_ptr(), out_f, in_f, tile_rows, out.ctypes.data) == 1     # HN_ERR_BAD_ARG
            continue
        out = np.zeros(out_f * in_f * 3, dtype=np.uint16)
        assert lib.hermnet_weight_fragments(w.data_ptr(), out_f, in_f, tile_rows, out.ctypes.data) == 0
        ref = ref_fn(w).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(out, ref), (tile_rows, int((out != ref).sum()))
    # the planes are an exact split: p0 + p1 + p2 == w (fp32 arithmetic, largest first), barring under / overflow of a residual
    planes = [p.float() for p in nodeops._bf16_planes(w)]          # smallest first
    normal = w.abs() >= 1.0e-30                                    # (a denormal's residual planes underflow: documented)
    assert torch.equal(((planes[2] + planes[1]) + planes[0])[normal], w[normal])
    assert lib.hermnet_weight_fragments(None, 32, 32, 32, out.ctypes.data) == 1


def test_library_options_round_trip():
    """hermnet_set_option / hermnet_get_option (ABI v12: they replace the environment variables the library read once per
    process): defaults as documented, a value set is the value read, unknown and retired options are refused."""
    lib = _lib.load()
    v = ctypes.c_int(0)
    for retired in range(4):         # the message kernels' template variants
        assert lib.hermnet_set_option(retired, 1) == 1 and lib.hermnet_get_option(retired, ctypes.byref(v)) == 1
    assert _lib.get_option("update_tile16") == 2 and _lib.get_option("bwd_lanes16") == 0
    with _lib.options(fwd_rows=17, node_chain_wide=1):
        assert _lib.get_option("fwd_rows") == 17 and _lib.get_option("node_chain_wide") == 1
    assert _lib.get_option("fwd_rows") == 0 and _lib.get_option("node_chain_wide") == 0
    assert lib.hermnet_set_option(99, 1) == 1 and lib.hermnet_set_option(-1, 1) == 1
    hdr = open(os.path.join(ROOT, "include", "hermnet_hip.h")).read()
    opts = dict((n.lower(), int(v)) for n, v in re.findall(r"#define HN_OPT_([A-Z0-9_]+) (\d+)", hdr))
    assert opts == _lib.OPTIONS and int(re.search(r"#define HN_NUM_OPTIONS (\d+)", hdr).group(1)) == max(opts.values()) + 1


def test_message_backward_refuses_split_t():
    """split_t (the per-relation 3-D grid of the 16-lanes-per-edge backward) is retired: hermnet_message_scatter_bwd refuses
    any value but 0 before it looks at the rows, so an empty graph shows it without a GPU."""
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float32)
    ptr = buf.ctypes.data
    g = _lib.Graph(0, 0, 1, ptr, ptr, ptr, ptr, ptr, ptr, 0, None)          # num_nodes = 0, one relation
    rbf = _lib.RbfDesc(ptr, 16, 0.2, -0.5, 0, 5)

    def bwd(split_t):
        return lib.hermnet_message_scatter_bwd(ctypes.byref(g), ctypes.byref(rbf), 64, ptr, None, None, ptr, ptr, None, ptr, ptr,
                                               ptr, None, ptr, None, split_t, None, None, None, None, 0, None)
    assert bwd(0) == 0 and bwd(1) == 1                                        # HN_OK, HN_ERR_BAD_ARG
