"""ctypes binding of `libhermnet_hip.so`, READ from its contract `include/hermnet_hip.h`.

Nothing of the C ABI is retyped here: `read_header` turns the header's `#define HN_*`, its four `typedef struct hn_*` and every
`hermnet_*` declaration into the constants, the `ctypes.Structure` classes (`Graph`, `RbfDesc`, `PendingGrads`, `RelationsOut`)
and `SIGNATURES` (name -> (restype, argtypes)) of this module, on the first use of any of them.  The reader is strict: a type it
does not know or a declaration it cannot read raises, naming it.
`call(c_name, *args)` is THE way to call an entry point that returns an HN_* code; launches that carry a timer label take
`ops._call`, which appends the stream.  Size queries (`*_workspace*`, `*_supported`, `*_tile_rows`) are plain calls on `load()`.

The library is built in-tree by `__graft_entry__.build()` / `make -C hermnet_amd/csrc`.
There is NO fallback: if it is missing the product path raises.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HERMNET_LIB_PATH") or os.path.join(_HERE, "csrc", "libhermnet_hip.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "hermnet_hip.h")

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t, "unsigned long": ctypes.c_ulong}


def _ctype(ctext, structs, where, named=True):
    """ctypes type of the C parameter, field (`named`) or return type `ctext`.  Device and host pointers travel as integers
    (c_void_p), except a pointer to one of the header's structs and the `const char*` a function returns."""
    words = [w for w in ctext.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        base = " ".join(words[:words.index("*")])
        if words.count("*") == 1 and base in structs:
            return ctypes.POINTER(structs[base])
        return ctypes.c_char_p if base == "char" and not named else ctypes.c_void_p
    base = " ".join(words[:-1] if named else words)
    if base not in _SCALARS:
        raise ValueError("include/hermnet_hip.h: unknown type `%s` in %s" % (ctext.strip(), where))
    return _SCALARS[base]


def read_header(text):
    """(defines, structs, signatures, notes) of the header `text`: every `#define HN_* <int>` by name, every `typedef struct
    hn_x` as a ctypes.Structure class by its C name, every `hermnet_*` declaration as name -> (restype, argtypes), and the
    comment behind each HN_ERR_* define."""
    raw = text
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(HN_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    # (an error code's message: the comment behind its define)
    notes = dict(re.findall(r"#[ \t]*define[ \t]+(HN_ERR_\w+)[ \t]+\d+[ \t]*/\*\s*(.*?)\s*\*/", raw))
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    structs = {}
    for name, body, alias in re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        if alias != name or not name.startswith("hn_"):
            raise ValueError("include/hermnet_hip.h: struct %s is typedef'd as %s" % (name, alias))
        fields = [f for f in body.split(";") if f.strip()]
        cls = "".join(p.capitalize() for p in name[3:].split("_"))
        structs[name] = type(cls, (ctypes.Structure,), {
            "__doc__": "%s of include/hermnet_hip.h" % name,
            "_fields_": [(f.split()[-1].lstrip("*"), _ctype(f, structs, "struct " + name)) for f in fields]})
    signatures = {}
    for res, name, params in re.findall(r"([\w\s\*]+?)\b(hermnet_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [] if params.strip() == "void" else params.split(",")
        signatures[name] = (_ctype(res, structs, name + "'s return type", named=False), [_ctype(p, structs, name) for p in params])
    seen = re.findall(r"\b(hermnet_\w+)\s*\(", text)
    if len(seen) != len(signatures):
        raise ValueError("include/hermnet_hip.h: %d declarations read, %d `hermnet_*(` present -- not read: %s"
                         % (len(signatures), len(seen), sorted(set(seen) - set(signatures)) or "a name declared twice"))
    return defines, structs, signatures, notes


def _bind():
    """Read the header (once) and publish what it declares as attributes of this module: every HN_* define, the struct
    classes, SIGNATURES, OPTIONS / HN_ENV (the HN_OPT_* / HN_ENV_* defines, lower-cased), ABI_VERSION, the error texts."""
    g = globals()
    if "SIGNATURES" in g:
        return
    try:
        with open(HEADER_PATH) as fh:
            text = fh.read()
    except OSError:
        raise RuntimeError("hermnet_amd: the C ABI's header %s not found -- the binding is read from it (it ships with the "
                           "sources, beside hermnet_amd/)" % HEADER_PATH)
    defines, structs, signatures, notes = read_header(text)
    g.update(defines)
    g.update({cls.__name__: cls for cls in structs.values()})
    prefixed = lambda p: {n[len(p):].lower(): v for n, v in defines.items() if n.startswith(p)}
    g.update(OPTIONS=prefixed("HN_OPT_"), HN_ENV=prefixed("HN_ENV_"), ABI_VERSION=defines["HN_ABI_VERSION"],
             _ERR={v: "%s (%s)" % (n, notes[n]) if n in notes else n for n, v in defines.items() if n.startswith("HN_ERR_")},
             SIGNATURES=signatures)


def __getattr__(name):
    """The names `_bind` derives from the header, on their first use (a missing header raises there, not at import)."""
    if name.startswith("__") or "SIGNATURES" in globals():
        raise AttributeError("module %r has no attribute %r" % (__name__, name))
    _bind()
    try:
        return globals()[name]
    except KeyError:
        raise AttributeError("module %r has no attribute %r" % (__name__, name))


_lib = None


def source_hash():
    """sha256 (first 16 hex digits) over the library's sources, as `csrc/Makefile` stamps it into
    `hermnet_build_info()` (`src=...`): *.hip, *.cpp, *.h of csrc/ in sorted order, then include/hermnet_hip.h."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(os.path.basename(f) for pat in ("*.hip", "*.cpp", "*.h") for f in glob.glob(os.path.join(csrc, pat)))
    paths = [os.path.join(csrc, f) for f in files] + [HEADER_PATH]
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build_info():
    """`hermnet_build_info()` of the loaded library (ABI, target, source hash, build date) as a str."""
    return load().hermnet_build_info().decode()


def load():
    """Load the native library (once).  Raises RuntimeError if it has not been built, or if the header is missing."""
    global _lib
    if _lib is not None:
        return _lib
    _bind()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "hermnet_amd: native library %s not found -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C hermnet_amd/csrc`).  There is no CPU/eager fallback for the hot path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.hermnet_abi_version() != ABI_VERSION:
        raise RuntimeError("hermnet_amd: %s has ABI version %d, the Python side expects %d -- rebuild it "
                           "(`make -C hermnet_amd/csrc`)" % (LIB_PATH, lib.hermnet_abi_version(), ABI_VERSION))
    # the library must have been built from the sources next to it: a stale prebuilt binary would otherwise be what
    # the tests and the benchmark measure (an explicitly chosen diagnostic build is not checked)
    if not os.environ.get("HERMNET_LIB_PATH") and os.environ.get("HERMNET_ALLOW_STALE_LIB", "0") == "0":
        info = lib.hermnet_build_info().decode()
        try:
            want = source_hash()
        except OSError:
            want = None                       # sources not shipped: nothing to compare with
        if want is not None and ("src=" + want) not in info:
            raise RuntimeError("hermnet_amd: %s was not built from the sources in hermnet_amd/csrc (library: %s; sources "
                               "hash to %s) -- rebuild it (`make -C hermnet_amd/csrc`)" % (LIB_PATH, info, want))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, _ERR.get(rc, "error %d" % rc)))


def call(c_name, *args):
    """The library's `c_name(*args)`; a return code other than HN_OK raises RuntimeError under the entry point's own name."""
    rc = getattr(load(), c_name)(*args)
    if rc != 0:
        check(rc, c_name)


# hermnet_set_option / hermnet_get_option (include/hermnet_hip.h: HN_OPT_*): tuning knobs and the alternative kernel forms
# that tests and A/Bs compare against -- process-wide, read by the launchers at every call (ids 0-3: retired)
def get_option(name):
    v = ctypes.c_int(0)
    load()
    call("hermnet_get_option", OPTIONS[name], ctypes.byref(v))
    return int(v.value)


def set_option(name, value):
    """Set a library option; returns the previous value."""
    old = get_option(name)
    call("hermnet_set_option", OPTIONS[name], int(value))
    return old


class options(object):
    """`with _lib.options(bwd_lanes16=1): ...` -- options set for a block, restored behind it (tests, A/Bs)."""

    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)


def ptr(t):
    """Device/host pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()
