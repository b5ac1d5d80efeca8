"""Writes tests/golden/cabi_v13.json: the ctypes binding of ABI v13 as `hermnet_amd._lib` holds it -- per entry point the restype
and the argtypes by ctypes name, per struct the fields in order with their ctypes names and `ctypes.sizeof`, the option ids, the
envelope kinds, the ABI version and the error codes.  Recorded once from the hand-written tables that `_lib` held before the
binding was read from include/hermnet_hip.h; tests/test_cabi_cpu.py compares the derived binding with it entry for entry, so the
header's "STABLE from v11 on" is a test.  Run from the repository root: python tests/golden/gen_cabi_fixture.py"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from hermnet_amd import _lib  # noqa: E402


def describe():
    structs = {}
    for cls in (_lib.RbfDesc, _lib.Graph, _lib.PendingGrads, _lib.RelationsOut):
        structs[cls.__name__] = {"fields": [[n, t.__name__] for n, t in cls._fields_], "sizeof": ctypes.sizeof(cls)}
    return {"abi_version": _lib.ABI_VERSION,
            "functions": {name: {"restype": res.__name__, "argtypes": [a.__name__ for a in args]}
                          for name, (res, args) in sorted(_lib.SIGNATURES.items())},
            "structs": structs,
            "options": _lib.OPTIONS,
            "env": _lib.HN_ENV,
            "error_codes": sorted(_lib._ERR)}


if __name__ == "__main__":
    with open(os.path.join(HERE, "cabi_v13.json"), "w") as fh:
        json.dump(describe(), fh, indent=1, sort_keys=True)
        fh.write("\n")
