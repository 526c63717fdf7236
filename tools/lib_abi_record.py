#!/usr/bin/env python
"""Record the ABI the ctypes binding presents, for tests/test_lib_binding.py.

    python tools/lib_abi_record.py [tests/golden/lib_abi.json]

Two parts: per function of ``_lib.SIGNATURES`` the restype and the class of every argument (``ptr`` for ``void*`` and
``POINTER(S)`` alike, ``char_p``, ``int``, ``int64``, ``size_t``, ``float``, ``double``), and per struct the modules fill
its ``sizeof`` and ``(field, offset, size)`` per field.  The committed record was taken from the hand-written binding that
preceded the one derived from include/aether_hip.h; the test iterates over the record, so a new entry needs no new record,
and a deliberate ABI change of a recorded entry edits the record by hand.
"""
from __future__ import annotations

import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# header struct -> (module, attribute) the package reaches it by
STRUCTS = {
    "AetherParams": ("_lib", "AetherParams"),
    "AetherGraphInfo": ("_lib", "AetherGraphInfo"),
    "AetherS2SLaunchRecord": ("_lib", "AetherS2SLaunchRecord"),
    "AetherS2SLaunchStats": ("_lib", "AetherS2SLaunchStats"),
    "AetherDynScenePack": ("_lib", "AetherDynScenePack"),
    "AetherAdamWTensor": ("_lib", "AetherAdamWTensor"),
    "AetherDynFieldParams": ("nn.state2state.dynamic_field_aether", "_DynFieldParams"),
    "AetherS2SFieldParams": ("nn.seq2seq.field", "_S2SFieldParams"),
    "AetherS2SDecoderParams": ("nn.seq2seq.decoder", "_DecoderParams"),
    "AetherS2SPriorParams": ("nn.seq2seq.encoder", "_PriorParams"),
    "AetherS2SMarkovParams": ("nn.seq2seq.markov", "_MarkovParams"),
    "AetherS2SGraphSummaryParams": ("nn.seq2seq.dynamic_field_aether", "_SummaryParams"),
    "AetherS2SFilmParams": ("nn.seq2seq.dynamic_field_aether", "_FilmParams"),
    "AetherS2SDnriPriorParams": ("nn.seq2seq.dnri", "_DnriPriorParams"),
    "AetherS2SDnriDecoderParams": ("nn.seq2seq.dnri", "_DnriDecoderParams"),
    "AetherS2SDnriMlpParams": ("nn.seq2seq.dnri", "_DnriMlpParams"),
    "AetherDynDecoderParams": ("nn.dynamicvars.decoder", "_DynDecoderParams"),
    "AetherDynPriorParams": ("nn.dynamicvars.encoder", "_DynPriorParams"),
    "AetherDynFieldQueryParams": ("nn.dynamicvars.aether_dynamicvars", "_DynFieldQueryParams"),
    "AetherDynStepConfig": ("nn.dynamicvars._scene", "_DynStepConfig"),
}

SCALARS = {C.c_char_p: "char_p", C.c_int: "int", C.c_int64: "int64", C.c_size_t: "size_t", C.c_float: "float",
           C.c_double: "double", None: "void"}


def arg_class(t):
    """The class of one restype / argtype; raises KeyError for anything the record has no word for."""
    if t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer)):
        return "ptr"
    return SCALARS[t]


def struct_layout(cls):
    return {"sizeof": C.sizeof(cls),
            "fields": [[name, getattr(cls, name).offset, getattr(cls, name).size] for name, *_ in cls._fields_]}


def record():
    from aether_amd import _lib
    functions = {name: {"restype": arg_class(res), "args": [arg_class(a) for a in args]}
                 for name, (res, args) in _lib.SIGNATURES.items()}
    structs = {name: struct_layout(getattr(importlib.import_module("aether_amd." + mod), attr))
               for name, (mod, attr) in STRUCTS.items()}
    return {"functions": functions, "structs": structs}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lib_abi.json")
    rec = record()
    with open(out, "w") as f:                      # one entry per line: a hand edit of one entry is a one-line diff
        parts = [json.dumps(part) + ": {\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in rec[part].items())
                 + "\n }" for part in ("functions", "structs")]
        f.write("{\n " + ",\n ".join(parts) + "\n}\n")
    print(f"{out}: {len(rec['functions'])} functions, {len(rec['structs'])} structs")
