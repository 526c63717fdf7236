"""The ctypes binding is derived from include/aether_hip.h (aether_amd/_header.py).  Host only, no GPU: the derived binding
is held to the record of the hand-written one it replaced (tests/golden/lib_abi.json, tools/lib_abi_record.py), the struct
layouts to what the compiler makes of the header, and the parser to its grammar: it refuses what it does not understand."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import pytest

from aether_amd import _lib, build
from aether_amd._header import AetherHipError, parse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import lib_abi_record as abi  # noqa: E402

RECORD = json.load(open(os.path.join(REPO, "tests", "golden", "lib_abi.json")))


def test_binding_equals_the_recorded_hand_written_one():
    """Every recorded function: restype and the class of every argument, in order.  Every recorded struct: sizeof and
    (field, offset, size) of every field, and the name the modules fill it under is the derived class itself."""
    assert len(RECORD["functions"]) >= 150 and len(RECORD["structs"]) >= 20
    for name, want in RECORD["functions"].items():
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert {"restype": abi.arg_class(res), "args": [abi.arg_class(a) for a in args]} == want, name
    for name, want in RECORD["structs"].items():
        assert abi.struct_layout(getattr(_lib, name)) == want, name
        mod, attr = abi.STRUCTS[name]
        assert getattr(importlib.import_module("aether_amd." + mod), attr) is getattr(_lib, name), (mod, attr)
    # The two structs of the variable-N dNRI had no hand-written mirror: the module filled their seq2seq twins.  The C side
    # relies on this equality today (csrc hands one host chain the tables of both engines), so it is held here.
    for dyn, s2s in (("AetherDynDnriPriorParams", "AetherS2SDnriPriorParams"),
                     ("AetherDynDnriDecoderParams", "AetherS2SDnriDecoderParams")):
        assert abi.struct_layout(getattr(_lib, dyn)) == RECORD["structs"][s2s], dyn


def test_typed_pointers_are_exactly_the_exported_structs():
    typed = {t._type_.__name__ for _, args in _lib.SIGNATURES.values() for t in args if issubclass(t, C._Pointer)}
    assert typed == set(_lib.TYPED_POINTERS)
    assert _lib.SIGNATURES["aether_profile_read"][1] == [C.c_void_p, C.c_void_p, C.c_int]
    assert _lib.SIGNATURES["aether_s2s_launch_stats_reset"] == (None, [])
    assert _lib.SIGNATURES["aether_version"] == (C.c_char_p, [])


def test_constants_come_from_the_header():
    assert _lib.CONSTANTS["AETHER_EINVAL"] == -1 and _lib.CONSTANTS["AETHER_HIDDEN"] == 64
    assert (_lib.FLAG_KEEP_INTERMEDIATES, _lib.FLAG_FORCE_STREAMED, _lib.FLAG_FORCE_FUSED, _lib.FLAG_WORKSPACE_REUSED,
            _lib.FLAG_WEIGHTS_PREPARED, _lib.FLAG_BACKWARD_ONLY, _lib.FLAG_DROPOUT) == (1, 2, 4, 8, 16, 32, 64)
    assert (_lib.EGNN_NORM_DIFF, _lib.EGNN_TANH, _lib.EGNN_KEEP) == (1, 2, 4)
    assert (_lib.CLOF_NORM_DIFF, _lib.CLOF_TANH, _lib.CLOF_KEEP, _lib.CLOF_RECURRENT) == (1, 2, 4, 8)
    assert _lib.S2S_LAUNCH_LOG == 96 and len(_lib.S2S_LAUNCH_KINDS) == _lib.CONSTANTS["AETHER_S2S_LAUNCH_KINDS"] == 5


def test_struct_layouts_equal_the_compilers(tmp_path):
    """sizeof and every offsetof as a host compiler sees the header, against the ctypes classes: not through the parser."""
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "aether_hip.h"', 'int main() {']
    want = []
    for name, cls in _lib.STRUCTS.items():
        lines.append(f'  std::printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {C.sizeof(cls)}")
        for field, *_ in cls._fields_:
            lines.append(f'  std::printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
            want.append(f"{name}.{field} {getattr(cls, field).offset}")
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert len(want) > 300 and got == want + [""]


GRAMMAR = """
/* a comment with int aether_not_here(int); inside */
#ifndef AETHER_TEST_H
#define AETHER_TEST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define AETHER_X 3
#define AETHER_NEG (-2)   // trailing comment
typedef struct AetherInner { int32_t a, b, c; int64_t n; } AetherInner;
typedef struct {
    const float* w[4]; float* const* pp;
    double m[2][AETHER_X];
    size_t bytes; float f;
    AetherInner log[AETHER_X];
    AetherInner one;
} AetherOuter;
const char* aether_name(void);
void aether_reset(void);
int64_t aether_mix(const AetherOuter* outer, AetherInner* inner, const char* name, float** pp, size_t n,
                   double, int64_t count, uint16_t* bits, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_grammar():
    constants, structs, signatures = parse(GRAMMAR, typed_pointers=("AetherOuter",))
    assert constants == {"AETHER_X": 3, "AETHER_NEG": -2}
    inner, outer = structs["AetherInner"], structs["AetherOuter"]
    assert list(structs) == ["AetherInner", "AetherOuter"] and outer.__name__ == "AetherOuter"
    assert inner._fields_ == [("a", C.c_int), ("b", C.c_int), ("c", C.c_int), ("n", C.c_int64)]
    assert [n for n, _ in outer._fields_] == ["w", "pp", "m", "bytes", "f", "log", "one"]
    kinds = dict(outer._fields_)
    assert kinds["w"] is C.c_void_p * 4 and kinds["pp"] is C.c_void_p and kinds["m"] is (C.c_double * 3) * 2
    assert kinds["bytes"] is C.c_size_t and kinds["f"] is C.c_float and kinds["log"] is inner * 3 and kinds["one"] is inner
    assert C.sizeof(outer) == 4 * 8 + 8 + 6 * 8 + 8 + 8 + 4 * 24
    assert signatures == {
        "aether_name": (C.c_char_p, []), "aether_reset": (None, []),
        "aether_mix": (C.c_int64, [C.POINTER(outer), C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_double, C.c_int64,
                                   C.c_void_p, C.c_void_p])}
    o = outer()
    o.w[1] = 4096                                     # pointer fields take data_ptr() integers
    assert o.w[1] == 4096 and o.pp is None


@pytest.mark.parametrize("text", [
    "typedef struct A { unsigned a; } A;",                                  # unknown type
    "typedef struct A { uint16_t a; } A;",                                  # a pointee only, no field type
    "int aether_f(long n);",                                                # unknown type of a parameter
    "long aether_f(int n);",                                                # ... of the result
    "int aether_f(void x);",
    "typedef struct A { void (*done)(int); } A;",                           # function pointer field
    "int aether_f(int (*callback)(int));",                                  # function pointer parameter
    "typedef struct A { int a : 3; } A;",                                   # bit-field
    "typedef struct A { B b; } A; typedef struct B { int x; } B;",          # struct used before it is defined
    "int aether_f(const B* b); typedef struct B { int x; } B;",
    "typedef struct A { int a[AETHER_N]; } A;",                             # array sized by an unknown name
    "typedef struct A { int a[]; } A;",
    "typedef struct A { int a; } A; typedef struct A { int a; } A;",        # defined twice
    "int aether_f(int a); int aether_f(int a);",
    "struct A { int a; };",                                                 # no typedef
    "#define AETHER_N 1.5",                                                 # not an integer
    "#define AETHER_N (1 << 3)",
    "#define OTHER 1",
    "#if 0\nint aether_f(int a);\n#endif",                                  # a conditional could hide a declaration
    "int aether_f(int a[4]);",
    "int aether_f();",                                                      # C's unprototyped form: (void) is the empty list
    "int other_f(int a);",                                                  # not an aether_ name
    "int aether_f(int a)",                                                  # no semicolon
    "static inline int aether_twice(int a) { return 2 * a; }",              # the loose pattern sees it, the grammar does not
    "int aether_f(int a) __attribute__((cold));",
    "int aether_Upper(int a);",                                             # the grammar sees it, the loose pattern does not
])
def test_parser_refuses(text):
    with pytest.raises(AetherHipError) as e:
        parse(text)
    assert "aether_hip.h" in str(e.value)


def test_missing_header_is_an_error_naming_the_path(monkeypatch, tmp_path):
    gone = str(tmp_path / "include" / "aether_hip.h")
    monkeypatch.setattr(_lib, "HEADER_PATH", gone)
    with pytest.raises(AetherHipError, match="aether_hip.h") as e:
        _lib._read_header()
    assert gone in str(e.value)

