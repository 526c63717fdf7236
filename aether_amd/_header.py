"""Reads include/aether_hip.h into ctypes: its integer #defines, its structs and its prototypes.

Regular expressions over the comment-stripped text, not a C front end: the header stays inside the grammar below
(DESIGN.md 1), and whatever falls outside it is refused with the offending text, never skipped.
"""
from __future__ import annotations

import ctypes as C
import re


class AetherHipError(RuntimeError):
    pass


SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float,
           "double": C.c_double}
POINTEES = set(SCALARS) | {"void", "char", "uint16_t"}          # what a pointer may point to, besides a header struct

_ITEM = re.compile(r"\s*(?:typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;|([^;]*);)")     # a struct, or a statement
_STARS = r"((?:\*\s*(?:const\b\s*)?)*)"
_TYPE = r"(?:const\s+)?(\w+)\s*"
_FIELDS = re.compile(_TYPE + r"(.*)", re.S)                            # type, then comma-separated declarators
_DECLARATOR = re.compile(_STARS + r"(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)")     # *name[4][AETHER_X]
_PARAM = re.compile(_TYPE + _STARS + r"(\w*)")                         # type, stars, optional name
_PROTOTYPE = re.compile(_TYPE + _STARS + r"(aether_\w+)\s*\(([^()]*)\)")
_LOOSE = re.compile(r"\b(aether_[a-z0-9_]+)\s*\(")


def _refuse(what, text):
    raise AetherHipError(f"aether_hip.h: {what}: {' '.join(text.split())!r}")


def parse(text, typed_pointers=()):
    """(constants, structs, signatures) of a header text: {AETHER_NAME: int}, {Name: ctypes.Structure subclass} in header
    order, {aether_name: (restype, argtypes)}.  A pointer to a struct named in ``typed_pointers`` is POINTER(that struct)
    in a signature; every other pointer, and every pointer field, is c_void_p."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, structs, signatures = {}, {}, {}

    def directive(m):
        word, rest = m.group(1), m.group(2).split(None, 1)
        if word == "define" and rest and rest[0].startswith("AETHER_"):
            if len(rest) == 2 and re.fullmatch(r"\(?\s*-?\d+\s*\)?", rest[1].strip()):
                constants[rest[0]] = int(rest[1].strip(" ()"))
            elif len(rest) == 2 or not rest[0].endswith("_H"):           # the include guard alone has no value
                _refuse("#define that is not an integer", m.group(0))
        elif word not in ("include", "ifdef", "ifndef", "endif"):
            _refuse("preprocessor line outside the grammar", m.group(0))
        return ""
    code = re.sub(r"^[ \t]*#[ \t]*(\w+)(.*)$", directive, text, flags=re.M)

    def ctype(base, stars, where, signature=False):
        if base not in SCALARS and base not in structs and not (stars and base in POINTEES):
            _refuse(f"unknown type {base!r}", where)
        if not stars:
            return SCALARS.get(base) or structs[base]
        if signature and stars.count("*") == 1:
            if base == "char":
                return C.c_char_p
            if base in typed_pointers:
                return C.POINTER(structs[base])
        return C.c_void_p

    def struct(body, name):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, declarators = (_FIELDS.fullmatch(decl) or _refuse(f"field of {name}", decl)).groups()
            for d in declarators.split(","):
                dm = _DECLARATOR.fullmatch(d.strip()) or _refuse(f"field of {name}", decl)
                t = ctype(base, dm.group(1), decl)
                for dim in reversed(re.findall(r"\w+", dm.group(3))):
                    if not dim.isdigit() and dim not in constants:
                        _refuse(f"array size {dim!r}", decl)
                    t = t * (int(dim) if dim.isdigit() else constants[dim])
                fields.append((dm.group(2), t))
        if name in structs:
            _refuse("struct defined twice", name)
        structs[name] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": f"include/aether_hip.h: struct {name}"})

    def prototype(stmt):
        base, stars, name, params = (_PROTOTYPE.fullmatch(stmt) or _refuse("declaration outside the grammar", stmt)).groups()
        if name in signatures:
            _refuse("function declared twice", name)
        restype = None if base == "void" and not stars else ctype(base, stars, stmt, signature=True)
        argtypes = []
        if params.strip() != "void":
            for p in params.split(","):
                pm = _PARAM.fullmatch(p.strip()) or _refuse(f"parameter of {name}", p)
                argtypes.append(ctype(pm.group(1), pm.group(2), stmt, signature=True))
        signatures[name] = (restype, argtypes)

    code, wrapped = re.subn(r'extern\s+"C"\s*\{', "", code)
    end = 0
    for m in _ITEM.finditer(code):                       # in header order: a struct is known from its definition on
        body, name, stmt = m.groups()
        if name:
            struct(body, name)
        elif stmt.strip():
            prototype(stmt.strip())
        end = m.end()
    if code[end:].strip() != "}" * wrapped:
        _refuse("text after the last declaration", code[end:])

    loose = set(_LOOSE.findall(text))
    if loose != set(signatures):
        _refuse("names followed by '(' that are no parsed prototype", " ".join(sorted(loose ^ set(signatures))))
    return constants, structs, signatures
