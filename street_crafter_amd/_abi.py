"""include/street_crafter_amd.h as Python reads it: the ctypes table, the struct classes and the integer #defines are
DERIVED from the header's text, once, when this module is imported.  Nothing here is typed a second time; whatever the
reader does not recognise is an ImportError, never a default.  tests/test_capi_cpu.py has a C++ compiler confirm that it
reads the header the way this module does.
"""
from __future__ import annotations

import ctypes as C
import re

from .build import HEADER as HEADER_PATH, abi_hash

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32,
            "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_OPAQUE = ("void", "sc_stream_t")      # pointees that only ever travel as addresses
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*(\**)\s*(\w+)\s*(?:\[(\w+)\])?")


def _fail(what):
    raise ImportError(f"street_crafter_amd: cannot read {HEADER_PATH}: {what}")


def _struct(name, body, constants):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, declarators = re.fullmatch(r"(?:const\s+)?(\w+)\s*(.*)", decl, flags=re.S).groups()
        for part in declarators.split(","):                                 # `int64_t start, end;`
            m = re.fullmatch(r"(\*?)\s*(\w+)\s*(?:\[(\w+)\])?", part.strip())
            if not m or not (base in _SCALARS or m.group(1) and base == "void"):
                _fail(f"field {decl!r} of {name}")
            ptr, field, length = m.groups()
            t = C.c_void_p if ptr else _SCALARS[base]                       # device pointers travel as integers
            if length:                                                      # `float basis[SC_COMPOSE_MAX_FOURIER]`
                if not (length.isdigit() or length in constants):
                    _fail(f"array length of {decl!r} in {name}")
                t = t * int(constants.get(length, length))
            fields.append((field, t))
    return type(name, (C.Structure,), {"_fields_": fields, "__doc__": f"{name} of include/street_crafter_amd.h"})


def _param(decl, structs, where):
    m = _DECL.fullmatch(decl)
    if not m or m.group(4) or len(m.group(2)) > 1:
        _fail(f"parameter {decl!r} of {where}")
    base, ptr, name = m.group(1), m.group(2), m.group(3)
    if not ptr:
        if base == "sc_stream_t":
            return C.c_void_p
        if base not in _SCALARS:
            _fail(f"unknown type {base!r} in {where}")
        return _SCALARS[base]
    if base == "char":
        return C.c_char_p
    pointee = _SCALARS.get(base) or structs.get(base)
    if pointee is None and base not in _OPAQUE:
        _fail(f"unknown type {base!r} in {where}")
    # "every pointer is a DEVICE pointer unless its name ends in _host": those travel as integers
    return C.POINTER(pointee) if pointee is not None and name.endswith("_host") else C.c_void_p


def _read():
    try:
        with open(HEADER_PATH, "rb") as f:
            raw = f.read()
    except OSError as e:
        raise ImportError(f"street_crafter_amd: the C ABI header is missing ({HEADER_PATH}): {e}") from None
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", raw.decode(), flags=re.S)
    constants = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs = {}

    def take_struct(m):
        structs[m.group(2)] = _struct(m.group(2), m.group(1), constants)
        return ""

    text = re.sub(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", take_struct, text)
    text = text.replace('extern "C" {', "").replace("typedef void* sc_stream_t;", "")
    signatures = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(const\s+char\s*\*|\w+)\s*(sc_\w+)\s*\(([^()]*)\)", stmt)
        if not m:
            if stmt == "}":             # closes extern "C"
                continue
            _fail(f"not a prototype: {stmt[:80]!r}")
        ret, name, params = m.groups()
        restype = C.c_char_p if ret.endswith("*") else _SCALARS.get(ret)
        if restype is None:
            _fail(f"unknown return type {ret!r} of {name}")
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        signatures[name] = (restype, [_param(p, structs, name) for p in params])
    return signatures, structs, constants, abi_hash(raw)


# name -> (restype, argtypes); typedef name -> ctypes.Structure; #define name -> int; digest of the text they came from
SIGNATURES, STRUCTS, CONSTANTS, ABI_HASH = _read()
