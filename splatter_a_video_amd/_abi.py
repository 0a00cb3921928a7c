"""Reader of the C ABI's headers (include/splat_hip.h and its extensions include/splat_hip_views.h,
include/splat_hip_views_grad.h, include/splat_hip_camera_grad.h, include/splat_hip_layers_cam.h, include/splat_hip_flow.h and
include/splat_hip_flow_occ.h): prototypes, structs and integer #defines as ctypes types.

The header is the only place a prototype is written; ``_lib.lib()`` applies what ``parse`` yields to every function.
Anything the reader does not understand raises ``HeaderError`` -- it never guesses a type.
"""
from __future__ import annotations

import ctypes
import re
from typing import Dict, List, NamedTuple, Optional, Tuple

SCALARS = {
    "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
    "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
    "uint8_t": ctypes.c_uint8,
}
# one declarator-less type: [const] base, then stars (each may carry a const), then an optional name
_PARAM = re.compile(r"(?:const\s+)?(\w+)((?:\s*\*\s*(?:const\b)?)*)\s*(\w+)?")
_PROTO = re.compile(r"(.+?)\b(\w+)\s*\((.*)\)", re.S)


class HeaderError(ValueError):
    pass


class Header(NamedTuple):
    functions: Dict[str, Tuple[Optional[type], List[type]]]     # name -> (restype, argtypes), in header order
    structs: Dict[str, type]                                    # typedef name -> ctypes.Structure
    defines: Dict[str, int]
    handles: Tuple[str, ...] = ()                               # handle typedefs (void *), an extension's base included


def _ctype(base: str, stars: int, known: set, where: str):
    """the fixed mapping: scalars by name, ``const char *`` -> c_char_p, every other pointer and handle -> c_void_p"""
    if stars == 0:
        if base in SCALARS:
            return SCALARS[base]
        if base in known:                  # a handle typedef (splat_stream_t)
            return ctypes.c_void_p
    elif base == "char" and stars == 1:
        return ctypes.c_char_p
    elif base in SCALARS or base in known or base in ("void", "char"):
        return ctypes.c_void_p
    raise HeaderError(f"{where}: unknown type '{base}{'*' * stars}'")


def _spec(spec: str, known: set, where: str):
    """ctypes type of a return type or of one parameter (its name is optional); None for plain ``void``"""
    p = _PARAM.fullmatch(spec.strip())
    if not p:
        raise HeaderError(f"{where}: cannot parse '{' '.join(spec.split())}'")
    if p[1] == "void" and not p[2]:
        return None
    return _ctype(p[1], p[2].count("*"), known, where + (f" '{p[3]}'" if p[3] else ""))


def parse(text: str, base: Optional[Header] = None) -> Header:
    """``base``: the header this one extends (an extension header includes it for its handles and structs; ``#include`` lines are
    blanked here, so the names come in through this argument).  The result lists the extension's own functions, structs and
    defines."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)

    handles = set(re.findall(r"typedef\s+void\s*\*\s*(\w+)\s*;", text))
    if base is not None:
        handles |= set(base.handles)
    text = re.sub(r"typedef\s+void\s*\*\s*\w+\s*;", " ", text)

    structs: Dict[str, type] = dict(base.structs) if base is not None else {}
    inherited = set(structs)
    for m in re.finditer(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", text, re.S):
        name, fields = m[2], []
        for decl in filter(None, (d.strip() for d in m[1].split(";"))):
            d = re.fullmatch(r"(?:const\s+)?(\w+)\b(.*)", decl, re.S)
            for part in (d[2].split(",") if d else [""]):
                f = re.fullmatch(r"\s*((?:\*\s*(?:const\b)?\s*)*)(\w+)\s*", part)
                if not f:
                    raise HeaderError(f"struct {name}: cannot parse field '{decl}'")
                fields.append((f[2], _ctype(d[1], f[1].count("*"), handles | set(structs), f"struct {name}, field {f[2]}")))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{name} of include/splat_hip.h"})
    text = re.sub(r"typedef\s+struct\s+\w*\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)

    known = handles | set(structs)
    functions = {}
    for stmt in filter(None, (s.strip(" \t\r\n}") for s in text.split(";"))):
        m = _PROTO.fullmatch(stmt)
        if not m:
            raise HeaderError(f"cannot parse declaration '{' '.join(stmt.split())[:80]}'")
        name, params = m[2], m[3].split(",")
        if len(params) == 1 and params[0].strip() in ("", "void"):
            params = []
        args = [_spec(s, known, f"{name}, parameter {k + 1}") for k, s in enumerate(params)]
        if None in args:
            raise HeaderError(f"{name}: a parameter of type void")
        functions[name] = (_spec(m[1], known, f"{name}, return type"), args)
    return Header(functions, {k: v for k, v in structs.items() if k not in inherited}, defines, tuple(sorted(handles)))


def load(path: str, base: Optional[Header] = None) -> Header:
    with open(path) as f:
        return parse(f.read(), base)
