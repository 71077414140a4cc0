"""include/hypel.h, read once per process: the prototypes, struct layouts and integer constants of libhypel_hip.so.

The header is the single statement of the C ABI; backend.py binds the library from what is read here, and the planners
name launch arguments by the header's parameter names.  Anything this reader does not understand is an error."""
import ctypes
import os
import re

import numpy as np


class HypelError(RuntimeError):
    pass


# where csrc/Makefile finds it (-I../../include), relative to the package
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "hypel.h")

_SCALARS = {"int32_t": (ctypes.c_int32, "<i4"), "int64_t": (ctypes.c_int64, "<i8"), "uint32_t": (ctypes.c_uint32, "<u4"),
            "uint64_t": (ctypes.c_uint64, "<u8"), "float": (ctypes.c_float, "<f4"), "double": (ctypes.c_double, "<f8"),
            "int": (ctypes.c_int, "<i4")}


def _ctype(ctype, decl, returned=False):
    ctype = " ".join(ctype.split())
    if "*" in ctype:
        return ctypes.c_char_p if returned and ctype.replace(" ", "") == "constchar*" else ctypes.c_void_p
    ctype = ctype.removeprefix("const ")
    if ctype == "hypel_stream_t":
        return ctypes.c_void_p
    if ctype not in _SCALARS:
        raise HypelError(f"include/hypel.h: unknown type {ctype!r} in `{' '.join(decl.split())}`")
    return _SCALARS[ctype][0]


def parse(text):
    """Header text -> (functions, structs, constants):
    functions  name -> (return ctype, [(parameter name, ctype)]), in declaration order
    structs    name -> aligned NumPy dtype with the header's field names
    constants  name -> int, from `#define HYPEL_X <integer literal | INT64_MIN>` and `enum { HYPEL_A = n, ... }`"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    functions, structs, constants = {}, {}, {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(HYPEL_\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+|INT64_MIN)[ \t]*$",
                                  text, flags=re.M):
        constants[name] = -(1 << 63) if value == "INT64_MIN" else int(value, 0)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def enum(m):
        for member in filter(None, (s.strip() for s in m.group(1).split(","))):
            mm = re.fullmatch(r"(HYPEL_\w+)\s*=\s*(0[xX][0-9a-fA-F]+|\d+)", member)
            if not mm:
                raise HypelError(f"include/hypel.h: enum member `{member}` has no integer value")
            constants[mm.group(1)] = int(mm.group(2), 0)
        return " "

    def struct(m):
        names, formats = [], []
        for field in filter(None, (s.strip() for s in m.group(1).split(";"))):
            ctype, _, rest = field.partition(" ")
            if ctype not in _SCALARS or not re.fullmatch(r"\w+(\s*,\s*\w+)*", rest.strip()):
                raise HypelError(f"include/hypel.h: cannot read field `{field}` of {m.group(2)}")
            for fname in rest.split(","):
                names.append(fname.strip())
                formats.append(_SCALARS[ctype][1])
        structs[m.group(2)] = np.dtype({"names": names, "formats": formats}, align=True)
        return " "

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(hypel_\w+)\s*;", struct, text)
    text = re.sub(r'\btypedef\s+void\s*\*\s*hypel_stream_t\s*;|\bextern\s+"C"\s*\{|\}', " ", text)
    for decl in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"([\w\s\*]+?)\b(hypel_\w+)\s*\(([^()]*)\)", decl)
        if not m:
            raise HypelError(f"include/hypel.h: cannot read the declaration `{' '.join(decl.split())}`")
        params = []
        plist = m.group(3).strip()
        for p in [] if plist in ("", "void") else plist.split(","):
            pm = re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", p, flags=re.S)
            if not pm or pm.group(2) in _SCALARS or pm.group(1).strip() in ("", "const"):
                raise HypelError(f"include/hypel.h: unnamed parameter `{p.strip()}` in `{' '.join(decl.split())}`")
            params.append((pm.group(2), _ctype(pm.group(1), decl)))
        functions[m.group(2)] = (_ctype(m.group(1), decl, returned=True), params)
    return functions, structs, constants


try:
    with open(HEADER) as _f:
        FUNCTIONS, STRUCTS, CONSTANTS = parse(_f.read())
except OSError as e:
    raise HypelError(f"{HEADER} is missing: the Python binding is built from it ({e})") from None


def struct(name):
    return STRUCTS[name]


def const(name):
    return CONSTANTS[name]
