"""The declarations of include/vp.h as ctypes: what the *_abi tests compare vision/_vp.py's bindings with."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCALARS = [(r"size_t", C.c_size_t), (r"double", C.c_double), (r"float", C.c_float), (r"int64_t", C.c_int64), (r"long long", C.c_longlong),
            (r"uint64_t", C.c_uint64), (r"unsigned long long", C.c_ulonglong), (r"int32_t", C.c_int32), (r"uint32_t", C.c_uint32),
            (r"unsigned int", C.c_uint), (r"unsigned", C.c_uint), (r"int", C.c_int)]


def _header_text():
    txt = open(os.path.join(ROOT, "include", "vp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return " ".join(l for l in txt.splitlines() if not l.strip().startswith("#"))


def _header_prototypes():
    """name -> (return type as written, list of ctypes argument types), from the declarations of include/vp.h.  Pointers are void*,
    as _vp.py binds them; an argument type this does not know stays a string, which equals no binding."""
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(vp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_text()):
        types = []
        for a in args.split(","):
            a = a.strip()
            if a in ("void", ""):
                continue
            if "*" in a:
                types.append(C.c_void_p)
                continue
            for pat, ctype in _SCALARS:
                if re.match(r"(const\s+)?" + pat + r"\b", a):
                    types.append(ctype)
                    break
            else:
                types.append(a)
        out[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), types)
    return out


def header_options():
    """VP_OPT_* name (without the prefix) -> value"""
    return {n: int(v) for n, v in re.findall(r"\bVP_OPT_([A-Z_]+)\s*=\s*(\d+)", _header_text())}
