"""The C prototypes of include/cris_hip.h as ctypes types, for the CPU tests that compare them with the signature table of
cris/pytorch_amd/hip.py (the regex approach of tests/test_abi.py).  Imports nothing of the package."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cris_hip.h")


def ctype_of(decl):
    """ctypes type of one C parameter declaration of the header"""
    decl = decl.strip()
    if "*" in decl:
        return C.c_void_p
    base = re.sub(r"\b(const|unsigned)\b", "", decl).split()[0]
    return {"int": C.c_int, "long": C.c_long, "float": C.c_float, "int32_t": C.c_int, "uint32_t": C.c_uint}[base]


def prototypes(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|long)\s+(cris_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)}
