"""CPU-only: the two entry points of gradient accumulation are declared the same way in include/cris_hip.h and in the ctypes
signature table of cris/pytorch_amd/hip.py, and the ABI version that announces them is the same number in both (the regex
approach of tests/test_abi.py)."""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cris.pytorch_amd import hip  # noqa: E402
from header_decls import HEADER, ctype_of, prototypes  # noqa: E402

NEW = ("cris_grad_accumulate", "cris_step_advance_micro")


def test_abi_version_is_8_in_header_and_binding():
    src = open(HEADER).read()
    assert int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1)) == hip.ABI_VERSION == 8
    comment = re.search(r"/\* CRIS_ABI_VERSION moves.*?\*/", src, flags=re.S).group(0)
    assert re.search(r"\b8: cris_grad_accumulate / cris_step_advance_micro", comment)      # the header says what 8 added


def test_new_signatures_match_the_prototypes():
    protos = prototypes(open(HEADER).read())
    for name in NEW:
        assert name in protos, name
        assert name in hip._SIGS and name in hip.EXPORTS, name
        ret, params = protos[name]
        res, args = hip._SIGS[name]
        assert res is {"int": C.c_int, "long": C.c_long}[ret], name
        want = [ctype_of(p) for p in params.split(",")]
        assert list(args) == want, (name, args, want)
    # the documented argument lists
    assert protos["cris_grad_accumulate"][1].replace("  ", " ") == "float* dst, const float* src, long n, int mode, void* stream"
    assert [p.split()[-1] for p in protos["cris_step_advance_micro"][1].split(",")] == ["step", "seed", "exchange_gen", "micro", "accum", "stream"]
    # cris_step_advance itself is unchanged
    assert [p.split()[-1] for p in protos["cris_step_advance"][1].split(",")] == ["step", "seed", "exchange_gen", "stream"]
    assert hip._SIGS["cris_step_advance"] == (C.c_int, [C.c_void_p] * 4)
