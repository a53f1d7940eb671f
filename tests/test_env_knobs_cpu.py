"""Every environment variable the native library reads is documented, and the tuning switches retired with the probe builds stay
out: tile selection decides the rows per BatchNorm-statistics partial, so a variable that changes it unseen changes numerics.
Reads source text only - no library, no GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cris", "pytorch_amd", "csrc")

RETIRED = [
    "CRIS_SKINNY_BLOCKS", "CRIS_GEMM8_MIN_TILES", "CRIS_GEMM8_MIN_K", "CRIS_GEMM8_T128_LO", "CRIS_GEMM8_T128_HI", "CRIS_GEMM_NARROW_128",
    "CRIS_GEMM_T128_MIN", "CRIS_GEMM_T64_MAX", "CRIS_GEMM_KS2", "CRIS_GEMM_KS2_MAX_BLOCKS", "CRIS_GEMM_KS2_MIN_K", "CRIS_WGRAD8_MIN_N",
    "CRIS_WGRAD8_MIN_K", "CRIS_WGRAD8_MIN_M", "CRIS_WGRAD8_MI", "CRIS_BN_RED_BLOCKS", "CRIS_BN_RED_ROWS", "CRIS_LN_BWD_BLOCKS",
    "CRIS_ATTN_LDS_MIN", "CRIS_DYNCONV_PPB"]
# the switches the library keeps (a lower bound on what the scan must find: an empty scan would pass everything)
KEPT = {"CRIS_GEMM8", "CRIS_WGRAD8", "CRIS_SKINNY_SPLIT", "CRIS_BN_APPLY_FAST", "CRIS_LN_BWD_V", "CRIS_P2P_MEM", "CRIS_P2P_ARENA_BLOCKS",
        "CRIS_RCCL_LIB"}


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert files
    return {f: open(f).read() for f in files}


def _knob_paragraph():
    paragraphs = [p for p in open(os.path.join(ROOT, "README.md")).read().split("\n\n") if "Environment knobs" in p]
    assert len(paragraphs) == 1
    return paragraphs[0]


def test_every_environment_read_is_documented():
    names = {}
    for f, text in _sources().items():
        # every call, whatever its argument: one that does not pass a string literal (other than cris_env_int's own forwarding
        # getenv(name)) would hide its name from this test
        for call in re.finditer(r"\b(cris_env_int|getenv)\(\s*([^,)]*)", text):
            arg = call.group(2).strip()
            if call.group(1) == "getenv" and arg == "name" and os.path.basename(f) == "common.h":
                continue
            if call.group(1) == "cris_env_int" and arg == "const char* name":
                continue
            lit = re.fullmatch(r'"(\w+)"', arg)
            assert lit, "%s: %s(%s) does not name its variable with a string literal" % (os.path.basename(f), call.group(1), arg)
            names.setdefault(lit.group(1), os.path.basename(f))
    assert KEPT <= set(names), sorted(KEPT - set(names))
    documented = set(re.findall(r"`(\w+)`", _knob_paragraph()))
    missing = {n: f for n, f in names.items() if n not in documented}
    assert not missing, "read by the library, absent from README's environment-knob paragraph: %r" % missing


def test_retired_switches_stay_out_of_the_library():
    assert len(RETIRED) == len(set(RETIRED)) == 20
    for f, text in _sources().items():
        found = [n for n in RETIRED if re.search(r"\b%s\b" % n, text)]
        assert not found, "%s names retired environment switches: %r" % (os.path.basename(f), found)
