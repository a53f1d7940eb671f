#!/usr/bin/env python
"""Compare two device-assembly files (hipcc <FLAGS> --cuda-device-only -S file.hip -o file.s) kernel by kernel: the set of
kernel symbols, each kernel's instruction sequence (mnemonics and operands; comments dropped, local labels renumbered in
order of appearance) and its register / scratch / LDS figures from the code-object metadata.  Prints one table row per kernel
and exits 1 when anything differs.   tools/isa_compare.py parent/gemm.s new/gemm.s [--md]"""
import re
import sys

FIELDS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".group_segment_fixed_size"]


def parse(path):
    text = open(path).read().splitlines()
    kernels = [l.split()[1] for l in text if l.startswith("\t.amdhsa_kernel ") or l.startswith(".amdhsa_kernel ")]
    body, cur, labels = {}, None, {}
    for l in text:
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if m and m.group(1) in kernels:
            cur, labels = m.group(1), {}
            body[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", l):
            cur = None
            continue
        l = l.split(";")[0].strip()
        if not l or (l.startswith(".") and not l.endswith(":")):
            continue
        l = re.sub(r"\.LBB\d+_\d+|\.Lpost_getpc\d+", lambda k: labels.setdefault(k.group(0), "L%d" % len(labels)), l)
        body[cur].append(" ".join(l.split()))
    meta, entry = {}, None
    for l in text:
        if l.startswith("  - ."):
            entry = {}
            l = "    " + l[4:]
        if entry is not None and l.startswith("    ."):
            k, _, v = l.strip().partition(":")
            entry[k] = v.strip()
            if k == ".name":
                meta[entry[".name"]] = entry
    return body, meta


def main():
    a_body, a_meta = parse(sys.argv[1])
    b_body, b_meta = parse(sys.argv[2])
    md = "--md" in sys.argv
    bad = 0
    if set(a_body) != set(b_body):
        print("kernel sets differ: only in parent %r, only in new %r" % (sorted(set(a_body) - set(b_body)), sorted(set(b_body) - set(a_body))))
        bad = 1
    sep = " | " if md else "\t"
    print(sep.join(["kernel", "instructions parent/new", "vgpr", "agpr", "sgpr", "scratch", "spills", "lds", "identical"]))
    if md:
        print(sep.join(["---"] * 9))
    for k in sorted(set(a_body) & set(b_body)):
        fa = [a_meta[k].get(f, "?") for f in FIELDS]
        fb = [b_meta[k].get(f, "?") for f in FIELDS]
        same = a_body[k] == b_body[k] and fa == fb
        bad |= not same
        name = k
        try:
            import subprocess
            name = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt", k], stdout=subprocess.PIPE).stdout.decode().strip() or k
        except OSError:
            pass
        name = re.sub(r"^void ", "", name).split("(")[0]
        cols = [x if x == y else "%s/%s" % (x, y) for x, y in zip(fa, fb)]
        print(sep.join([("`%s`" % name) if md else name, "%d/%d" % (len(a_body[k]), len(b_body[k]))] + cols + ["yes" if same else "NO"]))
    return bad


if __name__ == "__main__":
    sys.exit(main())
