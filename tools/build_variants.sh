#!/bin/bash
# A/B builds of libcris_hip.so: the same sources with extra compiler flags, cross-compiled here (no GPU needed) into
# cris/pytorch_amd/csrc/variants/libcris_hip_<tag>.so (git-ignored, travels with gpurun); CRIS_LIB_VARIANT=<tag> loads one (hip.py).
#   tools/build_variants.sh "o2:-O2" "base:"
# Run from a checkout of another commit it builds that commit's library the same way ("parent:"): copied into this tree's
# variants/ it is the other side of an A/B of two commits whose Python side is the same (profiles/strip_scaffolding.md).
set -e
cd "$(dirname "$0")/../cris/pytorch_amd/csrc"
mkdir -p variants
# source list and flags are build.py's, so that an A/B build cannot go stale against the library
SRC="$(python build.py --print-sources)"
FLAGS="$(python build.py --print-flags)"
for spec in "$@"; do
  tag="${spec%%:*}"; extra="${spec#*:}"
  d=variants/obj_$tag; mkdir -p $d
  for f in $SRC; do
    /opt/rocm/bin/hipcc $FLAGS $extra -c $f -o $d/${f%.hip}.o 2>/dev/null &
  done
  wait
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o variants/libcris_hip_$tag.so $d/*.o
  rm -rf $d
  echo "built variants/libcris_hip_$tag.so ($extra)"
done
