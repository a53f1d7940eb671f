#!/bin/bash
# A/B builds of libcris_hip.so: the same sources with extra -D switches, cross-compiled here (no GPU needed) into
# cris/pytorch_amd/csrc/variants/libcris_hip_<tag>.so (git-ignored, travels with gpurun); CRIS_LIB_VARIANT=<tag> loads one (hip.py).
#   tools/build_variants.sh "sc1:-DCRIS_STORE_POLICY=1" "nt:-DCRIS_STORE_POLICY=2"
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
