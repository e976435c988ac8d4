#!/bin/bash
# Build a tuning variant of the library: bash tools/build_variant.sh <name> "<extra hipcc flags>"
# -> variants/lib_<name>.so (git-ignored; select with SW_LIB_PATH=variants/lib_<name>.so)
# The sources are the Makefile's SRCS: _lib.load() looks up every prototype, a library short of one file does not load.
set -e
cd $(dirname $0)/..
N=$1; X=$2
SRCS=$(sed -n 's/^SRCS *= *//p' socialways_amd/csrc/Makefile)
[ -n "$SRCS" ] || { echo "no SRCS line in socialways_amd/csrc/Makefile" >&2; exit 1; }
mkdir -p variants/obj_$N
pids=
for f in $SRCS; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function -fno-gpu-rdc -fno-slp-vectorize $X -c socialways_amd/csrc/$f -o variants/obj_$N/${f%.hip}.o &
  pids="$pids $!"
done
for p in $pids; do wait $p; done      # `wait` alone hides a failed compile
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC variants/obj_$N/*.o -o variants/lib_$N.so
rm -rf variants/obj_$N
ls -la variants/lib_$N.so
