#!/bin/bash
# Build an experiment variant of libshirley_rt.so into exp/<name>/ (for tools/gpu.sh ab steps).
# Usage: tools/variant.sh <name> [extra hipcc flags...]   e.g. tools/variant.sh phase -DRT_PHASE_TIMING
# A/B partners that rebuild an earlier commit's kernels from this tree (trace.hip; equal disassembly hashes, checked with
# tools/disasm_hashes.sh on /tmp/variant_<name>/build/rt/trace.hip.o):
#   tools/variant.sh s0 -DRT_SERVE_Y=0         the HOP = 4 instances with the general serve body alone (DESIGN.md §3.1 serve_y)
#   -DRT_GROUND_FIRST=0                        ... and without the traversal's closed-form answer (as when that change landed)
# Lane thresholds of the HOP = 4 passes: -DRT_HOP4D_MIN_LANES_A/B/C=<n> (down pass), -DRT_HOP4_MIN_LANES_A/B=<n> (step 5').
# The tree is copied, so a variant can also be made from edited sources: set SRC=<dir> (default: the
# in-tree package).  LICM_FLAG= (empty) builds without -disable-machine-licm; TRK_FLAG=<flags> adds scheduler flags.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
src=${SRC:-shirley-raytracing-rs_amd}
tmp=/tmp/variant_$name
rm -rf "$tmp" && mkdir -p "$tmp"
cp -r "$src"/csrc "$src"/Makefile "$tmp"/
mkdir -p "$tmp/../include" 2>/dev/null || true
cp -r include "$tmp/../" 2>/dev/null || true
make -C "$tmp" -j8 lib/libshirley_rt.so ARCH="${ARCH:-gfx950}" \
  HIPFLAGS="--offload-arch=${ARCH:-gfx950} -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function ${LICM_FLAG--mllvm -disable-machine-licm} ${TRK_FLAG-} $*" >/dev/null
mkdir -p exp/$name
cp "$tmp/lib/libshirley_rt.so" exp/$name/
cp shirley-raytracing-rs_amd/lib/libshirley_host.so exp/$name/
echo "exp/$name/libshirley_rt.so"
