#!/bin/bash
# Register / spill / scratch / static-LDS figures of the kernel instances in a .hip object (code-object notes).
# Usage: tools/kstats.sh [object] [name pattern]
#   object:  default the in-tree build's trace.hip.o
#   pattern: awk regex on the mangled kernel name, default trace_kernel (the megakernel instances);
#            e.g. tools/kstats.sh shirley-raytracing-rs_amd/build/rt/direct.hip.o direct_kernel
# After a compiler update, re-check that the uniform nee_kernel instances (ADAPT = false, nee.hip.o) are what they
# were (their tile loop is a backward jump for the sake of these figures):
#   tools/kstats.sh shirley-raytracing-rs_amd/build/rt/nee.hip.o nee_kernel | sed 's/^[^ ]* *//' \
#     | diff - <(sed 's/^[^ ]* *//' profiles/nee_adaptive/kstats_new.txt)
# (an empty diff: all 60 keep their VGPRs, spills, SGPRs and scratch; if a new compiler moves them anyway, compare
# against a build of the kernel without the ADAPT parts before blaming the jump).
# Each line ends with the static LDS (`lds N`), which listings made before this field existed do not have.
obj=${1:-shirley-raytracing-rs_amd/build/rt/trace.hip.o}
pat=${2:-trace_kernel}
tmp=$(mktemp -d)
/opt/rocm/lib/llvm/bin/llvm-objcopy --dump-section=.hip_fatbin=$tmp/fb.bin "$obj" &&
/opt/rocm/lib/llvm/bin/clang-offload-bundler --unbundle --type=o --input=$tmp/fb.bin \
  --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$tmp/k.co &&
/opt/rocm/lib/llvm/bin/llvm-readelf --notes $tmp/k.co | awk -v pat="$pat" '
  /\.name:/ {name=$2}
  /\.sgpr_spill_count:/ {ss=$2} /\.vgpr_spill_count:/ {vs=$2} /\.vgpr_count:/ {vc=$2} /\.sgpr_count:/ {sc=$2}
  /\.private_segment_fixed_size:/ {ps=$2} /\.group_segment_fixed_size:/ {gs=$2}
  /\.wavefront_size:/ { if (name ~ pat) printf "%-60s vgpr %s (spill %s) sgpr %s (spill %s) scratch %s lds %s\n", name, vc, vs, sc, ss, ps, gs }'
rm -rf $tmp
