#!/bin/bash
# A hash, the instruction count and the static VALU count of every kernel instance's disassembly in a .hip object
# (the method behind profiles/*/disasm_hashes.txt): llvm-objdump -d of the gfx950 code object, per kernel symbol, with
# symbol names, address comments and the literal of each PC-relative s_add_u32 / s_addc_u32 (which moves with the
# object's layout) removed.
# Usage: tools/disasm_hashes.sh [object] [name pattern] [dump dir]
#   object:   default the in-tree build's trace.hip.o
#   pattern:  awk regex on the mangled kernel name, default trace_kernel
#   dump dir: if given, each instance's normalised listing is left there as <mangled name>.s
obj=${1:-shirley-raytracing-rs_amd/build/rt/trace.hip.o}
pat=${2:-trace_kernel}
dump=$3
llvm=/opt/rocm/lib/llvm/bin
tmp=$(mktemp -d)
$llvm/llvm-objcopy --dump-section=.hip_fatbin=$tmp/fb.bin "$obj" &&
$llvm/clang-offload-bundler --unbundle --type=o --input=$tmp/fb.bin \
  --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$tmp/k.co &&
$llvm/llvm-objdump -d --no-show-raw-insn $tmp/k.co | awk -v pat="$pat" -v dir="$tmp/s" '
  BEGIN { system("mkdir -p " dir) }
  /^[0-9a-f]+ <.*>:$/ { name = $2; gsub(/[<>:]/, "", name); keep = (name ~ pat && name !~ /\.kd$/); next }
  keep && NF {
    sub(/[ \t]*\/\/.*$/, "");                        # address comments
    gsub(/<[^>]*>/, "");                             # symbol names in branch targets
    if ($1 ~ /^s_addc?_u32$/ && $NF ~ /^0x/) $NF = "LIT";  # PC-relative address sums
    if (NF) print > (dir "/" name ".s")
  }'
for f in $tmp/s/*.s; do
  [ -e "$f" ] || continue
  n=$(basename "$f" .s)
  echo "$(md5sum < "$f" | cut -d' ' -f1) $(wc -l < "$f") $(grep -cE '^[[:space:]]*v_' "$f") $n"
  [ -n "$dump" ] && mkdir -p "$dump" && cp "$f" "$dump/"
done
rm -rf $tmp
