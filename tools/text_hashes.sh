#!/bin/bash
# sha256 of the gfx950 machine code in every object of a full build: the .text section of the device code object bundled into each
# .o.  Two builds whose lists agree carry byte-identical kernels, whatever changed on the host side (the code object as a whole also
# holds data derived from the source file's name, so it is the section that is compared).  With -t the sorted per-kernel table
# (name, code size, SGPRs, VGPRs, AGPRs, scratch, LDS) is hashed too: the weaker check for a unit whose layout had to move.
#   tools/text_hashes.sh [-t] [directory with the .o files, default: frankenz_amd/csrc]
set -e
TABLE=0
if [ "$1" = "-t" ]; then TABLE=1; shift; fi
DIR=${1:-$(dirname "$0")/../frankenz_amd/csrc}
BIN=${ROCM_PATH:-/opt/rocm}/llvm/bin
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
for o in "$DIR"/frankenz_hip.o "$DIR"/fz_inst_b*.o; do
  b=$(basename "$o" .o)
  "$BIN/llvm-objcopy" --dump-section .hip_fatbin="$TMP/$b.fat" "$o"
  "$BIN/clang-offload-bundler" --unbundle --type=o --input="$TMP/$b.fat" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$TMP/$b.co"
  "$BIN/llvm-objcopy" --dump-section .text="$TMP/$b.text" "$TMP/$b.co"
  line="$(sha256sum < "$TMP/$b.text" | cut -c1-64)  $b.text"
  if [ $TABLE = 1 ]; then
    "$BIN/llvm-readelf" --notes "$TMP/$b.co" | grep -E '\.(name|sgpr_count|vgpr_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size):' \
      | sed 's/^ *//' | paste -d' ' - - - - - - | sort > "$TMP/$b.meta"
    "$BIN/llvm-readelf" -sW "$TMP/$b.co" | awk '$4 == "FUNC" {print $8, $3}' | sort > "$TMP/$b.size"
    line="$line  table $(cat "$TMP/$b.meta" "$TMP/$b.size" | sha256sum | cut -c1-16) ($(wc -l < "$TMP/$b.meta") kernels)"
  fi
  echo "$line"
done
