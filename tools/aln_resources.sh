#!/bin/bash
# Compiler-reported resources and instruction counts of every alignment score kernel:
#     tools/aln_resources.sh [csrc directory = prograph_amd/csrc of this tree] [work directory = a fresh temporary one]
# One line per kernel instance: VGPRs, SGPRs, occupancy (waves/SIMD), LDS bytes per block, scratch bytes per lane and the
# instructions between the kernel's label and its s_endpgm.  The flags are the Makefile's.  profiles/aln_frame_resources.txt
# holds the output for two trees; tests/test_alignment_resources_cpu.py asserts the occupancy, scratch and LDS columns.
HERE=$(cd "$(dirname "$0")/.." && pwd)
SRC=${1:-$HERE/prograph_amd/csrc}
WORK=${2:-$(mktemp -d)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FILES="pg_aln pg_aln_affine pg_aln_local pg_aln_long pg_aln_semiglobal pg_aln_fit"
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -Wno-pass-failed"
mkdir -p "$WORK"
for f in $FILES; do
  (cd "$SRC" && $HIPCC $FLAGS -Rpass-analysis=kernel-resource-usage -S --cuda-device-only $f.hip -o "$WORK/$f.s" 2> "$WORK/$f.remarks") &
done
wait
printf '%-74s %5s %5s %4s %6s %7s %6s\n' kernel VGPRs SGPRs occ LDS scratch insts
for f in $FILES; do
  grep -q "error:" "$WORK/$f.remarks" && { grep "error:" "$WORK/$f.remarks" | head -5; exit 1; }
  sed 's/ *\[-Rpass-analysis=kernel-resource-usage\]//' "$WORK/$f.remarks" | awk -v asm="$WORK/$f.s" '
    BEGIN { while ((getline line < asm) > 0) {
              if (line ~ /^_Z[A-Za-z0-9_]+:/) { cur = line; sub(/:.*/, "", cur); n[cur] = 0; open = 1 }
              else if (open && line ~ /^\t[a-z]/) { n[cur]++; if (line ~ /^\ts_endpgm/) open = 0 } } }
    /remark: Function Name:/ { name = $0; sub(/.*Function Name: /, "", name); sub(/ .*/, "", name) }
    / TotalSGPRs: /          { s = $NF }
    / VGPRs: /               { v = $NF }
    /ScratchSize/            { sc = $NF }
    /Occupancy/              { o = $NF }
    /LDS Size/               { print name, v, s, o, $NF, sc, n[name] }
  '
done | while read -r name v s o l sc n; do
  short=$(echo "$name" | sed -E 's/^_Z[0-9]+//; s/Ev.*/>/; s/I/</; s/Lb0E/false,/; s/Lb1E/true,/; s/DF16_>/f16>/; s/x>/i64>/; s/i>/i32>/')
  # a class among the template arguments is length-prefixed: <13AlnGlobalLongi32> -> <AlnGlobalLong,i32>
  if [[ $short =~ ^([a-z0-9_]+)\<([0-9]+)(.*)$ ]]; then
    k=${BASH_REMATCH[2]}; rest=${BASH_REMATCH[3]}; short="${BASH_REMATCH[1]}<${rest:0:k},${rest:k}"
  fi
  printf '%-74s %5s %5s %4s %6s %7s %6s\n' "$short" "$v" "$s" "$o" "$l" "$sc" "$n"
done
