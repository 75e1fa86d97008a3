#!/bin/bash
# usage: tools/isa_diff.sh <csrc dir A> <csrc dir B>   -- the check for kernel refactors
# Compiles every *.hip unit of both directories to gfx950 device assembly with the flags of B's Makefile (JOBS at a time, default
# 14, at most 16; more flags through EXTRA=...) and prints one line per unit: "identical", or the number of differing lines
# and whether the per-kernel metadata (register counts, spills, scratch and LDS sizes) is equal.  Exit status 0 when every
# unit is identical; a unit that is missing or does not compile on either side counts as different.  Assembly is kept under OUT (default: a fresh temporary directory) for reading the differences:
# diff OUT/a/<unit>.s OUT/b/<unit>.s; KEEP_A=1 takes A's assembly from OUT/a as an earlier run left it.
set -u
[ $# -eq 2 ] || { echo "usage: $0 <csrc dir A> <csrc dir B>" >&2; exit 2; }
JOBS=${JOBS:-14}; [ "$JOBS" -le 16 ] || JOBS=16
OUT=${OUT:-$(mktemp -d)}
# FLAGS = ... of the Makefile, its $(ARCH) and $(EXTRA) filled in; the *_f64 rule's extra flags are repeated below
FLAGS=$(sed -n 's/^FLAGS *= *//p' "$2/Makefile" | sed "s/\$(ARCH)/gfx950/; s/\$(EXTRA)/${EXTRA:-}/")
[ -n "$FLAGS" ] || { echo "no FLAGS line in $2/Makefile" >&2; exit 2; }
compile() {   # <csrc dir> <out dir>
    mkdir -p "$2"
    (cd "$1" && ls *.hip) | xargs -P "$JOBS" -I{} sh -c '
        u={}; x=""; case $u in *_f64.hip) x="-mllvm -disable-machine-licm" ;; esac
        hipcc '"$FLAGS"' $x --offload-device-only -S "$0/$u" -o "$1/${u%.hip}.s" 2> "$1/${u%.hip}.log" || { rm -f "$1/${u%.hip}.s"; echo "$u: compile failed, see $1/${u%.hip}.log" >&2; }' "$1" "$2"
}
[ -n "${KEEP_A:-}" ] || compile "$1" "$OUT/a"
compile "$2" "$OUT/b"
meta() { grep -E '^ *\.(name|vgpr_count|sgpr_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):' "$1"; }
rc=0
for u in $( { (cd "$1" && ls *.hip); (cd "$2" && ls *.hip); } | sed 's/\.hip$//' | sort -u); do
    a="$OUT/a/$u.s"; b="$OUT/b/$u.s"
    [ -s "$a" ] || { echo "$u: no assembly for A (missing or failed to compile)"; rc=1; continue; }
    [ -s "$b" ] || { echo "$u: no assembly for B (missing or failed to compile)"; rc=1; continue; }
    # (the one symbol clang names after a hash of the unit's path, __hip_cuid_<hash>, is left out of the comparison)
    n=$(diff <(grep -v __hip_cuid_ "$a") <(grep -v __hip_cuid_ "$b") | grep -c '^[<>]')
    if [ "$n" -eq 0 ]; then echo "$u: identical"; continue; fi
    if [ "$(meta "$a")" = "$(meta "$b")" ]; then m=equal; else m=DIFFERENT; fi
    echo "$u: $n differing lines, metadata $m"; rc=1
done
echo "assembly kept in $OUT" >&2
exit $rc
