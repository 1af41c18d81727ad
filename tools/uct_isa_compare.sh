#!/bin/sh
# Compare the gfx950 instruction streams of kernels between two objects (hipcc -c outputs): by default k_uct_select / k_uct_backup /
# k_uct_advance / k_uct_select_paths / k_uct_backup_paths / k_uct_select_puct of two k_uct objects.
#   tools/uct_isa_compare.sh OLD.o NEW.o [SYMBOL_REGEXP] [all]
# Each object's gfx950 code object is extracted, disassembled, and cut into one listing per kernel symbol with addresses, raw encodings and
# branch-target comments dropped; the listings of the kernels whose (mangled) symbol matches the awk regexp must be identical.  A kernel
# is named by its template name and its action count (k_uct_select_pathsILi3E): a compile-time switch added after the count (a bool that
# is false, Lb0E, in the form that existed before) and the argument type do not enter the name, and the forms with the switch on (Lb1E)
# are new kernels, not compared.
# With `all` as the fourth argument (or UCT_ISA_ALL=1) every instantiation of the unit is compared, a refactor's check: a kernel is named
# by its template name and its whole template argument list (k_uct_select_puctILi3ELb1ELb1ELb0EE), still not by its argument struct, and
# SYMBOL_REGEXP defaults to every k_uct_ kernel.  Per kernel it prints VGPRs (with AGPRs), SGPRs, LDS and scratch bytes from the code
# object's notes, the waves per SIMD that follow from them (8 registers per VGPR allocation, 512 per lane and SIMD; 800 SGPRs per SIMD
# in blocks of 16 plus 16; 160 KiB of LDS per CU of four SIMDs), old -> new, and whether the listing is the same; it fails if one differs.
set -e
ROCM=${ROCM_PATH:-/opt/rocm}
ALL=${UCT_ISA_ALL:-0}
[ "$4" = all ] && ALL=1
if [ "$ALL" = 1 ]; then SYMS=${3:-'k_uct_'}; else SYMS=${3:-'k_uct_(select|backup|advance|select_paths|backup_paths|select_puct)I'}; fi
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
for side in old new; do
    [ $side = old ] && obj=$1 || obj=$2
    cp "$obj" "$T/$side.o"
    "$ROCM"/lib/llvm/bin/llvm-objdump --offloading "$T/$side.o" > /dev/null    # writes $side.o.0.hipv4-amdgcn-amd-amdhsa--gfx950
    "$ROCM"/lib/llvm/bin/llvm-objdump -d --no-show-raw-insn "$T/$side.o".*gfx950 |
        awk -v syms="$SYMS" -v all="$ALL" '
             BEGIN { key = all == 1 ? "k_uct_[a-z_]+(I(L[a-z][0-9]+E)+E)?" : "k_uct_[a-z_]+ILi[0-9]+E" }
             /^[0-9a-f]+ <.*>:$/ { keep = ($2 ~ syms && (all == 1 || $2 !~ /ILi[0-9]+ELb1E/))
                                   if (keep) { match($2, key); print "<" substr($2, RSTART, RLENGTH) ">" } next }
             keep { sub(/^[ \t]*/, ""); sub(/[ \t]*\/\/.*$/, ""); if ($0 != "" && $0 != "...") print }' > "$T/$side.txt"
    [ "$ALL" = 1 ] || continue
    # name vgpr sgpr lds scratch waves, one line per kernel, from the notes
    "$ROCM"/lib/llvm/bin/llvm-readelf --notes "$T/$side.o".*gfx950 |
        awk -v syms="$SYMS" '
             function put() { if (name ~ syms) { match(name, /k_uct_[a-z_]+(I(L[a-z][0-9]+E)+E)?/); v = int((vg + ag + 7) / 8) * 8; w = 8
                                  if (v > 0 && int(512 / v) < w) w = int(512 / v)
                                  s = int(800 / (int((sg + 15) / 16) * 16 + 16)); if (s < w) w = s
                                  if (lds > 0) { l = int(int(163840 / lds) * (wg / 64) / 4); if (l < w) w = l }
                                  print substr(name, RSTART, RLENGTH), vg + ag, sg, lds, scr, w } name = "" }
             $1 == "-" && $2 == ".agpr_count:" { put(); ag = $3 }
             $1 == ".agpr_count:" { ag = $2 }
             $1 == ".vgpr_count:" { vg = $2 }
             $1 == ".sgpr_count:" { sg = $2 }
             $1 == ".group_segment_fixed_size:" { lds = $2 }
             $1 == ".private_segment_fixed_size:" { scr = $2 }
             $1 == ".max_flat_workgroup_size:" { wg = $2 }
             $1 == ".name:" { name = $2 }
             END { put() }' | sort > "$T/$side.res"
done
n=$(grep -c '^<' "$T/old.txt")
if [ "$ALL" = 1 ]; then
    for side in old new; do     # one file per kernel, named by its key
        mkdir "$T/$side.d"
        awk -v d="$T/$side.d" '/^</ { f = d "/" substr($0, 2, length($0) - 2) } { print > f }' "$T/$side.txt"
    done
    rc=0
    printf '%-46s %9s %9s %11s %9s %7s  %s\n' kernel VGPR SGPR LDS scratch waves listing
    for k in $( (ls "$T/old.d"; ls "$T/new.d") | sort -u); do
        o=$(awk -v k="$k" '$1 == k' "$T/old.res"); w=$(awk -v k="$k" '$1 == k' "$T/new.res")
        if [ ! -f "$T/old.d/$k" ]; then same="new only"; rc=1
        elif [ ! -f "$T/new.d/$k" ]; then same="old only"; rc=1
        elif cmp -s "$T/old.d/$k" "$T/new.d/$k"; then same=identical
        else same="DIFFERS ($(wc -l < "$T/old.d/$k") -> $(wc -l < "$T/new.d/$k") lines)"; rc=1; fi
        set -- $o; ov=${2:--} os=${3:--} ol=${4:--} oc=${5:--} ow=${6:--}
        set -- $w; nv=${2:--} ns=${3:--} nl=${4:--} nc=${5:--} nw=${6:--}
        printf '%-46s %9s %9s %11s %9s %7s  %s\n' "$k" "$ov->$nv" "$os->$ns" "$ol->$nl" "$oc->$nc" "$ow->$nw" "$same"
    done
    [ $rc = 0 ] && echo "identical: $n kernels, $(wc -l < "$T/old.txt") lines"
    exit $rc
fi
if cmp -s "$T/old.txt" "$T/new.txt"; then
    echo "identical: $n kernels, $(wc -l < "$T/old.txt") lines"
else
    diff "$T/old.txt" "$T/new.txt" | head -40
    exit 1
fi
