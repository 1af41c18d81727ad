#!/bin/sh
# Compare the gfx950 instruction streams of kernels between two objects (hipcc -c outputs): by default k_uct_select / k_uct_backup /
# k_uct_advance / k_uct_select_paths / k_uct_backup_paths / k_uct_select_puct of two k_uct objects.
#   tools/uct_isa_compare.sh OLD.o NEW.o [SYMBOL_REGEXP]
# Each object's gfx950 code object is extracted, disassembled, and cut into one listing per kernel symbol with addresses, raw encodings and
# branch-target comments dropped; the listings of the kernels whose (mangled) symbol matches the awk regexp must be identical.  A kernel
# is named by its template name and its action count (k_uct_select_pathsILi3E): a compile-time switch added after the count (a bool that
# is false, Lb0E, in the form that existed before) and the argument type do not enter the name, and the forms with the switch on (Lb1E)
# are new kernels, not compared.
set -e
ROCM=${ROCM_PATH:-/opt/rocm}
SYMS=${3:-'k_uct_(select|backup|advance|select_paths|backup_paths|select_puct)I'}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
for side in old new; do
    [ $side = old ] && obj=$1 || obj=$2
    cp "$obj" "$T/$side.o"
    "$ROCM"/lib/llvm/bin/llvm-objdump --offloading "$T/$side.o" > /dev/null    # writes $side.o.0.hipv4-amdgcn-amd-amdhsa--gfx950
    "$ROCM"/lib/llvm/bin/llvm-objdump -d --no-show-raw-insn "$T/$side.o".*gfx950 |
        awk -v syms="$SYMS" '/^[0-9a-f]+ <.*>:$/ { keep = ($2 ~ syms && $2 !~ /ILi[0-9]+ELb1E/); if (keep) { match($2, /k_uct_[a-z_]+ILi[0-9]+E/); print "<" substr($2, RSTART, RLENGTH) ">" } next }
             keep { sub(/^[ \t]*/, ""); sub(/[ \t]*\/\/.*$/, ""); if ($0 != "" && $0 != "...") print }' > "$T/$side.txt"
done
n=$(grep -c '^<' "$T/old.txt")
if cmp -s "$T/old.txt" "$T/new.txt"; then
    echo "identical: $n kernels, $(wc -l < "$T/old.txt") lines"
else
    diff "$T/old.txt" "$T/new.txt" | head -40
    exit 1
fi
