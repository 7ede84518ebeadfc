#!/bin/bash
# Static ISA report of one kernel of the library (no GPU needed).  Usage: tools/isa_lean.sh [kernel_substring] [extra hipcc flags]
# kernel_substring: a piece of the mangled name that starts with the kernel's own, e.g. k_shade_leanILb0ELi1ELb0 or k_msaa_detect; the unit that
# defines the kernel is found by that name.  Leaves the unit's assembly and the kernel's in $TMPDIR/isa (for tools/isa_diff.py: whole directories).
K=${1:-k_shade_leanILb0ELi0ELb0}; shift
TOOLS="$(cd "$(dirname "$0")" && pwd)"
cd "$TOOLS/../awsm-renderer_amd/csrc" || exit 1
UNIT=$(grep -l "void ${K%%IL*}(" *.hip | head -1)
[ -n "$UNIT" ] || { echo "no unit in $(pwd) defines a kernel ${K%%IL*}" >&2; exit 1; }
OUT="${TMPDIR:-/tmp}/isa"; mkdir -p "$OUT"
/opt/rocm/bin/hipcc $(make -s print-CXXFLAGS) --cuda-device-only -S "$@" -o "$OUT/${UNIT%.hip}.s" "$UNIT" 2>&1 | grep -v "hip-link"
python "$TOOLS/isa_cost.py" "$OUT/${UNIT%.hip}.s" $K | head -4
L=$(grep -n "^_ZN4awsm[0-9]*$K" "$OUT/${UNIT%.hip}.s" | head -1 | cut -d: -f1)
awk -v s=$L 'NR>=s' "$OUT/${UNIT%.hip}.s" | awk '/s_endpgm/{print; exit} {print}' > "$OUT/kernel.s"
awk -v s=$L 'NR>=s' "$OUT/${UNIT%.hip}.s" | grep -m4 "NumVgprs\|ScratchSize\|Occupancy\|LDSByteSize"
