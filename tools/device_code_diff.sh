#!/bin/bash
# usage: tools/device_code_diff.sh OBJDIR_A OBJDIR_B [WORKDIR]     (OBJDIR: signed-heat-3d_amd/lib/obj of a build)
# Compares the gfx950 device code of two builds kernel by kernel: what a host-only change must leave identical.  Per object file the .hip_fatbin section is
# unbundled and disassembled, the text is cut per symbol and the trailing "// address: encoding" comments are dropped.  Symbols are then "identical", "literal only"
# (they differ in nothing but the 32-bit literal of a PC-relative s_add_u32 / s_addc_u32, which moves when code before a constant table disappears), "DIFFERENT",
# or present on one side only.  Exit status 1 if any symbol is DIFFERENT or exists only in B.
set -euo pipefail
LLVM=${ROCM_PATH:-/opt/rocm}/llvm/bin
W=${3:-$(mktemp -d)}
for side in A B; do
    dir=$1; [ $side = B ] && dir=$2
    rm -rf "$W/$side"; mkdir -p "$W/$side"
    for o in "$dir"/*.o; do
        u=$(basename "$o" .o)
        "$LLVM/llvm-objcopy" -O binary --only-section=.hip_fatbin "$o" "$W/$side/$u.fatbin"
        [ -s "$W/$side/$u.fatbin" ] || continue
        "$LLVM/clang-offload-bundler" --unbundle --type=o --input="$W/$side/$u.fatbin" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$W/$side/$u.co"
        "$LLVM/llvm-objdump" -d --no-show-raw-insn --no-leading-addr "$W/$side/$u.co" | sed -E 's,[[:space:]]*//.*$,,' |
            awk -v pre="$W/$side/$u." '/^<.*>:$/ { name = $0; gsub(/[<>:]/, "", name); f = pre name ".s"; next } f { print > f }'
    done
done
lit() { sed -E 's/^([[:space:]]*s_addc?_u32 [^,]+, [^,]+, )(0x[0-9a-f]+|-?[0-9]+)$/\1LIT/' "$1"; }
same=0; litonly=0; bad=0
for f in "$W"/B/*.s; do
    s=$(basename "$f")
    if [ ! -f "$W/A/$s" ]; then echo "only in B: ${s%.s}"; bad=$((bad + 1))
    elif cmp -s "$W/A/$s" "$f"; then same=$((same + 1))
    elif cmp -s <(lit "$W/A/$s") <(lit "$f"); then echo "literal only: ${s%.s}"; litonly=$((litonly + 1))
    else echo "DIFFERENT: ${s%.s}"; bad=$((bad + 1)); fi
done
for f in "$W"/A/*.s; do [ -f "$W/B/$(basename "$f")" ] || echo "only in A: $(basename "$f" .s)"; done
echo "identical $same, literal only $litonly, different or new $bad"
[ $bad -eq 0 ]
