#!/bin/sh
# Device code of every csrc/*.hip at a git revision (default: main) against the working tree: a device-only code object
# built with the Makefile's own flags, then .text, .rodata (kernel descriptors) and the notes (registers, LDS) compared.
# A host-only change leaves all three identical (the __hip_cuid_* symbol name aside).
# Usage: tools/devcode_diff.sh [rev]      exit status 0: identical for every file
set -eu
REV=${1:-main}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=lk-s-2022-estimacija-pokreta_amd/csrc
ROCM=${ROCM_PATH:-/opt/rocm}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir -p "$TMP/base" "$TMP/tree/$SRC" "$TMP/tree/include"
git -C "$ROOT" archive "$REV" "$SRC" include | tar -x -C "$TMP/base"
cp "$ROOT/$SRC"/*.hip "$ROOT/$SRC"/*.h "$ROOT/$SRC/Makefile" "$TMP/tree/$SRC/"
cp "$ROOT"/include/*.h "$TMP/tree/include/"
# hipcc with the Makefile's flags, plus: device code only, as a plain code object
printf '#!/bin/sh\nexec %s/bin/hipcc "$@" --offload-device-only --no-gpu-bundle-output\n' "$ROCM" > "$TMP/hipcc"
chmod +x "$TMP/hipcc"
status=0
for f in $(cd "$TMP/tree/$SRC" && ls *.hip); do
    for side in base tree; do
        make -s -B -C "$TMP/$side/$SRC" HIPCC="$TMP/hipcc" "${f%.hip}.o" 2>/dev/null
        co="$TMP/$side/$SRC/${f%.hip}.o"
        for what in "-x .text" "-x .rodata" "--notes"; do
            "$ROCM/llvm/bin/llvm-readelf" $what "$co" 2>/dev/null | grep -v __hip_cuid_ || true
        done > "$TMP/$side.$f.dump"
    done
    if cmp -s "$TMP/base.$f.dump" "$TMP/tree.$f.dump"; then
        echo "identical  $f"
    else
        echo "DIFFERENT  $f"; status=1
    fi
done
exit $status
