#!/bin/bash
# Build libewk.so from a git revision (or the working tree with "WT") into variants/<name>.so,
# optionally with extra -D flags:  scripts/build_variant.sh <rev|WT> <name> [-DFOO=1 ...]
# The sources are every *.hip and *.cpp the revision has in csrc/ (beside every header there).
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"
REV=$1; NAME=$2; shift 2
C=easywakeword_amd/csrc
T=$(mktemp -d)
mkdir -p "$T/$C" "$T/include" "$R/variants"
if [ "$REV" = "WT" ]; then
  cp "$R/$C"/*.hip "$R/$C"/*.cpp "$R/$C"/*.h "$T/$C/"
  cp "$R/include/ewk.h" "$T/include/ewk.h"
else
  git -C "$R" archive "$REV" "$C" include/ewk.h | tar -x -C "$T"
fi
objs=""
for f in "$T/$C"/*.hip "$T/$C"/*.cpp; do
  s=$(basename "$f")
  x=""; [ "$s" = ewk_mfcc.hip ] && x="-fno-slp-vectorize"   # as easywakeword_amd/build.py EXTRA
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function $x "$@" \
     -c "$f" -o "$T/$s.o" &
  objs="$objs $T/$s.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$R/variants/$NAME.so" $objs
rm -rf "$T"
echo "$R/variants/$NAME.so"
