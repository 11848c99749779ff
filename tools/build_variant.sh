#!/bin/bash
# A variant build of the library for same-box A/Bs (SMX_LIB_PATH, tools/ab_libs.sh):
#   bash tools/build_variant.sh <name> "<extra flags>" [file.hip[=replacement.hip] ...]   -> build/ab/libsmx_<name>.so
# Every listed file of build.SOURCES (default: smx_recon.hip) is recompiled with the flags -- from the replacement source where
# one is given -- and linked with the other objects of the in-tree build, which must be current (python -m surfelmeshing_amd.build).
set -e
NAME=$1; EXTRA=$2; shift; shift
[ $# -gt 0 ] || set -- smx_recon.hip
ROOT=$(cd "$(dirname "$0")/.." && pwd); C=$ROOT/surfelmeshing_amd/csrc; O=$ROOT/build/ab/obj_$NAME
mkdir -p $O
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -I $ROOT/include -I $C"
SOURCES=$(cd $ROOT && python3 -c "from surfelmeshing_amd.build import SOURCES; print(' '.join(SOURCES))")
for a in "$@"; do
  echo " $SOURCES " | grep -q " ${a%%=*} " || { echo "${a%%=*} is not in build.SOURCES" >&2; exit 1; }
done
OBJS=""; PIDS=""
for s in $SOURCES; do
  b=${s%.*}; src=""
  for a in "$@"; do
    if [ "${a%%=*}" = $s ]; then src=$C/$s; [ "$a" = "${a#*=}" ] || src=${a#*=}; fi
  done
  if [ -n "$src" ]; then
    /opt/rocm/bin/hipcc $FLAGS $EXTRA -x hip -c $src -o $O/$b.o & PIDS="$PIDS $!"
    OBJS="$OBJS $O/$b.o"
  else
    OBJS="$OBJS $C/$b.o"
  fi
done
for p in $PIDS; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/build/ab/libsmx_$NAME.so $OBJS
echo build/ab/libsmx_$NAME.so
