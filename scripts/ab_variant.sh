#!/bin/bash
# Developer helper: build ab/<name>.so = the library with ONE translation unit (or several: gemm,gemm256,gemm256_tn) recompiled
# under extra flags or from other sources: bash scripts/ab_variant.sh <name> <unit>[,<unit>...] [extra hipcc flags...]
# The other objects come from lib/*.o, which must be up to date (run csrc/build.sh first); the unit list, the flags and the
# staleness rule are csrc/units.sh's, the same as build.sh's.  With SRC=<file> the (single) unit is compiled from that file
# instead of csrc/<unit>.hip, with SRC=<directory> every named unit from <directory>/<unit>.hip (e.g. another commit's csrc/).
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
CSRC=$ROOT/mammo_clip_amd/csrc && . $CSRC/units.sh
NAME=$1; UNITS=${2//,/ }; shift 2
mkdir -p $ROOT/ab
trap 'rm -f $CSRC/_ab_*.hip' EXIT
for u in $UNITS; do
  SRCFILE=$CSRC/$u.hip
  if [ -d "$SRC" ]; then SRCFILE=$SRC/$u.hip; elif [ -n "$SRC" ]; then SRCFILE=$SRC; fi
  cp $SRCFILE $CSRC/_ab_$u.hip         # compiled from inside csrc/, so that its includes resolve as the library's do
  hipcc $FLAGS "$@" -c $CSRC/_ab_$u.hip -o $ROOT/ab/${NAME}_$u.o
done
objs=""
for f in $SRCS; do
  case " $UNITS " in
    *" $f "*) objs="$objs $ROOT/ab/${NAME}_$f.o" ;;
    *) if unit_stale $ROOT/mammo_clip_amd/lib $f; then echo "lib/$f.o is missing or stale: run csrc/build.sh first" >&2; exit 1; fi
       objs="$objs $ROOT/mammo_clip_amd/lib/$f.o" ;;
  esac
done
hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/ab/$NAME.so $objs
echo "built ab/$NAME.so"
