#!/bin/bash
# Build a diagnostic variant of libseb_bloom.so into tools/ab_lib/NAME/ (CPU, here): the product
# sources are copied with their Makefile, the given tools/diag/*.patch files applied to the copy,
# extra -D flags passed to hipcc.  The product sources carry no diagnostic code paths.
#   tools/diag_lib.sh NAME [PATCH...] [-- -DFLAG...]      e.g. tools/diag_lib.sh nogather phase_no_gather
# Run it on the box with SEB_LIB_PATH=tools/ab_lib/NAME/libseb_bloom.so.
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/tools/ab_lib/$NAME
SRC=$OUT/src
rm -rf "$SRC" && mkdir -p "$SRC/storage-engines_amd/csrc" "$SRC/include"
cp "$ROOT"/storage-engines_amd/csrc/{*.hip,*.h,*.cpp,Makefile} "$SRC/storage-engines_amd/csrc/"
cp "$ROOT"/include/*.h "$SRC/include/"
FLAGS=()
while [ $# -gt 0 ]; do
  if [ "$1" = "--" ]; then shift; FLAGS=("$@"); break; fi
  patch -s -d "$SRC" -p1 < "$ROOT/tools/diag/$1.patch"
  shift
done
make -s -j8 -C "$SRC/storage-engines_amd/csrc" OUTDIR="$OUT" EXTRAFLAGS="${FLAGS[*]}"
echo "$OUT/libseb_bloom.so"
