#!/bin/bash
# Build libseb_bloom.so from the product sources of a git revision into tools/ab_lib/NAME/ (CPU,
# here), for an A/B against the in-tree library on the box (SEB_LIB_PATH, tools/gpu_ab_lib.sh).
# The revision's own Makefile builds whatever files that revision has.
#   tools/rev_lib.sh NAME [REV]      (REV defaults to HEAD)
set -e
NAME=$1; REV=${2:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/tools/ab_lib/$NAME
SRC=$OUT/src
# git archive gives the sources the commit's time, so objects left by an earlier build under this
# NAME would look up to date: they go first
rm -rf "$SRC" "$OUT/obj" "$OUT/libseb_bloom.so" && mkdir -p "$SRC"
(cd "$ROOT" && git archive "$REV" storage-engines_amd/csrc include) | tar -x -C "$SRC"
make -s -j8 -C "$SRC/storage-engines_amd/csrc" OUTDIR="$OUT"
echo "$OUT/libseb_bloom.so"
