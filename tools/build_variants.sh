#!/bin/bash
# Cross-compiles engine variants (extra -D switches) into build/variants/ HERE (no GPU needed); they travel to
# the GPU box with the snapshot (build/ is git-ignored, not gpurun-ignored).  Usage: build_variants.sh "name:-Dflags" ...
# A variant is the Makefile's build with XFLAGS and its own object directory.  Its old library is deleted first and its compiler
# log kept (build/variants/<name>.log), so that a failed build can neither be overlooked nor leave a stale library to be timed.
# KFLAGS_AERO in the environment overrides the AERO unit's -mllvm flags, as it does for make.
cd "$(dirname "$0")/../gelato_amd/csrc" || exit 1
V=../../build/variants
mkdir -p $V
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}; [ "$flags" = "$spec" ] && flags=""
  rm -f $V/libgel_$name.so
  ( d=$(mktemp -d /tmp/gelvar.XXXXXX)
    make -j4 OBJDIR=$d OUT=$V/libgel_$name.so XFLAGS="$flags" > $V/$name.log 2>&1 \
      && echo "built $name [$flags]" || { echo "FAILED $name (build/variants/$name.log):"; tail -5 $V/$name.log; }
    rm -rf $d ) &
done
wait
