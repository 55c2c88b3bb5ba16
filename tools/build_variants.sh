#!/bin/bash
# Build A/B variants of lib/libdpe_mvs.so into dpe-mvs_amd/lib/variants/<name>.so (in parallel).
# Usage: tools/build_variants.sh "name:-DFLAG=1 -DOTHER=2" "base:" ...
# The units and their flags are the Makefile's table; the flags given here apply to every unit, and
# flags after a second colon ("name:all flags:main-unit flags") to csrc/dpe_mvs.hip only (the pass).
# TAP_SCHED / F32_SCHED / MAIN_FLAGS in the environment override the Makefile's defaults.
cd "$(dirname "$0")/../dpe-mvs_amd" || exit 1
jobs=$(( $# > 16 ? 1 : 16 / ($# > 0 ? $# : 1) ))   # at most 16 compilers over up to 16 variants
pids=()
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}; mflags=
  [[ $flags == *:* ]] && { mflags=${flags#*:}; flags=${flags%%:*}; }
  make -s -B -j$jobs OBJDIR=obj/variants/$name OUT=lib/variants/$name.so EXTRA_FLAGS="-w $flags" MAIN_EXTRA="$mflags" \
    lib/variants/$name.so &
  pids+=($!)
done
rc=0
for p in "${pids[@]}"; do wait $p || rc=1; done
exit $rc
