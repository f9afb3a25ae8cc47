#!/bin/bash
# A/B builds of the library: tools/build_variant.sh <name> <file.hip> "<extra hipcc flags>" [<file2.hip> "<flags2>"]
# -> _ab/<name>/libgdrnpp_hip.so, built by csrc/Makefile (same flags, version script and hazard check as the default library) with
# the named translation units compiled with the extra flags.
# Select it with GDRNPP_HIP_LIB=_ab/<name>/libgdrnpp_hip.so (hip_lib.LIB_PATH).  _ab/ is git-ignored and travels with gpurun.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
out=$R/_ab/$name
args=()
while [ $# -gt 0 ]; do
  base=${1%.hip}
  rm -f "$out/$base.o"   # make does not see a change of flags
  args+=("FLAGS_$base=$2")
  shift 2
done
make -C "$R/gdrnpp_bop2022_amd/csrc" -j16 OUT="$out" "${args[@]}" > /dev/null
echo "built _ab/$name/libgdrnpp_hip.so"
