#!/bin/bash
# Build the transport kernel of an earlier git revision as an A/B variant:
#   tools/build_rev.sh <rev> <name>  ->  cuda-grmonty_amd/ab/libgrmonty_amd_v<name>.so
# (csrc/ and include/ of <rev> as they are there, whichever of the known units it has; current host
#  objects; only for revisions with the same C ABI)
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"
rev=$1; name=$2
D="$R/cuda-grmonty_amd/build/rev_$name"
rm -rf "$D"; mkdir -p "$D"
git -C "$R" archive "$rev" cuda-grmonty_amd/csrc include | tar -x -C "$D"
S="$D/cuda-grmonty_amd/csrc"
make -s -C "$R/cuda-grmonty_amd" build/grm_host.o
FL="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-result -Wno-unused-value -mllvm -disable-machine-licm"
SF=""; [ -n "$SCHED" ] && SF="-mllvm -amdgpu-sched-strategy=$SCHED"  # revisions before 58fc566 were built with SCHED=iterative-ilp
objs=""; pids=""
for u in grm_engine grm_lone grm_split grm_probe grm_emit grm_tables grm_cellsums grm_rebin; do
  [ -f "$S/$u.hip" ] || continue
  case $u in
    grm_engine) fl="$FL $SF $VFLAGS";;
    grm_lone)   fl="${FL/-mllvm -disable-machine-licm/} -mllvm -amdgpu-sched-strategy=max-ilp $VFLAGS";;
    grm_split)  fl="$FL $VFLAGS";;
    *)          fl="$FL";;
  esac
  /opt/rocm/bin/hipcc $fl -c "$S/$u.hip" -o "$D/$u.o" &
  pids="$pids $!"; objs="$objs $D/$u.o"
done
for p in $pids; do wait "$p"; done
mkdir -p "$R/cuda-grmonty_amd/ab"
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o "$R/cuda-grmonty_amd/ab/libgrmonty_amd_v$name.so" \
  $objs "$R/cuda-grmonty_amd/build/grm_host.o" -L/opt/rocm/lib -lrccl -lpthread
echo "built ab/libgrmonty_amd_v$name.so from $rev"
