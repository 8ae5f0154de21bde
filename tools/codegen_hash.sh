#!/bin/bash
# Print a hash of the device code of each engine unit, as the Makefile and tools/build_variant.sh
# build it: one line per build with the unit, its extra flags and the sha256 of its disassembly.
#   tools/codegen_hash.sh [tree]     (tree: the root of a checkout, default this one; needs no GPU)
# A change that only moves source text leaves every line as it was; run it on both trees to see.
set -e -o pipefail
R="$(cd "${1:-$(dirname "$0")/..}" && pwd)"
LLVM=/opt/rocm/llvm/bin
T="$(mktemp -d)"; trap 'rm -r "$T"' EXIT
FL="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-result -Wno-unused-value -mllvm -disable-machine-licm"
LONE_FL="${FL/-mllvm -disable-machine-licm/} -mllvm -amdgpu-sched-strategy=max-ilp"

# hash <unit> <label> <flags...>: the disassembly without its header (it names the object file)
hash() {
  local unit=$1 label=$2; shift 2
  local o="$T/$unit$label.o"
  /opt/rocm/bin/hipcc "$@" --cuda-device-only --no-gpu-bundle-output -c "$R/cuda-grmonty_amd/csrc/$unit.hip" -o "$o"
  printf '%-10s %-16s %s\n' "$unit" "${label:-product}" \
    "$($LLVM/llvm-objdump -d "$o" | sed '1,/file format/d' | sha256sum | cut -d' ' -f1)" > "$o.txt"
}
hash grm_engine "" $FL &
hash grm_engine -DGRM_TIMING $FL -DGRM_TIMING &
hash grm_lone "" $LONE_FL &
hash grm_lone -DGRM_TIMING $LONE_FL -DGRM_TIMING &
hash grm_split -DGRM_WITH_SPLIT $FL -DGRM_WITH_SPLIT &
wait
cat "$T/grm_engine.o.txt" "$T/grm_engine-DGRM_TIMING.o.txt" "$T/grm_lone.o.txt" "$T/grm_lone-DGRM_TIMING.o.txt" \
  "$T/grm_split-DGRM_WITH_SPLIT.o.txt"
