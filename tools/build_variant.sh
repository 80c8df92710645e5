#!/bin/bash
# Builds a variant of libdeff_amd.so with extra compiler flags into tools/ab/<name>.so (git-ignored, travels with gpurun):
#   tools/build_variant.sh fence2 -DTB_FENCE_EVERY=2
# run it against the in-tree build with DEFF_AMD_LIB=tools/ab/<name>.so python tools/kbench.py ...
# The sweep kernels live in four units (api_sweep.hip and the three tiles_*.hip): those are compiled again, side by side, with
# the extra flags; the other objects are taken from the in-tree build (csrc/build/).
# Prints the VGPR / scratch budget of the streaming kernel's instantiations as a by-product.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
src=$root/effectivediffusivityfvm_amd/csrc
out=$root/tools/ab
sweep_units="tiles_tall tiles_8wave tiles_12wave api_sweep"
rest="build/api_core.o build/api_dict.o build/api_solve.o build/api_slab.o build/api_residual.o build/api_cg.o"
mkdir -p "$out/obj_$name"
make -s -C "$src" $rest
pids=
for u in $sweep_units; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden \
        -Wno-unused-function -Rpass-analysis=kernel-resource-usage "$@" -c -o "$out/obj_$name/$u.o" "$src/$u.hip" 2> "$out/obj_$name/$u.usage.txt" &
    pids="$pids $!"
done
for p in $pids; do wait $p; done
objs=
for u in $sweep_units; do objs="$objs $out/obj_$name/$u.o"; cat "$out/obj_$name/$u.usage.txt"; done > "$out/$name.usage.txt"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o "$out/$name.so" $objs $(cd "$src" && for o in $rest; do echo "$src/$o"; done) -L/opt/rocm/lib -lrccl
rm -rf "$out/obj_$name"
python3 - "$out/$name.usage.txt" <<'PY'
import re, sys
cur = None
for line in open(sys.argv[1]):
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1)
        continue
    if cur and "k_sweep_matfree_tbILi8ELb0ELb0E" in cur:
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m:
            print(" ", m.group(1), m.group(2))
PY
echo "$out/$name.so"
