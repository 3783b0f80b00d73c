#!/bin/bash
# usage: tools/build_variant.sh <name> [patch.py]  — copies stratum_amd/csrc and include/ to /tmp/variants/<name>/, applies the
# given python patch file (argument 2, optional, run inside the csrc copy), and builds _variants/<name>.so with the product's
# flags plus $EXTRA_FLAGS. Variants may be built in parallel (each has its own tree).
# The sources are every .hip and .cpp of csrc/ (a glob: all of them are product sources, as __graft_entry__.PRODUCT_SOURCES
# lists them), so a new unit needs no second list here.
set -e
name=$1; patch=$2
root=$(cd "$(dirname "$0")/.." && pwd)
base=/tmp/variants/$name
d=$base/pkg/csrc
rm -rf $base; mkdir -p $base/pkg; cp -r $root/stratum_amd/csrc $d; cp -r $root/include $base/include
if [ -n "$patch" ]; then (cd $d && python3 $patch); fi
mkdir -p $root/_variants
# one hipcc process per translation unit (as __graft_entry__.build_product), then the link; a unit that does not compile stops
# the build before the link
mkdir -p $base/obj
pids=()
max_jobs=${MAX_JOBS:-16}  # at most this many hipcc processes at once (as __graft_entry__.build_product)
for src in $d/*.hip $d/*.cpp; do
  while [ $(jobs -rp | wc -l) -ge $max_jobs ]; do sleep 0.2; done
  f=$(basename $src)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-cuda-compat $EXTRA_FLAGS -c -o $base/obj/$f.o $src &
  pids+=($!)
done
failed=0
for pid in "${pids[@]}"; do wait $pid || failed=1; done
if [ $failed -ne 0 ]; then echo "build_variant: a translation unit of $name did not compile" >&2; exit 1; fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--no-undefined -o $root/_variants/$name.so $base/obj/*.o
echo built _variants/$name.so
