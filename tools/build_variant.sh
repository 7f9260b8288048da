#!/bin/bash
# build_variant.sh <name> [FLAG ...] : builds an experimental libmas_hip variant into make-a-scene_amd/csrc/build/variants/<name>.so
# Every file gets the flags mas_hip/build.py gives it (the per-file ones included), then the extra ones.
set -e
name=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/make-a-scene_amd/csrc/build/variants /tmp/var_$name
for f in $R/make-a-scene_amd/csrc/*.hip; do
  b=$(basename $f .hip)
  hipcc $(python3 $R/make-a-scene_amd/mas_hip/build.py --flags $b.hip) "$@" -c $f -o /tmp/var_$name/$b.o &
done
wait
hipcc --offload-arch=gfx950 -shared -fPIC -o $R/make-a-scene_amd/csrc/build/variants/$name.so /tmp/var_$name/*.o
echo built $R/make-a-scene_amd/csrc/build/variants/$name.so
