#!/bin/bash
# usage: tools/build_variant.sh NAME "-DD2G_BS_EXP=1 ..."  -> dashing2_amd/libd2g_NAME.so (experiments; select with D2G_LIB=...)
set -e
cd "$(dirname "$0")/../dashing2_amd/csrc"
name=$1; shift
tmp=/tmp/d2g_variant_$name; mkdir -p $tmp
# the HIP sources are the library's own list: HIPSRC of csrc/Makefile
for f in $(sed -n 's/^HIPSRC *= *//p' Makefile); do
  f=${f%.hip}
  /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -ffp-contract=off "$@" -c $f.hip -o $tmp/$f.o &
done
g++ -O2 -std=c++17 -fPIC -fopenmp -c d2g_host.cpp -o $tmp/d2g_host.o &
g++ -O2 -std=c++17 -fPIC -c d2g_plan.cpp -o $tmp/d2g_plan.o &
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libd2g_$name.so $tmp/*.o -lz -lgomp -ldl
echo built dashing2_amd/libd2g_$name.so
