#!/bin/bash
# usage: tools/build_variant.sh NAME "-DD2G_BS_EXP=1 ..."  -> dashing2_amd/libd2g_NAME.so (experiments; select with D2G_LIB=...)
set -e
cd "$(dirname "$0")/../dashing2_amd/csrc"
name=$1; shift
tmp=/tmp/d2g_variant_$name; mkdir -p $tmp
# sources and host flags are the library's own: HIPSRC, HOSTSRC and CXXFLAGS of csrc/Makefile
mkvar() { sed -n "s/^$1 *?*= *//p" Makefile; }
for f in $(mkvar HIPSRC); do
  /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -ffp-contract=off "$@" -c $f -o $tmp/${f%.*}.o &
done
for f in $(mkvar HOSTSRC); do
  g++ $(mkvar CXXFLAGS) -c $f -o $tmp/${f%.*}.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libd2g_$name.so $tmp/*.o -lz -lgomp -ldl
echo built dashing2_amd/libd2g_$name.so
