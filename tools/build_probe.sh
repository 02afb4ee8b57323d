#!/bin/bash
# Measurement build of libvp with phase probes in the two-level labelling kernels (-DVP_PROBE): lib/libvp_probe.so, loaded with
# VP_LIB=<path>.  Not part of the product build.
set -e
root=$(cd $(dirname $0)/.. && pwd)
srcs=$(python3 $root/cuauv-vision-pipeline_amd/build.py --print-sources)   # build.py's VP_SOURCES: no second copy of the list
hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared -ffp-contract=off -DVP_PROBE -Wno-unused-value -Wno-unused-result -x hip \
  $srcs \
  -o $root/cuauv-vision-pipeline_amd/lib/libvp_probe.so
