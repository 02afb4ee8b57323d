#!/bin/bash
# Measurement build of libvp with phase stamps in the one-block contour bookkeeping (k_ct_jump, LDS form; -DVP_CT_PROBE, optional
# -DCTJ_HOPS=n): lib/libvp_ctprobe.so, loaded with VP_LIB=<path> by tools/exp_ct_probe.py.  Not part of the product build.
set -e
root=$(cd $(dirname $0)/.. && pwd)
srcs=$(python3 $root/cuauv-vision-pipeline_amd/build.py --print-sources)   # build.py's VP_SOURCES: no second copy of the list
hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared -ffp-contract=off -DVP_CT_PROBE $VP_CT_PROBE_DEFS -Wno-unused-value -Wno-unused-result -x hip \
  $srcs \
  -o $root/cuauv-vision-pipeline_amd/lib/libvp_ctprobe.so
