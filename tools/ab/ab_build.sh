#!/bin/bash
# builds build_tmp/libA.so from the sources of a git revision (default HEAD), with that revision's own slide_amd/build.py, for A/B
# timing against the working tree:
#   tools/ab/ab_build.sh [rev];  then on the GPU box:  SLIDE_HIP_LIB=$PWD/build_tmp/libA.so python tools/ab/time_chains.py
set -e
REV=${1:-HEAD}
cd "$(dirname "$0")/../.."
rm -rf build_tmp/a && mkdir -p build_tmp/a
git archive $REV slide_amd include | tar -x -C build_tmp/a
(cd build_tmp/a && python -m slide_amd.build > /dev/null)
cp build_tmp/a/slide_amd/libslide_hip.so build_tmp/libA.so
ls -la build_tmp/libA.so
