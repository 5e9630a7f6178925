#!/bin/bash
# build a kernel-variant library for A/B timing:
#   scripts/build_variant.sh NAME "-DS3D_...=..." [source=kernels_march]   ->  variants/libsift3d_hip_NAME.so
# One source is rebuilt with the extra macros; every other object is the default build's.  Sources and flags are the Makefile's.
# (the development switches -- -DS3D_DEV_SWITCHES: environment overrides of tuning values and hooks -- live in entry_test.hip)
set -e
cd "$(dirname "$0")/.."
name=$1; extra=$2; src=${3:-kernels_march}
csrc=3dsift_amd/csrc
B=build/variants/$name   # under csrc/build: git-ignored
[ -f $csrc/$src.hip ] || { echo "no such source: $csrc/$src.hip" >&2; exit 1; }
make -C $csrc -j8   # the default objects, up to date and built without the extra macros
mkdir -p variants $csrc/$B
cp -u $csrc/build/*.o $csrc/$B/
rm -f $csrc/$B/$src.o   # the only object make finds missing: the one built with EXTRA
make -C $csrc -j8 BUILD=$B OUT="$PWD/variants/libsift3d_hip_$name.so" EXTRA="$extra"
echo built variants/libsift3d_hip_$name.so
