#!/bin/bash
# Build a measurement variant of the library next to the product: xz_amd/libxz_amd_<name>.so (select it with XZ_AMD_LIB).
# Every HIP unit is compiled with the extra flags; the plain-C objects of the product build are reused.
# usage: tools/build_variant.sh <name> "<extra hipcc flags>"
set -e
NAME=$1; FLAGS=$2
cd "$(dirname "$0")/../xz_amd/csrc"
OBJS=
for u in *.hip; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -fno-strict-aliasing $FLAGS -c $u -o /tmp/${u%.hip}_$NAME.o
  OBJS="$OBJS /tmp/${u%.hip}_$NAME.o"
done
# the plain-C objects: whatever the Makefile links into the product
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libxz_amd_$NAME.so $OBJS $(make -s print-host-objs) \
  -Wl,-Bsymbolic -Wl,--version-script=libxz_amd.map -Wl,-soname,libxz_amd.so -lpthread
ls -la ../libxz_amd_$NAME.so
