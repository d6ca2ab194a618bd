#!/bin/bash
# Build variants/NAME.so from the current sources with extra compiler flags (developer tool, no GPU):
#   bash scripts/mkvariant.sh NAME -DFOO=1 ...
# Flags and sources are the library's own (build.FLAGS, build.SOURCES), so the variant is a whole,
# loadable library of the tree it is run in (QSP_LIB_PATH=variants/NAME.so), e.g. the parent commit's for an A/B.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p variants
FLAGS=$(python3 -c "from uclv_qs_pushing_matlab_amd.build import FLAGS; print(' '.join(FLAGS))")
SOURCES=$(python3 -c "from uclv_qs_pushing_matlab_amd.build import SOURCES; print(' '.join('uclv_qs_pushing_matlab_amd/csrc/' + f for f in SOURCES))")
/opt/rocm/bin/hipcc --offload-arch=gfx950 $FLAGS -I include "$@" $SOURCES -o variants/$name.so
echo "variants/$name.so"
