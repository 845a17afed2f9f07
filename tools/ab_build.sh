#!/bin/bash
# Build the current csrc/ into ab/ab_<name>.so (select it with RTREC_AMD_LIB=<path>). The source list and the flags are
# rtrec_amd.build's (SOURCES, HIPCC_FLAGS), so a kernel added there is in the A/B library too; $AB_FLAGS are appended.
# ab/ is scratch and git-ignored: delete it when the A/B is over (rm -rf ab).
set -e
cd "$(dirname "$0")/.."
mkdir -p ab
read -r -a FLAGS <<< "$(python -c 'from rtrec_amd import build; print(" ".join(build.HIPCC_FLAGS))')"
read -r -a SRCS <<< "$(python -c 'from rtrec_amd import build; print(" ".join("rtrec_amd/csrc/" + s for s in build.SOURCES))')"
"$(python -c 'from rtrec_amd import build; print(build._hipcc())')" "${FLAGS[@]}" $AB_FLAGS -o ab/ab_$1.so "${SRCS[@]}"
echo ab/ab_$1.so
