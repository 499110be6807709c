#!/bin/bash
# Builds tools/san_prep6/_build/san_prep6: the CPU emulation of the NCC kernels and their launchers with
# -fsanitize=address,undefined, linked into a program of its own (nothing sanitized is loaded into Python).
set -e
R=$(cd "$(dirname "$0")/../.." && pwd); C=$R/shoeprint-image-retrieval_amd/csrc; O=$R/tools/san_prep6/_build
CXX=${SPR_EMU_CXX:-/opt/rocm/lib/llvm/bin/clang++}
FLAGS="-std=c++17 -O1 -g -pthread -I $R/tests/emu -I $C -I $R/include -Wno-unknown-attributes -DSPR_EMU -DSPR_SAN_SUBSET \
       -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
mkdir -p $O
for f in $C/*.hip; do
  echo "$CXX -x c++ $FLAGS -c $f -o $O/$(basename $f).o"
done | xargs -P 8 -I{} sh -c "{}"
$CXX $FLAGS $R/tools/san_prep6/main.cpp $O/*.hip.o -o $O/san_prep6
echo "built $O/san_prep6"
