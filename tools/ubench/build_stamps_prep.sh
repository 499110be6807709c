#!/bin/bash
# Diagnostic builds of the library for tools/ubench/stamps_prep.py (after `make`):
#   libstamps_prep.so   -DSPR_PREP_STAMPS  in ncc_fft.hip    (prep_fft_kernel; run it with SPR_PREP6=0)
#   libstamps_prep6.so  -DSPR_PREP6_STAMPS in ncc_prep6.hip  (prep6_gallery_kernel)
R=$(cd "$(dirname "$0")/../.." && pwd); C=$R/shoeprint-image-retrieval_amd/csrc
T=$(mktemp -d)
HIPCC="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I. -Wall -Wno-unused-function"
cd $C && $HIPCC -DSPR_PREP_STAMPS -c ncc_fft.hip -o $T/fft_stamps.o && \
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $(ls build/*.o | grep -v ncc_fft.o) $T/fft_stamps.o -o $R/tools/ubench/libstamps_prep.so && \
$HIPCC -DSPR_PREP6_STAMPS -c ncc_prep6.hip -o $T/prep6_stamps.o && \
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $(ls build/*.o | grep -v ncc_prep6.o) $T/prep6_stamps.o -o $R/tools/ubench/libstamps_prep6.so && echo stamps ok
rm -rf $T
