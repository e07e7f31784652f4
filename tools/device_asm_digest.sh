#!/bin/bash
# tools/device_asm_digest.sh [extra flags]
# Compiles every .hip unit of lol_amd/csrc/Makefile's SRCS to device assembly (the Makefile's CXXFLAGS
# plus -S --cuda-device-only, at most 16 compiles at a time) into build/asm/<unit>.s and prints
# "sha256  unit" per file.  One thing in the compiler's output depends on where the tree lies: the symbol
# __hip_cuid_<hash>, a one-byte marker object named after a hash of the input path and the command line
# (clang's compilation-unit id).  Its hash is cut out of the written file (5 lines per unit: .type, .globl,
# the label, .size, .addrsig_sym); nothing else depends on the path or on line numbers, so two trees whose
# tables agree ship the same device code: the proof a behaviour-preserving refactor owes.
#   tools/device_asm_digest.sh                          all units, shipped configuration
#   UNITS="pow2_ar1.hip pow2_ar1_t1.hip" tools/device_asm_digest.sh -DLOLHIP_CSUB_EXEC=0
set -eo pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root/lol_amd/csrc"
var() { make -s --no-print-directory --eval "print-var: ; @echo \$($1)" print-var EXTRA="$2"; }
hipcc=$(var HIPCC); arch=$(var ARCH); flags=$(var CXXFLAGS "$*")
units=${UNITS:-$(var SRCS | tr ' ' '\n' | grep '\.hip$')}
out=$root/build/asm; mkdir -p "$out"
printf '%s\n' $units | xargs -P 16 -I{} sh -c \
  "$hipcc --offload-arch=$arch $flags -S --cuda-device-only -o $out/\$(basename {} .hip).s {} \
   && sed -i -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid/g' $out/\$(basename {} .hip).s"
for u in $units; do echo "$(sha256sum < "$out/$(basename $u .hip).s" | cut -d' ' -f1)  $u"; done
