#!/bin/sh
# Builds csrc/w2comm_msg.hip, csrc/status.cpp and tools/w2comm_msg_args_check.cpp into one stand-alone program whose HOST code runs under AddressSanitizer and
# UndefinedBehaviorSanitizer, and runs it.  For a machine without a GPU: every call of the program is refused before a launch.  (The device code is not
# instrumented; sanitised code is not loaded into Python.)
set -e
here=$(cd "$(dirname "$0")/.." && pwd)
out=${TMPDIR:-/tmp}/w2comm_msg_args_check
hipcc=$(command -v hipcc || echo /opt/rocm/bin/hipcc)
"$hipcc" -x hip -O1 -g -std=c++17 -ffp-contract=off -Wno-cuda-compat --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -I"$here/include" -I"$here/coalign_amd/csrc" "$here/coalign_amd/csrc/w2comm_msg.hip" "$here/coalign_amd/csrc/status.cpp" "$here/tools/w2comm_msg_args_check.cpp" \
    -o "$out"
"$out"
