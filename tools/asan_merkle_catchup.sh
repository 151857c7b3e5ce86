#!/bin/bash
# AddressSanitizer + UBSan run of the catch-up lane's header code (edv_merkle.h,
# row f-10) compiled for the CPU: a stand-alone program with its own main
# (tools/asan_merkle_catchup.cpp over csrc/edv_hostcheck.cpp), exact-size heap
# buffers, statuses checked for intact and altered replies.  Host code only (no
# GPU, no Python).  Builds into /tmp, leaves the in-tree libraries alone.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${ASAN_OUT:-/tmp/edv_asan}
mkdir -p $OUT
g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -std=c++17 \
  -Wall -Wno-unknown-pragmas -I$R/indy-plenum_amd/csrc $R/tools/asan_merkle_catchup.cpp -o $OUT/asan_merkle_catchup
ASAN_OPTIONS=abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 $OUT/asan_merkle_catchup
