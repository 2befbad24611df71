#!/usr/bin/env bash
# Builds liblion_hip.so for gfx950 (cross-compiles without a GPU).  -ffp-contract=off: the parity
# contract is "one IEEE rounding per written operation", same as the oracle.
# -fno-slp-vectorize -fno-vectorize: no packed fp32 VALU (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32) anywhere in the library.  Round 3
# located the FPS failures of round 2 there: ONE float2 expression (8 packed instructions) in fps_reg_kernel makes it
# return wrong samples in 37-40 of 40 graph replays when its waves share SIMDs with conv3d_split_kernel's dense
# v_mfma_f32_32x32x16_f16 stream; the same kernel without packed fp32 -- with or without s_setprio, at 52, 200 or 256
# registers -- is right in every one of 100+ replays (profiles/archive/r03_fps_*).  The SLP vectoriser
# bought nothing measurable anywhere (step, convolutions, 1x1 convolutions, operators: +-1 %) and had inflated
# fps_reg_kernel<8> from 52 to 194 registers.  tests/test_isa_cpu.py keeps the instruction class out.
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -fno-vectorize -munsafe-fp-atomics -I../../include -Wall -Wno-unused-function"
# An object is rebuilt when the hash of (compiler, flags, its source, the shared headers) differs from the one recorded
# beside it (FILE.o.key) -- content, not mtime: a flag change, a checkout of an older file or a fresh clone with stale
# objects all rebuild; LION_REBUILD=1 forces everything.
HDRS="common.h split_ops.h conv3d_tiles.h conv3d_split_kernel.h ../../include/lion_hip.h"
VER="$($HIPCC --version 2>/dev/null | head -3)"
OBJS=()
PIDS=()
KEYS=()
for f in voxelize devoxelize ball_query grouping sampling interpolate chamfer emd diffusion conv3d conv3d_split conv3d_half conv3d_wgrad pointwise norm_train scatter_csr pwconv pwconv_split pwconv_wgrad skinny attention optim ode perturb "$@"; do
  [ -f "$f.hip" ] || continue
  # shellcheck disable=SC2086
  key="$( { echo "$VER $FLAGS"; cat "$f.hip" $HDRS; } | sha256sum | cut -d' ' -f1)"
  if [ -n "${LION_REBUILD:-}" ] || [ ! -f "$f.o" ] || [ ! -f "$f.o.key" ] || [ "$(cat "$f.o.key")" != "$key" ]; then
    rm -f "$f.o" "$f.o.key"   # a failed compile must not leave the previous object behind to be linked silently
    # shellcheck disable=SC2086
    ( $HIPCC $FLAGS -c "$f.hip" -o "$f.o" && echo "$key" > "$f.o.key" ) &
    PIDS+=($!)
  fi
  OBJS+=("$f.o")
done
for p in "${PIDS[@]}"; do wait "$p"; done   # set -e: any failed compile aborts the build
$HIPCC --offload-arch=gfx950 -shared -fPIC -o liblion_hip.so "${OBJS[@]}"
echo "built $(pwd)/liblion_hip.so"
