#!/bin/bash
# Build ../libdove_hip.so in-tree for gfx950 (hipcc cross-compiles without a GPU).  One library, one mode: arguments are an error.
set -euo pipefail
cd "$(dirname "$0")"
if [ $# -ne 0 ]; then echo "build.sh takes no arguments (got: $*)" >&2; exit 2; fi
OUT=../libdove_hip.so
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result"
SRCS="capi igemm igemm_legacy norm attention attention_pipe attention_mx elementwise mxfp8 t5 graph metrics colorfix yuv video degrade conv_f32 flow percep niqe clipiqa musiq swin3d convnext3d maniqa png jpeg vcodec"
pids=()
for f in $SRCS; do
  hipcc $FLAGS -c $f.hip -o $f.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
objs=""
for f in $SRCS; do objs="$objs $f.o"; done
hipcc --offload-arch=gfx950 -shared -fPIC $objs -o $OUT
echo "built $(realpath $OUT)"
