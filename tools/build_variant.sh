#!/bin/bash
# Build a variant of libgcs.so for same-box A/B runs without touching the in-tree objects (every translation unit, through
# csrc/Makefile: the only source list):
#   tools/build_variant.sh <name> [extra hipcc flags, e.g. -DGCS_GABOR_STRIPS_BESIDE=0]   ->  build_ab/<name>.so
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
mkdir -p $ROOT/build_ab
make -s -j4 -C $ROOT/gabor_color_image_segmentation_amd/csrc O=/tmp/gcs_variant_$name LIB=$ROOT/build_ab/$name.so EXTRA="$*" all
ls -la $ROOT/build_ab/$name.so
