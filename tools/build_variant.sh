#!/bin/bash
# Build a library variant with extra -D flags for the message kernels (A/B timing with tools/kbench.py):
#   bash tools/build_variant.sh ko1 -DHN_KO_BWD=1   ->  hermnet_amd/csrc/variants/libhermnet_ko1.so
# then:  HERMNET_LIB_PATH=hermnet_amd/csrc/variants/libhermnet_ko1.so python tools/kbench.py
# The two message units are compiled with the flags; every other object is the product library's (csrc/Makefile: variant).
set -e
NAME=$1; shift
make -s -C "$(dirname "$0")/../hermnet_amd/csrc" -j4 variant NAME="$NAME" VARIANT_FLAGS="$*" \
  VARIANT_SRCS="message_kernels.hip message_bwd_cl.hip"
echo built variants/libhermnet_$NAME.so
