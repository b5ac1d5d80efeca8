#!/bin/bash
# Diagnostic builds of the node chain kernels -- the knobs their sources keep are HN_STAMPS (tools/chain_stamps.py,
# tools/fused_stamps.py), HN_KO_LOADS, HN_KO_STORES and HN_KO_BSTREAM=1|2 (results wrong, time meaningful):
#   bash tools/build_chain_variant.sh kob1 -DHN_KO_BSTREAM=1   ->  hermnet_amd/csrc/variants/libhermnet_kob1.so
# then:  HERMNET_LIB_PATH=hermnet_amd/csrc/variants/libhermnet_kob1.so python tools/chain_bench.py
# The three chain units are compiled with the flags; every other object is the product library's (csrc/Makefile: variant).
set -e
NAME=$1; shift
make -s -C "$(dirname "$0")/../hermnet_amd/csrc" -j4 variant NAME="$NAME" VARIANT_FLAGS="$*" \
  VARIANT_SRCS="node_chain.hip node_chain_wide.hip node_chain16.hip"
echo built variants/libhermnet_$NAME.so
