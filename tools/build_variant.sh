#!/bin/bash
# Build a kernel variant of the library for A/B timing: tools/build_variant.sh <name> [-DMACRO=VALUE ...]
#   -> build/variants/lib_<name>.so   (run with DS_HIP_LIBRARY=<that path> python tools/kernel_time.py ...)
# DS_VARIANT_TU names the translation unit the macros apply to (default ds_kernels.hip; ds_split.hip for the split-operand
# kernels). Sources, headers and per-file flags are those of deepsignal_amd/csrc/Makefile: this script only points it at
# build/obj and build/variants. The other translation units stay cached in build/obj while their sources do not change.
set -e
name=$1; shift
tu=${DS_VARIANT_TU:-ds_kernels.hip}
tu=${tu%.*}
mkdir -p build/variants build/obj
# make does not see the macros: the variant's translation unit is compiled afresh, and its object is not left for the next variant
rm -f build/obj/$tu.o
make -C deepsignal_amd/csrc OBJDIR=../../build/obj OUT=../../build/variants/lib_$name.so VARIANT_TU=$tu VARIANT_FLAGS="$*"
rm -f build/obj/$tu.o
