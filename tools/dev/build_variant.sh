#!/bin/bash
# Dev: build a stamped library variant with extra -D flags, e.g.
#   bash tools/dev/build_variant.sh nosplit -DQDEC_SSF_NOSPLIT
# -> exp_ldpc_amd/libqdec_hip_stamps_nosplit.so (load with QDEC_LIB=...).
# Sources, flags and the per-unit parallel compile are exp_ldpc_amd/build.py's.
set -eo pipefail
tag=$1; shift
cd "$(dirname "$0")/../.."
python -m exp_ldpc_amd.build --force --stamps --tag "$tag" "$@"
