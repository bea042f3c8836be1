#!/bin/bash
# Build a library variant of the current tree: tools/mkvar.sh NAME [-DFLAG=V ...]
# -> variants/lib_NAME.so (git-ignored; shipped to the GPU box by gpurun).
# The sources and flags are build()'s own (__graft_entry__.hipcc_cmd).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
mkdir -p "$R/variants"
cd "$R"
python -c 'import subprocess, sys, __graft_entry__ as g; subprocess.check_call(g.hipcc_cmd(sys.argv[1], sys.argv[2:]))' \
  "$R/variants/lib_$name.so" "$@"
