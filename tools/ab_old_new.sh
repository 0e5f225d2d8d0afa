#!/bin/bash
# Same-box A/B of two builds of the library (box-to-box variance on the pool is +-10 %, larger than most kernel changes).
# Build the reference build first, HERE (not on the GPU box), from any commit:
#   rm -rf /tmp/old_src && mkdir -p /tmp/old_src && git archive <commit> dps_ttc_amd/csrc include | tar -x -C /tmp/old_src
#   make -C /tmp/old_src/dps_ttc_amd/csrc OBJDIR=/tmp/old_src/obj OUT=$PWD/dps_ttc_amd/lib/libdpsx_old.so
# then:  gpurun -- 'bash tools/ab_old_new.sh [operator] [cases]'
# (arguments after the cases go to kbench on both sides, e.g. --particles 16 --norm-in-fwd)
# A library older than the Python tree's symbol table (one that lacks an entry point the tree binds) cannot be swapped in:
# unpack that commit's whole tree instead (git archive <commit> | tar -x -C DIR, with its library built into
# DIR/dps_ttc_amd/lib/libdpsx.so) and pass OLD_TREE=DIR: the old side then runs that tree's own kbench.
# pipefail: a kbench that fails, or prints no line for the cases asked for, ends the whole run instead of being skipped
set -e -o pipefail
cd "${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
OPER=${1:-gaussian_blur}; ONLY=${2:-fwd,bwd}
shift $(($# < 2 ? $# : 2))
old() {
  if [ -n "$OLD_TREE" ]; then (cd "$OLD_TREE" && python3 tools/kbench.py "$@")
  else DPSX_LIB=$PWD/dps_ttc_amd/lib/libdpsx_old.so python3 tools/kbench.py "$@"; fi
}
for rep in 1 2 3; do
  echo "== new"; python3 tools/kbench.py --operator $OPER --only $ONLY --reps 50 --no-x0 "$@" | grep -E "^(fwd|bwd|upd|op|adj|score)"
  echo "== old"; old --operator $OPER --only $ONLY --reps 50 --no-x0 "$@" | grep -E "^(fwd|bwd|upd|op|adj|score)"
done
