#!/bin/bash
# Is the DEVICE code of two commits the same?  (profiles are stamped with a hash of csrc/*.h*: a host-side or comment edit changes
# the stamp but not what was measured.)  Compiles every csrc/*.hip of both commits with --cuda-device-only -S and compares.
#   tools/device_asm_equal.sh <commit A> [<commit B> = working tree]
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
A=$1; B=${2:-WORKTREE}
T=$(mktemp -d)
for side in A B; do
  # (both sides are compiled at the SAME path, one after the other: the path goes into the anonymous namespaces' unique names)
  c=${!side}; rm -rf $T/work; mkdir -p $T/work/csrc $T/work/include $T/$side
  if [ "$c" = WORKTREE ]; then cp $R/q-mann_amd/csrc/*.h* $T/work/csrc/; cp $R/include/*.h $T/work/include/
  else for f in $(git -C $R ls-tree --name-only $c q-mann_amd/csrc/ include/); do git -C $R show $c:$f > $T/work/$( [[ $f == include/* ]] && echo include || echo csrc )/$(basename $f); done; fi
  sed -i "s#\.\./\.\./include/#$T/work/include/#" $T/work/csrc/*
  for s in $T/work/csrc/*.hip; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-gpu-rdc -ffp-contract=off -I $T/work/include --cuda-device-only -S $s -o $T/$side/$(basename $s .hip).s 2>/dev/null &
  done; wait
done
rc=0
norm() { grep -v '^\s*\.file\|^\s*\.ident\|\.loc\b' $1 | sed 's/__hip_cuid_[0-9a-f]*/__hip_cuid_X/g'; }    # (the compilation-unit id hashes the whole source text)
# (a DIFFERENT unit is listed kernel by kernel; KEEP=1 leaves the .s files of both sides in place for a closer look)
# A unit that B split or renamed is followed: its kernels are looked up in ALL of B's units (their names carry no file name), and
# it reads MOVED when each is the same where it went.  Last, the kernels that B has and no unit of A: an instantiation B added.
for s in $T/A/*.s; do
  b=$(basename $s)
  if [ -f $T/B/$b ] && cmp -s <(norm $s) <(norm $T/B/$b); then echo "same      $b"; continue; fi
  if out=$(python3 $R/tools/device_asm_kernels.py $s $T/B/*.s); then echo "MOVED     $b"; else echo "DIFFERENT $b"; rc=1; fi
  echo "$out" | sed 's/^/    /'
done
if ! out=$(python3 $R/tools/device_asm_kernels.py --only-b <(cat $T/A/*.s) $T/B/*.s); then echo "NEW IN B"; echo "$out" | sed 's/^/    /'; rc=1; fi
if [ -n "$KEEP" ]; then echo "kept: $T/A $T/B"; else rm -rf $T; fi; exit $rc
