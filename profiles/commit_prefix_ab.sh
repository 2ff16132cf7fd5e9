#!/bin/bash
# The commit's node-id prefix (plain SFF: k_commit no longer adds up the lower workgroups' accepted samples, the append
# launch derives the prefix from the workgroups' lines), new build against a second build of the library (the parent
# commit's: check the parent out into a scratch tree, run profiles/build_variant.sh parent there and copy
# space_filling_forest_star_amd/libsffgpu_parent.so beside the shipped library; at most 16 build jobs):
#   bash profiles/commit_prefix_ab.sh <out dir> [second library]
#   bench.py --dump-outputs of both builds, compared file by file; the bench line five times per build, alternating ->
#   <out>/commit_prefix_bench_lines.json ("build" names the library); the kernel trace of the driver's bench command
#   (without the legs behind the timed region) for the new build and twice for the second one (the second pair gives every
#   kernel's trace-to-trace difference) -> <out>/commit_prefix_*_kernel_stats.csv; the phase clocks of SFFGPU_PROFILE=1
#   for both builds and one k_commit timeline of the new build (SFFGPU_KC_TRACE) -> <out>/commit_prefix_phase_clocks.txt.
# Every step that uses the GPU has its own time limit; the first step that fails ends the script.
set -eu -o pipefail
out=$(mkdir -p "${1:-ab_out}" && cd "${1:-ab_out}" && pwd)
other=${2:-libsffgpu_parent.so}
root=$(cd "$(dirname "$0")/.." && pwd)
BENCH=("$root/bench.py" --gpus 1 --steps 20 --warmup 5 --cpu-iters 0 --no-sweep-micro --no-wave-sweep --no-extra-legs)
cd "$root"
test -f "space_filling_forest_star_amd/$other"
trace() {   # <tag> <library>
  SFFGPU_LIB=$2 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/$1_trace" -o t -- python3 "${BENCH[@]}" > "$out/$1_trace.log" 2>&1
  cp "$out/$1_trace/t_kernel_stats.csv" "$out/commit_prefix_$1_kernel_stats.csv"
  rm -rf "$out/$1_trace" "$out/$1_trace.log"
}
line() {    # <build name> <library> [extra bench args]
  local b=$1 l=$2; shift 2
  SFFGPU_LIB=$l timeout -k 10 240 python3 "${BENCH[@]}" "$@" > "$out/line.log" 2>"$out/line.err"
  grep -E '^\{"metric"' "$out/line.log" | tail -1 | sed "s/^{/{\"build\": \"$b\", /" >> "$out/commit_prefix_bench_lines.json"
  rm -f "$out/line.log" "$out/line.err"
}
clocks() {  # <build name> <library> <pattern> <lines of the last forest> [environment]
  local b=$1 l=$2 pat=$3 n=$4; shift 4
  echo "== $b $*" >> "$out/commit_prefix_phase_clocks.txt"
  env SFFGPU_LIB=$l SFFGPU_PROFILE=1 "$@" timeout -k 10 240 python3 "${BENCH[@]}" 2>&1 >/dev/null | grep -F "$pat" | tail -$n >> "$out/commit_prefix_phase_clocks.txt"
}
: > "$out/commit_prefix_bench_lines.json"
: > "$out/commit_prefix_phase_clocks.txt"
line new libsffgpu.so --dump-outputs "$out/dump_new"
line parent "$other" --dump-outputs "$out/dump_parent"
python3 - "$out/dump_new" "$out/dump_parent" <<'PY'
import os, sys
import numpy as np
a, b = sys.argv[1:3]
names = sorted(os.listdir(a))
assert names == sorted(os.listdir(b)) and names, (names, sorted(os.listdir(b)))
for n in names:
    assert np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n))), n
print("dump-outputs: %d files equal" % len(names))
PY
rm -rf "$out/dump_new" "$out/dump_parent"
trace new libsffgpu.so
trace parent "$other"
trace parent_again "$other"
for r in 1 2 3 4; do
  line new libsffgpu.so
  line parent "$other"
done
clocks new libsffgpu.so "k_commit us/commit" 1
clocks parent "$other" "k_commit us/commit" 1
clocks new libsffgpu.so "k_commit trace" 8 SFFGPU_KC_TRACE=400
echo done
