#!/bin/bash
# The commit's hand-off (k_commit ends at its walks, the append launch's finalize block writes the control block), new
# build against a second build of the library (the parent commit's, made with profiles/build_variant.sh parent):
#   bash profiles/commit_handoff_ab.sh <out dir> [second library]
#   bench.py --dump-outputs of both builds, compared file by file; the bench line five times per build, alternating ->
#   <out>/commit_handoff_bench_lines.json ("build" names the library); the kernel trace of the driver's bench command
#   (without the legs behind the timed region) for the new build and twice for the second one (the second pair gives every
#   kernel's trace-to-trace difference) -> <out>/commit_handoff_*_kernel_stats.csv; the phase clocks of SFFGPU_PROFILE=1
#   for both builds -> <out>/commit_handoff_phase_clocks.txt.
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
  cp "$out/$1_trace/t_kernel_stats.csv" "$out/commit_handoff_$1_kernel_stats.csv"
  rm -rf "$out/$1_trace" "$out/$1_trace.log"
}
line() {    # <build name> <library> [extra bench args]
  local b=$1 l=$2; shift 2
  SFFGPU_LIB=$l timeout -k 10 240 python3 "${BENCH[@]}" "$@" > "$out/line.log" 2>"$out/line.err"
  grep -E '^\{"metric"' "$out/line.log" | tail -1 | sed "s/^{/{\"build\": \"$b\", /" >> "$out/commit_handoff_bench_lines.json"
  rm -f "$out/line.log" "$out/line.err"
}
clocks() {  # <build name> <library>
  echo "== $1" >> "$out/commit_handoff_phase_clocks.txt"
  SFFGPU_LIB=$2 SFFGPU_PROFILE=1 timeout -k 10 240 python3 "${BENCH[@]}" 2>&1 >/dev/null | grep -F "k_commit us/commit" | tail -1 >> "$out/commit_handoff_phase_clocks.txt"
}
: > "$out/commit_handoff_bench_lines.json"
: > "$out/commit_handoff_phase_clocks.txt"
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
clocks new libsffgpu.so
clocks parent "$other"
echo done
