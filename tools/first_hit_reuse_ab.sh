#!/bin/bash
# usage (GPU box, repo root): tools/first_hit_reuse_ab.sh <parent library> <output directory>
# What profiles/r09/first_hit_reuse.json is made from (tools/first_hit_reuse_record.py): the headline command with the parent
# commit's library (STHIP_LIB) and with this tree's, alternating in one chain, this tree's once more with
# "reuse_first_hits" = 0, one kernel trace of each library (a trace only, no counters), and the last timed step's outputs of
# both for a byte comparison. Every step has its own time limit; the first failure ends the chain.
set -o pipefail
parent=$1
out=$2
mkdir -p "$out"
bench="python3 bench.py --gpus 1 --steps 20 --warmup 3 --reps 5"
trace="rocprofv3 --kernel-trace --stats --output-format csv"
run() {  # run <name> <seconds> <command...>: the bench line of the run goes to $out/<name>.json
  local name=$1 limit=$2
  shift 2
  echo "== $name" && timeout -k 10 "$limit" "$@" > "$out/$name.log" 2>&1 && grep '"metric"' "$out/$name.log" > "$out/$name.json" && cut -c1-200 "$out/$name.json"
}
sha256sum "$parent" stratum_amd/libstratum_hip.so > "$out/libraries.sha256" \
 && run parent_1 300 env STHIP_LIB="$parent" $bench --dump-outputs "$out/outputs_parent" \
 && run new_1 300 $bench --dump-outputs "$out/outputs_new" \
 && run off_1 300 $bench --option reuse_first_hits=0 \
 && run parent_2 300 env STHIP_LIB="$parent" $bench \
 && run new_2 300 $bench \
 && run trace_parent 300 env STHIP_LIB="$parent" $trace -d "$out/prof_parent" -- python3 bench.py --gpus 1 --steps 20 --warmup 3 --reps 1 \
 && run trace_new 300 $trace -d "$out/prof_new" -- python3 bench.py --gpus 1 --steps 20 --warmup 3 --reps 1 \
 && cp "$out"/prof_parent/*/*_kernel_stats.csv "$out/kernel_stats_parent.csv" && cp "$out"/prof_new/*/*_kernel_stats.csv "$out/kernel_stats_new.csv" \
 && rm -rf "$out/prof_parent" "$out/prof_new" \
 && python3 tools/first_hit_reuse_record.py "$out"
rc=$?
rm -rf "$out/outputs_parent" "$out/outputs_new"  # (2 x 133 MB: compared above, not kept)
exit $rc
