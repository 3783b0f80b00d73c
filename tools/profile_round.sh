#!/bin/bash
# usage (GPU box, repo root): tools/profile_round.sh <tag>
# Everything profiles/<round>/ holds, from one build: kernel-trace stats of the bench command, the PMC passes, traffic.json.
# Results go under $OUT_DIR (default profile_out/), tools/pmc.sh's included.
set -e
tag=$1; shift   # further arguments go to bench.py (e.g. --option wide_bvh=3)
export OUT_DIR=${OUT_DIR:-profile_out}
kernel=${KERNEL:-"k_trace<false, false, true, false, 1>"}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
# the oracle (bench.py's checker) is built BEFORE the profiler starts anything: a profiled, GPU-initialised process must
# not spawn make / g++; the profiled command itself carries no CPU leg (it would mix seconds of host time into the trace)
python3 -c "import __graft_entry__ as g; g.build_product(); g.build_oracle()"
mkdir -p "$OUT_DIR"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT_DIR/prof_${tag}" -- python3 bench.py --full --steps 10 --warmup 2 --reps 1 --no-cpu-baseline --no-last-ray-filter --sustained-seconds 0 --no-other-workloads "$@" > "$OUT_DIR/prof_${tag}.log" 2>&1
grep '"metric"' "$OUT_DIR/prof_${tag}.log" > "$OUT_DIR/prof_${tag}_bench_line.json"
cp "$OUT_DIR/prof_${tag}"/*/*_kernel_stats.csv "$OUT_DIR/prof_${tag}_kernel_stats.csv"
tools/pmc.sh ${tag} --sustained-seconds 0 --no-other-workloads "$@"
python3 tools/traffic.py "$OUT_DIR/pmc_${tag}_fetch"/*/*_counter_collection.csv "$OUT_DIR/pmc_${tag}_write"/*/*_counter_collection.csv "$kernel" "$OUT_DIR/pmc_${tag}_traffic.json"
python3 tools/counters.py "$OUT_DIR/pmc_${tag}_sq"/*/*_counter_collection.csv "$OUT_DIR/pmc_${tag}_tcc"/*/*_counter_collection.csv "$kernel" "$OUT_DIR/pmc_${tag}_counters.json"
echo done
