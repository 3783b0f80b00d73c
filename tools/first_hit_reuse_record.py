"""usage: tools/first_hit_reuse_record.py <directory of tools/first_hit_reuse_ab.sh> [<record.json>]
Puts the runs of the A/B chain into one record (profiles/r09/first_hit_reuse.json) and checks what the change promised: the
outputs of the last timed step are the parent's byte for byte, the median step is shorter than the parent's by at least 0.8 x
the parent's own k_trace_primary time per step (from its kernel trace), by more than either side's min-to-max spread, and with
"reuse_first_hits" = 0 the step lies inside the parent's spread. Prints the verdicts; exits non-zero if one fails."""
import csv
import json
import os
import sys

import numpy as np


def bench_line(path):
    with open(path) as f:
        return json.loads(f.readline())


def kernel_stats(path):
    rows = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row["Name"].split("(")[0].strip()
            for short in ("k_trace_primary", "k_trace<", "k_shade<", "k_replicate_first_hits", "k_generate", "k_resolve", "k_cull_terminal"):
                if name.startswith(short) or name.startswith("void " + short):
                    key = short.rstrip("<")
                    r = rows.setdefault(key, {"calls": 0, "total_ms": 0.0})
                    r["calls"] += int(row["Calls"])
                    r["total_ms"] += float(row["TotalDurationNs"]) / 1e6
    for r in rows.values():
        r["total_ms"] = round(r["total_ms"], 3)
        r["ms_per_call"] = round(r["total_ms"] / max(1, r["calls"]), 4)
    return rows


def main():
    d = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(d, "first_hit_reuse.json")
    runs = {}
    for name in ("parent_1", "new_1", "off_1", "parent_2", "new_2"):
        line = bench_line(os.path.join(d, name + ".json"))
        reps = line["repetitions"]["ms_per_step"]
        runs[name] = {"value_mray_s": line["value"], "ms_per_step_median": round(float(np.median(reps)), 3), "ms_per_step_reps": reps, "spread_ms": round(max(reps) - min(reps), 3), "options": line.get("config", {}).get("options")}
    pooled = {k: runs[k + "_1"]["ms_per_step_reps"] + runs[k + "_2"]["ms_per_step_reps"] for k in ("parent", "new")}
    stats = {k: kernel_stats(os.path.join(d, "kernel_stats_%s.csv" % k)) for k in ("parent", "new")}
    primary_per_step = stats["parent"]["k_trace_primary"]["ms_per_call"]
    same = {}
    for name in sorted(os.listdir(os.path.join(d, "outputs_parent"))):
        a, b = os.path.join(d, "outputs_parent", name), os.path.join(d, "outputs_new", name)
        same[name] = open(a, "rb").read() == open(b, "rb").read()
    p, n, o = runs["parent_1"], runs["new_1"], runs["off_1"]
    gain = round(p["ms_per_step_median"] - n["ms_per_step_median"], 3)
    lo, hi = min(p["ms_per_step_reps"]), max(p["ms_per_step_reps"])
    verdicts = {
        "outputs_identical_to_parent": all(same.values()) and len(same) >= 5,
        "gain_ms_per_step": gain,
        "gain_needed_ms (0.8 x parent k_trace_primary per step)": round(0.8 * primary_per_step, 3),
        "gain_is_enough": gain >= 0.8 * primary_per_step,
        "gain_exceeds_the_wider_spread": gain > max(p["spread_ms"], n["spread_ms"]),
        "option_off_inside_parent_spread": lo <= o["ms_per_step_median"] <= hi,
        "k_trace_primary_launches": {k: stats[k].get("k_trace_primary", {}).get("calls", 0) for k in stats},
        "option_off_inside_both_parent_runs_pooled": min(pooled["parent"]) <= o["ms_per_step_median"] <= max(pooled["parent"]),
        "traced_once_per_change_of_key": stats["new"].get("k_trace_primary", {}).get("calls", 0) == 1,
    }
    rec = {
        "what": "First bounce once per view (reuse_first_hits): the headline command with the parent commit's library and this one's, alternating in one job (tools/first_hit_reuse_ab.sh)",
        "command": "python3 bench.py --gpus 1 --steps 20 --warmup 3 --reps 5",
        "libraries_sha256": open(os.path.join(d, "libraries.sha256")).read().split("\n")[:2],
        "runs": runs,
        "second_round_medians": {k: runs[k + "_2"]["ms_per_step_median"] for k in ("parent", "new")},
        "kernel_trace": {"command": "rocprofv3 --kernel-trace --stats -- python3 bench.py --gpus 1 --steps 20 --warmup 3 --reps 1 (43 renders: 3 warm-up, 20 timed, 20 counted)", "kernels": stats},
        "outputs_of_the_last_timed_step_equal": same,
        "verdicts": verdicts,
    }
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(verdicts, indent=1))
    ok = all(verdicts[k] for k in ("outputs_identical_to_parent", "gain_is_enough", "gain_exceeds_the_wider_spread", "option_off_inside_parent_spread", "traced_once_per_change_of_key"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
