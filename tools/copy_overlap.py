#!/usr/bin/env python3
"""usage: tools/copy_overlap.py <kernel_trace.csv> [<memory_copy_trace.csv>]
Reads the CSVs of `rocprofv3 --kernel-trace --memory-copy-trace -f csv -- python tools/host_pipeline.py --frames 12 --reps 1
--forms pipelined --precisions binary32` and answers: do the device-to-host copies of frame i lie beside the kernels of frame
i + 1? A copy is either a row of the memory-copy trace (a copy engine moved it) or a dispatch of the runtime's own copy kernel
(`__amd_rocclr_copyBuffer`) on a hardware queue other than the one the path's kernels run on. Prints the counts, the share
of the copies' time during which a path kernel was running, and the timeline of two frames from the middle of the run."""
import csv
import sys


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    for r in rows:
        r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    path = [r for r in rows if not r["Kernel_Name"].startswith("__amd") and r["Kernel_Name"].lstrip("void ").startswith("k_")]
    render_queues = {r["Queue_Id"] for r in path}
    copies = [dict(r, what="copy kernel q" + r["Queue_Id"]) for r in rows if r["Kernel_Name"].startswith("__amd_rocclr_copyBuffer") and r["Queue_Id"] not in render_queues]
    engine = 0
    if len(sys.argv) > 2:
        for r in csv.DictReader(open(sys.argv[2])):
            if "DEVICE_TO_HOST" in r["Direction"]:
                engine += 1
                copies.append({"s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"]), "what": "copy engine"})
    path.sort(key=lambda r: r["s"])
    busy = []  # merged intervals in which a path kernel runs
    for r in path:
        if busy and r["s"] <= busy[-1][1]:
            busy[-1][1] = max(busy[-1][1], r["e"])
        else:
            busy.append([r["s"], r["e"]])
    total = covered = 0
    for c in copies:
        total += c["e"] - c["s"]
        covered += sum(max(0, min(c["e"], b[1]) - max(c["s"], b[0])) for b in busy)
    big = [c for c in copies if c["e"] - c["s"] > 100000]
    print("path kernels: %d on hardware queue(s) %s; device-to-host copies: %d (%d by copy engines, %d by the runtime's copy kernel on another queue)" % (len(path), sorted(render_queues), len(copies), engine, len(copies) - engine))
    if not copies:
        return
    print("copy time %.2f ms in all, %.2f ms of it (%.0f %%) while a path kernel was running; copies above 0.1 ms: %d, median %.0f us" % (total / 1e6, covered / 1e6, 100.0 * covered / max(1, total), len(big), sorted(c["e"] - c["s"] for c in big)[len(big) // 2] / 1e3 if big else 0))
    gen = [r for r in path if r["Kernel_Name"].startswith("k_generate")]
    if len(gen) < 4:
        return
    t0, t1 = gen[len(gen) // 2]["s"], gen[len(gen) // 2 + 2]["s"]
    print("timeline of two frames (us from the first k_generate):")
    events = [(r["s"], r["e"], "q%s %s" % (r["Queue_Id"], r["Kernel_Name"].replace("void ", "")[:24])) for r in path] + [(c["s"], c["e"], "    " + c["what"]) for c in big]
    for s, e, name in sorted(events):
        if t0 <= s < t1:
            print("  %-32s %8.1f -> %8.1f (%6.1f)" % (name, (s - t0) / 1e3, (e - t0) / 1e3, (e - s) / 1e3))


if __name__ == "__main__":
    main()
