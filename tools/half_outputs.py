#!/usr/bin/env python3
"""usage (GPU box): tools/half_outputs.py [reps] [width height]
The headline frame (atrium 1920x1080, one sample per pixel per call, default flags, every ray traced) through HOST output
pointers, binary32 against half colour precision (include/sthip.h "half_color_precision"), for all outputs and for radiance
only — the form where the bytes that cross PCIe are part of the call. The two precisions run in separate contexts, interleaved
call by call so that drift of the box hits both alike; prints one JSON line with the medians (as bench.py's host_outputs
record: a warm-up call first, then `reps` timed calls of each form)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from stratum_amd import camera, scenes
from stratum_amd.bdpt import BDPT


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1920, 1080)
    sc, cam = scenes.atrium()
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    ctx = {}
    for name, half in (("binary32", False), ("half", True)):
        r = BDPT(device=0)
        r.update(sc)
        r.set_option("answer_last_rays", 0)
        r.set_half_color_precision(half)
        ctx[name] = (r, r.render(fr, 0, 1))  # the caller's buffers, allocated and touched once (pageable memory)
    out = {"workload": "atrium %dx%d, one sample per pixel per call, default flags, every ray traced, HOST output pointers" % (W, H), "reps": reps}
    try:
        for aovs in (True, False):
            ts = {name: [] for name in ctx}
            for i in range(reps + 1):
                for name, (r, bufs) in ctx.items():
                    t = time.perf_counter()
                    r.render(fr, i, 1, aovs=aovs, host_outputs=bufs)
                    ts[name].append(time.perf_counter() - t)
            rec = {}
            for name, (r, bufs) in ctx.items():
                dt = float(np.median(ts[name][1:]))
                rays = int(bufs["ray_count"][0])
                nbytes = sum(int(v.nbytes) for k, v in bufs.items() if aovs or k in ("radiance", "ray_count"))
                rec[name] = {"value": round(rays / dt / 1e6, 2), "unit": "Mray/s", "ms_per_call": round(dt * 1e3, 3), "bytes_read_back": nbytes,
                             "spread_ms": [round(min(ts[name][1:]) * 1e3, 3), round(max(ts[name][1:]) * 1e3, 3)]}
            rec["half_over_binary32"] = round(rec["half"]["value"] / rec["binary32"]["value"], 3)
            out["all_outputs" if aovs else "radiance_only"] = rec
    finally:
        for r, _ in ctx.values():
            r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
