#!/usr/bin/env python3
"""usage (GPU box): tools/host_pipeline.py [--frames 200] [--reps 7] [--width 1920 --height 1080] [--ring 2] [--forms a,b,..]
                                            [--precisions binary32,half] [--out profiles/r05/host_pipeline.json] [--dry-run]
The workload of bench.py's host_outputs record (atrium, one sample per pixel per call, radiance plus the four AOVs, default
flags, every ray traced: "answer_last_rays" = 0) through the forms of the boundary, in one process:
  device     sthip_render with device pointers: only enqueues; the ceiling
  sync       sthip_render with host pointers into pageable memory: renders, copies and synchronises inside the call; the
             behaviour before sthip_render_async existed, the yardstick
  sync_pinned  the same call into pinned memory (sthip_host_alloc): what pinning alone buys, without any overlap
  pipelined  sthip_render_async with "output_ring" = --ring into pinned memory, three host sets: frame i + 1 renders while
             frame i copies back
A repetition runs --frames frames of every form, one form after the other (so drift of the box hits all alike), and ends
each form in a wait for its last frame: the time is taken on finished work. After one warm-up repetition, --reps timed ones;
per form the median and the min-max spread of the per-frame time. Bytes per frame come from the array shapes; the pipelined
form's device-to-host rate is set against the 63 GB/s of PCIe Gen5 x16. The limit of the pipelined form is
max(render, copy), not render: the record says which of the two binds. One JSON line; --out also writes it to a file.
--dry-run: no GPU; prints the argument and buffer sizing only."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PCIE_GEN5_X16_GBS = 63.0
FORMS = ("device", "sync", "sync_pinned", "pipelined")
PER_PIXEL = {"radiance": None, "albedo": None, "visibility": 8, "depth": 16, "prev_uv": 8}  # None: a colour image (16 B, 8 B with half colour precision)


def frame_bytes(width, height, half):
    """Bytes one frame's five images take in host memory, and their total with gRayCount."""
    color = 8 if half else 16
    per = {k: width * height * (v or color) for k, v in PER_PIXEL.items()}
    per["ray_count"] = 16
    return per, sum(per.values())


def parse(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200, help="frames per form and repetition")
    ap.add_argument("--reps", type=int, default=7, help="timed repetitions after one warm-up")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ring", type=int, default=2, help='"output_ring" of the pipelined form')
    ap.add_argument("--host-sets", type=int, default=3, help="pinned output sets the pipelined form cycles through")
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--precisions", default="binary32,half")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args(argv)
    a.forms = [f for f in a.forms.split(",") if f]
    a.precisions = [p for p in a.precisions.split(",") if p]
    bad = [f for f in a.forms if f not in FORMS] + [p for p in a.precisions if p not in ("binary32", "half")]
    if bad or a.frames < 1 or a.reps < 1 or not 1 <= a.ring <= 8 or a.host_sets < 1 or a.width < 1 or a.height < 1:
        ap.error("bad arguments: %s" % (bad or "frames / reps / ring / host-sets / size out of range"))
    return a


def stats_ms(per_frame_s):
    v = np.asarray(per_frame_s) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4), "spread_ms": round(float(v.max() - v.min()), 4)}


def measure(a, half):
    import torch

    from stratum_amd import camera, scenes
    from stratum_amd.bdpt import BDPT

    W, H, N = a.width, a.height, a.frames
    sc, cam = scenes.atrium()
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    r = BDPT(device=0)
    try:
        r.update(sc)
        r.set_option("answer_last_rays", 0)
        r.set_option("output_ring", a.ring)
        r.set_half_color_precision(half)
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        cdt = torch.float16 if half else torch.float32
        dev = {
            "radiance": torch.zeros((H, W, 4), dtype=cdt, device="cuda"),
            "albedo": torch.zeros((H, W, 4), dtype=cdt, device="cuda"),
            "visibility": torch.zeros((H, W, 2), dtype=torch.int32, device="cuda"),
            "depth": torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"),
            "prev_uv": torch.zeros((H, W, 2), dtype=torch.float32, device="cuda"),
            "ray_count": torch.zeros(2, dtype=torch.int64, device="cuda"),
        }
        ptrs = {k: v.data_ptr() for k, v in dev.items()}
        pageable = r.render(fr, 0, 1)  # the caller's buffers, allocated and touched once
        pinned = [r.alloc_host_outputs(fr) for _ in range(max(a.host_sets, 1))]
        rays = int(pageable["ray_count"][0])

        def run_device():
            for i in range(N):
                r.render(fr, i, 1, device_outputs=ptrs)
            torch.cuda.synchronize()

        def run_sync(bufs):
            for i in range(N):
                r.render(fr, i, 1, host_outputs=bufs)

        def run_pipelined():
            tickets = [0] * len(pinned)
            t = 0
            for i in range(N):
                k = i % len(pinned)
                if tickets[k]:
                    r.wait(tickets[k])  # the host set is the caller's again
                t = tickets[k] = r.render_async(fr, i, 1, host_outputs=pinned[k])
            r.wait(t)  # every earlier ticket is complete too
            r._tickets.clear()

        runs = {"device": run_device, "sync": lambda: run_sync(pageable), "sync_pinned": lambda: run_sync(pinned[0]), "pipelined": run_pipelined}
        ts = {f: [] for f in a.forms}
        for rep in range(a.reps + 1):
            for f in a.forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runs[f]()
                dt = (time.perf_counter() - t0) / N
                if rep:  # (the first repetition is the warm-up)
                    ts[f].append(dt)
        per, total = frame_bytes(W, H, half)
        assert total == sum(int(v.nbytes) for v in pinned[0].values()), "frame_bytes disagrees with the arrays"
        rec = {"bytes_per_frame": total, "bytes_per_image": per, "rays_per_frame": rays}
        for f in a.forms:
            rec[f] = stats_ms(ts[f])
            rec[f]["mray_per_s"] = round(rays / (rec[f]["median_ms"] * 1e-3) / 1e6, 1)
        if "pipelined" in rec:
            p = rec["pipelined"]
            p["d2h_gb_per_s"] = round(total / (p["median_ms"] * 1e-3) / 1e9, 2)
            p["d2h_fraction_of_pcie_gen5_x16"] = round(p["d2h_gb_per_s"] / PCIE_GEN5_X16_GBS, 3)
            if "sync" in rec:
                gain = rec["sync"]["median_ms"] - p["median_ms"]
                p["below_sync_by_ms"] = round(gain, 4)
                p["sync_over_pipelined"] = round(rec["sync"]["median_ms"] / p["median_ms"], 3)
                p["below_sync_by_more_than_syncs_spread"] = bool(gain > rec["sync"]["spread_ms"])
            if "device" in rec:
                p["fraction_of_device_form"] = round(rec["device"]["median_ms"] / p["median_ms"], 3)
                if "sync_pinned" in rec:  # the copy alone ~ the synchronous pinned call minus the render
                    copy_ms = rec["sync_pinned"]["median_ms"] - rec["device"]["median_ms"]
                    p["copy_alone_ms_estimate"] = round(copy_ms, 4)
                    p["binds"] = "copy" if copy_ms > rec["device"]["median_ms"] else "render"
                    p["limit_max_render_copy_ms"] = round(max(copy_ms, rec["device"]["median_ms"]), 4)
        return rec
    finally:
        r.close()


def main(argv=None):
    a = parse(sys.argv[1:] if argv is None else argv)
    out = {
        "workload": "atrium %dx%d, one sample per pixel per call, radiance + 4 AOVs, default flags, every ray traced" % (a.width, a.height),
        "frames_per_repetition": a.frames, "reps": a.reps, "output_ring": a.ring, "host_sets": a.host_sets, "forms": a.forms,
        "pcie_gen5_x16_gb_per_s": PCIE_GEN5_X16_GBS,
    }
    if a.dry_run:
        for name in a.precisions:
            per, total = frame_bytes(a.width, a.height, name == "half")
            out[name] = {"bytes_per_frame": total, "bytes_per_image": per, "pinned_host_bytes": total * a.host_sets, "device_staging_bytes": (total - 16) * a.ring}
        print(json.dumps(out))
        return out
    for name in a.precisions:
        out[name] = measure(a, name == "half")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
