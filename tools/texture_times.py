#!/usr/bin/env python3
"""usage (GPU box): tools/texture_times.py [reps] [width height] [image_size] [out.json]
The textured box with its four large images at image_size x image_size random texels (2048: 64 MB per image and 341 MB with
the chains as RGBA32F, 85 MB as RGBA8 — neither fits the 4 MB L2 of an XCD, the float form not even the 256 MB of the last-level
cache), rendered with the SAME texels resident in both formats (include/sthip.h: sthip_image_format): a float upload of
bytes / 255 against an 8-bit upload of the bytes. Two contexts, interleaved call by call so that drift of the box hits both
alike, medians of `reps` calls after a warm-up call, device output pointers left out (host pointers, as bench.py's frames): with
the default flags (ray cones pick the level whose texels match the pixel) and with eRayCones off (every lookup reads level 0).
Also the wall time of the upload per format (median of 3) and the resident texture bytes. Writes profiles/r09/textures.json."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import copy

import numpy as np

from stratum_amd import camera, scenes, wire
from stratum_amd.bdpt import BDPT


def chain_texels(h, w):
    n = levels = 0
    while True:
        n += h * w
        levels += 1
        if (h == 1 and w == 1) or levels == wire.MAX_MIPS:
            return n
        h, w = max(1, h // 2), max(1, w // 2)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    W, H = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1920, 1080)
    size = int(sys.argv[4]) if len(sys.argv) > 4 else 2048
    path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "r09", "textures.json")
    base, cam = scenes.textured_box()
    rng = np.random.RandomState(1)
    images = []
    for i, im in enumerate(base.images):  # checker, noise, bump, roughness: large; the emitter's image stays 16 x 16
        n = size if im.shape[0] > 16 else im.shape[0]
        images.append(np.ascontiguousarray(rng.randint(0, 256, size=(n, n, 4)).astype(np.uint8)))
    scene = {}
    for name in ("rgba32f", "rgba8"):
        sc = copy.copy(base)
        sc.images = [im if name == "rgba8" else im.astype(np.float32) / np.float32(255) for im in images]
        scene[name] = sc
    fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    out = {"workload": "textured_box %dx%d, one sample per pixel per call, images %s at %d x %d random texels" % (W, H, [i.shape[0] for i in images], size, size), "reps": reps}
    texels = sum(chain_texels(i.shape[0], i.shape[1]) for i in images)
    out["resident_texture_bytes"] = {"rgba32f": 16 * texels, "rgba8": 4 * texels}
    out["uploaded_texture_bytes"] = {"rgba32f": 16 * texels, "rgba8": 4 * sum(i.shape[0] * i.shape[1] for i in images)}
    ctx = {}
    try:
        upload = {}
        for name, sc in scene.items():
            r = BDPT(device=0)
            ctx[name] = r
            ts = []
            for _ in range(4):  # the first call allocates: left out of the median
                t = time.perf_counter()
                r.update(sc)
                ts.append(time.perf_counter() - t)
            upload[name] = {"ms": round(float(np.median(ts[1:])) * 1e3, 2), "first_ms": round(ts[0] * 1e3, 2)}
        out["sthip_scene_upload_ms"] = upload
        for label, flags in (("default_flags", []), ("ray_cones_off", ["~raycones"])):
            for r in ctx.values():
                r.mSamplingFlags = wire.DEFAULT_SAMPLING_FLAGS
                for f in flags:
                    r.set_flag(f)
            bufs = {name: r.render(fr, 0, 1) for name, r in ctx.items()}  # warm-up; the caller's buffers, touched once
            ts = {name: [] for name in ctx}
            for i in range(reps + 1):
                for name, r in ctx.items():
                    t = time.perf_counter()
                    r.render(fr, i, 1, host_outputs=bufs[name])
                    ts[name].append(time.perf_counter() - t)
            rec = {}
            for name in ctx:
                dt = ts[name][1:]
                rec[name] = {"ms_per_step": round(float(np.median(dt)) * 1e3, 3), "spread_ms": [round(min(dt) * 1e3, 3), round(max(dt) * 1e3, 3)], "rays": int(bufs[name]["ray_count"][0])}
            rec["rgba8_over_rgba32f_time"] = round(rec["rgba8"]["ms_per_step"] / rec["rgba32f"]["ms_per_step"], 3)
            out[label] = rec
    finally:
        for r in ctx.values():
            r.close()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
