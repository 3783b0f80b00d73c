"""The denoiser's filter, pass by pass: stream time of estimate_variance, of each a-trous pass at steps 1..16 and of copy_rgb
(sthip_denoise_filter), against the time of sthip_accumulate on the same frame (GPU box).

Workload: the atrium at 1920x1080, three noisy frames of one sample per pixel with a sliding camera, accumulated with
reprojection; the third frame's buffers stay on the device and every call below is the device-pointer form. Per precision
(binary32, RGBA16F), filter type and block shape (32x8, 16x16), RUNS calls of 5 iterations with the history tap at 1; per pass
the median of the HIP-event times the call reports (sthip_denoise_desc::pass_ms), the algorithmic bytes of the pass, and their
rate as a fraction of sthip_measure_ceiling(STHIP_CEILING_TRIAD) measured in the same process. sthip_accumulate is timed by
events on the same stream.

Algorithmic bytes per pixel (cb = 16 for RGBA32F, 8 for RGBA16F): variance cb + 8 + 8 + 16 in, cb + 16 out; an a-trous pass
cb + 16 in (colour, guide: each pixel is fetched from memory once however many taps read it), cb out; copy 2 cb in, cb out.

    python tools/denoise_times.py [--out profiles/r08/denoise.json] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from stratum_amd import _lib, camera, scenes, wire
from stratum_amd.bdpt import BDPT
from stratum_amd.post import TemporalAccumulation

RUNS = 9
ITERATIONS = 5


def med(xs):
    return round(statistics.median(xs), 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r08", "denoise.json"))
    ap.add_argument("--quick", action="store_true", help="a small scene and frame, few runs: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("denoise_times.py needs the GPU: nothing here can be measured without it")
    runs = 3 if args.quick else RUNS
    W, H = (480, 270) if args.quick else (1920, 1080)
    sc, cam = scenes.atrium(target_tris=60_000) if args.quick else scenes.atrium()
    n = W * H
    result = {"what": __doc__.strip().split("\n\n")[0], "scene": "atrium", "width": W, "height": H, "runs": runs, "quick": bool(args.quick), "iterations": ITERATIONS, "precisions": {}}
    L = _lib.lib()
    for half in (False, True):
        r = BDPT(0)
        try:
            r.set_option("bvh_builder", 1)
            r.set_half_color_precision(half)
            r.update(sc)
            cb = 8 if half else 16
            acc = TemporalAccumulation(r, reprojection=True, demodulate_albedo=True, history_limit=0.0)
            prev, hist_before, out, fr = None, None, None, None
            for k in range(3):
                eye = np.array(cam["eye"]) + np.array([0.02, 0.01, 0.0]) * k
                fr = camera.Frame(W, H, cam["fovy"], tuple(eye), cam["target"], prev=prev)
                out = r.render(fr, k, 1)
                hist_before = acc.history
                acc(out, fr.views)
                prev = fr
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
            t = {k: dev(out[k]) for k in ("radiance", "albedo", "visibility", "depth", "prev_uv")}
            t.update(prev_vis=dev(hist_before["visibility"]), prev_depth=dev(hist_before["depth"]), prev_color=dev(hist_before["accum_color"]), prev_moments=dev(hist_before["accum_moments"]))
            t.update(color=torch.zeros(n * cb, dtype=torch.uint8, device="cuda"), moments=torch.zeros(n * 8, dtype=torch.uint8, device="cuda"))
            t.update(f0=torch.zeros(n * cb, dtype=torch.uint8, device="cuda"), f1=torch.zeros(n * cb, dtype=torch.uint8, device="cuda"))
            views = np.ascontiguousarray(fr.views, dtype=wire.ViewData)
            r.set_stream(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()

            a = wire.AccumulateDesc()
            a.width, a.height, a.view_count, a.reprojection, a.demodulate_albedo, a.history_limit, a.device_ptrs = W, H, views.shape[0], 1, 1, 0.0, 1
            a.gViews = views.ctypes.data
            a.gRadiance, a.gAlbedo, a.gVisibility, a.gDepth, a.gPrevUVs = (t[k].data_ptr() for k in ("radiance", "albedo", "visibility", "depth", "prev_uv"))
            a.gPrevVisibility, a.gPrevDepth, a.gPrevAccumColor, a.gPrevAccumMoments = (t[k].data_ptr() for k in ("prev_vis", "prev_depth", "prev_color", "prev_moments"))
            a.gAccumColor, a.gAccumMoments = t["color"].data_ptr(), t["moments"].data_ptr()
            acc_ms = []
            for k in range(runs + 1):  # (the first call is not counted)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r._check(L.sthip_accumulate(r._h, C.byref(a)), "sthip_accumulate")
                e1.record()
                e1.synchronize()
                if k:
                    acc_ms.append(e0.elapsed_time(e1))
            triad = r.measure_ceiling("triad")
            color0 = t["color"].clone()  # (the history tap rewrites gAccumColor: every call starts from the same one)

            rec = {"accumulate_ms": med(acc_ms), "triad_gbytes_per_s": round(triad, 1), "color_bytes_per_pixel": cb, "filters": {}}
            bytes_of = {"variance": n * (cb + 8 + 8 + 16 + cb + 16), "atrous": n * (cb + 16 + cb), "copy": n * 3 * cb}
            for ftype in ("Atrous", "Box3"):
                for block, bname in ((0, "32x8"), (1, "16x16")):
                    r.set_option("denoise_block", block)
                    ms = np.zeros(10, np.float32)
                    d = wire.DenoiseDesc()
                    d.width, d.height, d.view_count, d.device_ptrs = W, H, views.shape[0], 1
                    d.iterations, d.filter_type, d.history_tap = ITERATIONS, wire.FILTER[ftype], 1
                    d.history_limit, d.variance_boost_length, d.sigma_luminance_boost = 4.0, 0.0, 3.0
                    d.gViews = views.ctypes.data
                    d.gVisibility, d.gDepth = t["visibility"].data_ptr(), t["depth"].data_ptr()
                    d.gAccumColor, d.gAccumMoments = t["color"].data_ptr(), t["moments"].data_ptr()
                    d.gFilterImages[0], d.gFilterImages[1] = t["f0"].data_ptr(), t["f1"].data_ptr()
                    d.pass_ms = ms.ctypes.data
                    samples = []
                    for k in range(runs + 1):
                        t["color"].copy_(color0)
                        r._check(L.sthip_denoise_filter(r._h, C.byref(d)), "sthip_denoise_filter")
                        if k:
                            samples.append(ms.copy())
                    m = np.median(np.array(samples), axis=0)
                    passes = {"variance": (float(m[0]), bytes_of["variance"]), "copy_rgb": (float(m[9]), bytes_of["copy"])}
                    for i in range(ITERATIONS):
                        passes["atrous_step_%d" % (1 << i)] = (float(m[1 + i]), bytes_of["atrous"])
                    entry = {}
                    for name, (t_ms, nbytes) in passes.items():
                        gbs = nbytes / (t_ms * 1e-3) / 1e9 if t_ms > 0 else 0.0
                        entry[name] = {"ms": round(t_ms, 5), "algorithmic_bytes": int(nbytes), "gbytes_per_s": round(gbs, 1), "fraction_of_triad": round(gbs / triad, 4)}
                    entry["total_ms"] = round(float(m.sum()), 5)
                    entry["total_over_accumulate"] = round(float(m.sum()) / rec["accumulate_ms"], 3)
                    rec["filters"].setdefault(ftype, {})[bname] = entry
                    print("half" if half else "binary32", ftype, bname, json.dumps(entry), flush=True)
            r.set_option("denoise_block", 0)
            result["precisions"]["rgba16f" if half else "rgba32f"] = rec
            r.stats()
            torch.cuda.synchronize()
        finally:
            r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
