"""Deforming meshes: what sthip_scene_update_vertices (gather + refit on the device) costs against the full upload it avoids,
and what a refitted tree costs the frames that walk it (GPU box).

For the 1M-triangle atrium and the instanced forest, with both builders: a smooth displacement of every vertex, and of one
instance's mesh only; the median of RUNS calls of update_vertices (device_ms and total_ms of sthip_refit_info) beside, in the
same process, the wall time of sthip_scene_upload of the same deformed scene with the device builder and with the host builder;
sah_cost / sah_cost_at_build; and for the atrium the headline frame (1920x1080, one sample per pixel, device outputs, every ray
traced) in ms per step on the refitted tree against a freshly built one, at three displacement amplitudes. The two trees
are resident side by side in two contexts and their timing passes alternate, so clock and thermal drift over the run
falls on both alike: the ratios of interest are a few per cent.

    python tools/refit_times.py [--out profiles/r06/refit.json] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from stratum_amd import camera, scenes
from stratum_amd.bdpt import BDPT

RUNS = 9  # calls per median: odd, and enough that one slow call (a page fault, another process's copy) does not move it
AMPLITUDES = (("small", 0.02), ("medium", 0.15), ("large", 1.0))  # metres of a 28 m atrium whose triangles are ~5 cm


def displaced(vertices, amp, phase, freq=0.8):
    v = vertices.copy()
    p = v["position"].astype(np.float64)
    v["position"] = (p + amp * np.sin(freq * p[:, [1, 2, 0]] + phase)).astype(np.float32)
    return v


def mesh_range(sc, instance):
    inst = sc.instances["packed"][instance]
    prims, stride, off = int((inst[1] >> 12) & 0xFFFF), int(inst[1] >> 28), int(inst[3])
    idx = np.frombuffer(sc.indices[off : off + 3 * prims * stride].tobytes(), dtype="<u2" if stride == 2 else "<u4").astype(np.int64)
    return int(inst[2]) + int(idx.min()), int(idx.max() - idx.min()) + 1


def med(xs):
    return round(statistics.median(xs), 4)


def spread(xs):
    return {"median": med(xs), "min": round(min(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def time_refits(r, sc, base, first, count, amp, runs):
    dev, tot, wall, ratio = [], [], [], []
    for k in range(runs + 1):  # (the first call also makes the schedule: reported on its own)
        sc.set_vertices(first, displaced(base[first : first + count], amp, 0.3 * k))
        t = time.perf_counter()
        info = r.update_vertices(sc)
        w = (time.perf_counter() - t) * 1e3
        assert info["rebuilt"] == 0
        if k == 0:
            first_call = {"device_ms": round(info["device_ms"], 4), "total_ms": round(info["total_ms"], 4), "wall_ms": round(w, 4)}
            continue
        dev.append(info["device_ms"])
        tot.append(info["total_ms"])
        wall.append(w)
        ratio.append(info["sah_cost"] / info["sah_cost_at_build"])
    return {"vertices": int(count), "amplitude": amp, "device_ms": spread(dev), "total_ms": spread(tot), "python_wall_ms": spread(wall), "first_call_with_schedule": first_call,
            "sah_cost_over_at_build": med(ratio)}


def time_uploads(r, sc, builder, runs):
    r.set_option("bvh_builder", builder)
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        r.update(sc)
        ts.append((time.perf_counter() - t) * 1e3)
    s = r.stats()
    return dict(spread(ts), build_ms=round(s["bvh_build_ms"], 3), build_gpu_ms=round(s["bvh_build_gpu_ms"], 3))


def frame_ms(renderers, frame, dev_out, steps, reps, torch):
    """ms per step of each renderer: `reps` timing passes each, taken in turn (a, b, a, b, ...), after a warm-up of each."""
    for r in renderers:
        r.set_option("answer_last_rays", 0)  # the headline traces every ray (bench.py)
        for i in range(3):
            r.render(frame, seed_begin=i, seed_count=1, device_outputs=dev_out)
    torch.cuda.synchronize()
    out = [[] for _ in renderers]
    for _ in range(reps):
        for k, r in enumerate(renderers):
            t = time.perf_counter()
            for i in range(steps):
                r.render(frame, seed_begin=i, seed_count=1, device_outputs=dev_out)
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t) * 1e3 / steps)
    for r in renderers:
        r.set_option("answer_last_rays", 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r06", "refit.json"))
    ap.add_argument("--quick", action="store_true", help="small scenes, few runs: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("refit_times.py needs the GPU: nothing here can be measured without it")
    runs = 3 if args.quick else RUNS
    cases = (
        ("atrium", (lambda: scenes.atrium(target_tris=60_000)) if args.quick else scenes.atrium),
        ("forest", (lambda: scenes.forest(n_instances=50, tree_tris=2000)) if args.quick else scenes.forest),
    )
    result = {"runs": runs, "quick": bool(args.quick), "what": __doc__.strip().split("\n\n")[0], "scenes": {}}
    for name, make in cases:
        sc, cam = make()
        base = sc.vertices.copy()
        ident = np.array([np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]])
        one = int(np.nonzero(~ident)[0][0])
        one_first, one_count = mesh_range(sc, one)
        rec = {"triangles": int(sc.triangle_count), "vertices": int(base.shape[0]), "instances": int(sc.instances.shape[0]), "builders": {}}
        for builder in (1, 0):
            r = BDPT(0)
            try:
                r.set_option("bvh_builder", builder)
                sc.set_vertices(0, base)
                r.update(sc)
                b = {"nodes": int(r.stats()["bvh_nodes"])}
                b["all_vertices"] = time_refits(r, sc, base, 0, base.shape[0], AMPLITUDES[0][1], runs)
                sc.set_vertices(0, base)
                r.update_vertices(sc)
                b["one_instance_mesh"] = time_refits(r, sc, base, one_first, one_count, AMPLITUDES[0][1], runs)
                # the upload the refit avoids, of the scene as it is deformed now, in this process
                sc.set_vertices(0, displaced(base, AMPLITUDES[0][1], 0.3 * runs))
                r.update_vertices(sc)
                b["upload_device_builder"] = time_uploads(r, sc, 1, 3 if args.quick else 7)
                b["upload_host_builder"] = time_uploads(r, sc, 0, 1 if args.quick else 3)
                b["refit_total_over_device_builder_upload"] = round(b["all_vertices"]["total_ms"]["median"] / b["upload_device_builder"]["median"], 4)
                rec["builders"]["lbvh_gpu" if builder else "sah_host"] = b
                print(name, "builder", builder, json.dumps(b), flush=True)
            finally:
                r.close()
        if name == "atrium":
            # the headline frame on the refitted tree against the tree a build makes of the same vertices
            W, H = (480, 270) if args.quick else (1920, 1080)
            frame = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
            bufs = {
                "radiance": torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"),
                "albedo": torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"),
                "visibility": torch.zeros((H, W, 2), dtype=torch.int32, device="cuda"),
                "depth": torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"),
                "prev_uv": torch.zeros((H, W, 2), dtype=torch.float32, device="cuda"),
            }
            dev_out = {k: v.data_ptr() for k, v in bufs.items()}
            steps, reps = (10, 2) if args.quick else (100, 5)
            rec["frame_ms_per_step"] = {}
            for builder in (1, 0):
                per = {}
                for label, amp in AMPLITUDES:
                    r, fresh = BDPT(0), BDPT(0)
                    try:
                        for x in (r, fresh):
                            x.set_option("bvh_builder", builder)
                            x.set_stream(torch.cuda.current_stream().cuda_stream)
                        sc.set_vertices(0, base)
                        r.update(sc)
                        (built_ms,) = frame_ms([r], frame, dev_out, steps, reps, torch)
                        sc.set_vertices(0, displaced(base, amp, 0.9))
                        info = r.update_vertices(sc)
                        fresh.update(sc)
                        refit_ms, fresh_ms = frame_ms([r, fresh], frame, dev_out, steps, reps, torch)
                        r.render(frame, seed_begin=0, seed_count=1, device_outputs=dev_out)
                        torch.cuda.synchronize()
                        radiance_refit = bufs["radiance"].clone()
                        fresh.render(frame, seed_begin=0, seed_count=1, device_outputs=dev_out)
                        torch.cuda.synchronize()
                        same = bool(torch.equal(radiance_refit.view(torch.int32), bufs["radiance"].view(torch.int32)))
                        per[label] = {"amplitude": amp, "undeformed": spread(built_ms), "refitted": spread(refit_ms), "freshly_built": spread(fresh_ms),
                                      "refitted_over_fresh": round(statistics.median(refit_ms) / statistics.median(fresh_ms), 4),
                                      "sah_cost_over_at_build": round(info["sah_cost"] / info["sah_cost_at_build"], 4), "frames_bit_identical": same}
                        print(name, "frames, builder", builder, label, json.dumps(per[label]), flush=True)
                    finally:
                        r.close()
                        fresh.close()
                rec["frame_ms_per_step"]["lbvh_gpu" if builder else "sah_host"] = per
        result["scenes"][name] = rec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
