"""Editing the materials of a resident scene: sthip_scene_set_images against the alternative without it, a read-back and
sthip_scene_upload of the whole scene (GPU box).

The small sky scene of tools/environment_times.py with one 4096 x 4096 parameter image bound by a material, once resident as
RGBA8_UNORM and once as RGBA32F. Per format, medians of RUNS calls after one that is not counted:
  (a) host_pixels    the wall time of the call and its stream time (sthip_images_info) with the texels in pageable host memory;
  (b) device_pixels  the same with the texels behind a device pointer, each call chained behind a sthip_convert_material (device
                     form, GltfPbr, 4096 x 4096) on the context's stream whose parameter output it takes; the conversion alone
                     is timed beside it;
  (c) k_image_range  the HIP-event time of the scan's two launches alone (STHIP_MATERIAL_TIMES, read once per process: a child
                     makes the calls), its algorithmic bytes (every texel of level 0 once) and their rate as a fraction of
                     sthip_measure_ceiling(STHIP_CEILING_TRIAD) measured in the same process as the calls of (a) and (b);
  (d) scene_upload   sthip_scene_upload(_formats) of the same scene in the same process: what the call replaces (the parent
                     commit's only route for (b) is this plus the copy of the converted images back to the host, timed too).
A field that could not be filled is null and "status" says "NOT MEASURED" with the reason.

    python tools/material_update_times.py [--out profiles/r11/material_update.json] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

RUNS = 9
SIDE = 4096


def params_image(side, as_bytes, seed):
    """R scales metallic, G scales roughness; rough everywhere."""
    rng = np.random.RandomState(seed)
    img = np.zeros((side, side, 4), np.uint8)
    img[..., 0] = 255
    img[..., 1] = rng.randint(100, 256, size=(side, side))
    img[..., 3] = 255
    return img if as_bytes else (img.astype(np.float32) / np.float32(255)).astype(np.float32)


def scene_with(image):
    from stratum_amd import scenes
    from stratum_amd.scene import SceneBuilder, translate

    b = SceneBuilder("material")
    floor = b.add_material((0.6, 0.6, 0.6), metallic=1.0, roughness=0.7)
    b.set_material_images(floor, params_image=b.add_image(image))
    lamp = b.add_emitter((9.0, 7.0, 5.0))
    S = 3.0
    b.add_instance(b.add_mesh(*scenes._quad((-S, 0, S), (S, 0, S), (S, 0, -S), (-S, 0, -S), (0, 1, 0))), floor)
    b.add_instance(b.add_mesh(*scenes._quad((-0.4, 0, -0.4), (0.4, 0, -0.4), (0.4, 0, 0.4), (-0.4, 0, 0.4), (0, -1, 0))), lamp, translate((0.0, 1.8, 0.0)))
    b.set_environment((1.0, 1.0, 1.0), b.add_image(scenes.sky_image(64, 32)))
    return b.build()


def median(v):
    return round(statistics.median(v), 5) if v else None


def converter(r, side, out8):
    """A closure that enqueues one device-form GltfPbr conversion on the context's stream, and its three output tensors."""
    import torch

    from stratum_amd import _lib, wire

    rng = np.random.RandomState(5)
    src = [torch.from_numpy(rng.randint(0, 256, size=(side, side, 4)).astype(np.uint8)).to("cuda:0") for _ in range(2)]
    dt = torch.uint8 if out8 else torch.float32
    outs = [torch.zeros((side, side, 4), dtype=dt, device="cuda:0") for _ in range(3)]
    mask = torch.zeros((side, side), dtype=dt, device="cuda:0")
    min_alpha = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d = wire.ConvertMaterialDesc()
    d.kind, d.width, d.height, d.device_ptrs, d.output_format = wire.CONVERT["GltfPbr"], side, side, 1, int(out8)
    d.gDiffuse, d.gSpecular, d.diffuse_format, d.specular_format = src[0].data_ptr(), src[1].data_ptr(), 1, 1
    for k in range(3):
        d.gOutput[k] = outs[k].data_ptr()
    d.gOutputAlphaMask, d.gOutputMinAlpha = mask.data_ptr(), min_alpha.data_ptr()
    torch.cuda.synchronize()
    keep = (src, mask, min_alpha, d)

    def convert():
        r._check(_lib.lib().sthip_convert_material(r._h, C.byref(keep[3])), "sthip_convert_material")

    return convert, outs


def kernel_child(spec):
    """bytes,side,runs: runs + 1 device-pointer calls under STHIP_MATERIAL_TIMES, which the parent set for this process."""
    import torch

    from stratum_amd.bdpt import BDPT

    as_bytes, side, runs = (int(v) for v in spec.split(","))
    r = BDPT(0)
    try:
        r.update(scene_with(params_image(side, bool(as_bytes), 1)))
        dev = torch.from_numpy(params_image(side, bool(as_bytes), 2)).to("cuda:0")
        torch.cuda.synchronize()
        for _ in range(runs + 1):
            r.set_images({0: dev}, device_ptr=True)
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r11", "material_update.json"))
    ap.add_argument("--quick", action="store_true", help="a 256 x 256 image, three runs: a rehearsal of the script, not a measurement")
    ap.add_argument("--kernel-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernel_child:
        return kernel_child(args.kernel_child)
    runs = 3 if args.quick else RUNS
    side = 256 if args.quick else SIDE
    result = {"what": __doc__.strip().split("\n\n")[0], "runs": runs, "quick": bool(args.quick), "status": "MEASURED", "side": side, "triad_gbytes_per_s": None, "formats": {}}
    for name in ("rgba8", "rgba32f"):
        result["formats"][name] = {"host_pixels": None, "device_pixels": None, "k_image_range": None, "scene_upload_ms": None, "read_back_ms": None, "parent_route_ms": None}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print("wrote", args.out)

    try:
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("no GPU in this process")
    except Exception as e:  # the fields stay null
        result["status"] = "NOT MEASURED: %s" % e
        write()
        return
    from stratum_amd.bdpt import BDPT

    tmp = tempfile.mkdtemp(prefix="material_times")
    times_path = os.path.join(tmp, "scan.jsonl")
    r = BDPT(0)
    try:
        triad = r.measure_ceiling("triad")
        result["triad_gbytes_per_s"] = round(triad, 1)
        for name, as_bytes in (("rgba8", True), ("rgba32f", False)):
            entry = result["formats"][name]
            A, B = params_image(side, as_bytes, 1), params_image(side, as_bytes, 2)
            sc = scene_with(A)
            r.update(sc)
            # (a) host pixels
            calls, streams = [], []
            for k in range(runs + 1):
                info = r.set_images({0: B})
                if k:
                    calls.append(info["total_ms"])
                    streams.append(info["device_ms"])
            entry["host_pixels"] = {"call_ms": median(calls), "stream_ms": median(streams)}
            print(name, "host_pixels", entry["host_pixels"], flush=True)
            # (b) a device pointer, chained behind the conversion
            convert, outs = converter(r, side, as_bytes)
            alone, chained, calls = [], [], []
            for k in range(runs + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                convert()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                convert()
                info = r.set_images({0: outs[1]}, device_ptr=True)  # (returns when its work on the stream has finished)
                t2 = time.perf_counter()
                if k:
                    alone.append((t1 - t0) * 1e3)
                    chained.append((t2 - t1) * 1e3)
                    calls.append(info["total_ms"])
            entry["device_pixels"] = {"convert_alone_ms": median(alone), "convert_then_set_images_ms": median(chained), "call_ms": median(calls)}
            print(name, "device_pixels", entry["device_pixels"], flush=True)
            # (d) what it replaces: the converted images back to the host, and the whole scene again
            backs = []
            for k in range(runs + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = [o.cpu().numpy() for o in outs]
                if k:
                    backs.append((time.perf_counter() - t0) * 1e3)
            sc.images[0] = np.ascontiguousarray(host[1])
            uploads = []
            for k in range(runs + 1):
                t0 = time.perf_counter()
                r.update(sc)
                if k:
                    uploads.append((time.perf_counter() - t0) * 1e3)
            entry["scene_upload_ms"], entry["read_back_ms"] = median(uploads), median(backs)
            entry["parent_route_ms"] = round(entry["device_pixels"]["convert_alone_ms"] + median(backs) + median(uploads), 4)
            print(name, "upload", entry["scene_upload_ms"], "read back", entry["read_back_ms"], flush=True)
            del outs, convert
            torch.cuda.empty_cache()
            # (c) the scan alone (the library reads the variable once per process: a child of this script makes the calls)
            open(times_path, "w").close()
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-child", "%d,%d,%d" % (int(as_bytes), side, runs)], env=dict(os.environ, STHIP_MATERIAL_TIMES=times_path),
                                   capture_output=True, text=True, timeout=300)
            lines = [json.loads(x) for x in open(times_path) if x.strip()][-runs:]
            if child.returncode != 0 or len(lines) != runs:
                result["status"] = "k_image_range NOT MEASURED for %s: %s" % (name, (child.stderr or child.stdout)[-300:])
                continue
            ms = median([x["k_image_range_ms"] for x in lines])
            nbytes = side * side * (4 if as_bytes else 16)
            gbs = nbytes / (ms * 1e-3) / 1e9
            entry["k_image_range"] = {"ms": ms, "blocks": lines[-1]["blocks"], "algorithmic_bytes": nbytes, "gbytes_per_s": round(gbs, 1), "fraction_of_triad": round(gbs / triad, 4)}
            print(name, "k_image_range", entry["k_image_range"], flush=True)
    finally:
        r.close()
    write()


if __name__ == "__main__":
    main()
