"""Source texel formats on the device: what decoding an asset's own formats costs, for a 4096 x 4096 glTF material (GPU box).

sthip_convert_material (GLTF_PBR: diffuse + metallic/roughness, 8-bit outputs, device-pointer form) in three source setups,
    (a) both sources RGBA8_UNORM                        the call as it was
    (b) diffuse RGBA8_SRGB                              the same bytes moved: the supposition to confirm is the same time
    (c) diffuse BC3_SRGB, metallic/roughness BC1_RGB    a .dds asset (and once more as plain BC3: what of it is the curve)
run alternately, RUNS rounds after one that is not counted; per setup the median of the HIP-event times and of the wall times
(a host clock around the call and a stream synchronise), the algorithmic bytes (every source read once, 13 B written per texel)
and their rate as a fraction of sthip_measure_ceiling(STHIP_CEILING_TRIAD) measured in the same process.
sthip_decode_texels to RGBA32F (device form) for RGBA8_SRGB, RGB8_UNORM, BC1_RGB, BC3, BC5_UNORM and BC3_SRGB, measured the same way.
The only route (b) had before the formats: a float32 decode of the sRGB bytes on 16 host threads (a 256-entry table, numpy
take over row bands), then the host form of the call with an RGBA32F diffuse from host memory; wall time, median of RUNS.

    python tools/texel_decode_times.py [--out profiles/r16/texel_decode.json] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from stratum_amd import _lib, wire
from stratum_amd.bdpt import BDPT

RUNS = 9
T = wire.TEXEL_FORMATS


def timed(torch, call):
    """(HIP-event ms, wall ms) of one call that only enqueues: events around it, the clock around it and a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def summary(ms, wall, nbytes, n, triad):
    t = statistics.median(ms)
    gbs = nbytes / (t * 1e-3) / 1e9
    return {"ms": round(t, 5), "ms_all": [round(x, 5) for x in ms], "wall_ms": round(statistics.median(wall), 5), "algorithmic_bytes": int(nbytes), "bytes_per_texel": round(nbytes / n, 3),
            "gbytes_per_s": round(gbs, 1), "fraction_of_triad": round(gbs / triad, 4), "gtexels_per_s": round(n / (t * 1e-3) / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r16", "texel_decode.json"))
    ap.add_argument("--quick", action="store_true", help="a 512 x 512 material, few runs: a rehearsal of the script, not a measurement")
    ap.add_argument("--size", type=int, default=4096)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("texel_decode_times.py needs the GPU: nothing here can be measured without it")
    runs = 3 if args.quick else RUNS
    W = H = 512 if args.quick else args.size
    n = W * H
    result = {"what": __doc__.strip().split("\n\n")[0], "width": W, "height": H, "runs": runs, "quick": bool(args.quick)}
    L = _lib.lib()
    r = BDPT(0)
    try:
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        triad = r.measure_ceiling("triad")
        result["triad_gbytes_per_s"] = round(triad, 1)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(16)

        def random_bytes(count):
            return torch.randint(0, 256, (count,), dtype=torch.uint8, device="cuda", generator=gen)

        # ---- sthip_convert_material, three setups, alternating ----
        diffuse = random_bytes(n * 4).view(n, 4)
        opaque = torch.rand(n, device="cuda", generator=gen) > 0.125  # about one texel in eight below alpha 1: the reduction runs
        diffuse[:, 3] = torch.where(opaque, torch.full_like(diffuse[:, 3], 255), diffuse[:, 3])
        specular = random_bytes(n * 4)
        blocks = (W // 4) * (H // 4)
        bc3, bc1 = random_bytes(blocks * 16), random_bytes(blocks * 8)
        outs = [torch.zeros(n * 4, dtype=torch.uint8, device="cuda") for _ in range(3)]
        mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
        min_alpha = torch.zeros(1, dtype=torch.int32, device="cuda")

        def convert_desc(d_format, d_ptr, s_format, s_ptr):
            d = wire.ConvertMaterialDesc()
            d.kind, d.width, d.height, d.device_ptrs, d.output_format = wire.CONVERT["GltfPbr"], W, H, 1, 1
            d.diffuse_format, d.specular_format = d_format, s_format
            d.gDiffuse, d.gSpecular = d_ptr, s_ptr
            for k in range(3):
                d.gOutput[k] = outs[k].data_ptr()
            d.gOutputAlphaMask, d.gOutputMinAlpha = mask.data_ptr(), min_alpha.data_ptr()
            return d

        setups = {
            "a_rgba8_unorm": (convert_desc(1, diffuse.data_ptr(), 1, specular.data_ptr()), n * (4 + 4 + 13)),
            "b_diffuse_rgba8_srgb": (convert_desc(T["RGBA8_SRGB"], diffuse.data_ptr(), 1, specular.data_ptr()), n * (4 + 4 + 13)),
            "c_bc3_srgb_bc1": (convert_desc(T["BC3_SRGB"], bc3.data_ptr(), T["BC1_RGB"], bc1.data_ptr()), blocks * 24 + n * 13),
            "c_without_the_curve_bc3_bc1": (convert_desc(T["BC3"], bc3.data_ptr(), T["BC1_RGB"], bc1.data_ptr()), blocks * 24 + n * 13),  # (what of (c) is det_powf)
        }
        times = {k: ([], []) for k in setups}
        torch.cuda.synchronize()
        for k in range(runs + 1):
            for name, (d, _) in setups.items():
                ms, wall = timed(torch, lambda: r._check(L.sthip_convert_material(r._h, C.byref(d)), "sthip_convert_material"))
                if k:
                    times[name][0].append(ms)
                    times[name][1].append(wall)
        result["convert_material"] = {name: summary(times[name][0], times[name][1], setups[name][1], n, triad) for name in setups}
        cm = result["convert_material"]
        result["ratios"] = {"b_over_a": round(cm["b_diffuse_rgba8_srgb"]["ms"] / cm["a_rgba8_unorm"]["ms"], 4), "c_over_a": round(cm["c_bc3_srgb_bc1"]["ms"] / cm["a_rgba8_unorm"]["ms"], 4),
                            "c_without_the_curve_over_a": round(cm["c_without_the_curve_bc3_bc1"]["ms"] / cm["a_rgba8_unorm"]["ms"], 4)}
        for name in setups:
            print(name, json.dumps(cm[name]), flush=True)

        # ---- sthip_decode_texels to RGBA32F ----
        dst = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        sources = {"RGBA8_SRGB": diffuse, "RGB8_UNORM": random_bytes(n * 3), "BC1_RGB": bc1, "BC3": bc3, "BC5_UNORM": random_bytes(blocks * 16), "BC3_SRGB": bc3}
        descs = {}
        for name, src in sources.items():
            d = wire.DecodeTexelsDesc()
            d.src_format, d.width, d.height, d.device_ptrs, d.dst_format, d.dst_channels = T[name], W, H, 1, 0, 4
            d.src, d.dst = src.data_ptr(), dst.data_ptr()
            descs[name] = d
        times = {k: ([], []) for k in descs}
        torch.cuda.synchronize()
        for k in range(runs + 1):
            for name, d in descs.items():
                ms, wall = timed(torch, lambda: r._check(L.sthip_decode_texels(r._h, C.byref(d)), "sthip_decode_texels"))
                if k:
                    times[name][0].append(ms)
                    times[name][1].append(wall)
        result["decode_texels_to_rgba32f"] = {name: summary(times[name][0], times[name][1], wire.texel_image_bytes(name, W, H) + n * 16, n, triad) for name in descs}
        for name in descs:
            print(name, json.dumps(result["decode_texels_to_rgba32f"][name]), flush=True)
        torch.cuda.synchronize()

        # ---- the route (b) had before: decode on the host, RGBA32F diffuse from host memory ----
        host_diffuse, host_specular = diffuse.cpu().numpy(), specular.cpu().numpy().reshape(H, W, 4)
        c = np.arange(256, dtype=np.float32) / np.float32(255)
        table = np.where(c <= 0.04045, c / np.float32(12.92), ((c + np.float32(0.055)) / np.float32(1.055)) ** np.float32(2.4)).astype(np.float32)
        linear = c
        decoded = np.empty((n, 4), np.float32)
        bands = np.array_split(np.arange(n), 16)

        def band(rows):
            lo, hi = rows[0], rows[-1] + 1
            decoded[lo:hi, :3] = table[host_diffuse[lo:hi, :3]]
            decoded[lo:hi, 3] = linear[host_diffuse[lo:hi, 3]]

        decode_ms, call_ms = [], []
        with ThreadPoolExecutor(16) as pool:
            for k in range(runs + 1):
                t0 = time.perf_counter()
                list(pool.map(band, bands))
                t1 = time.perf_counter()
                r.convert_material("GltfPbr", diffuse=decoded.reshape(H, W, 4), specular=host_specular, output_format=1)
                t2 = time.perf_counter()
                if k:
                    decode_ms.append((t1 - t0) * 1e3)
                    call_ms.append((t2 - t1) * 1e3)
        t0 = time.perf_counter()
        r.convert_material("GltfPbr", diffuse=wire.TexelImage(host_diffuse, "RGBA8_SRGB", W, H), specular=host_specular, output_format=1)
        result["host_route_for_b"] = {"host_decode_wall_ms": round(statistics.median(decode_ms), 3), "host_form_call_rgba32f_wall_ms": round(statistics.median(call_ms), 3),
                                      "total_wall_ms": round(statistics.median(decode_ms) + statistics.median(call_ms), 3), "host_threads": 16,
                                      "host_form_call_rgba8_srgb_wall_ms_once": round((time.perf_counter() - t0) * 1e3, 3)}
        print("host route", json.dumps(result["host_route_for_b"]), flush=True)
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
