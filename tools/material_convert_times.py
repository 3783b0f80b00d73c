"""The material conversion on the device: stream time of sthip_convert_material (GLTF_PBR, device-pointer form) for a 4096 x 4096
material, with three 8-bit sources and 8-bit outputs and with float sources and float outputs (GPU box).

Per form: the median of the HIP-event times of RUNS calls (the first call is not counted), the algorithmic bytes — every present
source read once, 13 B (three RGBA8 texels and a mask byte) or 52 B written per texel — and their rate as a fraction of
sthip_measure_ceiling(STHIP_CEILING_TRIAD) measured in the same process. The sources are random bytes (their decoded floats in
the float form) with about one texel in eight below alpha 1, so the min-alpha reduction runs.

    python tools/material_convert_times.py [--out profiles/r09/material_convert.json] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from stratum_amd import _lib, wire
from stratum_amd.bdpt import BDPT

RUNS = 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r09", "material_convert.json"))
    ap.add_argument("--quick", action="store_true", help="a 512 x 512 material, few runs: a rehearsal of the script, not a measurement")
    ap.add_argument("--size", type=int, default=4096, help="side of the square material (default 4096; 8192 shows what of the time is per call and what per byte)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("material_convert_times.py needs the GPU: nothing here can be measured without it")
    runs = 3 if args.quick else RUNS
    W = H = 512 if args.quick else args.size
    n = W * H
    result = {"what": __doc__.strip().split("\n\n")[0], "kind": "GLTF_PBR", "width": W, "height": H, "runs": runs, "quick": bool(args.quick), "forms": {}}
    L = _lib.lib()
    r = BDPT(0)
    try:
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        triad = r.measure_ceiling("triad")
        result["triad_gbytes_per_s"] = round(triad, 1)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(9)
        for form, texel_in, texel_out, mask_out in (("rgba8", 4, 4, 1), ("rgba32f", 16, 16, 4)):
            sources = []
            for k in range(3):
                b = torch.randint(0, 256, (n, 4), dtype=torch.uint8, device="cuda", generator=gen)
                if k == 0:
                    opaque = torch.rand(n, device="cuda", generator=gen) > 0.125
                    b[:, 3] = torch.where(opaque, torch.full_like(b[:, 3], 255), b[:, 3])
                sources.append(b if form == "rgba8" else (b.to(torch.float32) / 255.0).contiguous())
            outs = [torch.zeros(n * texel_out, dtype=torch.uint8, device="cuda") for _ in range(3)]
            mask = torch.zeros(n * mask_out, dtype=torch.uint8, device="cuda")
            min_alpha = torch.zeros(1, dtype=torch.int32, device="cuda")
            d = wire.ConvertMaterialDesc()
            d.kind, d.width, d.height, d.device_ptrs = wire.CONVERT["GltfPbr"], W, H, 1
            d.output_format = 1 if form == "rgba8" else 0
            d.diffuse_format = d.specular_format = d.transmittance_format = d.output_format
            d.gDiffuse, d.gSpecular, d.gTransmittance = (s.data_ptr() for s in sources)
            for k in range(3):
                d.gOutput[k] = outs[k].data_ptr()
            d.gOutputAlphaMask, d.gOutputMinAlpha = mask.data_ptr(), min_alpha.data_ptr()
            torch.cuda.synchronize()
            ms = []
            for k in range(runs + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r._check(L.sthip_convert_material(r._h, C.byref(d)), "sthip_convert_material")
                e1.record()
                e1.synchronize()
                if k:
                    ms.append(e0.elapsed_time(e1))
            t_ms = statistics.median(ms)
            nbytes = n * (3 * texel_in + 3 * texel_out + mask_out)
            gbs = nbytes / (t_ms * 1e-3) / 1e9
            entry = {"ms": round(t_ms, 5), "ms_all": [round(x, 5) for x in ms], "algorithmic_bytes": int(nbytes), "bytes_per_texel": 3 * texel_in + 3 * texel_out + mask_out,
                     "gbytes_per_s": round(gbs, 1), "fraction_of_triad": round(gbs / triad, 4), "gtexels_per_s": round(n / (t_ms * 1e-3) / 1e9, 2),
                     "min_alpha": "0x%08x" % (int(min_alpha.cpu().numpy().view(np.uint32)[0]))}
            result["forms"][form] = entry
            print(form, json.dumps(entry), flush=True)
            del sources, outs, mask
            torch.cuda.empty_cache()
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
