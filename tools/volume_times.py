"""The density grids on the device: sthip_build_volume from a dense box in device memory into device memory, and
sthip_scene_set_volume on the resident fog Cornell box, for boxes of 64^3 and 256^3 at about 30 % and 100 % occupancy.

Per box, medians over RUNS calls in one process (the first call is not counted): device_ms (HIP events) and the call's wall
time of sthip_build_volume; of sthip_scene_set_volume from a dense device pointer and from finished host bytes; beside them
what the calls replace and the library could already do — the C call sthip_scene_upload of the fog Cornell box with the same
grid bytes from host memory (the ctypes call alone, its descriptor made before) — and the numpy statement's time for the same
box (stratum_amd/nvdb.py, one run). Algorithmic bytes of the build: the dense box is read by two passes (scan, leaf emit) and
the grid is written once; their rate is given as a fraction of sthip_measure_ceiling(STHIP_CEILING_TRIAD) measured in the same
process.

    python tools/volume_times.py [--out profiles/r13/volume.json] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from stratum_amd import nvdb, scenes
from stratum_amd.bdpt import BDPT

RUNS = 9


def box(n, occupancy, seed):
    """A smooth blob of about `occupancy` of the box (1.0: every voxel active), values in (0, 1]."""
    rng = np.random.default_rng(seed)
    d = (rng.random((n, n, n), dtype=np.float32) * np.float32(0.9) + np.float32(0.1)).astype(np.float32)
    if occupancy < 1.0:
        g = (np.arange(n, dtype=np.float32) + 0.5) / n - 0.5
        r2 = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2
        radius = (occupancy * 3.0 / (4.0 * np.pi)) ** (1.0 / 3.0)  # a ball of that share of the unit cube
        d[r2 > radius * radius] = 0
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r13", "volume.json"))
    ap.add_argument("--quick", action="store_true", help="32^3 and 64^3, few runs: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("volume_times.py needs the GPU: nothing here can be measured without it")
    runs = 3 if args.quick else RUNS
    sizes = (32, 64) if args.quick else (64, 256)
    result = {"what": __doc__.strip().split("\n\n")[0], "runs": runs, "quick": bool(args.quick), "boxes": {}}
    r = BDPT(0)
    try:
        triad = r.measure_ceiling("triad")
        result["triad_gbytes_per_s"] = round(triad, 1)
        for n in sizes:
            for occupancy in (0.3, 1.0):
                dense = box(n, occupancy, 5)
                origin, voxel = (-(n // 2),) * 3, 1.6 / n
                t0 = time.perf_counter()
                want = nvdb.dense_to_nanovdb(dense, origin, voxel, name="density")
                numpy_ms = (time.perf_counter() - t0) * 1e3
                dev = torch.from_numpy(dense).to("cuda:0")
                out = torch.zeros(want.size, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                device_ms, call_ms = [], []
                for k in range(runs + 1):
                    _, info = r.build_volume(dev.data_ptr(), origin, voxel, name="density", dims=dense.shape, out=out.data_ptr(), capacity=out.numel())
                    if k:
                        device_ms.append(info["device_ms"])
                        call_ms.append(info["call_ms"])
                same = bool(np.array_equal(out.cpu().numpy(), want))
                sc, _ = scenes.cornell_box(fog=want)
                r.update(sc)
                desc = sc.desc()
                upload_ms, set_dense, set_dense_dev, set_bytes, set_bytes_dev = [], [], [], [], []
                for k in range(runs + 1):
                    t0 = time.perf_counter()
                    r._check(r._lib.sthip_scene_upload(r._h, C.byref(desc)), "sthip_scene_upload")
                    if k:
                        upload_ms.append((time.perf_counter() - t0) * 1e3)
                for k in range(runs + 1):
                    i1 = r.set_volume(0, dense=dev.data_ptr(), origin=origin, voxel_size=voxel, name="density", dims=dense.shape)
                    i2 = r.set_volume(0, grid=want)
                    if k:
                        set_dense.append(i1["call_ms"]), set_dense_dev.append(i1["device_ms"]), set_bytes.append(i2["call_ms"]), set_bytes_dev.append(i2["device_ms"])
                same = same and bool(np.array_equal(r.read_volume(0), want))
                t_ms = statistics.median(device_ms)
                nbytes = 2 * dense.nbytes + int(want.size)
                gbs = nbytes / (t_ms * 1e-3) / 1e9
                entry = {"voxels": int(dense.size), "active_share": round(float((dense != 0).mean()), 3), "grid_bytes": int(want.size), "leaves": info["leaf_count"], "equals_numpy": same,
                         "build_device_ms": round(t_ms, 4), "build_call_ms": round(statistics.median(call_ms), 4), "build_device_ms_all": [round(x, 4) for x in device_ms],
                         "set_volume_dense_device_call_ms": round(statistics.median(set_dense), 4), "set_volume_dense_device_device_ms": round(statistics.median(set_dense_dev), 4),
                         "set_volume_host_bytes_call_ms": round(statistics.median(set_bytes), 4), "set_volume_host_bytes_device_ms": round(statistics.median(set_bytes_dev), 4),
                         "scene_upload_fog_cornell_ms": round(statistics.median(upload_ms), 3), "numpy_ms": round(numpy_ms, 1), "algorithmic_bytes": int(nbytes), "gbytes_per_s": round(gbs, 1),
                         "fraction_of_triad": round(gbs / triad, 4)}
                result["boxes"]["%d^3 at %.0f %%" % (n, 100 * occupancy)] = entry
                print(n, occupancy, json.dumps(entry), flush=True)
                del dev, out
                torch.cuda.empty_cache()
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
