"""What moving every instance of a resident scene costs (profiles/r12/top_level.json; needs the GPU):

  (a) sthip_scene_update_transforms from host arrays (the host's binned-SAH top level),
  (b) what a producer that holds its matrices in device memory had to do before: three device-to-host copies, then (a),
  (c) sthip_scene_set_transforms with device pointers, derived inverse and motion, the device-built top level,
  (d) sthip_scene_set_transforms with host pointers and the device-built top level,

on the forest (1 000 instances) and on synthetic scenes of 8 192 and 65 533 instances of a small mesh (the most top-level
entries an upload takes: 0xFFFE and 0xFFFF are the traversal's stack sentinels); medians of `--runs` calls
after a warm-up, a host clock around calls that end in a device synchronise; device_ms / total_ms of the info struct for (c)
and (d); and the frame time of the default flags (1920 x 1080, device outputs, windows of frames that end in a synchronise)
under the host-built and under the device-built top level, taken in alternation, with their ratio and its spread over the windows.

  python tools/top_level_times.py [--runs 9] [--quick] [--out profiles/r12/top_level.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stratum_amd import camera, scenes, wire  # noqa: E402
from stratum_amd.bdpt import BDPT  # noqa: E402
from stratum_amd.scene import SceneBuilder, translate, scale  # noqa: E402


def synthetic(n):
    """n instances of a two-triangle quad on a jittered grid over a merged floor, a quad light above."""
    rng = np.random.default_rng(n)
    b = SceneBuilder("instances_%d" % n)
    white = b.add_material((0.73, 0.73, 0.73))
    lamp = b.add_emitter((18.0, 15.0, 10.0))
    pos = np.array([(-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0)], np.float32)
    nrm = np.tile(np.array((0, 0, 1), np.float32), (4, 1))
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    tri = np.array([[0, 1, 2], [0, 2, 3]])
    mesh = b.add_mesh(pos, nrm, uv, tri)
    side = int(np.ceil(np.sqrt(n - 2)))
    step = 1.8 / side
    for k in range(n - 2):
        j = (rng.random(3) - 0.5) * 0.3 * step
        b.add_instance(mesh, white, translate(((k % side + 0.5) * step - 0.9 + j[0], (k // side + 0.5) * step - 0.9 + j[1], j[2])) @ scale((0.6 * step,) * 3))
    floor = np.array([(-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1)], np.float32)
    b.add_instance(b.add_mesh(floor, np.tile(np.array((0, 1, 0), np.float32), (4, 1)), uv, tri), white)
    light = np.array([(-0.3, 0.99, 0.3), (0.3, 0.99, 0.3), (0.3, 0.99, 0.9), (-0.3, 0.99, 0.9)], np.float32)
    b.add_instance(b.add_mesh(light, np.tile(np.array((0, -1, 0), np.float32), (4, 1)), uv, tri), lamp, translate((0.0, 0.0, 0.001)))
    return b.build(), {"eye": (0.0, 0.0, 3.9), "target": (0.0, 0.0, 0.0), "fovy": np.radians(39.3)}


def inverse_batch(xf):
    """scene.transform_inverse over (n, 3, 4) float32, vectorised in binary64 in the same order."""
    a = xf.astype(np.float64)
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = (a[:, i, j] for i in range(3) for j in range(3))
    c00, c01, c02 = a11 * a22 - a12 * a21, a12 * a20 - a10 * a22, a10 * a21 - a11 * a20
    det = a00 * c00 + a01 * c01 + a02 * c02
    rows = [[c00 / det, (a02 * a21 - a01 * a22) / det, (a01 * a12 - a02 * a11) / det],
            [c01 / det, (a00 * a22 - a02 * a20) / det, (a02 * a10 - a00 * a12) / det],
            [c02 / det, (a01 * a20 - a00 * a21) / det, (a00 * a11 - a01 * a10) / det]]
    out = np.zeros_like(xf)
    for r in range(3):
        for c in range(3):
            out[:, r, c] = rows[r][c]
        out[:, r, 3] = 0.0 - (rows[r][0] * a[:, 0, 3] + rows[r][1] * a[:, 1, 3] + rows[r][2] * a[:, 2, 3])
    return out


def as_td(a):
    out = np.zeros(a.shape[0], wire.TransformData)
    out["m"] = a
    return out


def median_ms(fn, runs, sync):
    fn()
    sync()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def measure(name, sc, cam, runs, width, height):
    import torch

    sync = torch.cuda.synchronize
    n = sc.instances.shape[0]
    identity = np.eye(4, dtype=np.float32)[:3, :]
    movable = np.array([not np.array_equal(sc.transforms["m"][i], identity) for i in range(n)])
    rng = np.random.default_rng(1)
    ext = float(np.abs(sc.transforms["m"][:, :, 3]).max()) or 1.0

    def next_move():
        xf = sc.transforms["m"].copy()
        xf[movable, :, 3] += (rng.random((int(movable.sum()), 3)).astype(np.float32) - 0.5) * np.float32(0.01 * ext)
        inv = inverse_batch(xf)
        return xf, inv

    r = BDPT(device=0)
    r.update(sc)
    identity_motion = np.tile(identity, (n, 1, 1))
    rec = {"instances": n, "moved": int(movable.sum())}
    moves = [next_move() for _ in range(runs + 1)]
    tds = [(as_td(x), as_td(i), as_td(identity_motion)) for x, i in moves]
    devs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (x, i, identity_motion)) for x, i in moves]
    sync()
    it = {"k": 0}

    def pick(seq):
        it["k"] = (it["k"] + 1) % len(seq)
        return seq[it["k"]]

    def a_call():
        x, i, m = pick(tds)
        r._check(r._lib.sthip_scene_update_transforms(r._h, wire.ptr(x), wire.ptr(i), wire.ptr(m), n), "sthip_scene_update_transforms")

    def b_call():
        x, i, m = (t.cpu().numpy() for t in pick(devs))
        r._check(r._lib.sthip_scene_update_transforms(r._h, wire.ptr(as_td(x)), wire.ptr(as_td(i)), wire.ptr(as_td(m)), n), "sthip_scene_update_transforms")

    infos = {"c": [], "d": []}

    def c_call():
        infos["c"].append(r.set_transforms(pick(devs)[0], None, None, derive_motion=True, top_level="device"))

    def d_call():
        x, i = pick(moves)
        infos["d"].append(r.set_transforms(x, i, identity_motion, top_level="device"))

    for key, fn in (("a_update_transforms_host_arrays", a_call), ("b_copy_back_then_update_transforms", b_call), ("c_set_transforms_device_ptr_derived_device_builder", c_call),
                    ("d_set_transforms_host_ptr_device_builder", d_call)):
        med, lo, hi = median_ms(fn, runs, sync)
        rec[key] = {"call_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
    for key, tag in (("c_set_transforms_device_ptr_derived_device_builder", "c"), ("d_set_transforms_host_ptr_device_builder", "d")):
        tail = infos[tag][1:]
        rec[key]["info_device_ms"] = round(float(np.median([i["device_ms"] for i in tail])), 4)
        rec[key]["info_total_ms"] = round(float(np.median([i["total_ms"] for i in tail])), 4)
        rec[key]["top_level_nodes"] = tail[-1]["top_level_nodes"]
        rec[key]["top_level_depth"] = tail[-1]["top_level_depth"]
    # the frame under either top level: two renderers moved to the same matrices, one by each builder, device outputs, windows
    # of `steps` frames that end in a synchronise, taken in turn (host, device, host, ...) after a warm-up of each
    fr = camera.Frame(width, height, cam["fovy"], cam["eye"], cam["target"])
    x, i = moves[0]
    other = BDPT(device=0)
    other.update(sc)
    pair = {"host": r, "device": other}
    bufs = {"radiance": torch.zeros((height, width, 4), dtype=torch.float32, device="cuda"), "albedo": torch.zeros((height, width, 4), dtype=torch.float32, device="cuda"),
            "visibility": torch.zeros((height, width, 2), dtype=torch.int32, device="cuda"), "depth": torch.zeros((height, width, 4), dtype=torch.float32, device="cuda"),
            "prev_uv": torch.zeros((height, width, 2), dtype=torch.float32, device="cuda")}
    dev_out = {k: v.data_ptr() for k, v in bufs.items()}
    for builder, q in pair.items():
        q.set_transforms(x, i, identity_motion, top_level=builder)
        q.set_option("answer_last_rays", 0)  # every ray is traced, as in the bench line
        for k in range(3):
            q.render(fr, seed_begin=k, seed_count=1, device_outputs=dev_out)
    sync()
    steps = max(10, 4 * runs)
    times = {"host": [], "device": []}
    for rep in range(runs):
        for builder, q in pair.items():
            t0 = time.perf_counter()
            for k in range(steps):
                q.render(fr, seed_begin=k, seed_count=1, device_outputs=dev_out)
            sync()
            times[builder].append((time.perf_counter() - t0) * 1e3 / steps)
    ratios = np.array(times["device"]) / np.array(times["host"])
    rec["frame"] = {"extent": [width, height], "steps_per_window": steps, "windows": runs, "host_built_ms": round(float(np.median(times["host"])), 4),
                    "device_built_ms": round(float(np.median(times["device"])), 4), "ratio_device_over_host": round(float(np.median(ratios)), 4), "ratio_min": round(float(ratios.min()), 4),
                    "ratio_max": round(float(ratios.max()), 4)}
    other.close()
    r.close()
    print(name, json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--quick", action="store_true", help="small scenes (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "top_level.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("top_level_times.py measures on the GPU: none found")
    width, height = (256, 144) if args.quick else (1920, 1080)
    cases = [("forest", lambda: scenes.forest(n_instances=60, tree_tris=600, tree_kinds=2) if args.quick else scenes.forest()),
             ("instances_8192", lambda: synthetic(300 if args.quick else 8192)), ("instances_65533", lambda: synthetic(700 if args.quick else 65533))]
    out = {"what": __doc__.split("\n\n")[0], "runs": args.runs, "quick": args.quick, "status": "MEASURED", "device": torch.cuda.get_device_name(0), "scenes": {}}
    for name, make in cases:
        sc, cam = make()
        out["scenes"][name] = measure(name, sc, cam, args.runs, width, height)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
