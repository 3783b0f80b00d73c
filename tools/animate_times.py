"""Rigs posed on the device: what sthip_scene_animate (bones up, k_animate, gather + refit) costs against
sthip_scene_update_vertices with the same vertices computed elsewhere and sent up (GPU box).

On the 1M-triangle atrium with the device builder, two cases: a rig over all vertices with 4 blend targets and 64 bones,
and a rig over one instance's mesh. For each case RUNS poses; per pose one call of animate, then the posed records are read
back and the same records go through update_vertices in the same process, so both calls refit the same geometry and their
passes alternate. Medians of device_ms and total_ms of sthip_refit_info for both calls (device_ms of animate includes
k_animate; that of the vertex call does not include its upload, which is why total_ms is the figure to compare).

    python tools/animate_times.py [--out profiles/r07/animate.json] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from stratum_amd import scenes, wire
from stratum_amd.bdpt import BDPT

RUNS = 9  # calls per median: odd, and enough that one slow call (a page fault, another process's copy) does not move it


def mesh_range(sc, instance):
    inst = sc.instances["packed"][instance]
    prims, stride, off = int((inst[1] >> 12) & 0xFFFF), int(inst[1] >> 28), int(inst[3])
    idx = np.frombuffer(sc.indices[off : off + 3 * prims * stride].tobytes(), dtype="<u2" if stride == 2 else "<u4").astype(np.int64)
    return int(inst[2]) + int(idx.min()), int(idx.max() - idx.min()) + 1


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def make_rig(rest, first, n_targets, bone_count, seed):
    """Targets: smooth displacements of the rest pose by a few centimetres; weights: two bones per vertex chosen by position."""
    rng = np.random.default_rng(seed)
    targets = []
    for k in range(n_targets):
        t = rest.copy()
        p = t["position"].astype(np.float64)
        t["position"] = (p + 0.03 * np.sin((0.7 + 0.2 * k) * p[:, [1, 2, 0]] + k)).astype(np.float32)
        targets.append(t)
    weights = np.zeros(rest.shape[0], dtype=wire.VertexWeight)
    cell = np.floor(rest["position"][:, 0].astype(np.float64) * 2.0).astype(np.int64)
    weights["indices"][:, 0] = np.mod(cell, bone_count)
    weights["indices"][:, 1] = np.mod(cell + 1, bone_count)
    w = rng.random(rest.shape[0]).astype(np.float32)
    weights["weights"][:, 0], weights["weights"][:, 1] = w, np.float32(1) - w
    return {"first_vertex": first, "vertex_count": rest.shape[0], "blend_targets": targets, "weights": weights, "bone_count": bone_count}


def pose(n_targets, bone_count, k):
    bones = np.zeros((bone_count, 3, 4), dtype=np.float32)
    a = 0.01 * np.sin(0.5 * k + np.arange(bone_count))
    bones[:, 0, 0], bones[:, 0, 2], bones[:, 2, 0], bones[:, 2, 2], bones[:, 1, 1] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a), 1
    bones[:, :, 3] = 0.02 * np.sin(0.3 * k + np.arange(bone_count))[:, None]
    # (positive factors: the targets keep the rest pose's normals, so their blend keeps its length)
    return {"blend_factors": [0.1 + 0.1 * np.sin(0.4 * k + t) for t in range(n_targets)], "bones": bones}


def time_case(r, sc, first, count, n_targets, bone_count, runs):
    rig = make_rig(sc.vertices[first : first + count].copy(), first, n_targets, bone_count, 1)
    r.set_rigs([rig])
    anim = {"device_ms": [], "total_ms": [], "python_wall_ms": []}
    vert = {"device_ms": [], "total_ms": [], "python_wall_ms": []}
    for k in range(runs + 1):  # (the first pass also makes the refit's schedule: not counted)
        p = pose(n_targets, bone_count, k)
        t = time.perf_counter()
        info = r.animate([p])
        wall = (time.perf_counter() - t) * 1e3
        assert info["rebuilt"] == 0
        posed = r.read_vertices(first, count)
        sc.set_vertices(first, posed)
        t = time.perf_counter()
        vinfo = r.update_vertices(sc)
        vwall = (time.perf_counter() - t) * 1e3
        assert vinfo["rebuilt"] == 0 and vinfo["sah_cost"] == info["sah_cost"]  # (the same geometry)
        if k == 0:
            continue
        for rec, i, w in ((anim, info, wall), (vert, vinfo, vwall)):
            rec["device_ms"].append(i["device_ms"])
            rec["total_ms"].append(i["total_ms"])
            rec["python_wall_ms"].append(w)
    out = {"vertices": int(count), "blend_targets": n_targets, "bones": bone_count, "bytes_up_per_animate_call": bone_count * 48,
           "bytes_up_per_update_vertices_call": int(count) * 32,
           "animate": {k: spread(v) for k, v in anim.items()}, "update_vertices": {k: spread(v) for k, v in vert.items()}}
    out["animate_total_over_update_vertices_total"] = round(out["animate"]["total_ms"]["median"] / out["update_vertices"]["total_ms"]["median"], 4)
    out["animate_device_over_update_vertices_device"] = round(out["animate"]["device_ms"]["median"] / out["update_vertices"]["device_ms"]["median"], 4)
    r.set_rigs([])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r07", "animate.json"))
    ap.add_argument("--quick", action="store_true", help="a small scene, few runs: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("animate_times.py needs the GPU: nothing here can be measured without it")
    runs = 3 if args.quick else RUNS
    sc, _ = scenes.atrium(target_tris=60_000) if args.quick else scenes.atrium()
    base = sc.vertices.copy()
    ident = np.array([np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]])
    one_first, one_count = mesh_range(sc, int(np.nonzero(~ident)[0][0]))
    result = {"runs": runs, "quick": bool(args.quick), "what": __doc__.strip().split("\n\n")[0], "scene": "atrium", "builder": "lbvh_gpu", "triangles": int(sc.triangle_count),
              "vertices": int(base.shape[0])}
    r = BDPT(0)
    try:
        r.set_option("bvh_builder", 1)
        r.update(sc)
        result["all_vertices"] = time_case(r, sc, 0, base.shape[0], 4, 64, runs)
        print("all_vertices", json.dumps(result["all_vertices"]), flush=True)
        sc.set_vertices(0, base)
        r.update(sc)
        result["one_instance_mesh"] = time_case(r, sc, one_first, one_count, 4, 64, runs)
        print("one_instance_mesh", json.dumps(result["one_instance_mesh"]), flush=True)
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
