"""Vertices from device memory: what sthip_scene_set_vertices (pack, and normals made again, on the device) costs against
sthip_scene_update_vertices from finished host records, the only route there was (GPU box).

The 1M-triangle atrium with the device builder; every vertex displaced by a sine, and one instance's mesh only. Forms, taken
in turn inside every round so that they share the machine's state, medians of RUNS rounds after a warm-up round:
  (a) update_vertices from host records: 32 B per vertex go up                                   — the yardstick
  (b) set_vertices from device streams: positions, normals and uvs
  (c) set_vertices from device streams: positions only, recompute_normals
  (d) as (c), but the first call on a topology, which makes the adjacency (an upload before each)
Per form the call's wall time and sthip_refit_info's device_ms (HIP events around everything on the stream) and total_ms.
For (c) the HIP-event time of each kernel — k_pack_vertices, k_face_vectors, k_vertex_normals — from the library's
STHIP_VERTEX_TIMES lines (include/sthip.h; read once per process: a child of this script makes those calls), with the
kernel's algorithmic bytes and their rate as a fraction of STHIP_CEILING_TRIAD measured in the same run.

    python tools/vertices_times.py [--out profiles/r15/vertices.json] [--quick]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from stratum_amd import scenes
from stratum_amd.bdpt import BDPT

RUNS = 9  # rounds per median: odd, and enough that one slow call does not move it
STAGES = ("k_pack_vertices_ms", "k_face_vectors_ms", "k_vertex_normals_ms")


def displaced(positions, amp, phase, freq=0.8):
    p = positions.astype(np.float64)
    return np.ascontiguousarray((p + amp * np.sin(freq * p[:, [1, 2, 0]] + phase)).astype(np.float32))  # (rows of 12 bytes, whatever order the sum came in)


def mesh_range(sc, instance):
    inst = sc.instances["packed"][instance]
    prims, stride, off = int((inst[1] >> 12) & 0xFFFF), int(inst[1] >> 28), int(inst[3])
    idx = np.frombuffer(sc.indices[off : off + 3 * prims * stride].tobytes(), dtype="<u2" if stride == 2 else "<u4").astype(np.int64)
    return int(inst[2]) + int(idx.min()), int(idx.max() - idx.min()) + 1


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def meshes_of(sc):
    out = set()
    for p in sc.instances["packed"]:
        if int(p[0]) & 0xF == 0:
            out.add((int(p[3]), int(p[2]), int(p[1]) >> 28, (int(p[1]) >> 12) & 0xFFFF))
    return sorted(out)


def load(quick):
    sc, _ = scenes.atrium(target_tris=60_000) if quick else scenes.atrium()
    ident = np.array([np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]])
    return sc, mesh_range(sc, int(np.nonzero(~ident)[0][0]))


def timed(call):
    t = time.perf_counter()
    info = call()
    wall = (time.perf_counter() - t) * 1e3
    assert info["rebuilt"] == 0
    return {"device_ms": info["device_ms"], "total_ms": info["total_ms"], "python_wall_ms": wall}


def time_case(r, sc, base, first, count, runs, torch):
    forms = {k: {"device_ms": [], "total_ms": [], "python_wall_ms": []} for k in ("a", "b", "c")}
    rest = base[first : first + count]
    normals = torch.from_numpy(np.ascontiguousarray(rest["normal"])).to("cuda:0")
    uvs = torch.from_numpy(np.ascontiguousarray(np.stack([rest["u"], rest["v"]], axis=1))).to("cuda:0")
    for k in range(runs + 1):  # (the first round also makes the refit's schedule and the adjacency: not counted)
        moved = displaced(rest["position"], 0.02, 0.3 * k)
        records = rest.copy()
        records["position"] = moved
        dev = torch.from_numpy(moved).to("cuda:0")
        torch.cuda.synchronize()
        sc.set_vertices(first, records)
        one = {
            "a": timed(lambda: r.update_vertices(sc)),
            "b": timed(lambda: r.set_vertices(first, dev, normals, uvs)),
            "c": timed(lambda: r.set_vertices(first, dev, recompute_normals=True)),
        }
        if k == 0:
            continue
        for name, rec in one.items():
            for field, v in rec.items():
                forms[name][field].append(v)
    out = {"vertices": int(count), "bytes_up_per_update_vertices_call": int(count) * 32, "forms": {n: {f: spread(v) for f, v in rec.items()} for n, rec in forms.items()}}
    for name in ("b", "c"):
        out["%s_total_over_a_total" % name] = round(out["forms"][name]["total_ms"]["median"] / out["forms"]["a"]["total_ms"]["median"], 4)
        out["%s_device_over_a_device" % name] = round(out["forms"][name]["device_ms"]["median"] / out["forms"]["a"]["device_ms"]["median"], 4)
    return out


def time_first_calls(r, sc, base, torch, runs):
    """(d): the call that makes the adjacency, after an upload each time."""
    rec = {"device_ms": [], "total_ms": [], "python_wall_ms": []}
    dev = torch.from_numpy(displaced(base["position"], 0.02, 0.1)).to("cuda:0")
    torch.cuda.synchronize()
    for _ in range(runs):
        sc.set_vertices(0, base)
        r.update(sc)
        one = timed(lambda: r.set_vertices(0, dev, recompute_normals=True))
        for field, v in one.items():
            rec[field].append(v)
    return {f: spread(v) for f, v in rec.items()}


def stages_child(spec):
    """quick,runs: runs + 1 calls of form (c) over every vertex, then over one instance's mesh, under STHIP_VERTEX_TIMES, which
    the parent set for this process."""
    import torch

    quick, runs = (int(v) for v in spec.split(","))
    sc, (one_first, one_count) = load(bool(quick))
    r = BDPT(0)
    try:
        r.set_option("bvh_builder", 1)
        r.update(sc)
        for first, count in ((0, sc.vertices.shape[0]), (one_first, one_count)):
            for k in range(runs + 1):
                dev = torch.from_numpy(displaced(sc.vertices["position"][first : first + count], 0.02, 0.3 * k)).to("cuda:0")
                torch.cuda.synchronize()
                r.set_vertices(first, dev, recompute_normals=True)
    finally:
        r.close()


def stage_records(lines, count, tris, index_bytes, corners, triad):
    """Per kernel of (c): the median HIP-event time and what the kernel has to move at the least. The pack of (c) reads 12 B and
    writes 12 B per vertex; a face vector reads its three indices and three 16-byte position words and writes 16 B; a vertex
    reads its row's bounds (8 B), per corner a slot number (4 B) and a face vector (16 B), and writes 12 B. `corners`: of the
    rows the range walks, or None where the tool does not count them."""
    nbytes = {"k_pack_vertices_ms": 24 * count, "k_face_vectors_ms": index_bytes + tris * (48 + 16), "k_vertex_normals_ms": None if corners is None else count * 20 + corners * 20}
    out = {}
    for name in STAGES:
        ms = statistics.median(x[name] for x in lines)
        rec = {"ms": round(ms, 5), "algorithmic_bytes": nbytes[name]}
        if nbytes[name] is not None and ms > 0:
            rec["gbytes_per_s"] = round(nbytes[name] / (ms * 1e-3) / 1e9, 1)
            rec["fraction_of_triad"] = round(nbytes[name] / (ms * 1e-3) / 1e9 / triad, 4)
        out[name[:-3]] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r15", "vertices.json"))
    ap.add_argument("--quick", action="store_true", help="a small scene, few runs: a rehearsal of the script, not a measurement")
    ap.add_argument("--stages-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.stages_child:
        return stages_child(args.stages_child)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("vertices_times.py needs the GPU: nothing here can be measured without it")
    runs = 3 if args.quick else RUNS
    sc, (one_first, one_count) = load(args.quick)
    base = sc.vertices.copy()
    result = {"runs": runs, "quick": bool(args.quick), "what": __doc__.strip().split("\n\n")[0], "status": "MEASURED", "scene": "atrium", "builder": "lbvh_gpu",
              "triangles": int(sc.triangle_count), "vertices": int(base.shape[0]), "meshes": len(meshes_of(sc))}
    r = BDPT(0)
    try:
        r.set_option("bvh_builder", 1)
        r.update(sc)
        triad = r.measure_ceiling("triad")
        result["triad_gbytes_per_s"] = round(triad, 1)
        result["all_vertices"] = time_case(r, sc, base, 0, base.shape[0], runs, torch)
        print("all_vertices", json.dumps(result["all_vertices"]), flush=True)
        sc.set_vertices(0, base)
        r.update(sc)
        result["one_instance_mesh"] = time_case(r, sc, base, one_first, one_count, runs, torch)
        print("one_instance_mesh", json.dumps(result["one_instance_mesh"]), flush=True)
        result["first_call_with_adjacency"] = time_first_calls(r, sc, base, torch, 3 if args.quick else 5)
        print("first_call_with_adjacency", json.dumps(result["first_call_with_adjacency"]), flush=True)
    finally:
        r.close()
    # the kernels of (c) alone (the library reads the variable once per process: a child of this script makes the calls)
    times_path = os.path.abspath(args.out) + ".stages.tmp"
    os.makedirs(os.path.dirname(times_path), exist_ok=True)
    open(times_path, "w").close()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--stages-child", "%d,%d" % (int(args.quick), runs)], env=dict(os.environ, STHIP_VERTEX_TIMES=times_path),
                           capture_output=True, text=True, timeout=600)
    lines = [json.loads(x) for x in open(times_path) if x.strip()]
    os.remove(times_path)
    if child.returncode != 0 or len(lines) != 2 * (runs + 1):
        result["status"] = "the kernels of (c) NOT MEASURED: %s" % (child.stderr or child.stdout)[-300:]
    else:
        tris = sum(m[3] for m in meshes_of(sc))
        index_bytes = sum(m[3] * 3 * m[2] for m in meshes_of(sc))
        result["all_vertices"]["kernels_of_c"] = stage_records(lines[1 : runs + 1], int(base.shape[0]), tris, index_bytes, 3 * tris, triad)
        result["one_instance_mesh"]["kernels_of_c"] = stage_records(lines[runs + 2 :], int(one_count), tris, index_bytes, None, triad)
        print("kernels_of_c", json.dumps(result["all_vertices"]["kernels_of_c"]), json.dumps(result["one_instance_mesh"]["kernels_of_c"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
