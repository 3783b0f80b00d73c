"""Replacing the environment of a resident scene: sthip_scene_set_environment against the alternative without it, the host
build of the dist2d tables followed by sthip_scene_upload (GPU box).

Per size (2048 x 1024 and 4096 x 2048 RGBA32F skies over a small scene), medians of RUNS calls after one that is not counted:
  forms       the wall time of the call and its stream time (sthip_environment_info) with the pixels in pageable host memory,
              with the pixels behind a device pointer, and with no pixels (the tables of what is resident);
  parent      build_distributions of stratum_amd/host/stratum_hip.hpp (one thread, g++ -O2, compiled here into a helper that
              is loaded into this process) and sthip_scene_upload of the same scene, each on its own;
  kernels     per rows-per-wave value of k_env_rows (16, 64): the HIP-event time of each stage of the device-pointer form
              (STHIP_ENVIRONMENT_TIMES), its algorithmic bytes and their rate as a fraction of
              sthip_measure_ceiling(STHIP_CEILING_TRIAD) measured in the same process.
A field that could not be filled is null and "status" says "NOT MEASURED" with the reason.

    python tools/environment_times.py [--out profiles/r10/environment.json] [--quick]
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
SIZES = [(1024, 2048), (2048, 4096)]  # (H, W)

HELPER = r"""
#include <chrono>
#include "%s"
extern "C" double host_build_distributions_ms(const float* rgba, unsigned w, unsigned h, float* out) {
  stm::Image img;
  img.width = w, img.height = h;
  img.pixels.assign(rgba, rgba + (size_t)w * h * 4);
  std::vector<float> a, b, c, d;
  const auto t0 = std::chrono::steady_clock::now();
  stm::build_distributions(img, a, b, c, d);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  size_t at = 0;
  for (const std::vector<float>* v : {&a, &b, &c, &d}) {
    std::copy(v->begin(), v->end(), out + at);
    at += v->size();
  }
  return ms;
}
"""


def build_helper(tmp):
    src, lib = os.path.join(tmp, "host_tables.cpp"), os.path.join(tmp, "libhost_tables.so")
    with open(src, "w") as f:
        f.write(HELPER % os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp"))
    libdir = os.path.join(ROOT, "stratum_amd")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", lib, src, "-L" + libdir, "-lstratum_hip", "-Wl,-rpath," + libdir])
    h = C.CDLL(lib)
    h.host_build_distributions_ms.restype = C.c_double
    h.host_build_distributions_ms.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]
    return h


def sky(h, w, seed):
    rng = np.random.RandomState(seed)
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = (1e-2 * np.exp(rng.standard_normal((h, w, 3)))).astype(np.float32)
    img[h // 3, (2 * w) // 3, :3] = 1e5
    return img


def scene_with(image):
    from stratum_amd import scenes
    from stratum_amd.scene import SceneBuilder, translate

    b = SceneBuilder("sky")
    floor = b.add_material((0.6, 0.6, 0.6), roughness=0.7)
    lamp = b.add_emitter((9.0, 7.0, 5.0))
    S = 3.0
    b.add_instance(b.add_mesh(*scenes._quad((-S, 0, S), (S, 0, S), (S, 0, -S), (-S, 0, -S), (0, 1, 0))), floor)
    b.add_instance(b.add_mesh(*scenes._quad((-0.4, 0, -0.4), (0.4, 0, -0.4), (0.4, 0, 0.4), (-0.4, 0, 0.4), (0, -1, 0))), lamp, translate((0.0, 1.8, 0.0)))
    b.set_environment((1.0, 1.0, 1.0), b.add_image(image))
    return b.build(environment_tables="device")  # (the tables of the alternative come from the C++ helper below: the numpy loop is not what is measured)


def median(v):
    return round(statistics.median(v), 5) if v else None


def stage_bytes(h, w):
    mips, cw, ch = 0, w, h
    while cw > 1 or ch > 1:
        nw, nh = max(1, cw // 2), max(1, ch // 2)
        mips += 16 * cw * ch + 16 * nw * nh  # (every source texel is read once where the extent is even)
        cw, ch = nw, nh
    cdf = 4 * h * (w + 1)
    return {"copy_ms": 2 * 16 * w * h, "mips_ms": mips, "k_env_rows_ms": 16 * w * h + 8 * h + cdf + 4 * h, "k_env_marginal_ms": 3 * 4 * h + 2 * 4 * (h + 1),
            "k_env_normalise_ms": 16 * w * h + 2 * cdf + 4 * h * w + 4 * h}


def stages_child(spec):
    """h,w,rows,runs: runs + 1 device-pointer calls under STHIP_ENVIRONMENT_TIMES, which the parent set for this process."""
    import torch

    from stratum_amd.bdpt import BDPT

    h, w, rows, runs = (int(v) for v in spec.split(","))
    r = BDPT(0)
    try:
        r.set_option("env_rows_per_wave", rows)
        r.update(scene_with(sky(h, w, 1)))
        dev = torch.from_numpy(sky(h, w, 2)).to("cuda:0")
        torch.cuda.synchronize()
        for _ in range(runs + 1):
            r.set_environment(image=dev, device_ptr=True)
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "environment.json"))
    ap.add_argument("--quick", action="store_true", help="a 256 x 128 sky, three runs: a rehearsal of the script, not a measurement")
    ap.add_argument("--stages-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.stages_child:
        return stages_child(args.stages_child)
    runs = 3 if args.quick else RUNS
    sizes = [(128, 256)] if args.quick else SIZES
    result = {"what": __doc__.strip().split("\n\n")[0], "runs": runs, "quick": bool(args.quick), "status": "MEASURED", "triad_gbytes_per_s": None, "sizes": {}}
    for h, w in sizes:
        result["sizes"]["%dx%d" % (w, h)] = {"width": w, "height": h, "forms": {k: {"call_ms": None, "stream_ms": None} for k in ("host_pixels", "device_pixels", "tables_only")},
                                             "parent": {"host_build_distributions_ms": None, "scene_upload_ms": None, "sum_ms": None}, "kernels": {"16": None, "64": None},
                                             "pixel_call_faster_than_host_table_build": None}

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

    tmp = tempfile.mkdtemp(prefix="environment_times")
    try:
        helper = build_helper(tmp)
    except Exception as e:
        helper = None
        result["status"] = "parent alternative NOT MEASURED: the helper did not build (%s)" % e
    times_path = os.path.join(tmp, "stages.jsonl")
    r = BDPT(0)
    try:
        triad = r.measure_ceiling("triad")
        result["triad_gbytes_per_s"] = round(triad, 1)
        for h, w in sizes:
            entry = result["sizes"]["%dx%d" % (w, h)]
            A, B = sky(h, w, 1), sky(h, w, 2)
            sc = scene_with(A)
            r.update(sc)
            dev = torch.from_numpy(B).to("cuda:0")
            torch.cuda.synchronize()
            for form, kw in (("host_pixels", dict(image=B)), ("device_pixels", dict(image=dev, device_ptr=True)), ("tables_only", {})):
                calls, streams = [], []
                for k in range(runs + 1):
                    info = r.set_environment(**kw)
                    if k:
                        calls.append(info["total_ms"])
                        streams.append(info["device_ms"])
                entry["forms"][form] = {"call_ms": median(calls), "stream_ms": median(streams), "call_ms_all": [round(x, 4) for x in calls]}
                print(w, h, form, entry["forms"][form], flush=True)
            # the stages, per row ownership
            nbytes = stage_bytes(h, w)
            for rows in (16, 64):
                # (the library reads the variable once per process: a child of this script makes the calls)
                open(times_path, "w").close()
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--stages-child", "%d,%d,%d,%d" % (h, w, rows, runs)], env=dict(os.environ, STHIP_ENVIRONMENT_TIMES=times_path),
                                       capture_output=True, text=True, timeout=300)
                lines = [json.loads(x) for x in open(times_path) if x.strip() and json.loads(x)["rows_per_wave"] == rows][-runs:]
                if child.returncode != 0 or len(lines) != runs:
                    result["status"] = "stages NOT MEASURED for %d x %d, %d rows per wave: %s" % (w, h, rows, (child.stderr or child.stdout)[-300:])
                    continue
                stages = {}
                for name in ("copy_ms", "mips_ms", "sines_ms", "k_env_rows_ms", "k_env_marginal_ms", "k_env_normalise_ms"):
                    ms = median([x[name] for x in lines])
                    stages[name[:-3]] = {"ms": ms}
                    if name in nbytes and ms:
                        gbs = nbytes[name] / (ms * 1e-3) / 1e9
                        stages[name[:-3]].update(algorithmic_bytes=int(nbytes[name]), gbytes_per_s=round(gbs, 1), fraction_of_triad=round(gbs / triad, 4))
                entry["kernels"][str(rows)] = stages
                print(w, h, "rows_per_wave", rows, json.dumps(stages), flush=True)
            # the alternative: the host's tables, then the whole scene again
            if helper is not None:
                tables = np.zeros(sc.distributions.size, np.float32)
                build = [helper.host_build_distributions_ms(B.ctypes.data, w, h, tables.ctypes.data) for _ in range(runs + 1)][1:]
                assert np.array_equal(np.nan_to_num(tables).view(np.uint32), np.nan_to_num(r.read_distributions()).view(np.uint32)), "the device's tables are not the host's"
                sc.images[0] = B
                sc.distributions = tables
                sc.environment_tables = "host"
                uploads = []
                for k in range(runs + 1):
                    t0 = time.perf_counter()
                    r.update(sc)
                    if k:
                        uploads.append((time.perf_counter() - t0) * 1e3)
                entry["parent"] = {"host_build_distributions_ms": median(build), "scene_upload_ms": median(uploads), "sum_ms": round(median(build) + median(uploads), 4)}
                entry["pixel_call_faster_than_host_table_build"] = bool(entry["forms"]["host_pixels"]["call_ms"] < entry["parent"]["host_build_distributions_ms"])
                print(w, h, "parent", entry["parent"], flush=True)
            del dev
            torch.cuda.empty_cache()
    finally:
        r.close()
    write()


if __name__ == "__main__":
    main()
