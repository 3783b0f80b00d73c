"""Randomised differential test (GPU box): random scenes x supported flag combinations x limits x frame sizes, the HIP
path against the oracle, bit for bit. usage: tools/fuzz_parity.py [cases] [seed]. Prints every mismatch and exits non-zero."""
import os, sys, time
os.environ.setdefault("STHIP_STRICT_FLAGS", "1")  # a misspelt --bdptFlag name is an error in a tool that measures (the mirror ignores it, as upstream does)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from oracle import oracle_py
from stratum_amd import camera, scenes
from stratum_amd._lib import StratumHipError
from stratum_amd.bdpt import BDPT

FOG = np.load(os.path.join(ROOT, "tests", "golden", "fog_sphere.npz"))["grid"]
# STHIP_FUZZ_SET="name=value,name=": execution options forced on / dropped from every case.
# STHIP_FUZZ_ONLY=a[-b]: only these cases of the run touch the GPU (the others still draw their random numbers, so a case is the
# one the full run has at that number); STHIP_FUZZ_TRACE=1 prints every case before it runs (to find the one a fault belongs to)
ONLY = os.environ.get("STHIP_FUZZ_ONLY")
TRACE = os.environ.get("STHIP_FUZZ_TRACE") == "1"
# STHIP_FUZZ_HALF=1: every case is rendered once more with half colour precision and compared with RTNE of its binary32 frame
# (draws no random numbers: the cases of a seed stay the same)
HALF = os.environ.get("STHIP_FUZZ_HALF") == "1"


class _Dry:
    """Stands in for the renderer in the cases STHIP_FUZZ_ONLY leaves out."""

    def __init__(self, device=0, args=None):
        from stratum_amd import wire

        self.mPushConstants = wire.default_push_constants(0, 0, 0)
        self.mSamplingFlags = 0

    def set_option(self, *a): pass
    def set_shard(self, *a): pass
    def update(self, sc): pass
    def update_transforms(self, sc): pass
    def push_constants(self, fr): return self.mPushConstants
    def close(self): pass


def compare_frames(got, ref, W, H, shard_r=0, shard_n=1, connects=False, debug_mode=0, debug_start=None):
    """One frame of the HIP path against the oracle's, bit for bit: radiance, albedo, prev-uv, the visibility ids and packed
    normals, the three depth fields, the ray counts and, with a debug mode, the debug image. On a shard (16 x 8 tiles): its
    own pixels against the frame's, zeros elsewhere (the debug image: as it was), the ray counts the shard's own; `ref` is
    overwritten there with what cannot be compared. `connects`: eConnectToViews / eConnectToLightPaths is on (every shard
    traces all light paths). Shared by fuzz_parity.py and fuzz_sequences.py."""
    ok = True
    if shard_n > 1:  # a shard renders its own tiles and writes zeros elsewhere; ray counts are the shard's own
        from stratum_amd import shard as shard_mod

        own = shard_mod.owner_map(W, H, shard_n, 16, 8) == shard_r
        ok &= np.array_equal(got["radiance"].view(np.uint32)[own], ref["radiance"].view(np.uint32)[own]) and not got["radiance"][~own].any()
        if connects:
            ref["ray_count"] = got["ray_count"]  # every shard traces all light paths
        else:
            ref["ray_count"] = got["ray_count"] if own.sum() < W * H else ref["ray_count"]
        for k in ("albedo", "prev_uv"):
            ref[k] = got[k]
        for k in ("visibility", "depth"):
            ref[k] = got[k]
        ref["radiance"] = got["radiance"]
        if debug_mode:  # (a shard leaves the pixels of the others as they were; light tracing's splats land on its own pixels only)
            ok &= np.array_equal(got["debug"].view(np.uint32)[own], ref["debug"].view(np.uint32)[own]) and np.array_equal(got["debug"][~own], debug_start[~own])
            ref["debug"] = got["debug"]
    if debug_mode: ok &= np.array_equal(got["debug"].view(np.uint32), ref["debug"].view(np.uint32))
    for k in ("radiance", "albedo", "prev_uv"):
        ok &= np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32))
    ok &= np.array_equal(got["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
    ok &= np.array_equal(got["visibility"]["packed_normal"], ref["visibility"]["packed_normal"])
    for f in ("z", "prev_z", "dz_dxy"):
        ok &= np.array_equal(got["depth"][f].view(np.uint32), ref["depth"][f].view(np.uint32))
    ok &= np.array_equal(got["ray_count"], ref["ray_count"])
    return bool(ok)


def canon16(a):
    """A float16 array with every NaN as the one quiet NaN 0x7E00 (a copy): NaN payloads are not part of the contract."""
    a = np.array(a, dtype=np.float16, copy=True)
    a.view(np.uint16)[np.isnan(a)] = 0x7E00
    return a


def half_of(a32):
    """What half colour precision makes of a binary32 image: every value rounded to nearest even, NaN where it is NaN."""
    with np.errstate(over="ignore"):
        return canon16(np.asarray(a32, np.float32).astype(np.float16))


def same_half(got16, want32):
    """A float16 image against the RTNE of a binary32 one, bit for bit. The one statement of the rule, for both tools."""
    return got16.dtype == np.float16 and np.array_equal(canon16(got16).view(np.uint16), half_of(want32).view(np.uint16))


def compare_half(gh, got, debug=False):
    """A frame rendered with half colour precision against its binary32 frame `got`: radiance / albedo (and the debug image) =
    RTNE of the binary32 ones, NaN where they are NaN; the rest identical. Returns the names that differ."""
    wrong = [k for k in ("radiance", "albedo") + (("debug",) if debug else ()) if not same_half(gh[k], got[k])]
    for k in ("prev_uv", "visibility", "depth", "ray_count"):
        if not np.array_equal(gh[k].view(np.uint8), got[k].view(np.uint8)):
            wrong.append(k)
    return wrong


def run(cases=60, seed=1):
    rng = np.random.default_rng(seed)
    fog_params = {}

    def scene(kind):
        if kind == "cornell": return scenes.cornell_box()
        if kind == "fog":
            nonlocal fog_params
            fog_params = dict(anisotropy=float(rng.choice([0.0, 0.5, -0.4])), density=tuple(float(x) for x in rng.uniform(1, 8, 3)))
            if rng.integers(2):  # a moved / rotated / stretched cloud (the scatter position stays in the grid's world space upstream)
                from stratum_amd.scene import rotate_y, scale, translate

                fog_params["fog_transform"] = translate(tuple(rng.uniform(-0.3, 0.3, 3))) @ rotate_y(float(rng.uniform(-1, 1))) @ scale(tuple(rng.uniform(0.6, 1.3, 3)))
            return scenes.cornell_box(fog=FOG, **fog_params)
        if kind == "textured": return scenes.textured_box()
        if kind == "spheres": return scenes.spheres_room()
        if kind == "env": return scenes.environment_scene(image=bool(rng.integers(2)), emitter=bool(rng.integers(2)))
        if kind == "foliage": return scenes.foliage()
        if kind == "atrium": return scenes.atrium(target_tris=int(rng.integers(5000, 40000)))
        if kind == "forest": return scenes.forest(n_instances=int(rng.integers(5, 60)), tree_tris=int(rng.integers(200, 1500)), tree_kinds=int(rng.integers(1, 4)))
        raise KeyError(kind)

    FLAGS = ["~nee", "~mis", "~samplebsdfs", "~defershadowrays", "~raycones", "~normalmaps", "~remapthreads", "alphatest", "fliptriangleuvs", "flipnormalmaps",
             "shadingnormalshadowfix", "uniformspheresampling", "presamplelights", "neereservoirs", "connecttoviews", "connecttolightpaths", "sampleenvironmentmapdirectly",
             "coherentsampling"]
    bad = rejected = done = 0
    t0 = time.time()
    for case in range(cases):
        kind = str(rng.choice(["cornell", "fog", "fog", "textured", "spheres", "env", "foliage", "atrium", "forest"]))
        flags = [str(f) for f in rng.choice(FLAGS, size=int(rng.integers(0, 5)), replace=False)]
        args = {"bdptFlag": flags, "maxDiffuseVertices": int(rng.integers(1, 5)), "maxPathVertices": int(rng.integers(2, 9)), "minPathVertices": int(rng.integers(2, 6))}
        W, H = int(rng.integers(3, 20)) * 8, int(rng.integers(3, 16)) * 4
        if rng.integers(3) == 0: W, H = W + int(rng.integers(1, 8)), H + int(rng.integers(1, 4))
        # the estimators with a defined order: light vertex cache, the two hash grids, coherent roulette
        bundle = int(rng.integers(8))
        if bundle == 0:
            flags += ["connecttolightpaths", "lightvertexcache"] + (["lvcreservoirs"] if rng.integers(2) else []) + (["lvcreservoirs", "lvcreservoirreuse"] if rng.integers(3) == 0 else [])
            args.update(maxDiffuseVertices=int(rng.integers(2, 5)), lightPathCount=int(rng.integers(max(1, W * H // 4), W * H + 1)), reservoirM=int(rng.integers(1, 5)))
        elif bundle == 1:
            flags += ["neereservoirs", "neereservoirreuse"]
            args.update(reservoirM=int(rng.integers(1, 5)), reservoirSpatialM=int(rng.integers(1, 4)), hashGridBucketCount=int(rng.choice([64, 1000, 100000])))
        elif bundle == 3:  # coherent sampling where it has something to do: presampled lights and / or the light vertex cache
            flags += ["coherentsampling"] + (["presamplelights"] if rng.integers(3) else []) + (["neereservoirs"] if rng.integers(2) else [])
            if rng.integers(2):
                flags += ["connecttolightpaths", "lightvertexcache"] + (["lvcreservoirs"] if rng.integers(2) else [])
                args.update(maxDiffuseVertices=int(rng.integers(2, 5)), lightPathCount=int(rng.integers(max(1, W * H // 4), W * H + 1)))
            args.update(reservoirM=int(rng.integers(1, 5)), lightPresampleTileSize=int(rng.choice([16, 64, 100])), lightPresampleTileCount=int(rng.choice([1, 4, 16])))
        elif bundle == 2:
            flags += ["coherentrr"]
            args.update(minPathVertices=int(rng.integers(2, 4)), maxPathVertices=int(rng.integers(4, 9)))
        flags[:] = list(dict.fromkeys(f for f in flags if not (bundle in (0, 1, 3) and f in ("~nee", "~remapthreads"))))
        reuse = any(f.endswith("reuse") for f in flags)
        seeds, seed0 = int(rng.integers(1, 4)), int(rng.integers(0, 1000))
        sc, cam = scene(kind)
        if rng.integers(4) == 0:  # objects that moved since the previous frame (gInstanceMotionTransforms feeds prev-uv / prev_z)
            m = sc.motion_transforms["m"]
            m += rng.normal(scale=0.02, size=m.shape).astype(np.float32)
        for kv in filter(None, os.environ.get("STHIP_FUZZ_ARGS", "").split(",")):  # "maxPathVertices=3,...": renderer arguments forced (narrowing a case down)
            k, _, v = kv.partition("=")
            args[k] = int(v)
        selected = True
        if ONLY:
            lo, _, hi = ONLY.partition("-")
            selected = int(lo) <= case <= int(hi or lo)
        r = BDPT(0, args=args) if selected else _Dry()
        try:
            # execution options that must not change any result: how many seeds share a pass, the fused / split trace launches,
            # the first-bounce packets, the GPU LBVH builder (triangle soups without alpha masks only), pixel-tile sharding
            opts = {}
            if rng.integers(3) == 0: opts["max_paths_in_flight"] = int(rng.integers(1, 4)) * W * H
            if rng.integers(4) == 0: opts["fuse_trace"] = 0
            if rng.integers(4) == 0: opts["packet_primary"] = 0
            if rng.integers(4) == 0 and kind in ("cornell", "textured", "atrium", "forest", "foliage"): opts["bvh_builder"] = 1  # (alpha-masked scenes too: the uvs of the alpha test are filled on the device)
            if rng.integers(4) == 0: opts["treetop"] = 1  # the LDS treetop (off by default)
            if "bvh_builder" in opts:
                opts["lbvh_algorithm"] = int(rng.integers(2))
                opts["sah_top"] = int(rng.choice([0, 16, 64, 300]))  # the host-built SAH top over the GPU builder's subtrees
            if rng.integers(4) == 0: opts["lds_stack_levels"] = int(rng.integers(4, 14))  # bounded LDS stacks + k_trace_deep
            if rng.integers(4) == 0 and "bvh_builder" not in opts: opts["embed_leaves"] = 1  # leaf triangles inside the node array
            opts["cull_terminal"] = seed0 & 1  # k_cull_terminal in front of k_shade (without drawing: the cases of a seed stay the same)
            opts["answer_last_rays"] = (seed0 >> 1) & 1  # last rays answered from the emitters' bounds
            if os.environ.get("STHIP_FUZZ_WIDE") is not None: opts["wide_bvh"] = int(os.environ["STHIP_FUZZ_WIDE"])  # the 4-wide walk forced on / off (without drawing: the cases of a seed stay the same)
            elif (seed0 >> 2) & 1: opts["wide_bvh"] = 3  # the 8-wide compressed walk (host-built trees; the others fall back to the 4-wide one)
            if (seed0 >> 3) & 1: opts["tri_min_lanes"] = 1 + (seed0 >> 5) % 24
            if (seed0 >> 6) & 1: opts["leaf_pairs"] = 0  # leaves from the per-triangle array instead of their records (without drawing: the cases of a seed stay the same)
            for kv in filter(None, os.environ.get("STHIP_FUZZ_SET", "").split(",")):  # "name=value,name=": options forced / dropped (narrowing a case down)
                k, _, v = kv.partition("=")
                if v == "": opts.pop(k, None)
                else: opts[k] = int(v)
            # BDPTDebugMode in about a fifth of the cases: gDebugImage must come out of both sides bit for bit, started from noise
            dm = (seed0 >> 4) & 63
            debug_mode = dm if 0 < dm < 14 else 0
            if os.environ.get("STHIP_FUZZ_DEBUG_MODE") and selected: debug_mode = int(os.environ["STHIP_FUZZ_DEBUG_MODE"])  # (narrowing a case down: which part of the frame differs)
            for k, v in opts.items():
                r.set_option(k, v)
            shard_n = 1 if reuse else int(rng.choice([1, 1, 2, 3]))  # a hash grid is a whole-frame structure: rejected on a shard
            shard_r = int(rng.integers(shard_n))
            if shard_n > 1:
                r.set_shard(shard_r, shard_n, 16, 8)
            r.update(sc)
            if rng.integers(4) == 0:  # instances move after the upload: the transforms-only update (top level rebuilt)
                ident = np.array([np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]])
                movers = np.nonzero(~ident)[0]
                if movers.size:
                    for i in rng.choice(movers, size=min(movers.size, int(rng.integers(1, 6))), replace=False):
                        m = sc.transforms["m"][i].copy()
                        m[:, 3] += rng.uniform(-0.15, 0.15, 3).astype(np.float32)
                        sc.set_instance_transform(int(i), m)
                    r.update_transforms(sc)
            mode = int(rng.integers(5))
            if mode == 0:  # two views side by side
                fr = camera.Frame.stereo(W, H, cam["fovy"], cam["eye"], cam["target"], eye_separation=0.2)
            elif mode == 1:  # a camera that moved since the previous frame (prev-uv / prev_z outputs)
                eye = np.asarray(cam["eye"], np.float64)
                prev = camera.Frame(W, H, cam["fovy"], tuple(eye + rng.uniform(-0.1, 0.1, 3)), cam["target"])
                fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"], prev=prev)
            else:
                fr = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
            if TRACE and selected: print("CASE %d: %s %s opts %s shard %d/%d %dx%d seeds %d+%d mode %d debug %d" % (case, kind, args, opts, shard_r, shard_n, W, H, seed0, seeds, mode, debug_mode), flush=True)
            if not selected: continue
            debug_start = None
            if debug_mode:
                r.mPushConstants.gDebugViewPathLength = 1 + (seed0 >> 10) % 3
                r.mPushConstants.gDebugLightPathLength = (seed0 >> 12) & 3
                debug_start = np.random.default_rng(seed0).random((fr.height, fr.width, 4), dtype=np.float32)
            try:
                got = r.render(fr, seed0, seeds, debug_mode=debug_mode, debug_image=debug_start)
            except StratumHipError as e:
                try:
                    oracle_py.OracleScene(sc).render(fr, r.push_constants(fr), r.mSamplingFlags, seed0, seeds, debug_mode=debug_mode, debug_image=debug_start)
                except RuntimeError:
                    rejected += 1
                    if os.environ.get("STHIP_FUZZ_VERBOSE"): print("REJECTED (both): %s" % str(e).split("): ", 1)[-1][:110])
                    continue
                print("MISMATCH (GPU rejects, oracle accepts): %s %s %s: %s" % (kind, flags, args, e))
                bad += 1
                continue
            try:
                ref = oracle_py.OracleScene(sc).render(fr, r.push_constants(fr), r.mSamplingFlags, seed0, seeds, debug_mode=debug_mode, debug_image=debug_start)
            except RuntimeError as e:
                print("MISMATCH (oracle rejects, GPU accepts): %s %s %s: %s" % (kind, flags, args, e))
                bad += 1
                continue
            ref0_debug = ref["debug"].copy() if debug_mode else None
            ref0_rad = ref["radiance"].copy()
            ok = compare_frames(got, ref, W, H, shard_r, shard_n, "connecttoviews" in flags or "connecttolightpaths" in flags, debug_mode, debug_start)
            if HALF:  # the case again with half colour precision: radiance / albedo = RTNE of this binary32 frame, the rest identical
                r.set_half_color_precision(True)
                try:
                    gh = r.render(fr, seed0, seeds, debug_mode=debug_mode, debug_image=debug_start)
                finally:
                    r.set_half_color_precision(False)
                wrong = compare_half(gh, got)
                for k in wrong:
                    if k in ("radiance", "albedo"): print("MISMATCH (half %s) %s %s %s" % (k, kind, flags, args))
                ok &= not wrong
            done += 1
            if not ok:
                bad += 1
                nd = int((got["radiance"].view(np.uint32) != ref["radiance"].view(np.uint32)).any(axis=-1).sum())
                print("MISMATCH %s %s %s opts %s shard %d/%d %dx%d seeds %d+%d mode %d debug %d %s: %d radiance pixels differ, rays %s vs %s" % (kind, flags, args, opts, shard_r, shard_n, W, H, seed0, seeds, mode, debug_mode, fog_params if kind == "fog" else "", nd, got["ray_count"], ref["ray_count"]))
                if os.environ.get("STHIP_FUZZ_VERBOSE"):
                    rb = (got["radiance"].view(np.uint32) != ref0_rad.view(np.uint32)).any(axis=-1)
                    if shard_n > 1:  # (a shard: its own pixels against the frame's, the others' must be zero)
                        from stratum_amd import shard as shard_mod

                        mine = shard_mod.owner_map(W, H, shard_n, 16, 8) == shard_r
                        rb = np.where(mine, rb, got["radiance"].any(axis=-1))
                    ys, xs = np.nonzero(rb)
                    print("  radiance: %d pixels; first: %s" % (int(rb.sum()), [(int(x), int(y), got["radiance"][y, x].tolist(), ref0_rad[y, x].tolist()) for y, x in list(zip(ys, xs))[:6]]))
                if debug_mode and os.environ.get("STHIP_FUZZ_VERBOSE"):
                    dd = (got["debug"].view(np.uint32) != ref0_debug.view(np.uint32)).any(axis=-1)
                    if shard_n > 1:  # the others' pixels must be as they were
                        from stratum_amd import shard as shard_mod

                        mine = shard_mod.owner_map(W, H, shard_n, 16, 8) == shard_r
                        dd = np.where(mine, dd, (got["debug"].view(np.uint32) != debug_start.view(np.uint32)).any(axis=-1))
                    ys, xs = np.nonzero(dd)
                    print("  debug image: %d pixels differ; first: %s" % (int(dd.sum()), [(int(x), int(y), got["debug"][y, x].tolist(), ref0_debug[y, x].tolist(), debug_start[y, x].tolist()) for y, x in list(zip(ys, xs))[:4]]))
        finally:
            r.close()
    print("%d cases compared, %d rejected on both sides, %d mismatches, %.0f s" % (done, rejected, bad, time.time() - t0))
    return done, rejected, bad



def awkward_rays(rng, sc, n):
    """(rays, the style of each, the scene's bounds): axis-aligned and zero direction components, unnormalised and tiny / huge
    directions, origins on vertices and far away, tmin > 0, tmin >= tmax, finite tmax."""
    from stratum_amd import wire

    lo = np.minimum.reduce([v for v in sc.vertices["position"]]) if sc.vertices.shape[0] else np.array([-2.0, -2, -2])
    hi = np.maximum.reduce([v for v in sc.vertices["position"]]) if sc.vertices.shape[0] else np.array([2.0, 2, 2])
    rays = np.zeros(n, wire.Ray)
    o = rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (n, 3))
    d = rng.normal(size=(n, 3))
    style = rng.integers(0, 8, n)
    d[style == 1, int(rng.integers(3))] = 0.0                      # one zero component
    z = style == 2
    d[z] = 0.0
    d[z, rng.integers(0, 3, z.sum())] = rng.choice([-1.0, 1.0], z.sum())  # axis-aligned
    d[style == 3] *= 1e-6                                          # tiny, unnormalised
    d[style == 4] *= 1e5                                           # huge
    d[style == 5] = 0.0                                            # no direction at all
    o[style == 6] *= 50.0                                          # far away
    if sc.vertices.shape[0]:                                        # origins exactly on vertices
        on = style == 7
        o[on] = sc.vertices["position"][rng.integers(0, sc.vertices.shape[0], on.sum())]
    rays["origin"], rays["direction"] = o.astype(np.float32), d.astype(np.float32)
    rays["tmin"] = np.where(rng.integers(0, 4, n) == 0, rng.uniform(0, 1, n), 0).astype(np.float32)
    rays["tmax"] = np.where(rng.integers(0, 3, n) == 0, rng.uniform(0, 3, n), np.inf).astype(np.float32)
    return rays, style, lo, hi


def run_rays(cases=40, seed=1, n=20000):
    """The traversal contract on awkward rays: axis-aligned and zero direction components, unnormalised and tiny / huge
    directions, origins on surfaces and far away, tmin > 0, tmin >= tmax, finite tmax; closest hit and any hit against
    the oracle's brute force, bit for bit."""
    from stratum_amd import wire

    rng = np.random.default_rng(seed)
    bad = 0
    for case in range(cases):
        kind = str(rng.choice(["cornell", "fog", "spheres", "foliage", "forest", "textured"]))
        if kind == "fog": sc, _ = scenes.cornell_box(fog=FOG)
        elif kind == "forest": sc, _ = scenes.forest(n_instances=12, tree_tris=400, tree_kinds=2)
        elif kind == "spheres": sc, _ = scenes.spheres_room()
        elif kind == "foliage": sc, _ = scenes.foliage()
        elif kind == "textured": sc, _ = scenes.textured_box()
        else: sc, _ = scenes.cornell_box()
        rays, style, lo, hi = awkward_rays(rng, sc, n)
        alpha = bool(rng.integers(2)) and kind == "foliage"
        r = BDPT(0)
        try:
            r.update(sc)
            orc = oracle_py.OracleScene(sc)
            got = r.trace(rays, alpha_test=alpha)
            ref, _ = orc.trace(rays, brute=True, alpha_test=alpha)
            same = all(np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)) for f in ("instance_primitive_index", "t", "b1", "b2"))
            ga = r.trace(rays, any_hit=True, alpha_test=alpha)["instance_primitive_index"] != wire.MISS
            ra = orc.trace(rays, any_hit=True, brute=True, alpha_test=alpha)[0]["instance_primitive_index"] != wire.MISS
            rb = orc.trace(rays, any_hit=True, alpha_test=alpha)[0]["instance_primitive_index"] != wire.MISS
            same_any = np.array_equal(ga, ra)
            if not np.array_equal(ra, rb):
                w = np.nonzero(ra != rb)[0]
                print("  (the oracle's own BVH any-hit differs from its brute force on %d rays, styles %s, closest-hit says %s, tmin %s tmax %s)" % (w.size, style[w], ref["instance_primitive_index"][w] != wire.MISS, rays["tmin"][w], rays["tmax"][w]))
            if not (same and same_any):
                # A known hole of the CONTRACT, not of a traversal: from an origin hundreds of scene sizes away the sheared
                # vertices of a triangle collapse in single precision, edge functions come out as exact zeros, and the test
                # accepts a "hit" whose point o + t d lies nowhere near the triangle. No acceleration structure finds these, the oracle's
                # own BVH included. They are reported, and not counted, when (1) the HIP path agrees with the oracle's BVH
                # traversal and (2) every brute-force-only hit point lies outside the scene's bounds by more than its size.
                rbvh, _ = orc.trace(rays, alpha_test=alpha)
                agree_bvh = all(np.array_equal(got[f].view(np.uint32), rbvh[f].view(np.uint32)) for f in ("instance_primitive_index", "t", "b1", "b2")) and np.array_equal(ga, rb)
                w = np.nonzero((got["instance_primitive_index"] != ref["instance_primitive_index"]) | (ga != ra))[0]
                hp = rays["origin"][w].astype(np.float64) + ref["t"][w].astype(np.float64)[:, None] * rays["direction"][w].astype(np.float64)
                wlo, whi = lo - 3 * (hi - lo) - 20.0, hi + 3 * (hi - lo) + 20.0  # generous: instances are placed around the meshes
                outside = ((hp < wlo) | (hp > whi)).any(axis=1) | ~np.isfinite(hp).all(axis=1)
                if agree_bvh and outside.all():
                    print("  (%d spurious contract hit(s) from far origins, styles %s: brute force only; HIP == the oracle's BVH traversal)" % (w.size, style[w]))
                    continue
                bad += 1
                diff = np.nonzero(got["instance_primitive_index"] != ref["instance_primitive_index"])[0]
                w = np.nonzero(ga != ra)[0]
                print("RAY MISMATCH %s alpha %s: closest %s (%d differ, styles %s), any-hit %s (%d differ: styles %s gpu %s closest-hit says %s tmin %s tmax %s)" % (kind, alpha, same, diff.size, np.unique(style[diff]), same_any, w.size, style[w], ga[w], ref["instance_primitive_index"][w] != wire.MISS, rays["tmin"][w], rays["tmax"][w]))
        finally:
            r.close()
    print("%d ray batches of %d, %d mismatches" % (cases, n, bad))
    return bad


def run_post(cases=200, seed=1):
    """The step after the path (tonemap, ImageComparer metric) on hostile images: negatives, zeros, huge values, NaN and
    Inf, all eleven curves, exposure, gamma, albedo modulation; odd extents. Against the oracle, bit for bit."""
    from stratum_amd import wire
    from stratum_amd.post import ImageComparer, Tonemapper

    rng = np.random.default_rng(seed)
    r = BDPT(0)
    bad = 0
    try:
        for case in range(cases):
            W, H = int(rng.integers(1, 200)), int(rng.integers(1, 120))
            def image():
                img = (rng.normal(size=(H, W, 4)) * 10.0 ** rng.uniform(-3, 4)).astype(np.float32)
                kind = rng.integers(0, 5)
                if kind == 0: img = np.abs(img)
                if kind == 1: img[rng.random((H, W)) < 0.05] = np.nan
                if kind == 2: img[rng.random((H, W)) < 0.05] = np.inf
                if kind == 3: img[rng.random((H, W)) < 0.3] = 0
                return img
            a, b, alb = image(), image(), np.abs(image())
            mode = str(rng.choice(wire.TONEMAP_MODES))
            mod = bool(rng.integers(2))
            tm = Tonemapper(r, mode, float(rng.uniform(-4, 4)), bool(rng.integers(2)))
            got, gmax = tm(a, alb if mod else None, mod, return_max=True)
            ref, rmax = oracle_py.tonemap(a, alb if mod else None, wire.TONEMAP[mode], mod, tm.gamma_correction, tm.exposure)
            ok = np.array_equal(got.view(np.uint32), ref.view(np.uint32)) and np.array_equal(gmax.view(np.uint32), np.asarray(rmax, np.float32).view(np.uint32))
            metric = str(rng.choice(wire.COMPARE_MODES))
            q = int(rng.choice([1, 64, 1024, 65536]))
            ok2 = ImageComparer(r, metric, q).raw(a, b) == oracle_py.image_compare(a, b, wire.COMPARE[metric], q)
            if not (ok and ok2):
                bad += 1
                print("POST MISMATCH %dx%d tonemap %s (mod %s gamma %s exp %.2f): %s; compare %s q %d: %s" % (W, H, mode, mod, tm.gamma_correction, tm.exposure, ok, metric, q, ok2))
    finally:
        r.close()
    print("%d post cases, %d mismatches" % (cases, bad))
    return bad


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "post":
        sys.exit(1 if run_post(int(sys.argv[2]) if len(sys.argv) > 2 else 200, int(sys.argv[3]) if len(sys.argv) > 3 else 1) else 0)
    if len(sys.argv) > 1 and sys.argv[1] == "rays":
        sys.exit(1 if run_rays(int(sys.argv[2]) if len(sys.argv) > 2 else 40, int(sys.argv[3]) if len(sys.argv) > 3 else 1) else 0)
    d, rj, b = run(int(sys.argv[1]) if len(sys.argv) > 1 else 60, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    sys.exit(1 if b else 0)
