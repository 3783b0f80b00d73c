"""Randomised differential test of ONE LIVING CONTEXT (GPU box): a seeded walk of scene uploads, transforms / vertex updates,
rigs, option / flag / frame / shard / precision changes, sync and async renders, ray batches, post calls and refused calls, all
on one BDPT(0), every render compared with the oracle on a logical model of what the context should now hold, bit for bit.
usage: tools/fuzz_sequences.py [walks] [seed] [steps] [--upto N] [--drop i,j,...] [--dry]. Prints every mismatch, exits non-zero.

A walk is planned first (plan(): every random number of it, drawn from the seed alone), then run. Running draws nothing, so a
seed names the same sequence with or without a GPU, and with any steps left out. The model is host-side numpy: the scene as
handed to the library (instance transforms and vertices as last sent), the rigs with their rest poses (the records resident
at set_rigs, include/sthip.h), flags and renderer arguments, the frame, the shard, colour precision and the async frames in
flight (each with the oracle's frame of the model as it was at the submit). Execution options are NOT in the model: that
they change no output is what is under test.

Two limits keep the oracle a valid reference. The oracle knows float images only: 8-bit images are mip-exact ones or alpha
masks (level 0 only), so their float form gives the same frame. "reuse_grids_persist" stays 0: it changes what a call means
(the grids of one call feed the next) and tests/test_refit.py / test_gpu_parity.py cover it on its own.

STHIP_SEQ_TRACE=1 prints and flushes each step before it runs (after a GPU fault the last line names the step; the walk is
not run on the GPU again until the cause has been found from the code). --upto N runs only steps < N, --drop leaves steps out."""
import copy
import os
import sys
import time

os.environ.setdefault("STHIP_STRICT_FLAGS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
from oracle import oracle_py
from stratum_amd import camera, scenes, wire
from stratum_amd._lib import StratumHipError
from stratum_amd.bdpt import BDPT
from stratum_amd.scene import rotate_y, translate

import fuzz_parity
from test_animate import make_rig, posed
from test_image_formats import decode, small_foliage, small_textured
from test_refit import deformed, mesh_range

FOG = fuzz_parity.FOG
THREADS = min(16, os.cpu_count() or 1)
KINDS = ("upload", "option_now", "option_later", "transforms", "vertices", "rigs", "flags", "frame", "shard", "precision", "render", "async", "trace", "post", "refused")
SCENE_CALLS = ("upload", "transforms", "vertices", "animate")
WEIGHTS = {"upload": 2.0, "option_now": 2.4, "option_later": 2.4, "transforms": 3.2, "vertices": 3.2, "rigs": 6.0, "flags": 2.6, "frame": 5.6, "shard": 2.0, "precision": 2.2,
           "render": 9.5, "async": 4.5, "trace": 2.0, "post": 2.0, "refused": 2.2}
SCENE_KINDS = ("cornell", "spheres", "foliage", "foliage8", "textured", "textured8", "texturedf", "forest", "fog", "env", "cards8")
FLAGS = ["~nee", "~mis", "~samplebsdfs", "~defershadowrays", "~raycones", "~normalmaps", "~remapthreads", "alphatest", "fliptriangleuvs", "flipnormalmaps",
         "shadingnormalshadowfix", "uniformspheresampling", "presamplelights", "neereservoirs", "connecttoviews", "connecttolightpaths", "sampleenvironmentmapdirectly",
         "coherentsampling"]
OPTIONS_NOW = ("fuse_trace", "packet_primary", "answer_last_rays", "cull_terminal", "reuse_first_hits", "tri_min_lanes", "lds_materials", "max_paths_in_flight", "output_ring")
REFUSED_FORMS = ("upload", "render", "update_vertices", "animate", "set_rigs")
GPU_BUILDER_SCENES = ("cornell", "textured", "textured8", "texturedf", "forest", "foliage", "foliage8", "cards8")  # (as fuzz_parity.py: triangle soups)


# ---------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------
def clone(sc):
    """A scene of its own: the arrays a walk changes are copied (the bases are shared), the rest is shared."""
    c = copy.copy(sc)
    for a in ("vertices", "transforms", "inverse_transforms", "motion_transforms"):
        setattr(c, a, getattr(sc, a).copy())
    for a in ("_image_descs", "_image1_descs", "_volume_descs"):
        c.__dict__.pop(a, None)
    c.dirty_vertices = None
    return c


_BASES = {}


def cards8():
    """Fewer and smaller images than the textured box: a floor under an 8 x 8 and a light under a 4 x 4 mip-exact RGBA8 image,
    an alpha-masked card under a 5 x 7 R8 mask (tests/test_image_formats.py: card_scene, with images the oracle can stand in for)."""
    from stratum_amd.scene import SceneBuilder
    from test_image_formats import mask_bytes, mip_exact_image

    b = SceneBuilder("cards8")
    colour, glow = b.add_image(mip_exact_image(8, 31)), b.add_image(mip_exact_image(4, 32))
    floor = b.add_material((1.0, 1.0, 1.0), roughness=0.4)
    b.set_material_images(floor, base_color_image=colour)
    leaf = b.add_material((0.2, 0.6, 0.1), roughness=0.6)
    b.set_material_alpha_mask(leaf, b.add_image1(mask_bytes(5, 7, 93)))
    light = b.add_emitter((17.0, 12.0, 4.0))
    b.set_material_images(light, base_color_image=glow)

    def quad(p0, p1, p2, p3, n, mat, transform=None):
        pos, nrm, uv, tri = scenes._quad(p0, p1, p2, p3, n)
        b.add_instance(b.add_mesh(pos, nrm, uv * 2.0, tri), mat, transform)

    quad((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1), (0, 1, 0), floor)
    quad((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (0, 0, 1), floor)
    quad((-0.5, 0, 0.5), (0.5, 0, 0.5), (0.5, 0, -0.5), (-0.5, 0, -0.5), (0, 1, 0), leaf, translate((0.0, -0.3, 0.0)))
    quad((-0.3, 0.9, -0.3), (0.3, 0.9, -0.3), (0.3, 0.9, 0.3), (-0.3, 0.9, 0.3), (0, -1, 0), light)
    return b.build(), {"eye": (0.0, 0.2, 3.5), "target": (0.0, -0.2, 0.0), "fovy": np.radians(40.0)}


def make_scene(kind, p):
    """(scene, camera) of a kind; `p`: the upload step's drawn parameters."""
    key = kind if kind not in ("fog", "env", "foliage8") else None
    if key is not None and key in _BASES:
        sc, cam = _BASES[key]
        return clone(sc), cam
    if kind == "cornell": made = scenes.cornell_box()
    elif kind == "spheres": made = scenes.spheres_room()
    elif kind == "foliage": made = scenes.foliage()
    elif kind == "foliage8": made = small_foliage(True, p["mask_size"])  # R8 alpha masks: the alpha test reads level 0 only
    elif kind == "textured": made = scenes.textured_box()
    elif kind == "textured8": made = small_textured(False, "exact")  # five 16 x 16 mip-exact RGBA8 images
    elif kind == "texturedf": made = small_textured(False, "exact-float")
    elif kind == "forest": made = scenes.forest(n_instances=30, tree_tris=600, tree_kinds=2)
    elif kind == "fog": made = scenes.cornell_box(fog=FOG, anisotropy=p["fog_anisotropy"], density=p["fog_density"])
    elif kind == "cards8": made = cards8()
    elif kind == "env": made = scenes.environment_scene(image=p["env_image"], emitter=p["env_emitter"])
    else: raise KeyError(kind)
    if key is not None:
        _BASES[key] = made
    return clone(made[0]), made[1]


def float_form(sc):
    """The scene the oracle renders: 8-bit images as the float images bytes / 255 (equal frames: see the module docstring)."""
    if not any(im.dtype == np.uint8 for im in list(sc.images) + list(sc.images1)):
        return sc
    c = copy.copy(sc)
    for a in ("_image_descs", "_image1_descs", "_volume_descs"):
        c.__dict__.pop(a, None)
    c.images = [decode(im) if im.dtype == np.uint8 else im for im in sc.images]
    c.images1 = [decode(im) if im.dtype == np.uint8 else im for im in sc.images1]
    return c


def triangle_instances(sc):
    return np.nonzero((sc.instances["packed"][:, 0] & 0xF) == 0)[0]


# ---------------------------------------------------------------------------------------------------------------------------
# the plan: every random number of a walk
# ---------------------------------------------------------------------------------------------------------------------------
def _bundle_args(rng, W, H, media, env, sharded):
    """Flags and renderer arguments in fuzz_parity.py's way: a few free flags and one of the estimator bundles, steered away
    from what both sides reject (reuse on a shard, coherent sampling with media; with an environment: presampled lights, NEE
    reuse and light paths; eConnectToLightPaths without eRemapThreads at a width that is no multiple of 8)."""
    flags = [str(f) for f in rng.choice(FLAGS, size=int(rng.integers(0, 4)), replace=False)]
    args = {"maxDiffuseVertices": int(rng.integers(1, 5)), "maxPathVertices": int(rng.integers(2, 9)), "minPathVertices": int(rng.integers(2, 6))}
    bundle = int(rng.integers(5))
    d = {k: int(v) for k, v in zip("abcdefgh", rng.integers(0, 1 << 30, 8))}  # (drawn whatever the bundle)
    name = "none"
    if bundle == 0 and not env:
        name = "lvc"
        flags += ["connecttolightpaths", "lightvertexcache"] + (["lvcreservoirs"] if d["a"] % 2 else []) + (["lvcreservoirs", "lvcreservoirreuse"] if d["b"] % 3 == 0 and not sharded else [])
        args.update(maxDiffuseVertices=2 + d["c"] % 3, lightPathCount=max(1, W * H // 4) + d["d"] % max(1, W * H - W * H // 4), reservoirM=1 + d["e"] % 4,
                    hashGridBucketCount=(64, 1000, 100000)[d["f"] % 3])
    elif bundle == 1 and not env and not sharded:
        name = "nee-reuse"
        flags += ["neereservoirs", "neereservoirreuse"]
        args.update(reservoirM=1 + d["a"] % 4, reservoirSpatialM=1 + d["b"] % 3, hashGridBucketCount=(64, 1000, 100000)[d["c"] % 3])
    elif bundle == 3 and not media and not env:
        name = "coherent"
        flags += ["coherentsampling"] + (["presamplelights"] if d["a"] % 3 and not env else []) + (["neereservoirs"] if d["b"] % 2 else [])
        if d["c"] % 2:
            flags += ["connecttolightpaths", "lightvertexcache"] + (["lvcreservoirs"] if d["d"] % 2 else [])
            args.update(maxDiffuseVertices=2 + d["e"] % 3, lightPathCount=max(1, W * H // 4) + d["f"] % max(1, W * H - W * H // 4))
        args.update(reservoirM=1 + d["g"] % 4, lightPresampleTileSize=(16, 64, 100)[d["h"] % 3], lightPresampleTileCount=(1, 4, 16)[(d["h"] >> 8) % 3])
    elif bundle == 2:
        name = "coherent-rr"
        flags += ["coherentrr"]
        args.update(minPathVertices=2 + d["a"] % 2, maxPathVertices=4 + d["b"] % 5)
    drop = set()
    if name in ("lvc", "nee-reuse", "coherent"): drop |= {"~nee", "~remapthreads"}
    if env: drop |= {"presamplelights", "connecttoviews", "connecttolightpaths"}
    if "connecttolightpaths" in flags: drop |= {"~remapthreads"}
    if media: drop |= {"coherentsampling"}
    flags = list(dict.fromkeys(f for f in flags if f not in drop))
    args["bdptFlag"] = flags
    return name, args


def _frame_size(rng, how, W, H):
    if how == "shrink": W, H = max(8, W // int(rng.integers(2, 7))), max(8, H // int(rng.integers(2, 6)))
    elif how == "grow": W, H = min(144, W * int(rng.integers(2, 5))), min(80, H * int(rng.integers(2, 4)))
    else: W, H = int(rng.integers(1, 19)) * 8, int(rng.integers(2, 21)) * 4
    W, H = 8 * (W // 8), 4 * (H // 4)
    if rng.integers(3) == 0: W, H = min(151, W + int(rng.integers(1, 8))), min(83, H + int(rng.integers(1, 4)))
    return max(8, W), max(8, H)


def plan(seed, steps=40):
    """The steps of walk `seed`: a list of dicts with "kind" and every parameter the step needs, as fractions and choices that
    fit any state (a step left out by --drop does not unsettle the ones after it). The state kept here is only what steers the
    choice of the next step."""
    rng = np.random.default_rng(seed)
    out = []
    st = dict(kind=None, media=False, env=False, W=48, H=32, stereo=False, bundle="none", reuse=False, shard=1, shard_r=0, half=False, inflight=0, fresh=0, ring=2, rigs=0, kept=True,
              builder=0, prev=None, forced=None)

    # the forms of a kind go round, and each walk starts where the one before it has got to after a step or two: a few walks with
    # consecutive seeds meet every scene, every option that acts at once and every refusal
    scene_order, option_order, refused_order = SCENE_KINDS, OPTIONS_NOW, REFUSED_FORMS
    turn = dict(scene=2 * seed, option=3 * seed, refused=2 * seed)

    def take(order, key, n=1):
        got = [order[(turn[key] + k) % len(order)] for k in range(n)]
        turn[key] += n
        return got

    def upload():
        kind = take(scene_order, "scene")[0]
        p = dict(kind="upload", scene=kind, mask_size=(int(rng.integers(3, 20)), int(rng.integers(3, 20))), fog_anisotropy=float(rng.choice([0.0, 0.5, -0.4])),
                 fog_density=tuple(float(x) for x in rng.uniform(1, 8, 3)), env_image=bool(rng.integers(2)), env_emitter=bool(rng.integers(2)), motion=int(rng.integers(4)) == 0,
                 motion_seed=int(rng.integers(1 << 30)))
        o = {"bvh_builder": int(rng.integers(3) == 0 and kind in GPU_BUILDER_SCENES), "lbvh_algorithm": int(rng.integers(2)), "sah_top": int(rng.choice([0, 16, 64, 300])),
             "wide_bvh": int(rng.choice([0, 1, 1, 3])), "embed_leaves": int(rng.integers(4) == 0), "treetop": int(rng.integers(4) == 0),
             "lds_stack_levels": int(rng.integers(4, 14)) if rng.integers(3) == 0 else None, "keep_scene": int(rng.integers(8) != 0)}
        if o["bvh_builder"]: o["embed_leaves"] = 0
        if not o["keep_scene"]:  # without a kept scene to build from again, only layouts the refit serves (the others refuse update_vertices / animate as unsupported)
            o.update(embed_leaves=0, treetop=0, wide_bvh=o["wide_bvh"] % 3)
        if o["lds_stack_levels"] is None: del o["lds_stack_levels"]  # (stays as an earlier step left it)
        p["options"] = o
        media, env = kind == "fog", kind == "env"
        name, args = _bundle_args(rng, st["W"], st["H"], media, env, st["shard"] > 1)  # drawn always; applied only when the flags in force do not suit the new scene
        clash = (media and st["bundle"] == "coherent") or env or st["kind"] is None
        p["args"] = args if clash else None
        if clash: st.update(bundle=name, reuse=any(f.endswith("reuse") for f in args["bdptFlag"]))
        st.update(kind=kind, media=media, env=env, rigs=0, kept=bool(o["keep_scene"]), builder=o["bvh_builder"], fresh=0)
        return p

    def render(kind="render"):
        seed0 = int(rng.integers(0, 1000))
        mode = int(rng.integers(1, 14))
        debug = mode if int(rng.integers(3)) == 0 and kind == "render" and not st["half"] else 0  # (one in three of the binary32 renders, about one in five of all: gDebugImage is in / out and would start from rounded noise with half precision)
        return dict(kind=kind, seed0=seed0, seeds=int(rng.integers(1, 4)), debug_mode=debug, view_len=1 + (seed0 >> 10) % 3, light_len=(seed0 >> 12) & 3, own_buffers=bool(rng.integers(2)))

    # every kind is drawn in every walk: the agenda holds each once (the ones with several forms more often) among as many free
    # draws, in a random order; past its end the draws are free
    weights = np.array([WEIGHTS[k] for k in KINDS]) / sum(WEIGHTS.values())
    agenda = list(KINDS) + ["rigs", "rigs", "frame", "frame", "shard", "render", "render"]
    agenda = [str(k) for k in rng.permutation(agenda + [str(k) for k in rng.choice(KINDS, size=max(0, (6 * steps) // 10 - len(agenda)), p=weights)])]
    out.append(upload())
    while len(out) < steps:
        if st["forced"]:
            kind, st["forced"] = st["forced"], None
        elif st["prev"] in SCENE_CALLS + ("frame", "shard") and rng.random() < 0.65:  # what a call changed is rendered before the next change, more often than not
            kind = "render"
        else:
            free = str(rng.choice(KINDS, p=weights))  # (drawn whether or not the agenda still holds something)
            kind = agenda.pop(0) if agenda else free
        u = rng.random(8)  # (the sub-choices of the step: drawn whatever the kind)
        scene_call = kind in ("upload", "transforms", "vertices") or (kind == "rigs" and st["rigs"] and u[0] < 0.8)
        if scene_call and st["fresh"] == 0 and st["inflight"] < 3 and u[1] < 0.75 and len(out) + 2 < steps:  # frames in flight across the scene call
            out.append(dict(render("async"), sub="submit"))
            if u[2] < 0.6: out.append(dict(render("async"), sub="submit"))
            st["fresh"] = 2 if u[2] < 0.6 else 1
            st["inflight"] += st["fresh"]
            st["forced"], st["prev"] = kind, "async"
            continue
        sub = kind
        if kind == "upload":
            p = upload()
        elif kind == "option_now":
            settings = []
            for name in take(option_order, "option", 3):  # three of them a step
                value = int(rng.integers(2))
                if name == "tri_min_lanes": value = int(rng.integers(1, 25))
                if name == "max_paths_in_flight": value = -int(rng.integers(1, 4))  # (negative: times the paths of one seed of the frame in force)
                if name == "output_ring":
                    value = int(rng.integers(1, 4))
                    if value != st["ring"]: st["fresh"] = 0  # (a change completes the frames in flight)
                    st["ring"] = value
                settings.append((name, value))
            p = dict(kind=kind, settings=settings)
        elif kind == "option_later":
            name = str(rng.choice(["lds_stack_levels", "treetop", "embed_leaves", "wide_bvh"]))
            value = {"lds_stack_levels": int(rng.integers(4, 14)), "treetop": int(rng.integers(2)), "embed_leaves": int(rng.integers(2)) if not st["builder"] else 0, "wide_bvh": int(rng.choice([0, 1, 3]))}[name]
            if not st["kept"] and name != "lds_stack_levels": value = value % 3 if name == "wide_bvh" else 0  # (see upload)
            p = dict(kind=kind, name=name, value=value)
        elif kind == "transforms":
            p = dict(kind=kind, merged=bool(u[0] < 0.3 and st["kept"]), picks=[float(x) for x in rng.random(int(rng.integers(1, 5)))], offsets=rng.uniform(-0.15, 0.15, (4, 3)).tolist(), angle=float(rng.uniform(-0.4, 0.4)))
            st["fresh"] = 0
        elif kind == "vertices":
            p = dict(kind=kind, whole=bool(u[0] < 0.3), over_rig=bool(u[1] < 0.5), lo=float(u[2]), span=float(u[3]), amp=float(rng.uniform(0.01, 0.04)), phase=float(rng.uniform(0, 3)), freq=float(rng.uniform(2, 4)))
            st["fresh"] = 0
        elif kind == "rigs":
            if not st["rigs"] or u[0] >= 0.9:
                sub = "set_rigs"
                p = dict(kind=kind, sub=sub, picks=[float(x) for x in rng.random(2)], targets=[int(x) for x in rng.integers(0, 4, 2)], bones=[int(x) for x in rng.choice([0, 1, 3, 40], 2)], count=int(rng.integers(1, 3)), rig_seed=int(rng.integers(1000)))
                st["rigs"] = p["count"]
            elif u[0] < 0.8:
                sub = "animate"
                p = dict(kind=kind, sub=sub, scale=float(rng.uniform(0.2, 1.0)), stretch=float(rng.uniform(0.95, 1.08)))
                st["fresh"] = 0
            else:
                sub = "drop_rigs"
                p = dict(kind=kind, sub=sub)
                st["rigs"] = 0
        elif kind == "flags":
            name, args = _bundle_args(rng, st["W"], st["H"], st["media"], st["env"], st["shard"] > 1)
            p = dict(kind=kind, bundle=name, args=args)
            st.update(bundle=name, reuse=any(f.endswith("reuse") for f in args["bdptFlag"]))
        elif kind == "frame":
            how = "shrink" if u[0] < 0.5 else "grow" if u[0] < 0.8 else "any"
            W, H = _frame_size(rng, how, st["W"], st["H"])
            stereo = (not st["stereo"]) if u[1] < 0.7 else st["stereo"]
            p = dict(kind=kind, W=W, H=H, stereo=bool(stereo), moved=rng.uniform(-0.1, 0.1, 3).tolist() if u[2] < 0.3 and not stereo else None,
                     shrink=W * H < st["W"] * st["H"], mono=st["stereo"] and not stereo, bundle=st["bundle"])
            st.update(W=W, H=H, stereo=stereo)
        elif kind == "shard":
            n = 1 if st["reuse"] else int(rng.choice([1, 2, 2, 3, 3]))
            r = int(rng.integers(n))
            if st["inflight"] and len(out) + st["inflight"] < steps:  # the frames in flight are collected first: the shard changes between frames, not under them
                out.extend(dict(kind="async", sub="wait", which=0.0) for _ in range(st["inflight"]))
                st["inflight"] = st["fresh"] = 0
            if st["inflight"]: n, r = st["shard"], st["shard_r"]  # (no room left to wait: the shard stays)
            p = dict(kind=kind, n=n, r=r)
            st["shard"], st["shard_r"] = n, r
        elif kind == "precision":
            st["half"] = bool(u[0] < 0.35) if st["half"] == bool(u[1] < 0.5) else not st["half"]  # (mostly a change, more often to binary32)
            p = dict(kind=kind, half=st["half"])
        elif kind == "render":
            p = render()
        elif kind == "async":
            if st["inflight"] and (u[0] < 0.5 or st["inflight"] >= 3):
                sub = "wait"
                p = dict(kind=kind, sub=sub, which=float(u[1]))
                st["inflight"], st["fresh"] = st["inflight"] - 1, max(0, st["fresh"] - 1)  # (st["inflight"]: not collected yet; st["fresh"]: submitted since the last call that completes them)
            else:
                sub = "submit"
                p = dict(render("async"), sub=sub)
                st["inflight"], st["fresh"] = st["inflight"] + 1, st["fresh"] + 1
        elif kind == "trace":
            p = dict(kind=kind, ray_seed=int(rng.integers(1 << 30)), n=int(rng.integers(200, 500)), alpha=bool(u[0] < 0.5))
        elif kind == "post":
            p = dict(kind=kind, mode=str(rng.choice(wire.TONEMAP_MODES)), modulate=bool(u[0] < 0.5), gamma=bool(u[1] < 0.5), exposure=float(rng.uniform(-4, 4)), metric=str(rng.choice(wire.COMPARE_MODES)),
                     quantization=int(rng.choice([1, 64, 1024, 65536])), reprojection=bool(u[2] < 0.5), demodulate=bool(u[3] < 0.5), limit=float(rng.choice([0.0, 2.0])))
        else:
            p = dict(kind=kind, forms=take(refused_order, "refused", 2))  # two of them a step
        out.append(p)
        st["prev"] = sub if sub in SCENE_CALLS else kind if kind in SCENE_CALLS + ("frame", "shard") else "other"
    return out


def describe(p):
    return "%s %s" % (p["kind"], {k: v for k, v in p.items() if k != "kind"})


# ---------------------------------------------------------------------------------------------------------------------------
# the walk
# ---------------------------------------------------------------------------------------------------------------------------
class _Dry(BDPT):
    """Stands in for the renderer without a GPU: BDPT's own flags and arguments (BDPT.set_args, push_constants), no context."""

    def __init__(self, device=0, args=None):
        self._h, self.device, self._scene, self._prev_result, self.half_color_precision = None, device, None, None, False
        self.set_args(args)

    def update(self, sc): sc.dirty_vertices, self._scene = None, sc
    def update_transforms(self, sc): self._scene = sc
    def update_vertices(self, sc): sc.dirty_vertices, self._scene = None, sc
    def set_rigs(self, rigs): pass
    def animate(self, poses): pass
    def set_option(self, *a): pass
    def set_shard(self, *a): pass
    def set_half_color_precision(self, on): self.half_color_precision = bool(on)


def to_half(ref):
    """The oracle's binary32 frame as a half-colour-precision render must give it (fuzz_parity.half_of: the one statement of the rule)."""
    out = dict(ref)
    for k in ("radiance", "albedo", "debug"):
        if k in ref:
            out[k] = fuzz_parity.half_of(ref[k])
    return out


def same_color(got, want32, half):
    if not half:
        return got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want32, np.float32).view(np.uint32))
    return fuzz_parity.same_half(got, want32)


class Walk:
    """One context (or none: gpu=False runs the model and the oracle alone) and the model beside it."""

    def __init__(self, gpu=True, threads=THREADS, verbose=True):
        self.gpu, self.threads, self.verbose = gpu, threads, verbose
        self.r = BDPT(0) if gpu else _Dry()
        self.sc = self.cam = None
        self.kind = None
        self.merged = np.zeros(0, bool)  # per instance: part of the merged identity-transform mesh of the resident build
        self.kept = True
        self.rigs = []  # (rig, pose, rest pose: the records at set_rigs)
        self.W, self.H, self.stereo, self.moved = 48, 32, False, None
        self.shard = (0, 1)
        self.inflight = []  # dicts: ticket, ref (None: rejected), W, H, shard, connects, half
        self.ring = 2
        self.last = None  # the oracle's last whole frame and its Frame (the post step's input)
        self._oracle = None
        self.compared = self.rejected = self.bad = 0
        self.log = []  # (step index, kind, sub, outcome)
        self.frames = []  # per frame judged: step of its render / submit, W, H, views, bundle (an estimator bundle's buffers live), shard, half, debug, outcome
        self.crossings = []  # (step index, scene call): frames were in flight, rendering or copying, when the call came

    def close(self):
        self.r.close()

    # ---- the model's side ----
    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle_py.OracleScene(float_form(self.sc))
        return self._oracle

    def touched(self):
        if self._oracle is not None: self._oracle.close()
        self._oracle = None

    def frame(self):
        c = self.cam
        if self.stereo:
            return camera.Frame.stereo(self.W, self.H, c["fovy"], c["eye"], c["target"], eye_separation=0.2)
        prev = None
        if self.moved is not None:
            prev = camera.Frame(self.W, self.H, c["fovy"], tuple(np.asarray(c["eye"], np.float64) + np.asarray(self.moved)), c["target"])
        return camera.Frame(self.W, self.H, c["fovy"], c["eye"], c["target"], prev=prev)

    def meta(self, i, fr, debug_mode=0):
        on = lambda name: bool((self.r.mSamplingFlags >> wire.FLAG_NAMES.index(name)) & 1)
        lvc, nee = on("eLVC") and on("eConnectToLightPaths"), on("eNEE")
        bundle = lvc or (nee and on("eNEEReservoirs") and on("eNEEReservoirReuse")) or (on("eCoherentSampling") and (lvc or (nee and on("ePresampleLights"))))  # (eCoherentRR is on by default: not counted)
        return dict(step=i, W=fr.width, H=fr.height, views=int(fr.views.shape[0]), bundle=bundle, shard=self.shard, half=self.r.half_color_precision, debug=debug_mode)

    def judged(self, meta, outcome):
        self.frames.append(dict(meta, outcome=outcome))
        return outcome

    def connects(self):
        f = self.r.mSamplingFlags
        return bool((f >> wire.FLAG_NAMES.index("eConnectToViews")) & 1 or (f >> wire.FLAG_NAMES.index("eConnectToLightPaths")) & 1)

    def reference(self, fr, p, debug_start=None):
        try:
            return self.oracle().render(fr, self.r.push_constants(fr), self.r.mSamplingFlags, p["seed0"], p["seeds"], threads=self.threads, debug_mode=p.get("debug_mode", 0), debug_image=debug_start)
        except RuntimeError:
            return None

    def mismatch(self, i, text):
        self.bad += 1
        print("MISMATCH at step %d: %s" % (i, text), flush=True)

    def judge(self, i, got, ref, what, W, H, shard, connects, half, debug_mode=0, debug_start=None):
        """A frame of the context against the oracle's frame of the model."""
        if ref is None and got is None:
            self.rejected += 1
            return "rejected"
        if not self.gpu:
            self.compared += 1
            return "compared"
        if ref is None or got is None:
            self.mismatch(i, "%s: %s rejects, %s accepts" % (what, "GPU" if got is None else "oracle", "oracle" if got is None else "GPU"))
            return "bad"
        whole = ref
        if half:
            if got["radiance"].dtype != np.float16 or got["albedo"].dtype != np.float16: return self.mismatch(i, what + ": the colour images are not float16") or "bad"
            ref, got = to_half(ref), dict(got, radiance=fuzz_parity.canon16(got["radiance"]), albedo=fuzz_parity.canon16(got["albedo"]))
        else:
            ref = dict(ref)
        self.compared += 1
        if fuzz_parity.compare_frames(got, ref, W, H, shard[0], shard[1], connects, debug_mode, debug_start):
            return "compared"
        nd = int((np.ascontiguousarray(got["radiance"]).view(np.uint8) != np.ascontiguousarray(to_half(whole)["radiance"] if half else whole["radiance"]).view(np.uint8)).reshape(H, W, -1).any(axis=-1).sum())
        self.mismatch(i, "%s %dx%d shard %s half %s: %d radiance pixels differ from the whole frame's, rays %s vs %s" % (what, W, H, shard, half, nd, got["ray_count"], whole["ray_count"]))
        return "bad"

    # ---- the steps ----
    def step(self, i, p):
        kind = p["kind"]
        outcome = getattr(self, "do_" + kind)(i, p)
        if kind in ("render", "trace", "post"):  # (synchronous work on the stream: what was submitted before it has rendered by now)
            self.inflight_done()
        self.log.append((i, kind, p.get("sub", kind), outcome))

    def do_upload(self, i, p):
        r = self.r
        for k, v in p["options"].items():
            r.set_option(k, v)
        sc, cam = make_scene(p["scene"], p)
        if p["motion"]:  # objects that moved since the previous frame (gInstanceMotionTransforms feeds prev-uv / prev_z)
            m = sc.motion_transforms["m"]
            m += np.random.default_rng(p["motion_seed"]).normal(scale=0.02, size=m.shape).astype(np.float32)
        r.update(sc)
        self.sc, self.cam, self.kind, self.rigs, self.kept = sc, cam, p["scene"], [], bool(p["options"]["keep_scene"])
        self.merged = np.array([np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]])
        self.inflight_done(i, "upload")
        if p["args"] is not None:
            r.set_args(p["args"])
        self.touched()
        return "done"

    def do_option_now(self, i, p):
        for name, value in p["settings"]:
            if name == "max_paths_in_flight":
                value = -value * self.W * self.H
            if name == "output_ring":
                if value != self.ring: self.inflight_done()
                self.ring = value
            self.r.set_option(name, value)
        return "done"

    def do_option_later(self, i, p):
        self.r.set_option(p["name"], p["value"])
        return "done"

    def do_transforms(self, i, p):
        sc = self.sc
        tri = triangle_instances(sc)
        movers = [int(k) for k in tri if not self.merged[k]]
        merged = [int(k) for k in tri if self.merged[k]]
        moved = []
        if p["merged"] and merged and self.kept:  # an instance of the merged mesh: the scene is built again from the kept copy
            k = merged[int(p["picks"][0] * len(merged))]
            sc.set_instance_transform(k, translate(p["offsets"][0]) @ np.vstack([sc.transforms["m"][k].astype(np.float64), [0, 0, 0, 1]]))
            moved.append(k)
        elif movers:
            for pick, off in zip(p["picks"], p["offsets"]):
                k = movers[int(pick * len(movers))]
                if k in moved: continue
                m = np.vstack([sc.transforms["m"][k].astype(np.float64), [0, 0, 0, 1]])
                sc.set_instance_transform(k, translate(off) @ m @ rotate_y(p["angle"] if not moved else 0.0))
                moved.append(k)
        else:
            return "skipped: nothing to move"
        self.r.update_transforms(sc)
        if any(self.merged[k] for k in moved):  # the rebuild merges the instances that are at the identity now
            self.merged = np.array([np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]])
        self.inflight_done(i, "transforms")
        self.touched()
        return "done: merged" if p["merged"] and merged and self.kept else "done"

    def do_vertices(self, i, p):
        sc = self.sc
        n = sc.vertices.shape[0]
        if n == 0: return "skipped: no vertices"
        if p["over_rig"] and self.rigs:  # part of a rigged range: the rest pose must not move
            rig = self.rigs[0][0]
            first, count = rig["first_vertex"], max(1, rig["vertex_count"] // 2)
        elif p["whole"]:
            first, count = 0, n
        else:
            first = int(p["lo"] * n)
            count = max(1, int(p["span"] * (n - first)))
        sc.set_vertices(first, deformed(sc.vertices[first : first + count], p["amp"], p["freq"], p["phase"]))
        self.r.update_vertices(sc)
        self.inflight_done(i, "vertices")
        self.touched()
        return "done: over a rig" if p["over_rig"] and self.rigs else "done"

    def do_rigs(self, i, p):
        sc, r = self.sc, self.r
        if p["sub"] == "drop_rigs":
            r.set_rigs([])
            self.rigs = []
            return "done"
        if p["sub"] == "set_rigs":
            tri = triangle_instances(sc)
            made, taken = [], []
            for k in range(p["count"]):
                first, count = mesh_range(sc, int(p["instances"][k]) if "instances" in p else int(tri[int(p["picks"][k] * len(tri))]))
                if any(first < b and a < first + count for a, b in taken): continue
                taken.append((first, first + count))
                rig, pose, _ = make_rig(sc.vertices, first, count, p["targets"][k], p["bones"][k] or (0 if p["targets"][k] else 1), p["rig_seed"] + k)
                made.append((rig, pose, sc.vertices[first : first + count].copy()))
            r.set_rigs([rig for rig, _, _ in made])
            self.rigs = made
            return "done"
        if not self.rigs: return "skipped: no rigs"
        poses = []
        for rig, pose, rest in self.rigs:
            q = dict(pose, blend_factors=tuple(np.float32(f) * np.float32(p["scale"]) for f in pose["blend_factors"]))
            if "bones" in pose: q["bones"] = pose["bones"] * np.float32(p["stretch"])
            poses.append(q)
            first = rig["first_vertex"]
            sc.vertices[first : first + rig["vertex_count"]] = posed(rest, rig["blend_targets"], q["blend_factors"], rig.get("weights"), q.get("bones"))
        r.animate(poses)
        self.inflight_done(i, "animate")
        self.touched()
        return "done"

    def do_flags(self, i, p):
        self.r.set_args(p["args"])
        return "done"

    def do_frame(self, i, p):
        self.W, self.H, self.stereo, self.moved = p["W"], p["H"], p["stereo"], p["moved"]
        return "done"

    def do_shard(self, i, p):
        if self.inflight: return "skipped: frames in flight"
        self.r.set_shard(p["r"], p["n"], 16, 8)
        self.shard = (p["r"], p["n"])
        return "done"

    def do_precision(self, i, p):
        self.r.set_half_color_precision(p["half"])
        return "done"

    def do_render(self, i, p):
        r, fr = self.r, self.frame()
        half = r.half_color_precision
        debug_mode = 0 if half else p["debug_mode"]
        debug_start = None
        saved = (r.mPushConstants.gDebugViewPathLength, r.mPushConstants.gDebugLightPathLength)
        if debug_mode:
            r.mPushConstants.gDebugViewPathLength, r.mPushConstants.gDebugLightPathLength = p["view_len"], p["light_len"]
            debug_start = np.random.default_rng(p["seed0"]).random((fr.height, fr.width, 4), dtype=np.float32)
        try:
            ref = self.reference(fr, dict(p, debug_mode=debug_mode), debug_start)
            got = None
            if self.gpu:
                try:
                    got = r.render(fr, p["seed0"], p["seeds"], debug_mode=debug_mode, debug_image=debug_start)
                except StratumHipError as e:
                    if self.verbose and ref is not None: print("  GPU: %s" % e)
            elif ref is not None:
                got = ref
        finally:
            r.mPushConstants.gDebugViewPathLength, r.mPushConstants.gDebugLightPathLength = saved
        if ref is not None and self.shard[1] == 1:
            self.last = (ref, fr)
        return self.judged(self.meta(i, fr, debug_mode), self.judge(i, got, ref, "render", fr.width, fr.height, self.shard, self.connects(), half, debug_mode, debug_start))

    def do_async(self, i, p):
        r = self.r
        if p["sub"] == "submit":
            fr = self.frame()
            ref = self.reference(fr, p)
            entry = dict(ref=ref, W=fr.width, H=fr.height, shard=self.shard, connects=self.connects(), half=r.half_color_precision, ticket=None, step=i, complete=False, meta=self.meta(i, fr))
            if self.gpu:
                own = p["own_buffers"] or len(self.inflight) >= self.ring  # at most "output_ring" frames in the buffers render_async makes itself
                try:
                    entry["ticket"] = r.render_async(fr, p["seed0"], p["seeds"], host_outputs=r.alloc_host_outputs(fr) if own else None)
                except StratumHipError as e:
                    if self.verbose and ref is not None: print("  GPU: %s" % e)
            elif ref is not None:
                entry["ticket"] = -1
            if entry["ticket"] is None:  # rejected at the submit: judged now
                return self.judged(entry["meta"], self.judge(i, None, ref, "render_async", fr.width, fr.height, self.shard, entry["connects"], entry["half"]))
            if ref is None:
                return self.judged(entry["meta"], self.judge(i, {}, None, "render_async", fr.width, fr.height, self.shard, entry["connects"], entry["half"]))
            self.inflight.append(entry)
            return "submitted"
        if not self.inflight: return "skipped: nothing in flight"
        k = int(p["which"] * len(self.inflight))
        return self.collect(i, self.inflight.pop(k))

    def collect(self, i, e):
        got = self.r.wait(e["ticket"]) if self.gpu else e["ref"]
        for other in self.inflight:  # (a wait completes every earlier ticket)
            other["complete"] |= other["step"] < e["step"]
        if self.gpu and got is None:
            self.mismatch(i, "wait(%d) returned nothing" % e["ticket"])
            return "bad"
        return self.judged(e["meta"], self.judge(i, got, e["ref"], "frame submitted at step %d" % e["step"], e["W"], e["H"], e["shard"], e["connects"], e["half"]))

    def inflight_done(self, i=None, what=None):
        """A call that completes the frames in flight went by; the tickets stay to be collected."""
        if what and any(not e["complete"] for e in self.inflight):
            self.crossings.append((i, what))
        for e in self.inflight:
            e["complete"] = True

    def drain(self, i):
        while self.inflight:
            self.log.append((i, "async", "wait", self.collect(i, self.inflight.pop(0))))

    def do_trace(self, i, p):
        sc = self.sc
        rays, style, lo, hi = fuzz_parity.awkward_rays(np.random.default_rng(p["ray_seed"]), sc, p["n"])
        alpha = p["alpha"] and bool(sc.images1)
        orc = self.oracle()
        ref, _ = orc.trace(rays, brute=True, alpha_test=alpha, threads=self.threads)
        ra = orc.trace(rays, any_hit=True, brute=True, alpha_test=alpha, threads=self.threads)[0]["instance_primitive_index"] != wire.MISS
        if not self.gpu: return "traced"
        got = self.r.trace(rays, alpha_test=alpha)
        ga = self.r.trace(rays, any_hit=True, alpha_test=alpha)["instance_primitive_index"] != wire.MISS
        if all(np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)) for f in ("instance_primitive_index", "t", "b1", "b2")) and np.array_equal(ga, ra):
            return "traced"
        # the known hole of the contract (fuzz_parity.run_rays): spurious brute-force hits from far origins, reported and not counted
        # when the HIP path agrees with the oracle's own BVH traversal and every such hit point lies far outside the scene
        rbvh, _ = orc.trace(rays, alpha_test=alpha, threads=self.threads)
        rb = orc.trace(rays, any_hit=True, alpha_test=alpha, threads=self.threads)[0]["instance_primitive_index"] != wire.MISS
        agree = all(np.array_equal(got[f].view(np.uint32), rbvh[f].view(np.uint32)) for f in ("instance_primitive_index", "t", "b1", "b2")) and np.array_equal(ga, rb)
        w = np.nonzero((got["instance_primitive_index"] != ref["instance_primitive_index"]) | (ga != ra))[0]
        hp = rays["origin"][w].astype(np.float64) + ref["t"][w].astype(np.float64)[:, None] * rays["direction"][w].astype(np.float64)
        wlo, whi = lo - 3 * (hi - lo) - 20.0, hi + 3 * (hi - lo) + 20.0
        outside = ((hp < wlo) | (hp > whi)).any(axis=1) | ~np.isfinite(hp).all(axis=1)
        if agree and w.size and outside.all():
            print("  (%d spurious contract hit(s) from far origins, styles %s: brute force only; HIP == the oracle's BVH traversal)" % (w.size, style[w]))
            return "traced"
        self.mismatch(i, "trace alpha %s: %d rays differ (styles %s)" % (alpha, w.size, np.unique(style[w])))
        return "bad"

    def do_post(self, i, p):
        from stratum_amd.post import ImageComparer, TemporalAccumulation, Tonemapper

        if self.last is None: return "skipped: no frame yet"
        ref, fr = self.last
        half = self.r.half_color_precision
        cd = np.float16 if half else np.float32
        with np.errstate(over="ignore"):
            rad, alb = ref["radiance"].astype(cd), ref["albedo"].astype(cd)
            other = (ref["radiance"] * np.float32(1.25) + np.float32(0.01)).astype(cd)
        up = lambda a: a.astype(np.float32)
        want, wmax = oracle_py.tonemap(up(rad), up(alb) if p["modulate"] else None, wire.TONEMAP[p["mode"]], p["modulate"], p["gamma"], p["exposure"])
        wcmp = oracle_py.image_compare(up(rad), up(other), wire.COMPARE[p["metric"]], p["quantization"])
        hist = {"accum_color": np.zeros((fr.height, fr.width, 4), np.float32), "accum_moments": np.zeros((fr.height, fr.width, 2), np.float32), "visibility": np.zeros((fr.height, fr.width), wire.VisibilityInfo),
                "depth": np.zeros((fr.height, fr.width), wire.DepthInfo)}
        hist["visibility"]["instance_primitive_index"] = wire.MISS
        wacc = []
        for _ in range(2):  # twice: the second call blends into the history of the first
            c, m = oracle_py.accumulate(dict(ref, radiance=up(rad), albedo=up(alb)), hist, fr.views, p["reprojection"], p["demodulate"], p["limit"])
            if half:
                with np.errstate(over="ignore"):
                    c = up(c.astype(np.float16))  # (the history a half-precision context carries on from)
            wacc.append((c, m))
            hist = {"accum_color": c, "accum_moments": m, "visibility": ref["visibility"], "depth": ref["depth"]}
        if not self.gpu: return "posted"
        ok = []
        got, gmax = Tonemapper(self.r, p["mode"], p["exposure"], p["gamma"])(rad, alb if p["modulate"] else None, p["modulate"], return_max=True)
        ok.append(same_color(got, want, half) and np.array_equal(gmax.view(np.uint32), np.asarray(wmax, np.float32).view(np.uint32)))
        ok.append(ImageComparer(self.r, p["metric"], p["quantization"]).raw(rad, other) == wcmp)
        acc = TemporalAccumulation(self.r, p["reprojection"], p["demodulate"], p["limit"])
        for c, m in wacc:
            gc, gm = acc(dict(ref, radiance=rad, albedo=alb), fr.views)
            ok.append(same_color(gc, c, half) and np.array_equal(gm.view(np.uint32), m.view(np.uint32)))
        if all(ok): return "posted"
        self.mismatch(i, "post %dx%d half %s: tonemap %s (%s), compare %s (%s), accumulate %s" % (fr.width, fr.height, half, ok[0], p["mode"], ok[1], p["metric"], ok[2:]))
        return "bad"

    def do_refused(self, i, p):
        """Calls the library must refuse, in the middle of other work: each raises, and the model is unchanged (what follows shows it)."""
        if not self.gpu: return "refused"
        for what in p["forms"]:
            try:
                self.refused_call(i, what)
            except StratumHipError:
                continue
            self.mismatch(i, "a refused call was accepted: %s" % what)
            return "bad"
        return "refused"

    def refused_call(self, i, what):
        r, sc = self.r, self.sc
        if what == "upload":  # an instance whose material lies outside gMaterialData
            bad = clone(sc)
            bad.instances = sc.instances.copy()
            bad.instances["packed"][0, 0] |= 0xFFFFFFF0
            r.update(bad)
        elif what == "render":  # a sampling flag neither side builds
            flags = r.mSamplingFlags
            r.mSamplingFlags |= 1 << wire.FLAG_NAMES.index("eSampleLightPower")
            fr = self.frame()
            try:
                try:
                    self.oracle().render(fr, r.push_constants(fr), r.mSamplingFlags, 0, 1, threads=self.threads)
                    self.mismatch(i, "the oracle accepts eSampleLightPower")
                except RuntimeError:
                    pass
                r.render(fr, 0, 1)
            finally:
                r.mSamplingFlags = flags
        elif what == "update_vertices":  # a range that ends past the vertex count (the records handed over exist: the host array is longer than the scene)
            n = sc.vertices.shape[0]
            longer = clone(sc)
            longer.vertices = np.concatenate([sc.vertices, sc.vertices[:8]])
            longer.dirty_vertices = (max(0, n - 3), n + 5)
            r.update_vertices(longer)
        elif what == "animate":  # one pose too many (or no rigs at all)
            r.animate([pose for _, pose, _ in self.rigs] + [{"blend_factors": (0.1,)}])
        else:  # two rigs over ranges that overlap
            first, count = mesh_range(sc, int(triangle_instances(sc)[0]))
            w = np.zeros(count, wire.VertexWeight)
            w["weights"][:, 0] = 1
            rig = {"first_vertex": first, "vertex_count": count, "bone_count": 1, "weights": w}
            r.set_rigs([rig, dict(rig, first_vertex=first + count - 1, vertex_count=1, weights=w[:1])])


def run_walk(seed, steps=40, gpu=True, upto=None, drop=(), verbose=True, threads=THREADS, planned=None):
    """One walk: plan(seed, steps), or the steps given as `planned` (a directed sequence; `seed` then only labels it).
    Returns the Walk (its counts and its log) after closing the context."""
    trace = os.environ.get("STHIP_SEQ_TRACE") == "1"
    planned = plan(seed, steps) if planned is None else planned
    steps = len(planned)
    w = Walk(gpu, threads, verbose)
    try:
        for i, p in enumerate(planned):
            if (upto is not None and i >= upto) or i in drop or (w.sc is None and p["kind"] != "upload"):
                continue
            if trace: print("STEP %d.%d: %s" % (seed, i, describe(p)), flush=True)
            before = w.bad
            w.step(i, p)
            if w.bad > before and not trace: print("  (walk %d, step %d: %s)" % (seed, i, describe(p)), flush=True)
        w.drain(steps)
    finally:
        w.touched()
        w.close()
    return w


def run(walks=6, seed=1, steps=40, gpu=True, upto=None, drop=()):
    """Walks seed .. seed + walks - 1. Returns (compared, rejected, bad)."""
    compared = rejected = bad = 0
    t0 = time.time()
    for s in range(seed, seed + walks):
        w = run_walk(s, steps, gpu, upto, drop)
        compared, rejected, bad = compared + w.compared, rejected + w.rejected, bad + w.bad
        if w.bad: print("walk %d: %d mismatches" % (s, w.bad), flush=True)
    print("%d walks of %d steps: %d frames compared, %d rejected on both sides, %d mismatches, %.0f s" % (walks, steps, compared, rejected, bad, time.time() - t0), flush=True)
    return compared, rejected, bad


if __name__ == "__main__":
    argv = sys.argv[1:]
    opt = {"--upto": None, "--drop": ""}
    for name in list(opt):
        if name in argv:
            k = argv.index(name)
            opt[name] = argv[k + 1]
            del argv[k : k + 2]
    dry = "--dry" in argv
    argv = [a for a in argv if a != "--dry"]
    n, s, st = (int(argv[k]) if len(argv) > k else d for k, d in enumerate((6, 1, 40)))
    sys.exit(1 if run(n, s, st, not dry, int(opt["--upto"]) if opt["--upto"] else None, tuple(int(x) for x in opt["--drop"].split(",") if x))[2] else 0)
