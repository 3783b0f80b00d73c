"""Parity on generated scenes: what the library decides from the CONTENT of a scene, against the oracle, bit for bit.

tools/fuzz_scenes.py draws the scene itself. Here: its committed seeds (their plans are pinned by the coverage conditions below
and checked without a GPU against the oracle alone), and one directed test per content-dependent rule, so that a failure names
the rule:
  the specular thresholds of the material analysis (scene_prepare.cpp: analyse_materials) ... test_specular_thresholds
  the can_eval / emits bits of k_cull_terminal ..................................................... test_black_and_negative_materials
  the LDS staging of gMaterialData around its 32768 bytes .......................................... test_material_table_at_the_lds_bound
  the emitter-bounds table of answer_last_rays around STHIP_MAX_EMITTER_BOUNDS = 16 ................ test_emitter_count_at_the_bounds_table
  the merged identity mesh against the top level, mirrored / sheared instances, leaf records ....... test_instance_shapes
and one test per defect the generator found (EXPERIMENTS.md: "Generated scenes"): a NaN in a path's throughput under an
environment and on a light path, the pdf of an emissive sphere seen through a medium, and the visibility ray of a light
reservoir under a throughput that is black where the light is not.
Every comparison is of bits: there are no tolerances."""
import functools
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from oracle import oracle_py
from stratum_amd import camera, scenes, wire
from stratum_amd.scene import SceneBuilder, rotate_x, rotate_y, scale, translate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = tuple(range(1039, 1087))
THREADS = min(16, os.cpu_count() or 1)
W, H, FRAME_SEEDS = 48, 32, 2  # the frames of the directed tests: 1536 pixels x 2 seeds


def _tool():
    if "fuzz_scenes" not in sys.modules:
        spec = importlib.util.spec_from_file_location("fuzz_scenes", os.path.join(ROOT, "tools", "fuzz_scenes.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["fuzz_scenes"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["fuzz_scenes"]


def _fog():
    return np.load(os.path.join(ROOT, "tests", "golden", "fog_sphere.npz"))["grid"]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the plans of the committed seeds
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_seed_names_one_scene():
    """plan() is a pure function of the seed and returns a plain description; the scene built from it is the same twice."""
    fs = _tool()
    for seed in SEEDS[:12]:
        a, b = fs.plan(seed), fs.plan(seed)
        assert a == b and json.loads(json.dumps(a)) == a, seed
        assert fs.describe(a) == fs.describe(b) and "\n" not in fs.describe(a)
    assert fs.plan(SEEDS[0]) != fs.plan(SEEDS[1])
    s1, s2 = fs.make_scene(fs.plan(SEEDS[3]))[0], fs.make_scene(fs.plan(SEEDS[3]))[0]
    for name in ("vertices", "indices", "instances", "transforms", "inverse_transforms", "motion_transforms", "materials", "lights"):
        assert np.array_equal(getattr(s1, name).view(np.uint8), getattr(s2, name).view(np.uint8)), name


def coverage(plans):
    """name -> whether some committed plan has it: every edge the generator exists for, spelt out."""
    fs = _tool()
    used = []  # the materials instances and spheres refer to, per plan
    for p in plans:
        ids = {i["material"] for i in p["instances"]} | {s["material"] for s in p["spheres"]}
        used.append([p["materials"][k] for k in sorted(ids)])
    mats = [m for ms in used for m in ms]
    meshes = [m for p in plans for m in p["meshes"]]
    moving = [i for p in plans for i in p["instances"] if i["xf"] is not None and not i["bake"]]
    images = [im for p in plans for im in p["images"]]
    untextured = [p for p in plans if not p["textured"]]
    shapes = [fs.identity_count(p) for p in plans if p["kind"] == "room"]
    c = {}
    # every threshold of analyse_materials with both binary32 neighbours, as constants
    for name, index, values in (("metallic", 0, fs.T999), ("roughness", 1, fs.T01), ("transmission", 6, fs.T999)):
        for k, v in enumerate(values):
            c["%s %s the threshold" % (name, ("below", "at", "above")[k])] = any(m["params"][index] == v for m in mats)
    for k, v in enumerate(fs.T999):
        c["medium |anisotropy| %s 0.999" % ("below", "at", "above")[k]] = any(p["medium"] and abs(p["medium"]["anisotropy"]) == v for p in plans)
    c["a medium with a negative anisotropy"] = any(p["medium"] and p["medium"]["anisotropy"] < 0 for p in plans)
    for v in fs.ETAS:
        c["eta %r" % v] = any(m["eta"] == v for m in mats)
    c["a black base colour"] = any(not any(m["base"]) for m in mats)
    c["a base colour black in one channel"] = any(any(m["base"]) and not all(m["base"]) for m in mats)
    c["emission < 0"] = any(m["emission"] < 0 for m in mats)
    c["emission > 0"] = any(m["emission"] > 0 for m in mats)
    # the table's size around the 32768 bytes of the LDS staging (untextured scenes: the others do not stage)
    c["table of 32760 bytes (455 records: staged)"] = any(fs.table_bytes(p) == 455 * fs.RECORD for p in untextured)
    c["table of 32832 bytes (456 records: not staged)"] = any(fs.table_bytes(p) == 456 * fs.RECORD for p in untextured)
    c["a medium or environment record carries the table across the bound"] = any(p["pad"] == 455 and fs.table_bytes(p) > fs.LDS_BOUND for p in untextured)
    c["a medium or environment record ends just inside the bound"] = any(p["pad"] == 454 and 454 * fs.RECORD < fs.table_bytes(p) <= fs.LDS_BOUND for p in untextured)
    # emitters around STHIP_MAX_EMITTER_BOUNDS = 16, in scenes of the plain instantiation (the one that answers last rays)
    for n in (15, 16, 17):
        c["%d emissive triangle instances in a plain scene" % n] = any(p["plain"] and p["lights"] - p["emissive_spheres"] == n for p in plans)
    for n in (0, 1, 40):
        c["%d emitters" % n] = any(p["lights"] == n and p["kind"] == "room" for p in plans)
    c["no emitter under an environment"] = any(p["lights"] == 0 and p["environment"] for p in plans)
    c["emissive spheres beside emissive meshes"] = any(0 < p["emissive_spheres"] < p["lights"] for p in plans)
    c["an emissive textured material"] = any(m["emission"] > 0 and "base" in m["images"] for m in mats)
    c["a constant environment"] = any(p["environment"] and p["environment"]["image"] is None for p in plans)
    c["an image environment"] = any(p["environment"] and p["environment"]["image"] is not None for p in plans)
    # the merged identity mesh against the top level
    c["every triangle instance at the identity"] = any(a == n > 0 for a, n in shapes)
    c["no triangle instance at the identity"] = any(a == 0 < n for a, n in shapes)
    c["exactly one triangle instance moved"] = any(a == n - 1 > 0 for a, n in shapes)
    c["a mix of identity and moved instances"] = any(1 < a < n - 1 for a, n in shapes)
    c["a mirrored instance"] = any(i["xf"]["mirror"] for i in moving)
    c["a sheared instance"] = any(i["xf"]["shear"] != 0 for i in moving)
    c["a scale below 0.05"] = any(min(i["xf"]["s"]) < 0.05 for i in moving)
    c["one mesh 64 times"] = any(p["shape"] == "many_64" and p["kind"] == "room" for p in plans)
    c["one mesh 65 times"] = any(p["shape"] == "many_65" and p["kind"] == "room" for p in plans)
    c["motion transforms that differ"] = any(p["motion"] is not None for p in plans)
    c["a scene of spheres only"] = any(p["kind"] == "spheres_only" and not p["instances"] and p["spheres"] for p in plans)
    c["a scene of one triangle only"] = any(p["kind"] == "one_triangle" and len(p["instances"]) == 1 and not p["spheres"] for p in plans)
    c["three spheres"] = any(len(p["spheres"]) >= 3 for p in plans)
    # leaf records: what the pairs of a mesh look like
    for kind in ("soup", "grid", "single", "pair"):
        c["a %s mesh" % kind] = any(m["kind"] == kind for m in meshes)
    for pattern in fs.PAIRS:
        c["the pairing %s" % pattern] = any(m.get("pattern") == pattern for m in meshes)
    for what in fs.DEGENERATES:
        c["a %s triangle" % what] = any(what in m.get("degenerate", ()) for m in meshes)
    for what in ("random", "zero", "opposed"):
        c["%s normals" % what] = any(m.get("normals") == what for m in meshes)
    c["uvs outside [0, 1]"] = any(m.get("uvs") == "wide" for m in meshes)
    c["three equal uvs"] = any(m.get("uvs") == "equal" for m in meshes)
    c["16-bit indices"] = any(m.get("stride") == 2 for m in meshes)
    # the kernel instantiations: textured or not, extended or not
    c["an untextured scene"], c["a textured scene"] = bool(untextured), any(p["textured"] and p["images"] for p in plans)
    for extent in fs.IMAGE_EXTENTS:
        c["an image of %d x %d" % extent] = any((im["h"], im["w"]) == extent for im in images)
    c["8-bit images"], c["float images"] = any(im["bytes"] for im in images), any(not im["bytes"] for im in images)
    for role in ("params", "lobes"):
        c["%s texels that cross a threshold" % role] = any(im["role"] == role and im["crossing"] for im in images)
        c["%s texels that cross none" % role] = any(im["role"] == role and not im["crossing"] for im in images)
    c["a normal map"] = any(im["role"] == "normal" for im in images)
    c["an alpha mask under eAlphaTest"] = any(p["masks"] and "alphatest" in p["args"]["bdptFlag"] for p in plans)
    c["8-bit and float masks"] = any(mk["bytes"] for p in plans for mk in p["masks"]) and any(not mk["bytes"] for p in plans for mk in p["masks"])
    for name, value in fs.OPTIONS:
        c["a render under %s = %d" % (name, value)] = any([name, value] in p["options"] for p in plans)
    return c


def test_the_committed_seeds_cover_what_they_are_for():
    """An edit to the generator that thins the cases out fails here."""
    fs = _tool()
    plans = [fs.plan(seed) for seed in SEEDS]
    missing = [name for name, there in coverage(plans).items() if not there]
    assert not missing, missing
    for p in plans:
        f = p["frame"]
        assert f["W"] <= 72 and f["H"] <= 40 and f["seeds"] <= 2 and 2 <= len(p["options"]) <= 3
        assert all(1 <= len(fs.mesh_arrays(m)[3]) <= 46 for m in p["meshes"])


@pytest.fixture(scope="module")
def dry_slice(built):
    fs = _tool()
    runner = fs.Runner(gpu=False, threads=THREADS)
    try:
        return [runner.run_case(fs.plan(seed)) for seed in SEEDS], runner
    finally:
        runner.close()


def test_the_oracle_alone_accepts_every_committed_case(dry_slice):
    """The conditions under which the GPU comparison means anything: the oracle renders every committed case (at most a tenth
    may be rejected; none is), its radiance is finite, and its own traversal equals its brute force on the case's rays."""
    results, runner = dry_slice
    assert runner.bad == 0
    rejected = sum(r["outcome"] == "rejected" for r in results)
    assert rejected <= 0.1 * len(SEEDS) and rejected == runner.rejected
    for seed, r in zip(SEEDS, results):
        if r["outcome"] == "rejected":
            continue
        assert r["outcome"] == "compared" and r["finite"] and r["bvh_equals_brute"], (seed, r)
    assert sum(r["instances_seen"] >= 5 for r in results) >= len(SEEDS) // 2  # (the frames look at something)


# ---------------------------------------------------------------------------------------------------------------------------
# the directed scenes
# ---------------------------------------------------------------------------------------------------------------------------
BOX = [((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1), (0, 1, 0)), ((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1), (0, -1, 0)), ((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (0, 0, 1)),
       ((1, -1, 1), (-1, -1, 1), (-1, 1, 1), (1, 1, 1), (0, 0, -1)), ((-1, -1, 1), (-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (1, 0, 0)), ((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1), (-1, 0, 0))]
BOX_CAM = {"eye": (0.0, 0.0, 0.9), "target": (0.0, 0.0, -1.0), "fovy": np.radians(60.0)}
LIMITS = dict(maxDiffuseVertices=1, maxPathVertices=8, minPathVertices=9)  # (no roulette: a path ends by its budgets alone)


def closed_box(material, light=True, images=(), params_image=None, lobes_image=None, medium=None, walls=None):
    """A closed box [-1, 1]^3 of one material (`material`: SceneBuilder.add_material's arguments) around the camera, a small
    lamp under its ceiling; `walls`: six materials instead of one; `medium`: the anisotropy of a cloud in it."""
    b = SceneBuilder("closed_box")
    handles = [b.add_image(im) for im in images]
    mats = [b.add_material(**m) for m in (walls or [material])]
    for m in mats:
        b.set_material_images(m, params_image=None if params_image is None else handles[params_image], lobes_image=None if lobes_image is None else handles[lobes_image])
    if walls:
        for k, q in enumerate(BOX):
            b.add_instance(b.add_mesh(*scenes._quad(*q)), mats[k])
    else:
        b.add_instance(b.add_mesh(*scenes._merge([scenes._quad(*q) for q in BOX])), mats[0])
    if light:
        b.add_instance(b.add_mesh(*scenes._quad((-0.3, 0.98, -0.6), (0.3, 0.98, -0.6), (0.3, 0.98, -0.1), (-0.3, 0.98, -0.1), (0, -1, 0))), b.add_emitter((17.0, 12.0, 4.0)))
    if medium is not None:
        b.add_medium(b.add_volume(_fog()), density_scale=(4.0, 4.0, 4.0), albedo_scale=(0.9, 0.9, 0.9), anisotropy=medium, transform=translate((-0.1, 0.0, -0.4)) @ scale((0.6, 0.6, 0.6)))
    return b.build()


def frame_of(cam, w=W, h=H):
    return camera.Frame(w, h, cam["fovy"], cam["eye"], cam["target"])


def oracle_frame(sc, fr, args, seed0=0, seeds=FRAME_SEEDS):
    """The oracle's frame of a scene under renderer arguments `args` (through BDPT's own flags and push constants, without a context)."""
    fs = _tool()
    dry = fs.fuzz_sequences._Dry(args=args)
    dry.update(sc)
    o = oracle_py.OracleScene(fs.fuzz_sequences.float_form(sc))
    try:
        return o.render(fr, dry.push_constants(fr), dry.mSamplingFlags, seed0, seeds, threads=THREADS)
    finally:
        o.close()


def rays_of(ref):
    return [int(x) for x in ref["ray_count"]]


def same_as_oracle(got, ref, w=W, h=H):
    return _tool().fuzz_parity.compare_frames(got, dict(ref), w, h)


METAL = dict(base_color=(0.9, 0.8, 0.7), metallic=1.0, roughness=0.0)


def threshold_cases():
    """(name, scene factory, specular: whether some hit is specular by the rule of disney_material.hlsli:125 / medium.hlsli:22)."""
    fs = _tool()
    below, at, above = 0, 1, 2
    cases = []
    for k, word in enumerate(("below", "at", "above")):
        cases.append(("metallic %s 0.999" % word, functools.partial(closed_box, dict(METAL, metallic=fs.T999[k])), k == above))
        cases.append(("transmission %s 0.999" % word, functools.partial(closed_box, dict(METAL, metallic=0.0, transmission=fs.T999[k], eta=1.5)), k == above))
        cases.append(("roughness %s 1e-2" % word, functools.partial(closed_box, dict(METAL, roughness=fs.T01[k])), k != above))

    def row(values, channel, rest):
        im = np.zeros((1, len(values), 4), np.float32)
        im[...] = rest
        im[0, :, channel] = values
        return im

    t, r = fs.T999, fs.T01
    one = dict(METAL, metallic=1.0, roughness=1.0)  # constants of one: value * texel is the texel
    # metallic in the params image's r, roughness in its g; transmission in the lobes image's b (its alpha scales eta)
    cases.append(("metallic texels up to 0.999", functools.partial(closed_box, one, images=[row([0.5, t[below], t[at]], 0, (0, 0, 0, 0))], params_image=0), False))
    cases.append(("metallic texels, one above 0.999", functools.partial(closed_box, one, images=[row([0.5, t[at], t[above], t[at]], 0, (0, 0, 0, 0))], params_image=0), True))
    cases.append(("roughness texels all above 1e-2", functools.partial(closed_box, one, images=[row([0.5, r[above], 1.0], 1, (1, 0, 0, 0))], params_image=0), False))
    cases.append(("roughness texels, one at 1e-2", functools.partial(closed_box, one, images=[row([0.5, r[above], r[at], r[above]], 1, (1, 0, 0, 0))], params_image=0), True))
    glass = dict(METAL, metallic=0.0, transmission=1.0, eta=1.5)
    cases.append(("transmission texels up to 0.999", functools.partial(closed_box, glass, images=[row([0.25, t[at], t[below]], 2, (0, 0, 0, 1))], lobes_image=0), False))
    cases.append(("transmission texels, one above 0.999", functools.partial(closed_box, glass, images=[row([t[above], 0.25, t[at]], 2, (0, 0, 0, 1))], lobes_image=0), True))
    # a constant that is not one: 0.9995f * texel crosses 0.999 between the texels 0.9994 and 1
    scaled = dict(METAL, metallic=float(np.float32(0.9995)), roughness=1.0)
    cases.append(("0.9995 x metallic texels up to 0.9994", functools.partial(closed_box, scaled, images=[row([0.5, 0.9994], 0, (0, 0, 0, 0))], params_image=0), False))
    cases.append(("0.9995 x metallic texels up to 1", functools.partial(closed_box, scaled, images=[row([0.5, 0.9994, 1.0], 0, (0, 0, 0, 0))], params_image=0), True))
    # 8-bit texels: 254 / 255 < 0.999 < 255 / 255 (a 1 x 1 image has no further levels: its float form gives the same frame)
    for byte, word in ((254, "below"), (255, "above")):
        cases.append(("an 8-bit metallic texel %s 0.999" % word, functools.partial(closed_box, one, images=[np.array([[[byte, 0, 0, 0]]], np.uint8)], params_image=0), byte == 255))
    for k, word in enumerate(("below", "at", "above")):
        for sign in (1.0, -1.0):
            cases.append(("medium anisotropy %s %s0.999" % (word, "-" if sign < 0 else ""), functools.partial(closed_box, dict(base_color=(0.7, 0.7, 0.7)), medium=sign * fs.T999[k]), k == above))
    return cases


@functools.lru_cache(maxsize=None)
def threshold_references():
    """name -> (scene, the oracle's frame under LIMITS, specular); made once, shared by the CPU and the GPU test."""
    fr = frame_of(BOX_CAM)
    out = {}
    for name, make, specular in threshold_cases():
        sc = make()
        out[name] = (sc, oracle_frame(sc, fr, LIMITS), specular)
    return out


def test_the_oracle_ray_counts_differ_across_each_specular_threshold(built):
    """Why the directed GPU tests would notice a wrong host rule: in a closed box of one material under gMaxDiffuseVertices = 1,
    a path goes on past its first bounce only through specular vertices, so the oracle's gRayCount jumps when the material
    crosses a threshold by one binary32 step (the four cases of the issue's table, and the texel and medium forms)."""
    refs = threshold_references()
    rays = {name: rays_of(ref) for name, (_, ref, _) in refs.items()}
    for a, b in (("roughness at 1e-2", "roughness above 1e-2"), ("metallic at 0.999", "metallic above 0.999"), ("transmission at 0.999", "transmission above 0.999"),
                 ("metallic texels up to 0.999", "metallic texels, one above 0.999"), ("roughness texels all above 1e-2", "roughness texels, one at 1e-2"),
                 ("transmission texels up to 0.999", "transmission texels, one above 0.999"), ("0.9995 x metallic texels up to 0.9994", "0.9995 x metallic texels up to 1"),
                 ("an 8-bit metallic texel below 0.999", "an 8-bit metallic texel above 0.999"), ("medium anisotropy at 0.999", "medium anisotropy above 0.999"),
                 ("medium anisotropy at -0.999", "medium anisotropy above -0.999")):
        assert refs[a][2] != refs[b][2]
        assert rays[a] != rays[b], (a, b, rays[a])
    pixels = W * H * FRAME_SEEDS
    for name, (_, ref, specular) in refs.items():
        assert np.isfinite(ref["radiance"]).all(), name
        # the camera is inside the closed box: every pixel's first ray hits, the first vertex samples a direction and its ray is
        # traced, and the vertex it finds is diffuse vertex 2 of a budget of 1 unless something was specular: the path rays
        # (gRayCount[1]) are two per pixel and seed exactly when nothing is
        assert (rays[name][1] == 2 * pixels) == (not specular), (name, rays[name])


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: one test per rule
# ---------------------------------------------------------------------------------------------------------------------------
def make_renderer(args=None, **options):
    from stratum_amd.bdpt import BDPT

    r = BDPT(0, args=args)
    for k, v in options.items():
        r.set_option(k, v)
    return r


def traced_rays_match(r, sc, seed=5, n=1500):
    """closest hit and any hit of the resident scene on awkward rays against the oracle's brute force."""
    fs = _tool()
    rays, style, lo, hi = fs.fuzz_parity.awkward_rays(np.random.default_rng(seed), sc, n)
    o = oracle_py.OracleScene(fs.fuzz_sequences.float_form(sc))
    try:
        return fs.compare_rays(r, o, sc, rays, style, lo, hi, False, THREADS).size == 0
    finally:
        o.close()


@pytest.mark.gpu
def test_specular_thresholds(built):
    """metallic, transmission and roughness at their thresholds and at both binary32 neighbours, as constants and as constant x
    texel range (float and 8-bit), and a medium at |anisotropy| 0.999 and its neighbours: has_specular cuts the bounce and shadow
    rounds and gates the coherent roulette, so a host rule one step off the device's loses or gains rays. Frames and ray counts
    equal the oracle's, without the roulette (the path ends by its budgets) and with the default eCoherentRR."""
    fr = frame_of(BOX_CAM)
    roulette = dict(LIMITS, minPathVertices=2)
    r, r2 = make_renderer(LIMITS), make_renderer(roulette)
    try:
        for name, (sc, ref, _) in threshold_references().items():
            r.update(sc)
            got = r.render(fr, 0, FRAME_SEEDS)
            print(name, rays_of(got), rays_of(ref))
            assert same_as_oracle(got, ref), (name, rays_of(got), rays_of(ref))
            if "texels" in name or " at " in name or name.startswith("medium anisotropy above"):
                r2.update(sc)
                assert same_as_oracle(r2.render(fr, 3, FRAME_SEEDS), oracle_frame(sc, fr, roulette, 3)), (name, "with the roulette")
    finally:
        r.close()
        r2.close()


@pytest.mark.gpu
def test_black_and_negative_materials(built):
    """A black base colour (nothing to evaluate), emission < 0 (neither an emitter nor a scatterer: can_eval asks emission <= 0,
    emits asks base_color * emission > 0), emission > 0 under a black base colour (a light instance that emits nothing) and under
    a base colour black in two channels: the can_eval and emits bits of k_cull_terminal's table, with the kernel and without."""
    walls = [dict(base_color=(0.0, 0.0, 0.0)), dict(base_color=(0.8, 0.7, 0.6), emission=-2.0), dict(base_color=(0.0, 0.0, 0.0), emission=3.0), dict(base_color=(0.0, 0.9, 0.0), emission=2.0, eta=0.0),
             dict(base_color=(0.7, 0.7, 0.7)), dict(base_color=(0.0, 0.6, 0.8), metallic=1.0, roughness=0.0)]
    sc = closed_box(None, walls=walls)
    assert sc.light_count == 3  # (the black emitter is a light instance too: Scene.cpp asks emission > 0)
    fr = frame_of(BOX_CAM)
    r = make_renderer()
    try:
        r.update(sc)
        for k, args in enumerate((dict(maxDiffuseVertices=1, maxPathVertices=3), dict(maxDiffuseVertices=2, maxPathVertices=5, minPathVertices=6), dict(maxDiffuseVertices=3, maxPathVertices=4))):
            ref = oracle_frame(sc, fr, args, seed0=k)
            assert np.isfinite(ref["radiance"]).all() and ref["radiance"][..., :3].max() > 0
            r.set_args(args)
            for cull in (1, 0):
                r.set_option("cull_terminal", cull)
                got = r.render(fr, k, FRAME_SEEDS)
                assert same_as_oracle(got, ref), (args, cull, rays_of(got), rays_of(ref))
    finally:
        r.close()


GRID_W, GRID_H, GRID_NX, GRID_NY = 72, 40, 28, 17
GRID_CAM = {"eye": (0.0, 0.0, 2.0), "target": (0.0, 0.0, 0.0), "fovy": np.radians(40.0)}


def quad_grid(records, medium=False, environment=False):
    """`records` material records of 72 bytes, every one on a small quad of its own in a 28 x 17 grid that fills the view
    (one of them the lamp's); then a medium's 40 bytes and / or a constant environment's 16."""
    fs = _tool()
    rng = np.random.default_rng(records)
    b = SceneBuilder("quad_grid_%d" % records)
    half_h = 2.0 * np.tan(0.5 * GRID_CAM["fovy"])
    half_w = half_h * GRID_W / GRID_H
    mesh = b.add_mesh(*scenes._quad((-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0), (0, 0, 1)))
    assert records <= GRID_NX * GRID_NY
    for k in range(records):
        if k == records // 2:
            m = b.add_emitter((9.0, 8.0, 7.0))
        else:
            p = fs._specular_material(rng) if k % 7 == 0 else fs._material(rng, emission=0.0)
            q = p["params"]
            m = b.add_material(tuple(p["base"]), metallic=q[0], roughness=q[1], anisotropic=q[2], subsurface=q[3], clearcoat=q[4], clearcoat_gloss=q[5], transmission=q[6], eta=p["eta"])
        x, y = (k % GRID_NX + 0.5) / GRID_NX * 2 - 1, (k // GRID_NX + 0.5) / GRID_NY * 2 - 1
        b.add_instance(mesh, m, translate((x * half_w, y * half_h, 0.02 * np.sin(k))) @ rotate_x(0.2 * np.cos(k)) @ scale((1.96 * half_w / GRID_NX, 1.96 * half_h / GRID_NY, 1.0)))
    if medium:
        b.add_medium(b.add_volume(_fog()), density_scale=(2.0, 2.0, 2.0), albedo_scale=(0.9, 0.9, 0.9), anisotropy=0.3, transform=translate((0.0, 0.0, 0.8)) @ scale((0.4, 0.4, 0.4)))
    if environment:
        b.set_environment((0.5, 0.6, 0.7))
    return b.build()


@pytest.mark.gpu
def test_material_table_at_the_lds_bound(built):
    """k_shade stages gMaterialData in LDS when the table is at most 32768 bytes, and reads a record from LDS when it ends inside
    the staged bytes. 455 records (32760 bytes) are staged, 456 (32832) are not; a medium's 40 bytes or an environment's 16 carry
    a table of 455 records across the bound and leave one of 454 inside it, with the last surface record ending 40 / 16 / 56 bytes
    before the table does. Most records are hit: the oracle sees at least 300 instances. lds_materials = 1 and 0 give the
    oracle's frame."""
    args = dict(maxDiffuseVertices=2, maxPathVertices=5)
    fr = frame_of(GRID_CAM, GRID_W, GRID_H)
    r = make_renderer(args)
    try:
        for records, medium, environment, size in ((455, False, False, 32760), (456, False, False, 32832), (454, True, False, 32728), (455, True, False, 32800), (454, False, True, 32704),
                                                   (455, False, True, 32776), (454, True, True, 32744)):
            sc = quad_grid(records, medium, environment)
            assert sc.materials.nbytes == size and not sc.images
            ref = oracle_frame(sc, fr, args)
            seen = ref["visibility"]["instance_primitive_index"]
            assert np.unique(seen[seen != wire.MISS] & 0xFFFF).size >= 300 and np.isfinite(ref["radiance"]).all()
            r.update(sc)
            for lds in (1, 0):
                r.set_option("lds_materials", lds)
                got = r.render(fr, 0, FRAME_SEEDS)
                assert same_as_oracle(got, ref, GRID_W, GRID_H), (size, lds, rays_of(got), rays_of(ref))
    finally:
        r.close()


ROOM_CAM = {"eye": (0.0, 0.3, 3.5), "target": (0.0, 0.2, 0.0), "fovy": np.radians(45.0)}


def lamp_room(lamps, spheres=0):
    """A room with a block in it under `lamps` small emissive quads (instances of one mesh, every third one at the identity with
    a mesh of its own) and `spheres` emissive spheres."""
    fs = _tool()
    b = SceneBuilder("lamp_room_%d_%d" % (lamps, spheres))
    white, grey = b.add_material((0.73, 0.73, 0.73)), b.add_material((0.4, 0.5, 0.6), roughness=0.5)
    for wall in fs._WALLS.values():
        b.add_instance(b.add_mesh(*scenes._quad(*wall)), white)
    faces = [scenes._quad(*q) for q in BOX[:3] + BOX[4:]]
    b.add_instance(b.add_mesh(*scenes._merge(faces)), grey, translate((0.3, -0.6, 0.0)) @ rotate_y(0.4) @ scale((0.4, 0.4, 0.4)))
    glow = b.add_emitter((12.0, 10.0, 8.0))
    lamp = np.array([(-0.08, 0, -0.08), (0.08, 0, -0.08), (0.08, 0, 0.08), (-0.08, 0, 0.08)], np.float32)
    down, (_, _, uv, tri) = np.tile(np.array((0, -1, 0), np.float32), (4, 1)), scenes._quad(*BOX[0])
    shared = b.add_mesh(lamp, down, uv, tri)
    side = int(np.ceil(np.sqrt(lamps)))
    for k in range(lamps):
        at = np.array([-1.5 + (k % side + 0.5) * 3.0 / side, 2.9 - 0.01 * k, -1.5 + (k // side + 0.5) * 3.0 / side])
        if k % 3 == 0:
            b.add_instance(b.add_mesh((lamp + at).astype(np.float32), down, uv, tri), glow)
        else:
            b.add_instance(shared, glow, translate(tuple(at)) @ rotate_y(0.3 * k))
    for k in range(spheres):
        b.add_sphere(glow, 0.12, translate((-0.9 + 0.9 * k, 1.6, 0.4)))
    sc = b.build()
    assert sc.light_count == lamps + spheres
    return sc


@pytest.mark.gpu
def test_emitter_count_at_the_bounds_table(built):
    """15, 16, 17 and 40 emitters. The bounds table of answer_last_rays holds at most STHIP_MAX_EMITTER_BOUNDS = 16 emissive
    triangle instances (scene_prepare.h: emitter_bounds) and is dropped beyond; it is consulted by the plain k_shade instantiation
    only, so a scene with a sphere answers nothing whatever its count (include/sthip.h: rays_answered). answer_last_rays = 1
    and 0 give the oracle's frame and ray counts; rays_answered > 0 exactly where the table is in use."""
    args = dict(maxDiffuseVertices=2, maxPathVertices=4)
    fr = frame_of(ROOM_CAM)
    r = make_renderer(args)
    try:
        for lamps, spheres in ((15, 0), (16, 0), (17, 0), (40, 0), (14, 1), (16, 2), (38, 2)):
            sc = lamp_room(lamps, spheres)
            ref = oracle_frame(sc, fr, args)
            r.update(sc)
            for answer in (1, 0):
                r.set_option("answer_last_rays", answer)
                got = r.render(fr, 0, FRAME_SEEDS)
                answered = r.stats()["rays_answered"]
                print(lamps, spheres, answer, answered, rays_of(got))
                assert same_as_oracle(got, ref), (lamps, spheres, answer, rays_of(got), rays_of(ref))
                assert (answered > 0) == (answer == 1 and lamps <= 16 and spheres == 0), (lamps, spheres, answer, answered)
    finally:
        r.close()


def shape_scene(kind):
    """The scene shapes that pick different paths in traverse.h and bvh_build.h: see test_instance_shapes."""
    fs = _tool()
    b = SceneBuilder("shape_" + kind)
    white, red, glow = b.add_material((0.73, 0.73, 0.73)), b.add_material((0.65, 0.05, 0.05), roughness=0.3), b.add_emitter((17.0, 12.0, 4.0))
    if kind == "spheres_only":
        b.add_sphere(white, 0.5, translate((-0.4, 0.0, 0.0)))
        b.add_sphere(red, 0.3, translate((0.5, 0.3, 0.4)))
        b.add_sphere(glow, 0.2, translate((0.2, 1.3, 0.8)))
        return b.build()
    if kind == "one_triangle":
        b.add_instance(b.add_mesh(np.array([(-1.2, -0.8, 0), (1.2, -0.8, 0.2), (0, 1.2, -0.2)], np.float32), None, None, np.array([[0, 1, 2]])), red)
        b.set_environment((0.8, 0.9, 1.1))
        return b.build()
    block = scenes._merge([scenes._quad(*q) for q in BOX[:3] + BOX[4:]])
    moves = [translate((0.6, -0.5, 0.2)) @ rotate_y(0.5) @ scale((0.4, 0.5, 0.3)), translate((-0.7, -0.4, -0.3)) @ rotate_x(0.3) @ scale((0.35, 0.6, 0.35))]
    if kind == "mirrored": moves = [m @ scale((-1.0, 1.0, 1.0)) for m in moves]
    if kind == "sheared":
        for m in moves: m[0, 1] += 0.6
    hair = translate((0.0, 0.0, -0.01))
    walls = list(fs._WALLS.values()) + [((-0.5, 2.95, -0.5), (0.5, 2.95, -0.5), (0.5, 2.95, 0.5), (-0.5, 2.95, 0.5), (0, -1, 0))]
    for k, wall in enumerate(walls):
        b.add_instance(b.add_mesh(*scenes._quad(*wall)), glow if k == len(walls) - 1 else white, hair if kind == "none_identity" else None)
    if kind in ("many_64", "many_65"):
        mesh = b.add_mesh(*block)
        for k in range(int(kind[5:])):
            b.add_instance(mesh, red if k % 3 else white, translate((-1.4 + 0.4 * (k % 8), -0.6 + 0.35 * (k // 8), -1.0 + 0.01 * k)) @ rotate_y(0.1 * k) @ scale((0.12, 0.12, 0.12)))
        return b.build()
    for k, m in enumerate(moves):
        baked = kind == "all_identity" or (kind == "one_moved" and k == 0)
        if baked:
            pos, nrm, uv, tri = block
            b.add_instance(b.add_mesh((pos.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32), nrm, uv, tri), red)
        else:
            b.add_instance(b.add_mesh(*block), red, m)
    return b.build()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["all_identity", "none_identity", "one_moved", "mirrored", "sheared", "many_64", "many_65", "spheres_only", "one_triangle"])
def test_instance_shapes(built, kind):
    """All instances at the identity (the merged mesh is the whole scene: top_is_world_blas), none, exactly one moved; mirrored
    (negative determinant) and sheared instances; one mesh 64 and 65 times; spheres only (no triangle at all); one triangle only.
    Frames, ray counts and traced rays equal the oracle's under the host builder and, for scenes of triangles, the device's."""
    sc = shape_scene(kind)
    ident = np.array([np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]])
    tri = (sc.instances["packed"][:, 0] & 0xF) == 0
    want = {"all_identity": tri.sum() == (ident & tri).sum() > 0, "none_identity": (ident & tri).sum() == 0, "one_moved": (~ident & tri).sum() == 1, "spheres_only": tri.sum() == 0,
            "one_triangle": sc.triangle_count == 1}.get(kind, (~ident & tri).sum() >= 2)
    assert want
    args = dict(maxDiffuseVertices=2, maxPathVertices=5)
    fr = frame_of(ROOM_CAM)
    ref = oracle_frame(sc, fr, args)
    assert np.isfinite(ref["radiance"]).all() and ref["radiance"][..., :3].max() > 0
    for builder in (0, 1) if kind != "spheres_only" else (0,):
        r = make_renderer(args, bvh_builder=builder)
        try:
            r.update(sc)
            got = r.render(fr, 0, FRAME_SEEDS)
            assert same_as_oracle(got, ref), (kind, builder, rays_of(got), rays_of(ref))
            assert traced_rays_match(r, sc), (kind, builder)
        finally:
            r.close()


@pytest.mark.gpu
def test_a_path_whose_throughput_went_nan_ends_at_its_miss_under_an_environment(built):
    """Found by the generator (quad grids and seeds 1043, 1058, 1072, 1084 under an environment): a material with eta = 1 or 0
    and a base colour black in one channel leaves a NaN in one channel of beta. The loop of bdpt.hlsl:298 then ends the path
    before next_vertex() looks at the background; k_shade added the environment's term at the miss all the same, the sample
    became NaN and k_resolve dropped it with its weight (radiance.w one short, the pixel twice as bright or black)."""
    args = dict(maxDiffuseVertices=2, maxPathVertices=5)
    fr = frame_of(GRID_CAM, GRID_W, GRID_H)
    sc = quad_grid(20, environment=True)
    ref = oracle_frame(sc, fr, args)
    assert np.isfinite(ref["radiance"]).all()
    r = make_renderer(args)
    try:
        r.update(sc)
        got = r.render(fr, 0, FRAME_SEEDS)
        assert np.array_equal(got["radiance"][..., 3], ref["radiance"][..., 3])  # no sample was dropped that the reference keeps
        assert same_as_oracle(got, ref, GRID_W, GRID_H)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1042, 1066, 1076])
def test_a_light_path_whose_throughput_went_nan_ends(built, seed):
    """Found by the generator: the loop of bdpt.hlsl:145 ends a light path whose beta holds a NaN; k_shade_light tested only
    all(beta <= 0) and went on, tracing rays the reference does not trace (seed 1042, eConnectToViews: equal frames, 33 rays
    too many) and storing vertices it does not store (seeds 1066 and 1076, the light vertex cache: 982 and 2504 pixels)."""
    fs = _tool()
    runner = fs.Runner(gpu=True, threads=THREADS)
    try:
        assert runner.run_case(fs.plan(seed))["outcome"] == "compared"
    finally:
        runner.close()
    assert runner.bad == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [100825, 100827, 100901])
def test_an_emissive_sphere_seen_through_a_medium(built, seed):
    """Found by the generator's long run (7 of 2000 cases, one to three pixels each, all with a medium and an emissive sphere;
    only with eNEE, eSampleBSDFs and eMIS together): the solid-angle pdf of a sphere that a sampled direction hits
    (intersection.hlsli:150-158) is taken from the `origin` of the trace_ray call that found it, which with media is the start
    of the walk's last segment, a volume boundary. k_shade took the path's previous vertex, so the MIS weight of the sphere's
    emission differed wherever the ray had crossed the cloud's box on its way."""
    fs = _tool()
    p = fs.plan(seed)
    assert p["medium"] and p["emissive_spheres"] and not p["args"]["bdptFlag"]
    runner = fs.Runner(gpu=True, threads=THREADS)
    try:
        assert runner.run_case(p)["outcome"] == "compared"
    finally:
        runner.close()
    assert runner.bad == 0


@pytest.mark.gpu
def test_a_reservoir_shadow_ray_is_traced_whatever_the_throughput(built):
    """Found by the generator's long run (case 762 of 2000, plan seed 100762: every image equal, gRayCount[0] one short). Without
    eDeferShadowRays, connect_light_reservoir traces its visibility ray as soon as Le * f * G * W has a positive channel
    (path.hlsli:450,476); beta and the MIS weight only scale what an unoccluded ray adds (:485). k_shade dropped the record when
    beta * contrib * weight was all <= 0, which is trace_shadows' rule for DEFERRED records (bdpt.hlsl:313): a throughput that is
    black in the channels where the light's contribution is not (base colours black in one channel) cost the reference a ray
    that the device never queued. The case, then the same scene with nothing but eNEEReservoirs on top of the defaults."""
    fs = _tool()
    p = fs.plan(100762)
    flags = p["args"]["bdptFlag"]
    assert "neereservoirs" in flags and "~defershadowrays" in flags and not p["medium"]
    assert any(any(m["base"]) and not all(m["base"]) for m in p["materials"])  # a base colour black in one channel
    q = dict(p, bundle="none", args=dict(maxDiffuseVertices=4, maxPathVertices=5, minPathVertices=4, reservoirM=2, bdptFlag=["~defershadowrays", "neereservoirs"]), options=[["cull_terminal", 0], ["answer_last_rays", 0]])
    runner = fs.Runner(gpu=True, threads=THREADS)
    try:
        for case in (p, q):
            out = runner.run_case(case)
            print(fs.describe(case), out)
            assert out["outcome"] == "compared", fs.describe(case)
    finally:
        runner.close()
    assert runner.bad == 0


@pytest.mark.gpu
def test_generated_scene_slice(built):
    """The committed seeds through the runner: the frame against the oracle, the same frame under two or three execution options,
    closest and any hit against the oracle's brute force. No mismatch, and at most a tenth rejected on both sides."""
    fs = _tool()
    runner = fs.Runner(gpu=True, threads=THREADS)
    try:
        for seed in SEEDS:
            runner.run_case(fs.plan(seed))
    finally:
        runner.close()
    print("%d compared, %d rejected, %d mismatches" % (runner.compared, runner.rejected, runner.bad))
    assert runner.bad == 0 and runner.rejected <= 0.1 * len(SEEDS) and runner.compared + runner.rejected == len(SEEDS)
