"""Randomised differential test of SCENE CONTENT (GPU box): generated scenes, the HIP path against the oracle, bit for bit.
usage: tools/fuzz_scenes.py [cases] [seed] [--only a[-b]] [--trace] [--dry]. Prints every mismatch and exits non-zero.

tools/fuzz_parity.py and tools/fuzz_sequences.py vary flags, limits, frames, options and call order over eight hand-made scenes.
Here the scene itself is drawn: meshes (soups, small grids, the single triangle, the two-triangle pairings of
profiles/r14/coverage.txt, duplicate / coplanar / zero-area / sliver triangles, odd normals and uvs), instances (all, none, one or
some at the identity; rotated, scaled over three decades, sheared, mirrored; one mesh many times), spheres, materials whose values
sit on the thresholds of the host's material analysis (csrc/scene_prepare.cpp: analyse_materials) and on their binary32
neighbours, images whose texels carry value * texel across those thresholds, 0 .. 40 emitters around the emitter-bounds table
(STHIP_MAX_EMITTER_BOUNDS), media at |anisotropy| = 0.999, and material tables padded to the 32768-byte bound of the LDS staging.

A case is planned first (plan(seed): a plain description drawn from the seed alone; the dimensions with few values go round with
the seed, so a run of consecutive seeds meets every one of them), then built (make_scene) and run (run_case): the frame against
the oracle, the same frame again under two or three execution options that must change nothing, and closest / any hit on
fuzz_parity.awkward_rays against the oracle's brute force. Case k of `[cases] [seed]` is plan(seed * 100000 + k).

Every input is finite, every transform invertible, coordinates stay within a few units of the origin. An error of the library
that is not a refusal of arguments ends the run at once (exit status 2, the case's description printed): after a HIP error nothing
more is launched. --only a[-b]: only these cases run; --trace prints and flushes each case before it runs; --dry: the oracle alone (a case
whose radiance is not finite, or whose traversal differs from its brute force by the rule of the rays above, is a mismatch)."""
import os
import re
import sys
import time

os.environ.setdefault("STHIP_STRICT_FLAGS", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
from oracle import oracle_py
from stratum_amd import camera, wire
from stratum_amd._lib import StratumHipError
from stratum_amd.bdpt import BDPT
from stratum_amd.scene import SceneBuilder, rotate_x, rotate_y, scale, translate

import fuzz_parity
import fuzz_sequences
from test_image_formats import mip_exact_image  # (tests/: 8-bit images whose float chain equals their decoded byte chain, as fuzz_sequences.py uses them)

F32 = np.float32
THREADS = min(16, os.cpu_count() or 1)
CAM = {"eye": (0.0, 0.3, 3.5), "target": (0.0, 0.2, 0.0), "fovy": float(np.radians(45.0))}
RECORD, MEDIUM_RECORD, LDS_BOUND = 72, 40, 32768  # bytes: a material record, a medium record, the largest table k_shade stages


def neighbours(x):
    """(the binary32 below, x as binary32, the binary32 above), as Python floats."""
    x = F32(x)
    return [float(np.nextafter(x, F32(-np.inf))), float(x), float(np.nextafter(x, F32(np.inf)))]


# the thresholds of analyse_materials: metallic / transmission > 0.999f, roughness <= 1e-2f, |anisotropy| <= 0.999f (media)
T999, T01 = neighbours(0.999), neighbours(1e-2)
EDGES = [0.0, 1.0, float(F32(1e-3))] + T999 + T01
ETAS = [0.0, 1.0, neighbours(1.0)[0], neighbours(1.0)[2], float(F32(0.7)), 1.5, float(F32(2.4))]
ANISOTROPIES = T999 + [-v for v in T999]
BYTE_TEXELS = [0, 2, 3, 128, 254, 255]  # 2 / 255 < 1e-2 < 3 / 255, 254 / 255 < 0.999 < 255 / 255
KINDS = ("room", "room", "room", "room", "room", "room", "spheres_only", "one_triangle")
SHAPES = ("mix", "all_identity", "none_identity", "one_moved", "mix", "many_64", "mix", "many_65", "all_identity", "mix", "none_identity")
LIGHTS = (1, 0, 15, 16, 17, 40, 2)  # emitters; 0: an environment lights the scene
PADS = (None, None, 455, 456, 454)  # records of 72 bytes in gMaterialData (455: 32760 bytes, 456: 32832; 454: room for a medium record)
PAIRS = {"fan": (0, 2, 3), "fan_swapped": (0, 3, 1), "strip": (1, 3, 2), "strip_swapped": (3, 0, 2), "split_a": (2, 1, 3), "split_b": (3, 1, 0), "one_shared": (2, 4, 5), "none_shared": (3, 4, 5)}
DEGENERATES = ("duplicate", "coplanar_overlap", "collinear", "repeated_index", "point", "sliver")
IMAGE_EXTENTS = ((1, 1), (1, 9), (9, 1), (7, 13), (16, 16))  # (height, width)
# (option, value): each is rendered against the defaults (lds_materials, answer_last_rays, cull_terminal, leaf_pairs, wide_bvh = 1, bvh_builder = 0)
OPTIONS = (("lds_materials", 0), ("answer_last_rays", 0), ("cull_terminal", 0), ("leaf_pairs", 0), ("wide_bvh", 0), ("wide_bvh", 3), ("bvh_builder", 1))
DEFAULTS = {"lds_materials": 1, "answer_last_rays": 1, "cull_terminal": 1, "leaf_pairs": 1, "wide_bvh": 1, "bvh_builder": 0}
LAYOUT_OPTIONS = ("wide_bvh", "bvh_builder")  # read at the next upload


class Fatal(Exception):
    """An error that is not a refusal of arguments: the run ends here and launches nothing more."""


_HALTED = []


# ---------------------------------------------------------------------------------------------------------------------------
# the plan: every random number of a case
# ---------------------------------------------------------------------------------------------------------------------------
def _value(rng, edges=EDGES):
    return float(edges[int(rng.integers(len(edges)))]) if rng.integers(2) else float(F32(rng.uniform(0, 1)))


def _material(rng, emission=None):
    base = [_value(rng, [0.0, 1.0, 0.5]) for _ in range(3)]
    how = int(rng.integers(6))
    if how == 0: base = [0.0, 0.0, 0.0]  # black
    elif how == 1: base[int(rng.integers(3))] = 0.0  # black in one channel
    if emission is None:
        emission = float(rng.choice([0.0, 0.0, 0.0, 0.0, -1.0, -0.25]))  # (an emitter is placed on purpose: the light count is a dimension of its own)
    return dict(base=base, emission=emission, params=[_value(rng) for _ in range(7)],  # metallic, roughness, anisotropic, subsurface, clearcoat, clearcoat_gloss, transmission
                eta=float(ETAS[int(rng.integers(len(ETAS)))]), images={}, alpha=None, bump_strength=1.0)


def _specular_material(rng):
    """A material on the thresholds themselves: metallic or transmission around 0.999, roughness around 1e-2."""
    m = _material(rng, emission=0.0)
    m["base"] = [0.8, 0.7, 0.9]
    m["params"][0 if rng.integers(2) else 6] = float(T999[int(rng.integers(3))])
    m["params"][1] = float(T01[int(rng.integers(3))])
    return m


def _transform(rng, where=1.2):
    s = [float(np.exp(rng.uniform(np.log(0.02), np.log(2.0)))) if rng.integers(4) == 0 else float(rng.uniform(0.3, 1.2)) for _ in range(3)]
    return dict(t=[float(x) for x in rng.uniform(-where, where, 3)], ry=float(rng.uniform(-3, 3)), rx=float(rng.uniform(-1, 1)) if rng.integers(2) else 0.0, s=s,
                shear=float(rng.uniform(-0.5, 0.5)) if rng.integers(3) == 0 else 0.0, mirror=bool(rng.integers(3) == 0))


def _mesh(rng):
    kind = str(rng.choice(["soup", "soup", "grid", "grid", "single", "pair"]))
    m = dict(kind=kind, seed=int(rng.integers(1 << 30)), degenerate=[], normals=str(rng.choice(["geometric", "random", "random", "zero", "opposed"])),
             uvs=str(rng.choice(["wide", "wide", "equal", "unit"])), stride=int(rng.choice([2, 4])))
    if kind == "soup":
        m["n"] = int(rng.choice([1, 2, 3, 7, 20, 40])) if rng.integers(2) else int(rng.integers(1, 41))
    elif kind == "grid":
        m["nu"], m["nv"] = int(rng.integers(1, 5)), int(rng.integers(1, 6))  # at most 4 x 5 quads = 40 triangles
    elif kind == "pair":
        m["pattern"] = str(rng.choice(sorted(PAIRS)))
    if kind in ("soup", "grid") and rng.integers(2):
        m["degenerate"] = [str(d) for d in rng.choice(DEGENERATES, size=int(rng.integers(1, 4)), replace=False)]
    return m


def _image(rng, role, as_bytes, crossing):
    """role: "base", "params" (metallic / roughness in r / g), "lobes" (transmission in b), "normal", "emission", "environment"."""
    h, w = IMAGE_EXTENTS[int(rng.integers(len(IMAGE_EXTENTS)))]
    if role == "environment": h, w, as_bytes = int(rng.choice([2, 4, 8])), int(rng.choice([4, 8, 16])), False  # (an 8-bit environment is refused at render)
    if as_bytes and (h, w) not in ((1, 1), (16, 16)): h, w = ((1, 1), (16, 16))[int(rng.integers(2))]  # the oracle knows float images: 8-bit ones must be mip-exact
    return dict(h=h, w=w, bytes=bool(as_bytes), role=role, crossing=bool(crossing), seed=int(rng.integers(1 << 30)))


def plan(seed):
    """The case `seed`: a plain description (dicts, lists, numbers, strings) with everything make_scene and run_case need."""
    seed = int(seed)
    rng = np.random.default_rng(seed)
    kind, shape, lights, pad = KINDS[seed % len(KINDS)], SHAPES[seed % len(SHAPES)], LIGHTS[seed % len(LIGHTS)], PADS[seed % len(PADS)]
    # a scene of the plain k_shade instantiation (no images, spheres, environment or media): the only one that consults the
    # emitter-bounds table, so the counts around its size come with it every other time
    plain = lights in (15, 16, 17) and seed % 2 == 0 and kind == "room"
    textured = seed % 3 == 0 and pad is None and not plain  # (the table's size matters to the untextured instantiations only)
    medium = None
    if kind == "room" and not plain and rng.integers(4) == 0:
        medium = dict(anisotropy=float(ANISOTROPIES[int(rng.integers(len(ANISOTROPIES)))]) if rng.integers(3) else float(rng.choice([0.0, 0.5, -0.4])), density=[float(x) for x in rng.uniform(1, 8, 3)],
                      t=[float(x) for x in rng.uniform(-0.3, 0.3, 3)], s=float(rng.uniform(0.5, 1.0)))
    environment = None
    if lights == 0 or (not plain and rng.integers(5) == 0):
        environment = dict(value=[float(x) for x in rng.uniform(0.3, 1.5, 3)], image=None)
    materials, images, masks, meshes, instances, spheres = [], [], [], [], [], []

    def add_material(m):
        materials.append(m)
        return len(materials) - 1

    def add_image(role, crossing=False):
        images.append(_image(rng, role, as_bytes=bool(rng.integers(3) == 0), crossing=crossing))
        return len(images) - 1

    def surface():
        m = _specular_material(rng) if rng.integers(4) == 0 else _material(rng)
        if textured:
            if rng.integers(3) == 0: m["images"]["base"] = add_image("base")
            if rng.integers(3) == 0:
                # constants of 1 under an image: value * texel is the texel, which crosses the thresholds for some texels or for none
                m["images"]["params"] = add_image("params", crossing=bool(rng.integers(2)))
                m["params"][0], m["params"][1] = 1.0, 1.0
            if rng.integers(4) == 0:
                m["images"]["lobes"] = add_image("lobes", crossing=bool(rng.integers(2)))
                m["params"][6] = 1.0
                m["eta"] = 1.5  # (eta is the constant times the texel's alpha, which the lobes image leaves at one)
            if rng.integers(4) == 0:
                m["images"]["bump"] = add_image("normal")
                m["bump_strength"] = float(rng.choice([1.0, 0.5, 2.0]))
            if rng.integers(4) == 0:
                masks.append(dict(h=int(rng.choice([1, 5, 7])), w=int(rng.choice([1, 5, 8])), bytes=bool(rng.integers(2)), seed=int(rng.integers(1 << 30))))
                m["alpha"] = len(masks) - 1
        return add_material(m)

    identity_all = shape == "all_identity"

    def place(mesh, material, xf, bake=False):
        instances.append(dict(mesh=mesh, material=material, xf=xf, bake=bool(bake or (identity_all and xf is not None))))

    if kind == "room":
        # a floor, three walls and a ceiling, open towards the camera; under "none_identity" they are moved by a hair too
        hair = dict(t=[0.0, 0.0, -0.01], ry=0.0, rx=0.0, s=[1.0, 1.0, 1.0], shear=0.0, mirror=False) if shape == "none_identity" else None
        for wall in ("floor", "back", "left", "right", "ceiling"):
            meshes.append(dict(kind="wall", wall=wall))
            place(len(meshes) - 1, surface(), hair)
        first = len(meshes)
        for _ in range(int(rng.integers(1, 9))):
            meshes.append(_mesh(rng))
        for mesh in range(first, len(meshes)):
            for _ in range(int(rng.integers(1, 3))):
                at_identity = shape == "mix" and rng.integers(3) == 0
                place(mesh, surface(), None if at_identity else _transform(rng), bake=shape == "one_moved")
        if shape == "one_moved":
            instances[-1]["bake"] = False
        if shape in ("many_64", "many_65"):  # one mesh many times
            m = surface()
            for k in range(int(shape[5:])):
                place(first, m if k % 3 else surface(), dict(t=[-1.4 + 0.4 * (k % 8), -0.6 + 0.35 * (k // 8), -1.0 + 0.01 * k], ry=0.1 * k, rx=0.0, s=[0.25, 0.25, 0.25], shear=0.0, mirror=bool(k % 5 == 0)))
        for _ in range(0 if plain else int(rng.choice([0, 0, 1, 2, 3]))):
            spheres.append(dict(material=surface(), radius=float(rng.uniform(0.1, 0.5)), t=[float(x) for x in rng.uniform(-1, 1, 3)]))
    elif kind == "spheres_only":
        for _ in range(int(rng.integers(1, 4))):
            spheres.append(dict(material=surface(), radius=float(rng.uniform(0.2, 0.6)), t=[float(x) for x in rng.uniform(-0.8, 0.8, 3)]))
    else:  # one triangle
        meshes.append(dict(kind="single", seed=int(rng.integers(1 << 30)), degenerate=[], normals="geometric", uvs="unit", stride=4))
        place(0, surface(), dict(t=[0.0, 0.2, 0.0], ry=0.0, rx=0.0, s=[3.0, 3.0, 3.0], shear=0.0, mirror=False) if shape != "all_identity" else None)
    # the emitters: small lamps under the ceiling, instances of one mesh, and up to two emissive spheres beside them
    if kind != "room":
        lights = min(lights, 2)
        if lights == 0 or kind == "one_triangle":
            environment = environment or dict(value=[0.8, 0.9, 1.1], image=None)
    emissive_spheres = 0 if (plain or lights < 2) else int(rng.integers(0, 3))
    if kind == "spheres_only": emissive_spheres = lights
    if kind == "one_triangle": lights = emissive_spheres = 0
    lamp = None
    if lights - emissive_spheres > 0:
        meshes.append(dict(kind="lamp"))
        lamp = len(meshes) - 1
    glow = _material(rng, emission=float(rng.choice([4.0, 10.0, 25.0])))
    glow["base"], glow["eta"] = [1.0, 0.9, 0.8], 0.0
    if textured and lights and rng.integers(2): glow["images"]["base"] = add_image("emission")  # an emissive textured material
    glow = add_material(glow) if lights else None
    side = int(np.ceil(np.sqrt(max(1, lights - emissive_spheres))))
    for k in range(lights - emissive_spheres):
        step = 3.0 / side
        place(lamp, glow, dict(t=[-1.5 + (k % side + 0.5) * step, 2.9 - 0.01 * k, -1.5 + (k // side + 0.5) * step], ry=0.3 * k, rx=0.0, s=[1.0, 1.0, 1.0], shear=0.0, mirror=False), bake=shape == "one_moved")
    for k in range(emissive_spheres):
        spheres.append(dict(material=glow, radius=0.12, t=[-0.9 + 0.9 * k, 1.6, 0.4] if kind == "room" else [-0.5 + 1.0 * k, 1.2, 0.5]))
    if environment is not None and textured and rng.integers(2):
        environment["image"] = add_image("environment")
    motion = int(rng.integers(1 << 30)) if rng.integers(4) == 0 else None  # motion transforms that differ from the current ones
    # the frame: at most 72 x 40 x 2 seeds, flags and limits drawn as fuzz_sequences.py draws them (fuzz_parity.run's, steered
    # away from what both sides reject)
    W, H = int(rng.integers(2, 10)) * 8, int(rng.integers(2, 11)) * 4
    if rng.integers(3) == 0: W, H = min(72, W + int(rng.integers(1, 8))), min(40, H + int(rng.integers(1, 4)))
    bundle, args = fuzz_sequences._bundle_args(rng, W, H, medium is not None, environment is not None, False)
    if masks and rng.integers(2) and "alphatest" not in args["bdptFlag"]: args["bdptFlag"].append("alphatest")
    args = {k: (list(v) if isinstance(v, list) else int(v)) for k, v in args.items()}
    view = str(rng.choice(["mono", "mono", "mono", "stereo", "moved"]))
    frame = dict(W=W, H=H, seed0=int(rng.integers(0, 1000)), seeds=int(rng.integers(1, 3)), view=view, moved=[float(x) for x in rng.uniform(-0.1, 0.1, 3)])
    # two or three execution options, of those that act on this scene (include/sthip.h says where each is ignored)
    has_spheres, media, env = bool(spheres), medium is not None, environment is not None
    usable = [o for o in OPTIONS if not (
        (o[0] == "lds_materials" and textured) or (o[0] == "answer_last_rays" and (textured or has_spheres or media or env)) or (o[0] == "leaf_pairs" and (masks or media))
        or (o[0] == "bvh_builder" and (has_spheres or media or not instances)))]
    order = [usable[int(i)] for i in rng.permutation(len(usable))][: int(rng.integers(2, 4))]
    return dict(seed=seed, kind=kind, shape=shape, lights=lights, emissive_spheres=emissive_spheres, pad=pad, plain=plain, textured=textured, medium=medium, environment=environment, materials=materials,
                images=images, masks=masks, meshes=meshes, instances=instances, spheres=spheres, motion=motion, bundle=bundle, args=args, frame=frame, options=[list(o) for o in order],
                rays=dict(seed=int(rng.integers(1 << 30)), n=1500, alpha=bool(masks and rng.integers(2))))


def describe(p):
    f = p["frame"]
    return ("scene %d: %s %s, %d meshes, %d instances, %d spheres, %d materials, %d images, %d masks, %d emitters (%d spheres), pad %s, medium %s, environment %s, motion %s; %dx%d seeds %d+%d %s %s %s; "
            "options %s" % (p["seed"], p["kind"], p["shape"], len(p["meshes"]), len(p["instances"]), len(p["spheres"]), len(p["materials"]), len(p["images"]), len(p["masks"]), p["lights"],
                            p["emissive_spheres"], p["pad"], p["medium"] and p["medium"]["anisotropy"], p["environment"] and ("image" if p["environment"]["image"] is not None else "constant"),
                            p["motion"] is not None, f["W"], f["H"], f["seed0"], f["seeds"], f["view"], p["bundle"], p["args"], p["options"]))


def identity_count(p):
    """(triangle instances at the identity, triangle instances): the three shapes traverse.h tells apart."""
    return sum(i["xf"] is None or i["bake"] for i in p["instances"]), len(p["instances"])


def table_bytes(p):
    """The size of gMaterialData the plan asks for: the surface records (padded), the medium's 40 bytes, the environment's 16 or 32."""
    used = len({i["material"] for i in p["instances"]} | {s["material"] for s in p["spheres"]})
    n = max(used, p["pad"] or 0)
    env = p["environment"]
    return n * RECORD + (MEDIUM_RECORD if p["medium"] else 0) + (0 if env is None else 32 if env["image"] is not None else 16)


# ---------------------------------------------------------------------------------------------------------------------------
# the scene of a plan
# ---------------------------------------------------------------------------------------------------------------------------
def matrix(xf):
    if xf is None:
        return np.eye(4)
    s = np.array(xf["s"], np.float64)
    if xf["mirror"]: s[0] = -s[0]
    shear = np.eye(4)
    shear[0, 1] = xf["shear"]
    return translate(tuple(xf["t"])) @ rotate_y(xf["ry"]) @ rotate_x(xf["rx"]) @ shear @ scale(tuple(s))


def _geometric_normals(pos, tri):
    n = np.zeros_like(pos, dtype=np.float64)
    for a, b, c in tri:
        g = np.cross(pos[b].astype(np.float64) - pos[a], pos[c].astype(np.float64) - pos[a])
        length = np.linalg.norm(g)
        g = g / length if length > 0 else np.array([0.0, 1.0, 0.0])
        for v in (a, b, c):
            if not n[v].any(): n[v] = g
    n[~n.any(axis=1)] = (0.0, 1.0, 0.0)
    return n


_WALLS = {"floor": ((-2, -1, -2), (2, -1, -2), (2, -1, 2), (-2, -1, 2), (0, 1, 0)), "back": ((-2, -1, -2), (-2, 3, -2), (2, 3, -2), (2, -1, -2), (0, 0, 1)),
          "left": ((-2, -1, -2), (-2, -1, 2), (-2, 3, 2), (-2, 3, -2), (1, 0, 0)), "right": ((2, -1, -2), (2, 3, -2), (2, 3, 2), (2, -1, 2), (-1, 0, 0)),
          "ceiling": ((-2, 3, -2), (-2, 3, 2), (2, 3, 2), (2, 3, -2), (0, -1, 0))}


def mesh_arrays(m):
    """(positions, normals, uvs, triangles, index stride) of a planned mesh."""
    quad_uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    if m["kind"] == "wall":
        p0, p1, p2, p3, n = _WALLS[m["wall"]]
        return np.array([p0, p1, p2, p3], np.float32), np.tile(np.array(n, np.float32), (4, 1)), quad_uv, np.array([[0, 1, 2], [0, 2, 3]]), 4
    if m["kind"] == "lamp":
        pos = np.array([(-0.08, 0, -0.08), (0.08, 0, -0.08), (0.08, 0, 0.08), (-0.08, 0, 0.08)], np.float32)
        return pos, np.tile(np.array((0, -1, 0), np.float32), (4, 1)), quad_uv, np.array([[0, 1, 2], [0, 2, 3]]), 4
    rng = np.random.default_rng(m["seed"])
    if m["kind"] == "soup":
        n = m["n"]
        pos = (rng.uniform(-0.35, 0.35, (n, 1, 3)) + rng.uniform(-0.25, 0.25, (n, 3, 3))).reshape(-1, 3)
        tri = np.arange(3 * n).reshape(n, 3)
    elif m["kind"] == "grid":
        nu, nv = m["nu"], m["nv"]
        u, v = np.meshgrid(np.linspace(-0.5, 0.5, nu + 1), np.linspace(-0.5, 0.5, nv + 1), indexing="ij")
        pos = np.stack([u, 0.12 * rng.normal(size=u.shape), v], -1).reshape(-1, 3)
        idx = np.arange((nu + 1) * (nv + 1)).reshape(nu + 1, nv + 1)
        a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
        tri = np.stack([np.stack([a, b, c], -1), np.stack([a, c, d], -1)], axis=2).reshape(-1, 3)  # shared edges: fans and strips
    elif m["kind"] == "single":
        pos = np.array([(-0.4, -0.3, 0.0), (0.4, -0.3, 0.1), (0.0, 0.4, -0.1)]) + rng.uniform(-0.05, 0.05, (3, 3))
        tri = np.array([[0, 1, 2]])
    else:  # "pair": B beside A = (p0, p1, p2) in each of the patterns build_leaf_pairs tells apart
        pos = np.array([(-0.4, -0.4, 0.0), (0.4, -0.4, 0.0), (0.4, 0.4, 0.0), (-0.4, 0.4, 0.0), (0.5, 0.1, 0.2), (0.1, 0.6, 0.2)]) + rng.uniform(-0.05, 0.05, (6, 3))
        tri = np.array([(0, 1, 2), PAIRS[m["pattern"]]])
        pos = pos[: tri.max() + 1]
    pos = pos.astype(np.float32)
    extra_pos, extra_tri = [], []

    def corners(t):
        return [pos[i].astype(np.float64) for i in tri[t % tri.shape[0]]]

    for k, what in enumerate(m["degenerate"]):
        a, b, c = corners(k)
        base = pos.shape[0] + 3 * len(extra_tri)
        if what == "duplicate": new = [a, b, c]  # the same triangle again: the tie goes by id
        elif what == "coplanar_overlap": new = [a + 0.3 * (b - a), b + 0.3 * (b - a), c + 0.3 * (b - a)]
        elif what == "collinear": new = [a, b, a + 0.25 * (b - a)]  # three points on a line
        elif what == "point": new = [a, a, a]
        elif what == "sliver": new = [a, b, 0.5 * (a + b) + 1e-6 * (c - a)]
        else: new = [a, b, c]  # "repeated_index": two corners are one vertex
        extra_pos += new
        extra_tri.append((base, base, base + 1) if what == "repeated_index" else (base, base + 1, base + 2))
    if extra_tri:
        pos = np.concatenate([pos, np.array(extra_pos, np.float32)])
        tri = np.concatenate([tri, np.array(extra_tri)])
    geometric = _geometric_normals(pos, tri)
    if m["normals"] == "random":
        nrm = rng.normal(size=pos.shape)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    elif m["normals"] == "zero": nrm = np.zeros(pos.shape)
    elif m["normals"] == "opposed": nrm = -geometric
    else: nrm = geometric
    if m["uvs"] == "wide": uv = rng.uniform(-1, 2, (pos.shape[0], 2))  # outside [0, 1]
    elif m["uvs"] == "equal": uv = np.tile(rng.uniform(0, 1, (1, 2)), (pos.shape[0], 1))  # all equal: a degenerate uv Jacobian
    else: uv = rng.uniform(0, 1, (pos.shape[0], 2))
    return pos, nrm.astype(np.float32), uv.astype(np.float32), tri, m["stride"]


def image_array(im):
    """The texels of a planned image: float32 (H, W, 4) in [0, 1], or uint8."""
    rng = np.random.default_rng(im["seed"])
    h, w, role = im["h"], im["w"], im["role"]
    if im["bytes"]:
        if (h, w) == (16, 16):
            return np.ascontiguousarray(mip_exact_image(16, 20 + im["seed"] % 4).astype(np.uint8))  # (a few of them, made once each)
        a = rng.choice(np.array(BYTE_TEXELS if im["crossing"] else [64, 128, 200], np.uint8), size=(h, w, 4))
        if role in ("lobes", "base", "emission"): a[..., 3] = 255
        if role == "normal": a = rng.integers(96, 160, (h, w, 4)).astype(np.uint8); a[..., 2] = 255
        return np.ascontiguousarray(a)
    if role in ("params", "lobes"):
        pool = np.array([0.5, 1.0] + T999 + T01 if im["crossing"] else [0.25, 0.5, 0.75, 0.9], np.float32)  # texels on both sides of the thresholds, or on one
        a = rng.choice(pool, size=(h, w, 4))
        if role == "lobes": a[..., 3] = 1.0
    elif role == "normal":
        a = np.concatenate([rng.uniform(0.35, 0.65, (h, w, 2)), np.ones((h, w, 2))], -1)
    elif role == "environment":
        a = np.concatenate([rng.uniform(0.2, 2.0, (h, w, 3)), np.ones((h, w, 1))], -1)
    else:
        a = np.concatenate([rng.uniform(0.0, 1.0, (h, w, 3)), np.ones((h, w, 1))], -1)
    return np.ascontiguousarray(a, np.float32)


def mask_array(mk):
    rng = np.random.default_rng(mk["seed"])
    a = rng.choice(np.array([0, 64, 190, 191, 192, 193, 255], np.uint8), size=(mk["h"], mk["w"]))  # around the 0.75 of the alpha test
    return np.ascontiguousarray(a if mk["bytes"] else a.astype(np.float32) / np.float32(255))


def pad_materials(sc, records, seed=0):
    """Unused 72-byte records behind the surface records of a built scene, up to `records` of them: the medium records and the
    environment record move back, and the instances and the scene that name them follow."""
    types = sc.instances["packed"][:, 0] & 0xF
    surface = types != wire.INSTANCE_TYPE_VOLUME
    end = int((sc.instances["packed"][surface, 0] >> 4).max()) + RECORD if surface.any() else 0
    extra = records - end // RECORD
    if extra <= 0:
        return sc
    rng = np.random.default_rng(seed)
    fill = np.zeros(extra, wire.MaterialRecord)
    fill["values"]["value"] = rng.uniform(0, 1, fill["values"]["value"].shape).astype(np.float32)
    fill["values"]["image_index"], fill["alpha_mask_index"], fill["bump_index"], fill["bump_strength"] = 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1.0
    sc.materials = np.ascontiguousarray(np.concatenate([sc.materials[:end], fill.view(np.uint8).reshape(-1), sc.materials[end:]]))
    shift = extra * RECORD
    for i in np.nonzero(~surface)[0]:
        sc.instances["packed"][i, 0] = (int(sc.instances["packed"][i, 0]) + (shift << 4)) & 0xFFFFFFFF
    if sc.environment_address != 0xFFFFFFFF:
        sc.environment_address += shift
    return sc


def make_scene(p):
    """(scene, camera) of a plan, through SceneBuilder."""
    b = SceneBuilder("generated_%d" % p["seed"])
    images = [b.add_image(image_array(im)) for im in p["images"]]
    masks = [b.add_image1(mask_array(mk)) for mk in p["masks"]]
    handles = []
    for m in p["materials"]:
        q = m["params"]
        h = b.add_material(tuple(m["base"]), emission=m["emission"], metallic=q[0], roughness=q[1], anisotropic=q[2], subsurface=q[3], clearcoat=q[4], clearcoat_gloss=q[5], transmission=q[6], eta=m["eta"])
        im = {k: images[v] for k, v in m["images"].items()}
        if im:
            b.set_material_images(h, base_color_image=im.get("base"), params_image=im.get("params"), lobes_image=im.get("lobes"), bump_image=im.get("bump"), bump_strength=m["bump_strength"])
        if m["alpha"] is not None:
            b.set_material_alpha_mask(h, masks[m["alpha"]])
        handles.append(h)
    arrays, plain_mesh = {}, {}
    for i in p["instances"]:
        k = i["mesh"]
        if k not in arrays: arrays[k] = mesh_arrays(p["meshes"][k])
        pos, nrm, uv, tri, stride = arrays[k]
        if i["bake"] and i["xf"] is not None:  # the transform goes into the vertices: a mesh of its own at the identity
            m = matrix(i["xf"])
            n = nrm.astype(np.float64) @ np.linalg.inv(m[:3, :3])  # (inverse transpose, as a row vector product)
            length = np.linalg.norm(n, axis=1, keepdims=True)
            n = np.where(length > 0, n / np.where(length > 0, length, 1.0), 0.0)
            t = tri[:, ::-1] if np.linalg.det(m[:3, :3]) < 0 else tri
            b.add_instance(b.add_mesh((pos.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32), n.astype(np.float32), uv, t, index_stride=stride), handles[i["material"]])
            continue
        if k not in plain_mesh: plain_mesh[k] = b.add_mesh(pos, nrm, uv, tri, index_stride=stride)
        b.add_instance(plain_mesh[k], handles[i["material"]], None if i["xf"] is None else matrix(i["xf"]))
    for s in p["spheres"]:
        b.add_sphere(handles[s["material"]], s["radius"], translate(tuple(s["t"])))
    if p["medium"]:
        md = p["medium"]
        b.add_medium(b.add_volume(fuzz_parity.FOG), density_scale=tuple(md["density"]), albedo_scale=(0.9, 0.9, 0.9), anisotropy=md["anisotropy"], transform=translate(tuple(md["t"])) @ scale((md["s"],) * 3))
    if p["environment"]:
        env = p["environment"]
        b.set_environment(tuple(env["value"]), None if env["image"] is None else images[env["image"]])
    sc = b.build()
    if p["pad"]:
        pad_materials(sc, p["pad"], p["seed"])
    if p["motion"] is not None:
        m = sc.motion_transforms["m"]
        m += np.random.default_rng(p["motion"]).normal(scale=0.02, size=m.shape).astype(np.float32)
    return sc, dict(CAM)


def frame_of(p, cam=CAM):
    f = p["frame"]
    if f["view"] == "stereo":
        return camera.Frame.stereo(f["W"], f["H"], cam["fovy"], cam["eye"], cam["target"], eye_separation=0.2)
    prev = None
    if f["view"] == "moved":
        prev = camera.Frame(f["W"], f["H"], cam["fovy"], tuple(np.asarray(cam["eye"], np.float64) + np.asarray(f["moved"])), cam["target"])
    return camera.Frame(f["W"], f["H"], cam["fovy"], cam["eye"], cam["target"], prev=prev)


# ---------------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------------
def is_refusal(e):
    """A StratumHipError that refuses arguments (STHIP_ERR_INVALID_ARGUMENT, STHIP_ERR_UNSUPPORTED); anything else is fatal."""
    m = re.search(r"failed \((-?\d+)\)", str(e))
    return bool(m) and int(m.group(1)) in (-1, -4)


def guarded(what, p, call):
    """`call()`; None where the library refuses its arguments. Any other error of the library halts this process's runs."""
    if _HALTED:
        raise Fatal("an earlier case ended with an error of the library (%s): nothing more is launched" % _HALTED[0])
    try:
        return call()
    except StratumHipError as e:
        if is_refusal(e):
            return None
        _HALTED.append(str(e))
        raise Fatal("%s: %s\n  %s" % (what, e, describe(p)))


def same_frames(a, b):
    """Two frames of the device, bit for bit, ray counts included."""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in ("radiance", "albedo", "prev_uv", "visibility", "depth", "ray_count"))


def frame_difference(got, ref):
    """Which outputs of two frames differ, in how many pixels, and the first radiance pixel that does."""
    parts = []
    for k in ("radiance", "albedo", "prev_uv", "visibility", "depth"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        d = (a.view(np.uint8).reshape(a.shape[0], a.shape[1], -1) != b.view(np.uint8).reshape(b.shape[0], b.shape[1], -1)).any(axis=-1)
        if d.any():
            parts.append("%s in %d pixels" % (k, int(d.sum())))
            if k == "radiance":
                y, x = (int(v[0]) for v in np.nonzero(d))
                parts.append("first (%d, %d): %s vs %s, hit %08x" % (x, y, got[k][y, x].tolist(), ref[k][y, x].tolist(), int(ref["visibility"]["instance_primitive_index"][y, x])))
    return "; ".join(parts) or "the images are equal"


def compare_rays(r, orc, sc, rays, style, lo, hi, alpha=False, threads=THREADS):
    """Closest hit and any hit of the device against the oracle's brute force, bit for bit; the one exemption is the one
    fuzz_parity.run_rays makes (spurious brute-force hits from far origins, which no acceleration structure finds: allowed when the
    device agrees with the oracle's own traversal and every such hit point lies far outside the scene). Returns the rays that differ.
    r = None: the oracle's own traversal stands in for the device (--dry: the oracle's BVH against its brute force, by the same rule)."""
    fields = ("instance_primitive_index", "t", "b1", "b2")
    ref, _ = orc.trace(rays, brute=True, alpha_test=alpha, threads=threads)
    ra = orc.trace(rays, any_hit=True, brute=True, alpha_test=alpha, threads=threads)[0]["instance_primitive_index"] != wire.MISS

    def traversal():
        return orc.trace(rays, alpha_test=alpha, threads=threads)[0], orc.trace(rays, any_hit=True, alpha_test=alpha, threads=threads)[0]["instance_primitive_index"] != wire.MISS

    if r is None:
        got, ga = traversal()
    else:
        got = r.trace(rays, alpha_test=alpha)
        ga = r.trace(rays, any_hit=True, alpha_test=alpha)["instance_primitive_index"] != wire.MISS
    differ = np.zeros(rays.shape[0], bool)
    for f in fields:
        differ |= got[f].view(np.uint32) != ref[f].view(np.uint32)
    differ |= ga != ra
    w = np.nonzero(differ)[0]
    if not w.size:
        return w
    rbvh, rb = (got, ga) if r is None else traversal()
    agree = all(np.array_equal(got[f].view(np.uint32), rbvh[f].view(np.uint32)) for f in fields) and np.array_equal(ga, rb)
    hp = rays["origin"][w].astype(np.float64) + ref["t"][w].astype(np.float64)[:, None] * rays["direction"][w].astype(np.float64)
    wlo, whi = lo - 3 * (hi - lo) - 20.0, hi + 3 * (hi - lo) + 20.0
    outside = ((hp < wlo) | (hp > whi)).any(axis=1) | ~np.isfinite(hp).all(axis=1)
    if agree and outside.all() and (style[w] == 6).all():
        print("  (%d spurious contract hit(s) from far origins: brute force only%s)" % (w.size, "" if r is None else "; HIP == the oracle's BVH traversal"))
        return w[:0]
    return w


class Runner:
    """One context (or none: gpu=False runs the oracle alone) for the cases of a run."""

    def __init__(self, gpu=True, threads=THREADS):
        self.gpu, self.threads = gpu, threads
        self.r = BDPT(0) if gpu else fuzz_sequences._Dry()
        self.compared = self.rejected = self.bad = 0

    def close(self):
        self.r.close()

    def mismatch(self, p, text):
        self.bad += 1
        print("MISMATCH %s\n  %s" % (text, describe(p)), flush=True)
        return "bad"

    def run_case(self, p, scene=None):
        """One case. Returns a dict: outcome ("compared", "rejected", "bad"), and what the oracle said on its own: `finite`
        (its radiance), `bvh_equals_brute` (its traversal against its brute force on the case's rays), `ray_count`, `instances_seen`."""
        r = self.r
        sc, cam = scene or make_scene(p)
        fr = frame_of(p, cam)
        f = p["frame"]
        out = dict(outcome="bad", finite=None, bvh_equals_brute=None, ray_count=None, instances_seen=0)
        try:
            orc = oracle_py.OracleScene(fuzz_sequences.float_form(sc))
        except RuntimeError:
            orc = None
        def set_options(settings):
            """Every execution option to its value; the ones the library refuses (an option left at another value would make the
            render under it compare equal for nothing)."""
            return ["%s = %d" % (k, v) for k, v in settings.items() if guarded("set_option", p, lambda: r.set_option(k, v) or True) is None]

        try:
            r.set_args(p["args"])
            if self.gpu:
                refused = set_options(DEFAULTS)
                if refused:
                    return dict(out, outcome=self.mismatch(p, "set_option refuses %s" % ", ".join(refused)))
            up = guarded("upload", p, lambda: r.update(sc) or True)
            if orc is None or up is None:
                if orc is None and (up is None or not self.gpu):
                    self.rejected += 1
                    return dict(out, outcome="rejected")
                return dict(out, outcome=self.mismatch(p, "upload: %s refuses, %s accepts" % (("the oracle", "GPU") if orc is None else ("GPU", "the oracle"))))
            try:
                ref = orc.render(fr, r.push_constants(fr), r.mSamplingFlags, f["seed0"], f["seeds"], threads=self.threads)
            except RuntimeError:
                ref = None
            got = guarded("render", p, lambda: r.render(fr, f["seed0"], f["seeds"])) if self.gpu else ref
            if ref is None or got is None:
                if ref is None and got is None:
                    self.rejected += 1
                    return dict(out, outcome="rejected")
                return dict(out, outcome=self.mismatch(p, "render: %s refuses, %s accepts" % (("the oracle", "GPU") if ref is None else ("GPU", "the oracle"))))
            self.compared += 1
            seen = ref["visibility"]["instance_primitive_index"]
            out.update(finite=bool(np.isfinite(ref["radiance"]).all()), ray_count=[int(x) for x in ref["ray_count"]], instances_seen=int(np.unique(seen[seen != wire.MISS] & 0xFFFF).size))
            rays, style, lo, hi = fuzz_parity.awkward_rays(np.random.default_rng(p["rays"]["seed"]), sc, p["rays"]["n"])
            alpha = p["rays"]["alpha"] and bool(sc.images1)
            if not self.gpu:  # the oracle's traversal against its brute force: closest and any hit, the exemption of run_rays alone
                out["bvh_equals_brute"] = compare_rays(None, orc, sc, rays, style, lo, hi, alpha, self.threads).size == 0
                if not (out["finite"] and out["bvh_equals_brute"]):
                    return dict(out, outcome=self.mismatch(p, "the oracle alone: radiance finite %s, its traversal equals its brute force %s" % (out["finite"], out["bvh_equals_brute"])))
                return dict(out, outcome="compared")
            flags = p["args"]["bdptFlag"]
            ok = fuzz_parity.compare_frames(got, dict(ref), f["W"], f["H"], 0, 1, "connecttoviews" in flags or "connecttolightpaths" in flags)
            if not ok:
                self.mismatch(p, "frame: %s, rays %s vs %s" % (frame_difference(got, ref), got["ray_count"], ref["ray_count"]))
            # the same frame under execution options that must change nothing, one at a time against the defaults
            resident = dict(DEFAULTS)
            for name, value in p["options"]:
                settings = dict(DEFAULTS, **{name: value})
                refused = set_options(settings)
                if refused:  # (the plan draws only options that act on its scene: the library has no reason to refuse one)
                    self.mismatch(p, "set_option refuses %s" % ", ".join(refused))
                    ok = False
                    continue
                if any(settings[k] != resident[k] for k in LAYOUT_OPTIONS):
                    if guarded("upload under %s = %d" % (name, value), p, lambda: r.update(sc) or True) is None:
                        self.mismatch(p, "%s = %d: the upload is refused" % (name, value))
                        ok, resident = False, None
                        break
                    resident = settings
                again = guarded("render under %s = %d" % (name, value), p, lambda: r.render(fr, f["seed0"], f["seeds"]))
                if again is None or not same_frames(again, got):
                    self.mismatch(p, "%s = %d: %s" % (name, value, "the render is refused" if again is None else "the frame or its ray counts differ from the first render's (rays %s vs %s)" % (again["ray_count"], got["ray_count"])))
                    ok = False
            if resident is None or any(resident[k] != DEFAULTS[k] for k in LAYOUT_OPTIONS):
                if set_options(DEFAULTS) or guarded("upload", p, lambda: r.update(sc) or True) is None:
                    self.mismatch(p, "the defaults are refused after the options")
                    return dict(out, outcome="bad")
            w = guarded("trace", p, lambda: compare_rays(r, orc, sc, rays, style, lo, hi, alpha, self.threads))
            if w is None or w.size:
                self.mismatch(p, "rays (alpha %s): %s" % (alpha, "refused" if w is None else "%d differ, styles %s" % (w.size, np.unique(style[w]))))
                ok = False
            return dict(out, outcome="compared" if ok else "bad")
        finally:
            if orc is not None: orc.close()


def run(cases=60, seed=1, gpu=True, only=None, trace=False):
    """Cases seed * 100000 + k, k < cases. Returns (compared, rejected, bad)."""
    lo, hi = only if only else (0, cases - 1)
    runner = Runner(gpu)
    t0 = time.time()
    try:
        for k in range(cases):
            if not lo <= k <= hi:
                continue
            p = plan(seed * 100000 + k)
            if trace: print("CASE %d: %s" % (k, describe(p)), flush=True)
            runner.run_case(p)
    finally:
        runner.close()
    print("%d cases compared, %d rejected on both sides, %d mismatches, %.0f s" % (runner.compared, runner.rejected, runner.bad, time.time() - t0), flush=True)
    return runner.compared, runner.rejected, runner.bad


if __name__ == "__main__":
    argv = sys.argv[1:]
    only = None
    if "--only" in argv:
        k = argv.index("--only")
        a, _, b = argv[k + 1].partition("-")
        only = (int(a), int(b or a))
        del argv[k : k + 2]
    flags = {name: name in argv for name in ("--trace", "--dry")}
    argv = [a for a in argv if a not in flags]
    try:
        bad = run(int(argv[0]) if argv else 60, int(argv[1]) if len(argv) > 1 else 1, not flags["--dry"], only, flags["--trace"])[2]
    except Fatal as e:
        print("FATAL %s" % e, flush=True)
        sys.exit(2)
    sys.exit(1 if bad else 0)
