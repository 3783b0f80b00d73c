"""Long-lived contexts: tools/fuzz_sequences.py walks one BDPT(0) through uploads, transforms / vertex updates, rigs, option,
flag, frame, shard and precision changes, sync and async renders, ray batches, post calls and refused calls, and compares every
frame with the oracle on a host-side model of what the context should hold, bit for bit. Here: the committed seeds (their plans
are pinned by the coverage conditions below, checked without a GPU against the oracle alone), and the orders no other test
has, one test each, so that a failure names its sequence."""
import importlib.util
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (11, 12, 13, 14, 15, 16)
STEPS = 40


def _tool():
    if "fuzz_sequences" not in sys.modules:
        spec = importlib.util.spec_from_file_location("fuzz_sequences", os.path.join(ROOT, "tools", "fuzz_sequences.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["fuzz_sequences"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["fuzz_sequences"]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the plans of the committed seeds, run against the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dry_walks():
    fs = _tool()
    return {seed: fs.run_walk(seed, STEPS, gpu=False, threads=min(16, os.cpu_count() or 1)) for seed in SEEDS}


def test_a_seed_names_one_sequence(dry_walks):
    """The plan draws every random number, the run none: the same seed gives the same steps planned twice, and the steps a run
    (every step selected) went through are the planned ones, in order, whatever the steps did."""
    fs = _tool()
    for seed in SEEDS:
        a, b = fs.plan(seed, STEPS), fs.plan(seed, STEPS)
        assert len(a) == STEPS and [fs.describe(p) for p in a] == [fs.describe(p) for p in b]
        ran = [(i, kind, sub) for i, kind, sub, _ in dry_walks[seed].log if i < STEPS]
        assert ran == [(i, p["kind"], p.get("sub", p["kind"])) for i, p in enumerate(a)]
        cut = fs.run_walk(seed, STEPS, gpu=False, upto=12, drop=(3, 7))  # a walk cut down by hand keeps the steps it keeps
        assert [(i, kind, sub) for i, kind, sub, _ in cut.log if i < STEPS] == [r for r in ran if r[0] < 12 and r[0] not in (3, 7)]
    assert fs.plan(SEEDS[0], STEPS) != fs.plan(SEEDS[1], STEPS)


def test_the_committed_walks_cover_what_they_are_for(dry_walks):
    """Conditions on what the committed seeds DID, read from the walks' logs (an edit to the generator that thins the walks out
    fails here): a step that was skipped counts for nothing."""
    fs = _tool()
    kinds, followed, crossed, scenes_up, options, refusals = Counter(), Counter(), Counter(), Counter(), Counter(), Counter()
    shrinks = monos = compared = rejected = sharded = other_rank = debug = 0
    for seed in SEEDS:
        w = dry_walks[seed]
        steps = fs.plan(seed, STEPS)
        assert w.bad == 0
        frames = sum(1 for _, kind, _, outcome in w.log if kind in ("render", "async") and outcome == "compared")
        assert frames >= 10 and frames == w.compared == sum(f["outcome"] == "compared" for f in w.frames), (seed, frames)
        compared, rejected = compared + w.compared, rejected + w.rejected
        pending = None  # the last scene call, until the next one or a synchronous render
        for i, kind, sub, outcome in w.log:
            if outcome.startswith("skipped"):
                continue
            kinds[kind] += 1
            if i < STEPS and kind == "upload": scenes_up[steps[i]["scene"]] += 1
            if i < STEPS and kind == "option_now": options.update(name for name, _ in steps[i]["settings"])
            if i < STEPS and kind == "refused": refusals.update(steps[i]["forms"])
            call = sub if sub == "animate" else kind if kind in ("upload", "transforms", "vertices") else None
            if call and outcome.startswith("done"):
                pending = call
            elif kind == "render" and outcome == "compared" and pending:
                followed[pending] += 1
                pending = None
        for _, call in w.crossings:
            crossed[call] += 1
        done = sorted((f for f in w.frames if f["outcome"] == "compared"), key=lambda f: f["step"])  # in the order they were rendered
        sharded += sum(f["shard"][1] > 1 for f in done)
        other_rank += sum(f["shard"][0] > 0 for f in done)
        debug += sum(f["debug"] != 0 for f in done)
        for a, b in zip(done, done[1:]):  # a compared frame, a change of the frame, a compared frame, an estimator bundle on in both
            if a["bundle"] and b["bundle"]:
                shrinks += b["W"] * b["H"] < a["W"] * a["H"]
                monos += a["views"] == 2 and b["views"] == 1
    assert set(kinds) == set(fs.KINDS) and min(kinds.values()) >= 5, kinds
    for call in fs.SCENE_CALLS:
        assert followed[call] >= 3 and crossed[call] >= 2, (call, followed, crossed)
    assert shrinks >= 5 and monos >= 3, (shrinks, monos)
    assert rejected <= 0.15 * (compared + rejected), (compared, rejected)
    # the forms of a kind: frames on a shard through the owner map (some of them not rank 0), debug modes about one render in
    # five of the synchronous ones, every option that acts at once, every refusal, every scene
    assert sharded >= 12 and other_rank >= 4, (sharded, other_rank)
    assert debug >= 6, debug
    assert set(options) == set(fs.OPTIONS_NOW) and set(refusals) == set(fs.REFUSED_FORMS), (options, refusals)
    assert set(scenes_up) == set(fs.SCENE_KINDS), scenes_up


def test_the_model_keeps_the_rest_pose_of_set_rigs():
    """set_rigs, update_vertices over the rigged range, animate: the model's vertices are test_animate.apply of the pose to the
    rest pose taken at set_rigs, and the deformed records elsewhere."""
    from test_animate import apply, posed
    from test_refit import deformed

    fs = _tool()
    w = fs.Walk(gpu=False)
    try:
        w.step(0, upload("cornell"))
        original = w.sc.vertices.copy()
        w.step(1, set_rigs([5, 0], targets=[2, 1], bones=[3, 0]))
        assert len(w.rigs) == 2
        rests = [rest.copy() for _, _, rest in w.rigs]
        for (rig, _, rest) in w.rigs:
            assert np.array_equal(rest, original[rig["first_vertex"] : rig["first_vertex"] + rig["vertex_count"]])
        w.step(2, vertices(whole=True, amp=0.03))
        assert not np.array_equal(w.sc.vertices, original)
        for (_, _, rest), before in zip(w.rigs, rests):
            assert np.array_equal(rest, before)  # the rest pose did not move
        w.step(3, animate(0.5, 1.02))
        expected, _ = fs.make_scene("cornell", {})
        expected.set_vertices(0, deformed(original, 0.03, 3.0, 0.0))
        done = []
        for rig, pose, rest in w.rigs:
            q = dict(blend_factors=tuple(np.float32(f) * np.float32(0.5) for f in pose["blend_factors"]), bones=pose["bones"] * np.float32(1.02) if "bones" in pose else None)
            done.append((rig, q, posed(rest, rig["blend_targets"], q["blend_factors"], rig.get("weights"), q["bones"])))
        apply(expected, done)
        assert np.array_equal(w.sc.vertices.view(np.uint8), expected.vertices.view(np.uint8))
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the walks
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS, ids=lambda s: "seed_%d" % s)
def test_walk(built, seed):
    w = _tool().run_walk(seed, STEPS)
    print(Counter(outcome for *_, outcome in w.log))
    assert w.bad == 0 and w.compared >= 10


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: directed sequences (steps written by hand, run by the walk's own machinery: every render against the oracle)
# ---------------------------------------------------------------------------------------------------------------------------
def upload(scene, args=None, **options):
    o = dict(bvh_builder=0, lbvh_algorithm=1, sah_top=64, wide_bvh=1, embed_leaves=0, treetop=0, keep_scene=1)
    o.update(options)
    return dict(kind="upload", scene=scene, mask_size=(5, 7), fog_anisotropy=0.0, fog_density=(3.0, 3.0, 3.0), env_image=True, env_emitter=True, motion=False, motion_seed=0, options=o, args=args)


def render(seed0, seeds=2):
    return dict(kind="render", seed0=seed0, seeds=seeds, debug_mode=0, view_len=1, light_len=0)


def submit(seed0, seeds=1, own_buffers=True):
    return dict(kind="async", sub="submit", seed0=seed0, seeds=seeds, own_buffers=own_buffers)


def wait():
    return dict(kind="async", sub="wait", which=0.0)


def move(merged=False, picks=(0.0, 0.6)):
    return dict(kind="transforms", merged=merged, picks=list(picks), offsets=[[0.05, 0.1, -0.04], [-0.08, 0.0, 0.06], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], angle=0.3)


def vertices(whole=False, over_rig=False, lo=0.0, span=1.0, amp=0.03):
    return dict(kind="vertices", whole=whole, over_rig=over_rig, lo=lo, span=span, amp=amp, phase=0.0, freq=3.0)


def set_rigs(instances, targets, bones, rig_seed=7):
    return dict(kind="rigs", sub="set_rigs", instances=list(instances), targets=list(targets), bones=list(bones), count=len(instances), rig_seed=rig_seed)


def animate(scale, stretch=1.0):
    return dict(kind="rigs", sub="animate", scale=scale, stretch=stretch)


def frame(W, H, stereo=False):
    return dict(kind="frame", W=W, H=H, stereo=stereo, moved=None)


def flags(**args):
    return dict(kind="flags", args=args)


def directed(steps, compared, crossings=()):
    """Runs the steps on one context. No step may be skipped, `compared` frames must have been compared with the oracle, none
    rejected, none different; `crossings`: the scene calls that found frames in flight."""
    w = _tool().run_walk(0, planned=steps)
    outcomes = [outcome for *_, outcome in w.log]
    assert w.bad == 0, outcomes
    assert not any(o.startswith("skipped") or o == "rejected" for o in outcomes), outcomes
    assert w.compared == compared and outcomes.count("compared") == compared, outcomes
    assert [call for _, call in w.crossings] == list(crossings), w.crossings
    return w


CORNELL_BOXES = 5  # an instance of the mesh the two boxes share (tests/test_animate.py: FRAME_RIGS)


@pytest.mark.gpu
def test_two_frames_in_flight_across_every_scene_call(built):
    """update_transforms (a plain move, and one of the merged mesh that rebuilds), update_vertices, animate and an upload of
    another scene, each with two frames submitted just before it: the frames waited for afterwards are the old state's, the next
    render is the new state's."""
    steps = [upload("cornell"), frame(96, 64), render(0)]
    for k, call in enumerate([move(False), move(True), vertices(whole=True), set_rigs([CORNELL_BOXES, 0], [2, 1], [3, 0]), animate(0.7, 1.03), upload("forest", bvh_builder=1)]):
        if call.get("sub") == "set_rigs":
            steps.append(call)
            continue
        steps += [submit(10 + k, 1, own_buffers=False), submit(20 + k, 2, own_buffers=True), call, wait(), wait(), render(30 + k)]
    w = directed(steps, compared=1 + 5 * 3, crossings=["transforms", "transforms", "vertices", "animate", "upload"])
    assert [o for _, kind, _, o in w.log if kind == "transforms"] == ["done", "done: merged"]


LVC = dict(bdptFlag=["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "lvcreservoirreuse"], maxDiffuseVertices=3, maxPathVertices=6, lightPathCount=4000, reservoirM=3, hashGridBucketCount=1000)
LARGE_SMALL_LARGE = [upload("cornell"), flags(**LVC), frame(144, 80, stereo=True), render(0), flags(**dict(LVC, hashGridBucketCount=64)), frame(24, 16), render(1), flags(**LVC), frame(144, 80, stereo=True), render(2),
                     frame(24, 16), render(3, 1)]


@pytest.mark.gpu
def test_large_small_large_frames_with_the_cache_and_the_grids_live(built):
    """144 x 80 stereo with the light vertex cache, reservoirs and reuse, then 24 x 16 mono with 64 hash-grid buckets, then
    144 x 80 again: the small frame runs inside the large frame's buffers, the second large one inside what the small one left."""
    directed(LARGE_SMALL_LARGE, compared=4)


def refused(what):
    return dict(kind="refused", forms=[what])


@pytest.mark.gpu
def test_refused_calls_between_good_renders(built):
    """A refused render, update_vertices, animate (with rigs resident, and without), set_rigs and upload, each between two
    renders of different seeds: every call raises and leaves the context as the model has it."""
    steps = [upload("cornell"), frame(40, 24), set_rigs([CORNELL_BOXES], [1], [2]), animate(0.6), render(1)]
    for k, what in enumerate(["render", "update_vertices", "animate", "set_rigs", "upload"]):
        steps += [refused(what), render(2 + k)]
    steps += [animate(0.9, 1.05), render(9), dict(kind="rigs", sub="drop_rigs"), refused("animate"), render(10)]  # (the rigs outlived the refusals)
    w = directed(steps, compared=8)
    assert [o for _, kind, _, o in w.log if kind == "refused"] == ["refused"] * 6


@pytest.mark.gpu
def test_rigs_with_a_vertex_update_and_a_rebuild_between_poses(built):
    """set_rigs; update_vertices over half the rigged range (the rest pose must not move); animate; a move of a merged
    instance, which rebuilds from the kept scene and must read the posed ranges back first; animate again."""
    steps = [upload("cornell"), frame(96, 64), set_rigs([CORNELL_BOXES, 0], [2, 1], [3, 0]), vertices(over_rig=True), render(0), animate(0.5), render(1), move(True), render(2), animate(1.0, 1.04), render(3)]
    w = directed(steps, compared=4)
    assert [o for _, kind, _, o in w.log if kind in ("vertices", "transforms")] == ["done: over a rig", "done: merged"]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "forest"])
def test_layout_options_set_after_an_upload_are_picked_up_by_a_transforms_update(built, scene):
    """lds_stack_levels = 4 and treetop = 1 after the upload: the transforms-only update reads them."""
    steps = [upload(scene), frame(72, 40), render(0), dict(kind="option_later", name="lds_stack_levels", value=4), dict(kind="option_later", name="treetop", value=1), render(1), move(False), render(2),
             vertices(whole=True), render(3)]
    directed(steps, compared=4)


@pytest.mark.gpu
def test_float_then_8_bit_then_float_images_with_the_alpha_test(built):
    """Five float images, then two smaller mip-exact RGBA8 images and an R8 mask, then float images again, eAlphaTest on: the
    image tables of one upload do not leak into the next."""
    args = dict(bdptFlag=["alphatest"], maxPathVertices=5)
    steps = [upload("textured", args=args), frame(56, 40), render(0), upload("cards8"), render(1), upload("foliage8"), render(2), upload("texturedf"), render(3), upload("foliage"), render(4)]
    directed(steps, compared=5)


def shard(r, n):
    return dict(kind="shard", r=r, n=n)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["texturedf", "cornell"])
def test_a_shard_that_owns_no_tile_of_a_small_frame(built, scene):
    """Found by the walks (seeds 159, 167, 211, 226, 300, 477, 499): with eCoherentRR, on by default, the roulette's reduce was
    launched with a grid of 0 blocks on a shard without a path, and the render failed with "invalid configuration argument". An
    11 x 10 frame has two 16 x 8 tiles: rank 2 of 3 owns none. Its frame is zeros and no rays, sync and async, with the coherent
    estimators on and off; the context then renders the whole frame and a shard that owns a tile."""
    coherent = dict(bdptFlag=["coherentsampling", "presamplelights", "connecttolightpaths", "lightvertexcache"], maxDiffuseVertices=3, maxPathVertices=6, minPathVertices=2, lightPathCount=300)
    steps = [upload(scene), frame(11, 10), render(0), shard(2, 3), render(1), submit(2), wait(), flags(**coherent), render(3), flags(bdptFlag=["~coherentrr"]), render(4), shard(1, 3), render(5),
             shard(0, 1), render(6)]
    directed(steps, compared=7)


@pytest.mark.gpu
def test_sequences_with_poisoned_allocations():
    """One walk and the frame-size sequence once more in a fresh child process with STHIP_POISON_ALLOC (read once per process):
    every new device buffer starts as 0x7F bytes, so a read of what nothing has written shows in a fresh process too."""
    if os.environ.get("STHIP_SEQUENCES_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="127", STHIP_SEQUENCES_POISON_CHILD="1")
    out = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "seed_%d or large_small_large" % SEEDS[-1]],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0 and "2 passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
