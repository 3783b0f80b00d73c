"""The first bounce once per view ("reuse_first_hits", stratum_amd/csrc/first_hits.h): the hits of the primary rays do not
depend on the seed, so sthip_render keeps them on the device and runs the packet kernel again only when something they depend
on changed.

The claim under test is identity: with the option on (the default) a frame's radiance, its four AOVs and gRayCount hold, byte
for byte, what a FRESH context with "reuse_first_hits" = 0 renders from the same arguments. Both sides are this library, so
every comparison is np.array_equal on the raw bytes. An invalidation case also asserts that its two states differ in the
reference's visibility image, so that kept hits of the first state, used by mistake, could not pass."""
import os
import subprocess
import sys

import numpy as np
import pytest

from stratum_amd import camera, scenes
from stratum_amd.scene import rotate_y, scale, translate

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_animate import apply, make_rig  # noqa: E402
from test_refit import deform, mesh_range  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = ("radiance", "albedo", "visibility", "depth", "prev_uv", "ray_count")


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def renderer(sc, args=None, flags=(), options=None, shard=None):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0, args=dict(args or {}, bdptFlag=list(flags)))
    for k, v in (options or {}).items():
        r.set_option(k, v)
    if shard:
        r.set_shard(*shard)
    r.update(sc)
    return r


def copy(out):
    return {k: v.copy() for k, v in out.items()}


def same(got, want, what):
    assert set(IMAGES) <= set(got) and set(IMAGES) <= set(want), (what, sorted(got), sorted(want))
    for k in IMAGES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, k)


def reference(sc, frame, seed_begin, seed_count, args=None, flags=(), options=None, shard=None, max_path_vertices=None):
    """The frame and the stats of a fresh context that keeps nothing."""
    r = renderer(sc, args, flags, dict(options or {}, reuse_first_hits=0), shard)
    try:
        if max_path_vertices is not None:
            r.mPushConstants.gMaxPathVertices = max_path_vertices
        out = copy(r.render(frame, seed_begin, seed_count))
        return out, r.stats()
    finally:
        r.close()


def visibility_differs(a, b):
    return not np.array_equal(a["visibility"].view(np.uint8), b["visibility"].view(np.uint8))


def frame_of(cam, w, h, **kw):
    return camera.Frame(w, h, kw.get("fovy", cam["fovy"]), kw.get("eye", cam["eye"]), kw.get("target", cam["target"]))


SMALL_FOREST = dict(n_instances=30, tree_tris=600, tree_kinds=2)
REPEAT = {
    # one whole 64x32 tile plus partial ones: dead slots and packets without a live lane
    "cornell": (lambda: scenes.cornell_box(), 72, 40, {}, ()),
    "spheres_room": (lambda: scenes.spheres_room(), 64, 32, {"maxDiffuseVertices": 3}, ()),
    "foliage": (lambda: scenes.foliage(), 64, 32, {}, ("alphatest",)),
}


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_documents_the_option():
    hdr = open(os.path.join(ROOT, "include", "sthip.h")).read()
    assert '"reuse_first_hits"' in hdr
    for word in ("20 bytes per path", "drops the kept hits", "0 for a call served entirely from kept hits"):
        assert word in hdr, word


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REPEAT))
def test_repeat_calls_equal_a_context_that_keeps_nothing(built, name):
    """Seeds 0, 1, 2 in three calls of one context: each frame is the reference's; from the second call on the packet kernel
    has traced nothing, and the ray counts are the reference's all the same."""
    make, w, h, args, flags = REPEAT[name]
    sc, cam = make()
    frame = frame_of(cam, w, h)
    r = renderer(sc, args, flags)
    ref = renderer(sc, args, flags, {"reuse_first_hits": 0})
    try:
        for seed in range(3):
            got, st = copy(r.render(frame, seed, 1)), r.stats()
            want, st_ref = copy(ref.render(frame, seed, 1)), ref.stats()
            same(got, want, "%s seed %d" % (name, seed))
            assert st_ref["rays_primary_packets"] > 0 and st["rays_total"] == st_ref["rays_total"] and st["rays_path"] == st_ref["rays_path"], (name, seed)
            assert st["rays_primary_packets"] == (st_ref["rays_primary_packets"] if seed == 0 else 0), (name, seed, st["rays_primary_packets"])
    finally:
        r.close()
        ref.close()


@pytest.mark.gpu
def test_several_seeds_in_flight(built):
    """Five seeds in batches of 2, 2 and 1: the first batch traces one seed's paths and copies them to both seeds' slots, the
    second only copies, the third shades from the kept hits; then a second such call, which traces nothing."""
    sc, cam = scenes.cornell_box()
    frame = frame_of(cam, 72, 40)
    per_seed = 4 * 64 * 32  # 2 x 2 tiles of 64 x 32 slots
    options = {"max_paths_in_flight": 2 * per_seed}
    r = renderer(sc, options=options)
    try:
        for call, seed_begin in enumerate((0, 5)):
            got, st = copy(r.render(frame, seed_begin, 5)), r.stats()
            want, st_ref = reference(sc, frame, seed_begin, 5, options=options)
            assert st["paths_per_seed"] == per_seed and st["seeds_in_flight"] == 2 and st_ref["seeds_in_flight"] == 2
            same(got, want, "call %d" % call)
            assert st["rays_total"] == st_ref["rays_total"]
            assert st_ref["rays_primary_packets"] == 5 * 72 * 40 and st["rays_primary_packets"] == (72 * 40 if call == 0 else 0)
    finally:
        r.close()


def _cornell():
    sc, cam = scenes.cornell_box()
    return sc, cam


def _case_view_moved():
    sc, cam = _cornell()
    return dict(sc=sc, frame_a=frame_of(cam, 64, 32), frame_b=frame_of(cam, 64, 32, eye=(0.7, 0.4, 3.9)))


def _case_projection():
    sc, cam = _cornell()
    return dict(sc=sc, frame_a=frame_of(cam, 64, 32), frame_b=frame_of(cam, 64, 32, fovy=np.radians(60.0)))


def _case_extent():
    sc, cam = _cornell()
    return dict(sc=sc, frame_a=frame_of(cam, 64, 32), frame_b=frame_of(cam, 32, 64))


def _case_view_count():
    sc, cam = _cornell()
    return dict(sc=sc, frame_a=frame_of(cam, 64, 32), frame_b=camera.Frame.stereo(64, 32, cam["fovy"], cam["eye"], cam["target"], eye_separation=0.5))


def _case_max_path_vertices():
    sc, cam = _cornell()
    return dict(sc=sc, frame_a=frame_of(cam, 64, 32), vertices_a=1, vertices_b=4)


def _case_max_path_vertices_back():
    sc, cam = _cornell()
    return dict(sc=sc, frame_a=frame_of(cam, 64, 32), vertices_a=4, vertices_b=1)


def _case_shard():
    sc, cam = _cornell()
    return dict(sc=sc, frame_a=frame_of(cam, 128, 64), shard_a=(0, 2, 64, 32), shard_b=(1, 2, 64, 32))


def _case_scene():
    sc, cam = _cornell()
    other, _ = scenes.spheres_room()
    return dict(sc=sc, frame_a=frame_of(cam, 64, 32, eye=(0.0, 1.0, 3.9), target=(0.0, 0.5, 0.0)), sc_b=other, change=lambda r, sc_b: r.update(sc_b))


def _case_update_transforms():
    sc, cam = _cornell()

    def move(r, s):  # the short block, across the floor
        s.set_instance_transform(5, translate((-0.4, -1.0, 0.6)) @ rotate_y(0.5) @ scale((0.6, 0.6, 0.6)))
        r.update_transforms(s)

    return dict(sc=sc, frame_a=frame_of(cam, 64, 32), change=move, mutate_for_reference=lambda s: s.set_instance_transform(5, translate((-0.4, -1.0, 0.6)) @ rotate_y(0.5) @ scale((0.6, 0.6, 0.6))))


def _case_update_vertices():
    sc, cam = _cornell()

    def bend(r, s):
        deform(s, 0.2)
        r.update_vertices(s)

    return dict(sc=sc, frame_a=frame_of(cam, 64, 32), change=bend, mutate_for_reference=lambda s: deform(s, 0.2))


def _case_animate():
    sc, cam = scenes.forest(**SMALL_FOREST)
    first, count = mesh_range(sc, 1)  # a tree mesh: every instance of it moves
    rig = make_rig(sc.vertices, first, count, 2, 5, 1)

    def pose(r, s):
        r.set_rigs([rig[0]])
        r.animate([rig[1]])

    return dict(sc=sc, frame_a=frame_of(cam, 64, 32), change=pose, mutate_for_reference=lambda s: apply(s, [rig]))


def _case_alpha_test_flag():
    sc, cam = scenes.foliage()
    return dict(sc=sc, frame_a=frame_of(cam, 64, 32), flags_a=("alphatest",), flags_b=("~alphatest",))


INVALIDATION = {
    "view-transform-moved": _case_view_moved,
    "projection-changed": _case_projection,
    "extent-64x32-to-32x64": _case_extent,
    "one-view-to-two-views": _case_view_count,
    "max-path-vertices-1-to-4": _case_max_path_vertices,
    "max-path-vertices-4-to-1": _case_max_path_vertices_back,
    "shard-0-of-2-to-1-of-2": _case_shard,
    "another-scene-uploaded": _case_scene,
    "update-transforms": _case_update_transforms,
    "update-vertices": _case_update_vertices,
    "animate": _case_animate,
    "alpha-test-flag": _case_alpha_test_flag,
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INVALIDATION))
def test_a_change_of_the_key_traces_again(built, name):
    """Render state A (which keeps its first hits), change ONE thing the first bounce depends on, render state B: the frame is
    the one a fresh context without the option renders in state B. The states differ in the reference's visibility image, so
    A's hits would show. A second render of B is then served from B's kept hits and is the same frame again."""
    import copy as copy_module

    c = INVALIDATION[name]()
    sc = c["sc"]
    frame_a, frame_b = c["frame_a"], c.get("frame_b", c["frame_a"])
    flags_a = tuple(c.get("flags_a", ()))
    # the reference's two states, from scratch
    sc_b = c.get("sc_b")
    if sc_b is None:
        sc_b = copy_module.deepcopy(sc)
        if "mutate_for_reference" in c:
            c["mutate_for_reference"](sc_b)
    flags_b = tuple(c.get("flags_b", flags_a))
    # (a flag switched off is a flag the reference never had)
    ref_flags_b = tuple(f for f in flags_b if f[0] not in "~!")
    want_a, _ = reference(sc, frame_a, 0, 1, flags=flags_a, shard=c.get("shard_a"), max_path_vertices=c.get("vertices_a"))
    want_b, st_ref = reference(sc_b, frame_b, 1, 1, flags=ref_flags_b, shard=c.get("shard_b", c.get("shard_a")), max_path_vertices=c.get("vertices_b", c.get("vertices_a")))
    assert want_a["visibility"].shape != want_b["visibility"].shape or visibility_differs(want_a, want_b), "the case is vacuous: both states see the same first hits"

    r = renderer(sc, flags=flags_a, shard=c.get("shard_a"))
    try:
        if "vertices_a" in c:
            r.mPushConstants.gMaxPathVertices = c["vertices_a"]
        same(copy(r.render(frame_a, 0, 1)), want_a, name + ": state A")
        if "change" in c:
            c["change"](r, c["sc_b"] if "sc_b" in c else sc)
        if "shard_b" in c:
            r.set_shard(*c["shard_b"])
        if "vertices_b" in c:
            r.mPushConstants.gMaxPathVertices = c["vertices_b"]
        for f in flags_b if "flags_b" in c else ():
            r.set_flag(f)
        same(copy(r.render(frame_b, 1, 1)), want_b, name + ": state B")
        assert r.stats()["rays_primary_packets"] == st_ref["rays_primary_packets"]  # (it was traced, where the state traces at all)
        same(copy(r.render(frame_b, 1, 1)), want_b, name + ": state B again")
        assert r.stats()["rays_primary_packets"] == 0
    finally:
        r.close()


@pytest.mark.gpu
def test_volumes_bypass_the_kept_hits(built):
    """The packet path is not taken with media: two renders of the fog box are the reference's, nothing is kept or reused."""
    sc, cam = scenes.fog_box()
    frame = frame_of(cam, 64, 32)
    args = {"maxDiffuseVertices": 3}
    want, _ = reference(sc, frame, 0, 1, args=args)
    r = renderer(sc, args)
    try:
        for k in range(2):
            same(copy(r.render(frame, 0, 1)), want, "fog box, render %d" % k)
    finally:
        r.close()


@pytest.mark.gpu
def test_count_traversal_bypasses_the_kept_hits(built):
    """The diagnostic passes describe the kernels: with count_traversal a second identical call walks the first bounce again."""
    sc, cam = scenes.cornell_box()
    frame = frame_of(cam, 72, 40)
    want, _ = reference(sc, frame, 0, 1)
    r = renderer(sc)
    try:
        same(copy(r.render(frame, 0, 1)), want, "before the option")  # (keeps its hits)
        r.set_option("count_traversal", 1)
        visited = []
        for k in range(2):
            same(copy(r.render(frame, 0, 1)), want, "count_traversal, render %d" % k)
            st = r.stats()
            assert st["nodes_visited_primary"] > 0 and st["rays_primary_packets"] == 72 * 40, (k, st["nodes_visited_primary"], st["rays_primary_packets"])
            visited.append(st["nodes_visited_primary"])
        assert visited[0] == visited[1]
        r.set_option("count_traversal", 0)
        same(copy(r.render(frame, 0, 1)), want, "after the option")
        assert r.stats()["rays_primary_packets"] == 0  # (the hits kept before the diagnostic passes are still the view's)
    finally:
        r.close()


@pytest.mark.gpu
def test_async_frames_of_one_view(built):
    """Two frames of sthip_render_async in flight (output_ring 2), same view, seeds 0 and 1: the second is shaded from the hits
    the first traced, on the same stream; both equal the synchronous reference frames."""
    sc, cam = scenes.cornell_box()
    frame = frame_of(cam, 72, 40)
    ref = renderer(sc, options={"reuse_first_hits": 0})
    try:
        want = [copy(ref.render(frame, seed, 1)) for seed in range(2)]
    finally:
        ref.close()
    r = renderer(sc, options={"output_ring": 2})
    try:
        tickets = [r.render_async(frame, seed, 1) for seed in range(2)]
        for seed, t in enumerate(tickets):
            same(r.wait(t), want[seed], "async frame %d" % seed)
        assert r.stats()["rays_primary_packets"] == 0
    finally:
        r.close()


@pytest.mark.gpu
def test_repeat_with_poisoned_allocations():
    """The repeat case on the Cornell box once more in a fresh child process with STHIP_POISON_ALLOC (read once per process):
    the kept buffers start as 0x7F bytes instead of the zero pages of a fresh process, so a slot that is read before the packet
    kernel wrote it shows."""
    if os.environ.get("STHIP_FIRST_HITS_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="127", STHIP_FIRST_HITS_POISON_CHILD="1")
    out = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "(repeat_calls and cornell) or several_seeds"],
        env=env, cwd=ROOT, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0 and " passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
