"""Parity of the HIP path against the CPU oracle, through the C ABI (needs an MI355X)."""
import os

import numpy as np
import pytest

from stratum_amd import camera, scenes, wire

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a = a[..., :3].astype(np.float64)
    b = b[..., :3].astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b**2).sum()), 1e-300))


@pytest.fixture(scope="module")
def renderer(built):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0)
    yield r
    r.close()


def random_rays(n, seed, lo, hi, tmax=np.inf):
    rng = np.random.RandomState(seed)
    rays = np.zeros(n, wire.Ray)
    rays["origin"] = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["direction"] = d.astype(np.float32)
    rays["tmin"] = 0
    rays["tmax"] = tmax
    return rays


def test_trace_contract_cornell(renderer, cornell):
    from oracle import oracle_py

    sc, _ = cornell
    renderer.update(sc)
    o = oracle_py.OracleScene(sc)
    rays = random_rays(50000, 1, -0.99, 0.99)
    got = renderer.trace(rays)
    ref, _ = o.trace(rays, brute=True)
    assert np.array_equal(got["instance_primitive_index"], ref["instance_primitive_index"])
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32))
    assert np.array_equal(got["b1"].view(np.uint32), ref["b1"].view(np.uint32))
    assert np.array_equal(got["b2"].view(np.uint32), ref["b2"].view(np.uint32))
    # occlusion
    rays["tmax"] = 0.7
    got = renderer.trace(rays, any_hit=True)
    ref, _ = o.trace(rays, any_hit=True, brute=True)
    assert np.array_equal(got["instance_primitive_index"], ref["instance_primitive_index"])


def test_cornell_256_one_sample(renderer, cornell):
    """configs[0]: Cornell box, 256x256, 1 sample, default flags."""
    from oracle import oracle_py

    sc, cam = cornell
    renderer.update(sc)
    frame = camera.Frame(256, 256, cam["fovy"], cam["eye"], cam["target"])
    got = renderer.render(frame, 0, 1)
    ref = oracle_py.OracleScene(sc).render(frame, renderer.push_constants(frame), renderer.mSamplingFlags, 0, 1)
    assert np.array_equal(got["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
    assert np.array_equal(got["visibility"]["packed_normal"], ref["visibility"]["packed_normal"])
    assert np.array_equal(got["albedo"], ref["albedo"])
    assert np.array_equal(got["ray_count"], ref["ray_count"])
    d = rel_l2(got["radiance"], ref["radiance"])
    nd = int((got["radiance"].view(np.uint32) != ref["radiance"].view(np.uint32)).any(axis=-1).sum())
    print("rel-L2 %.3e, pixels that differ in any bit: %d" % (d, nd))
    assert d <= 1e-4  # north_star tolerance on the HDR framebuffer
    assert np.array_equal(got["depth"]["z"].view(np.uint32), ref["depth"]["z"].view(np.uint32))
    assert np.allclose(got["prev_uv"], ref["prev_uv"], rtol=0, atol=0)


@pytest.fixture(scope="module")
def atrium_scene():
    return scenes.atrium()


def edge_rays(sc, n, seed):
    """Rays aimed exactly at vertices and edge points of random triangles (ties and watertightness)."""
    rng = np.random.RandomState(seed)
    inst = sc.instances["packed"]
    rays = np.zeros(n, wire.Ray)
    verts = sc.vertices["position"]
    k = 0
    while k < n:
        i = rng.randint(0, inst.shape[0])
        pc = (inst[i, 1] >> 12) & 0xFFFF
        stride = inst[i, 1] >> 28
        prim = rng.randint(0, pc)
        off = int(inst[i, 3]) + prim * 3 * int(stride)
        idx = np.frombuffer(sc.indices[off : off + 3 * int(stride)].tobytes(), dtype="<u2" if stride == 2 else "<u4").astype(np.int64) + int(inst[i, 2])
        m = np.vstack([sc.transforms["m"][i].astype(np.float64), [0, 0, 0, 1]])
        p = (m @ np.concatenate([verts[idx].astype(np.float64), np.ones((3, 1))], axis=1).T).T[:, :3]
        w = rng.dirichlet([1, 1, 1])
        mode = rng.randint(0, 3)
        if mode == 0:
            w = np.eye(3)[rng.randint(0, 3)]  # a vertex
        elif mode == 1:
            w[rng.randint(0, 3)] = 0  # an edge
            w /= w.sum()
        target = (w[:, None] * p).sum(0)
        o = target + rng.normal(size=3) * rng.uniform(0.5, 5.0)
        d = target - o
        d /= np.linalg.norm(d)
        rays["origin"][k] = o
        rays["direction"][k] = d
        rays["tmin"][k] = 0
        rays["tmax"][k] = np.inf
        k += 1
    return rays


def test_trace_contract_atrium(renderer, atrium_scene):
    """BVH traversal == the oracle's own BVH on 1M triangles (merged world mesh + 20 transformed instances),
    and == brute force on a subset, including rays through vertices and edges."""
    from oracle import oracle_py

    sc, _ = atrium_scene
    renderer.update(sc)
    o = oracle_py.OracleScene(sc)
    rays = np.concatenate([random_rays(200000, 2, [-14, 0.2, -5.5], [14, 9.5, 5.5]), edge_rays(sc, 20000, 3)])
    got = renderer.trace(rays)
    ref, _ = o.trace(rays)
    for f in ("instance_primitive_index", "t", "b1", "b2"):
        assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f
    sub = np.concatenate([rays[:300], rays[-300:]])
    ref_b, _ = o.trace(sub, brute=True)
    got_b = renderer.trace(sub)
    for f in ("instance_primitive_index", "t", "b1", "b2"):
        assert np.array_equal(got_b[f].view(np.uint32), ref_b[f].view(np.uint32)), f
    rays["tmax"] = 3.0
    got = renderer.trace(rays, any_hit=True)
    ref, _ = o.trace(rays, any_hit=True)
    assert np.array_equal(got["instance_primitive_index"], ref["instance_primitive_index"])


def test_atrium_quarter_res(renderer, atrium_scene):
    """configs[2] scene at 480x270 (the oracle finishes in seconds): bit-exact ids, rel-L2 <= 1e-4."""
    from oracle import oracle_py

    sc, cam = atrium_scene
    renderer.update(sc)
    frame = camera.Frame(480, 270, cam["fovy"], cam["eye"], cam["target"])
    got = renderer.render(frame, 0, 2)
    ref = oracle_py.OracleScene(sc).render(frame, renderer.push_constants(frame), renderer.mSamplingFlags, 0, 2)
    assert np.array_equal(got["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
    assert np.array_equal(got["ray_count"], ref["ray_count"])
    d = rel_l2(got["radiance"], ref["radiance"])
    nd = int((got["radiance"].view(np.uint32) != ref["radiance"].view(np.uint32)).any(axis=-1).sum())
    print("atrium rel-L2 %.3e, differing pixels %d" % (d, nd))
    assert d <= 1e-4
    assert np.array_equal(got["radiance"][..., 3], ref["radiance"][..., 3])


def test_shards_sum_to_the_full_frame(renderer, cornell):
    """sthip_set_shard: rank r renders tiles t % world == r, zero elsewhere; the sum over ranks is the frame."""
    from stratum_amd import shard

    sc, cam = cornell
    renderer.update(sc)
    W, H = 200, 120  # not a multiple of the tile size on purpose
    frame = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    renderer.set_shard(0, 1, 64, 32)
    full = renderer.render(frame, 5, 3)
    acc = np.zeros_like(full["radiance"])
    rays = 0
    try:
        for r in range(3):
            renderer.set_shard(r, 3, 16, 8)
            part = renderer.render(frame, 5, 3)
            mask = shard.owned_mask(W, H, r, 3, 16, 8)
            assert (part["radiance"][~mask] == 0).all()
            assert (part["radiance"][mask][:, 3] == 3).all()
            acc += part["radiance"]
            rays += int(part["ray_count"][0])
    finally:
        renderer.set_shard(0, 1, 64, 32)
    assert np.array_equal(acc.view(np.uint32), full["radiance"].view(np.uint32))
    assert rays == int(full["ray_count"][0])


@pytest.mark.parametrize("flags", ["~nee", "~samplebsdfs", "~mis", "~defershadowrays"])
def test_flag_combinations(renderer, cornell, flags):
    from oracle import oracle_py
    from stratum_amd.bdpt import BDPT

    sc, cam = cornell
    r = BDPT(device=0, args={"bdptFlag": [flags]})
    try:
        r.update(sc)
        frame = camera.Frame(128, 96, cam["fovy"], cam["eye"], cam["target"])
        got = r.render(frame, 11, 2)
        ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 11, 2)
        assert np.array_equal(got["ray_count"], ref["ray_count"])
        assert np.array_equal(got["radiance"].view(np.uint32), ref["radiance"].view(np.uint32)), flags
    finally:
        r.close()


def material_scene():
    """Cornell-like box whose blocks and walls use every Disney lobe (metal, glass, clearcoat, subsurface)."""
    from stratum_amd.scene import SceneBuilder, rotate_y, scale, translate

    b = SceneBuilder("materials")
    mats = [
        b.add_material((0.73, 0.73, 0.73), roughness=0.5, subsurface=0.3),
        b.add_material((0.9, 0.6, 0.2), metallic=1.0, roughness=0.25),
        b.add_material((0.95, 0.95, 0.95), transmission=1.0, roughness=0.15, eta=1.5),
        b.add_material((0.2, 0.3, 0.8), clearcoat=1.0, clearcoat_gloss=0.7, roughness=0.6),
        b.add_material((0.6, 0.6, 0.6), metallic=0.4, roughness=0.35, transmission=0.3, clearcoat=0.4, anisotropic=0.5),
        b.add_material((0.95, 0.95, 0.95), metallic=1.0, roughness=0.0),  # specular: no NEE, not a diffuse vertex
    ]
    light = b.add_emitter((17.0, 12.0, 4.0))
    q = scenes._quad
    walls = [
        (q((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1), (0, 1, 0)), mats[0]),
        (q((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1), (0, -1, 0)), mats[0]),
        (q((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (0, 0, 1)), mats[5]),
        (q((-1, -1, 1), (-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (1, 0, 0)), mats[3]),
        (q((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1), (-1, 0, 0)), mats[1]),
    ]
    for part, m in walls:
        b.add_instance(b.add_mesh(*part), m)
    sphere = scenes.grid_surface(
        lambda U, V: np.stack([np.sin(V * np.pi) * np.cos(U * 2 * np.pi), np.cos(V * np.pi), np.sin(V * np.pi) * np.sin(U * 2 * np.pi)], -1), 24, 16, flip=True
    )
    ball = b.add_mesh(*sphere)
    b.add_instance(ball, mats[2], translate((0.4, -0.6, 0.3)) @ scale(0.4))
    b.add_instance(ball, mats[4], translate((-0.4, -0.55, -0.2)) @ rotate_y(0.7) @ scale((0.45, 0.45, 0.3)))
    b.add_instance(ball, mats[1], translate((0.0, 0.2, -0.5)) @ scale(0.25))
    lq = q((-0.24, 0.995, -0.2), (0.24, 0.995, -0.2), (0.24, 0.995, 0.18), (-0.24, 0.995, 0.18), (0, -1, 0))
    b.add_instance(b.add_mesh(*lq), light)
    return b.build(), {"eye": (0.0, 0.0, 3.9), "target": (0.0, 0.0, 0.0), "fovy": np.radians(39.3)}


def test_all_disney_lobes_and_long_paths(renderer):
    """Metal / glass / clearcoat / subsurface / specular materials, shared meshes under non-uniform
    transforms, 8 diffuse vertices + Russian roulette (the configs[4] path limits)."""
    from oracle import oracle_py
    from stratum_amd.bdpt import BDPT

    sc, cam = material_scene()
    r = BDPT(device=0, args={"maxDiffuseVertices": 8, "maxPathVertices": 10, "minPathVertices": 4, "bdptFlag": ["~coherentrr"]})
    try:
        r.update(sc)
        frame = camera.Frame(160, 120, cam["fovy"], cam["eye"], cam["target"])
        got = r.render(frame, 0, 2)
        ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, 2)
        assert np.array_equal(got["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
        assert np.array_equal(got["ray_count"], ref["ray_count"])
        d = rel_l2(got["radiance"], ref["radiance"])
        nd = int((got["radiance"].view(np.uint32) != ref["radiance"].view(np.uint32)).any(axis=-1).sum())
        print("materials rel-L2 %.3e, differing pixels %d, rays %s" % (d, nd, got["ray_count"]))
        assert d <= 1e-4
        assert int(got["ray_count"][1]) > 2.2 * 160 * 120 * 2  # paths go beyond the default budget where surfaces allow
    finally:
        r.close()


@pytest.mark.parametrize("flags,args", [
    (["coherentsampling", "presamplelights"], {"lightPresampleTileSize": 64, "lightPresampleTileCount": 8}),
    (["coherentsampling", "presamplelights", "neereservoirs", "~defershadowrays"], {"lightPresampleTileSize": 128, "lightPresampleTileCount": 4, "reservoirM": 4}),
    (["coherentsampling", "connecttolightpaths", "lightvertexcache", "~defershadowrays"], {"maxDiffuseVertices": 3, "lightPathCount": 4000}),
    (["coherentsampling", "presamplelights", "neereservoirs", "connecttolightpaths", "lightvertexcache", "lvcreservoirs", "~defershadowrays", "~coherentrr"],
     {"maxDiffuseVertices": 3, "lightPathCount": 6000, "reservoirM": 3, "lightPresampleTileSize": 32, "lightPresampleTileCount": 16}),
    (["coherentsampling", "presamplelights", "connecttolightpaths", "lightvertexcache", "lvcreservoirs", "~defershadowrays"],
     {"maxDiffuseVertices": 4, "maxPathVertices": 7, "minPathVertices": 2, "lightPathCount": 5000, "reservoirM": 2}),
])
def test_coherent_sampling(flags, args):
    """eCoherentSampling (path.hlsli:317-318,379-387,688,703): an index drawn at random becomes WaveReadLaneFirst(index) +
    WaveGetLaneIndex(), so the lanes of a workgroup read consecutive presampled lights / cached light vertices. Defined over
    the 8x4 pixel group like the coherent roulette: "first lane" = the lowest lane whose path executes that statement at that
    path length. Oracle: group replay (a path that finds no group value reports its own draw and stops); HIP: one probe pass
    and a half-wave reduction per site (the NEE index, then connect_lvc's, whose position in the random stream depends on the
    first). Frames, ids and ray counts agree bit for bit, also together with the coherent roulette (last case: it runs from
    the second vertex on) and on frame sizes with partial groups; and the flag does change the frame."""
    from oracle import oracle_py
    from stratum_amd.bdpt import BDPT

    for make in (scenes.cornell_box, material_scene):
        sc, cam = make()
        W, H, seeds = 104, 76, 2
        frame = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
        r = BDPT(device=0, args=dict(args, bdptFlag=flags))
        try:
            r.update(sc)
            got = r.render(frame, 5, seeds)
            ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 5, seeds)
            assert np.array_equal(got["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
            assert np.array_equal(got["ray_count"], ref["ray_count"])
            nd = int((got["radiance"].view(np.uint32) != ref["radiance"].view(np.uint32)).any(axis=-1).sum())
            assert nd == 0, (flags, nd, rel_l2(got["radiance"], ref["radiance"]))
            r.set_flag("~coherentsampling")
            plain = r.render(frame, 5, seeds)
            assert not np.array_equal(plain["radiance"], got["radiance"])
        finally:
            r.close()


def test_coherent_sampling_with_media_is_rejected():
    from stratum_amd import _lib
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box(fog=_fog())
    r = BDPT(device=0, args={"bdptFlag": ["coherentsampling", "presamplelights"]})
    try:
        r.update(sc)
        with pytest.raises(_lib.StratumHipError, match="eCoherentSampling with media"):
            r.render(camera.Frame(32, 32, cam["fovy"], cam["eye"], cam["target"]))
    finally:
        r.close()


@pytest.mark.parametrize("scene_name,args", [("materials", {"maxDiffuseVertices": 8, "maxPathVertices": 10, "minPathVertices": 4}), ("cornell", {"maxDiffuseVertices": 5, "maxPathVertices": 7, "minPathVertices": 2}),
                                             ("textured", {"maxDiffuseVertices": 4, "maxPathVertices": 8, "minPathVertices": 3, "bdptFlag": ["connecttoviews"]})])
def test_coherent_russian_roulette(scene_name, args):
    """eCoherentRR, the reference's default (BDPT.cpp:58): the survival probability of a Russian roulette is the maximum over
    the 8x4 workgroup's lanes that run it in that iteration, the verdict the first lane's (path.hlsli:829-845). The
    oracle gets there by replaying each group until every decision is known, the HIP path by a probe pass, a group
    reduction and the round proper; both agree bit for bit in ids and ray counts, the frame differs from the per-path
    roulette's (~coherentrr), and pixel-tile shards (whole groups per tile) reproduce the unsharded frame."""
    from oracle import oracle_py
    from stratum_amd import shard
    from stratum_amd.bdpt import BDPT

    sc, cam = {"materials": material_scene, "cornell": scenes.cornell_box, "textured": scenes.textured_box}[scene_name]()
    W, H, seeds = 104, 76, 2  # not multiples of the group size: partial groups at the right and bottom edges
    frame = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    r = BDPT(device=0, args=args)
    try:
        assert (r.mSamplingFlags >> wire.FLAG_NAMES.index("eCoherentRR")) & 1  # on by default
        r.update(sc)
        got = r.render(frame, 0, seeds)
        ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, seeds)
        assert np.array_equal(got["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
        assert np.array_equal(got["ray_count"], ref["ray_count"])
        d = rel_l2(got["radiance"], ref["radiance"])
        nd = int((got["radiance"].view(np.uint32) != ref["radiance"].view(np.uint32)).any(axis=-1).sum())
        print("coherent RR %s: rel-L2 %.3e, differing pixels %d, rays %s" % (scene_name, d, nd, got["ray_count"]))
        assert d <= 1e-4
        # it is a different estimator from the per-path roulette
        r.set_flag("~coherentrr")
        plain = r.render(frame, 0, seeds)
        r.set_flag("coherentrr")
        assert not np.array_equal(plain["ray_count"], got["ray_count"])
        # shards: tiles are whole 8x8 blocks, so a group never straddles two ranks
        if scene_name != "textured":
            total = np.zeros_like(got["radiance"])
            rays = np.zeros(2, np.uint64)
            for rank in range(3):
                r.set_shard(rank, 3, 16, 8)
                part = r.render(frame, 0, seeds, aovs=False)
                assert np.all(part["radiance"][shard.owner_map(W, H, 3, 16, 8) != rank] == 0)
                total += part["radiance"]
                rays += part["ray_count"]
            assert np.array_equal(total.view(np.uint32), got["radiance"].view(np.uint32))
            assert np.array_equal(rays, got["ray_count"])
    finally:
        r.close()


def test_golden_fixtures(renderer, cornell):
    """The committed fixtures (tests/golden/make_golden.py) without the oracle in the loop."""
    import os

    here = os.path.dirname(os.path.abspath(__file__))
    sc, cam = cornell
    renderer.update(sc)
    g = np.load(os.path.join(here, "golden", "cornell_256_seed0.npz"))
    frame = camera.Frame(256, 256, cam["fovy"], cam["eye"], cam["target"])
    got = renderer.render(frame, 0, 1)
    assert np.array_equal(got["radiance"].view(np.uint32), g["radiance"].view(np.uint32))
    assert np.array_equal(got["visibility"]["instance_primitive_index"], g["instance_primitive_index"])
    assert np.array_equal(got["visibility"]["packed_normal"], g["packed_normal"])
    assert np.array_equal(got["albedo"], g["albedo"])
    assert np.array_equal(got["depth"]["z"].view(np.uint32), g["depth_z"].view(np.uint32))
    assert np.array_equal(got["ray_count"], g["ray_count"])
    gr = np.load(os.path.join(here, "golden", "cornell_rays.npz"))
    hits = renderer.trace(gr["rays"])
    for f in ("instance_primitive_index", "t", "b1", "b2"):
        assert np.array_equal(hits[f].view(np.uint32), gr["hits"][f].view(np.uint32)), f


def test_estimator_golden_fixture_on_the_gpu():
    """The defined-order estimators against committed frames (tests/golden/estimators.npz), without the oracle in the loop:
    light vertex cache, reservoir reuse through both hash grids, coherent roulette, coherent sampling."""
    import importlib.util

    from stratum_amd.bdpt import BDPT

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_estimator_golden", os.path.join(here, "make_estimator_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    # (only its CASES table is used: the module imports the oracle binding, which this test never calls)
    spec.loader.exec_module(mk)
    g = np.load(os.path.join(here, "estimators.npz"))
    sc, cam = scenes.cornell_box()
    frame = camera.Frame(mk.W, mk.H, cam["fovy"], cam["eye"], cam["target"])
    key = {"gLightPathCount": "lightPathCount", "gMaxDiffuseVertices": "maxDiffuseVertices", "gReservoirM": "reservoirM", "gHashGridBucketCount": "hashGridBucketCount",
           "gMinPathVertices": "minPathVertices", "gMaxPathVertices": "maxPathVertices", "gLightPresampleTileSize": "lightPresampleTileSize", "gLightPresampleTileCount": "lightPresampleTileCount"}
    for name, (names, overrides) in mk.CASES.items():
        from stratum_amd.bdpt import _flag_key

        flags = [("~" + _flag_key(n[1:])) if n.startswith("~") else _flag_key(n) for n in names]
        r = BDPT(device=0, args=dict({key[k]: v for k, v in overrides.items()}, bdptFlag=flags))
        try:
            assert r.mSamplingFlags == mk.flags_of(names), name
            r.update(sc)
            got = r.render(frame, 3, mk.SEEDS)
        finally:
            r.close()
        assert np.array_equal(got["radiance"].view(np.uint32), g[name + "_radiance"].view(np.uint32)), name
        assert np.array_equal(got["ray_count"], g[name + "_ray_count"]), name


def test_errors_are_reported_not_ignored(renderer, cornell):
    from stratum_amd._lib import StratumHipError
    from stratum_amd.bdpt import BDPT

    sc, cam = cornell
    r = BDPT(device=0, args={"bdptFlag": ["samplelightpower"]})  # reads a table upstream never fills: rejected, not ignored
    try:
        r.update(sc)
        with pytest.raises(StratumHipError, match="outside the built hot path"):
            r.render(camera.Frame(64, 32, cam["fovy"], cam["eye"], cam["target"]))
    finally:
        r.close()
    r = BDPT(device=0)
    try:
        with pytest.raises(StratumHipError, match="before BDPT.update"):
            r.render(camera.Frame(64, 32, cam["fovy"], cam["eye"], cam["target"]))
    finally:
        r.close()


@pytest.mark.parametrize("algorithm", [0, 1])
def test_gpu_lbvh_builder_gives_the_same_image(atrium_scene, algorithm):
    """The hit contract does not depend on the acceleration structure: the GPU builders (0: Karras radix tree over the
    Morton codes, 1: PLOC, agglomerative clustering along the Morton curve) and the host SAH tree give bit-identical
    frames and ray batches."""
    from stratum_amd.bdpt import BDPT

    sc, cam = atrium_scene
    frame = camera.Frame(320, 180, cam["fovy"], cam["eye"], cam["target"])
    rays = np.concatenate([random_rays(100000, 5, [-14, 0.2, -5.5], [14, 9.5, 5.5]), edge_rays(sc, 10000, 6)])
    res = {}
    for kind in (0, 1):
        r = BDPT(device=0)
        try:
            r.set_option("bvh_builder", kind)
            r.set_option("lbvh_algorithm", algorithm)
            r.update(sc)
            res[kind] = (r.render(frame, 3, 2), r.trace(rays), r.stats())
        finally:
            r.close()
    a, b = res[0], res[1]
    assert np.array_equal(a[0]["radiance"].view(np.uint32), b[0]["radiance"].view(np.uint32))
    assert np.array_equal(a[0]["visibility"]["instance_primitive_index"], b[0]["visibility"]["instance_primitive_index"])
    assert np.array_equal(a[0]["ray_count"], b[0]["ray_count"])
    for f in ("instance_primitive_index", "t", "b1", "b2"):
        assert np.array_equal(a[1][f].view(np.uint32), b[1][f].view(np.uint32)), f
    print("build ms: sah/host %.1f, lbvh %.1f (gpu kernels %.2f)" % (a[2]["bvh_build_ms"], b[2]["bvh_build_ms"], b[2]["bvh_build_gpu_ms"]))
    assert b[2]["bvh_build_gpu_ms"] > 0


@pytest.mark.parametrize("algorithm", [0, 1])
def test_gpu_lbvh_builder_on_coincident_and_clustered_triangles(algorithm):
    """100 k triangles that defeat a Morton-code builder — 60 k exact copies of one triangle and 40 k inside a 1e-4 ball,
    next to walls metres away: the radix tree is deep (equal codes are split by index below a long common prefix), the
    traversal stack grows with it (more LDS per block, fewer blocks per CU), and the frame is still the SAH tree's frame,
    bit for bit, and the oracle's."""
    from oracle import oracle_py
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.clustered_box()
    assert sc.triangle_count >= 100_000
    frame = camera.Frame(160, 160, cam["fovy"], cam["eye"], cam["target"])
    rays = random_rays(20000, 9, -0.99, 0.99)
    res = {}
    for kind in (0, 1):
        r = BDPT(device=0)
        try:
            r.set_option("bvh_builder", kind)
            r.set_option("lbvh_algorithm", algorithm)
            r.update(sc)
            res[kind] = (r.render(frame, 0, 1), r.trace(rays), r.stats())
            flags, pc = r.mSamplingFlags, r.push_constants(frame)
        finally:
            r.close()
    a, b = res[0], res[1]
    assert np.array_equal(a[0]["radiance"].view(np.uint32), b[0]["radiance"].view(np.uint32))
    assert np.array_equal(a[0]["visibility"]["instance_primitive_index"], b[0]["visibility"]["instance_primitive_index"])
    for f in ("instance_primitive_index", "t", "b1", "b2"):
        assert np.array_equal(a[1][f].view(np.uint32), b[1][f].view(np.uint32)), f
    ref = oracle_py.OracleScene(sc).render(frame, pc, flags, 0, 1)
    assert np.array_equal(b[0]["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
    assert rel_l2(b[0]["radiance"], ref["radiance"]) <= 1e-4
    print("clustered (algorithm %d): lbvh build %.1f ms (gpu %.2f), sah %.1f ms" % (algorithm, b[2]["bvh_build_ms"], b[2]["bvh_build_gpu_ms"], a[2]["bvh_build_ms"]))


@pytest.mark.parametrize("algorithm", [0, 1])
def test_gpu_lbvh_rebuild_is_device_resident(atrium_scene, algorithm):
    """bvh_builder = 1 builds in place from the uploaded scene arrays (lbvh.hip: lbvh_build_device): no triangle and no
    node goes through the host except the one copy of the unpacked nodes the treetop selection reads. A REbuild (arena,
    device arrays and the pinned host buffer exist) of the 1 M-triangle atrium must stay under 15 ms for the builder and
    the frame must not change."""
    import time

    from stratum_amd.bdpt import BDPT

    sc, cam = atrium_scene
    frame = camera.Frame(160, 90, cam["fovy"], cam["eye"], cam["target"])
    r = BDPT(device=0)
    try:
        r.set_option("bvh_builder", 1)
        r.set_option("lbvh_algorithm", algorithm)
        r.update(sc)
        first = r.render(frame, 0, 1)
        build_ms, call_ms = [], []
        for _ in range(4):
            t0 = time.perf_counter()
            r.update(sc)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            build_ms.append(r.stats()["bvh_build_ms"])
        again = r.render(frame, 0, 1)
        st = r.stats()
    finally:
        r.close()
    assert np.array_equal(first["radiance"].view(np.uint32), again["radiance"].view(np.uint32))
    print("atrium %d triangles, algorithm %d, stack depth %d: rebuild %.1f ms (builder, min of 4; GPU kernels %.2f ms), whole sthip_scene_upload call %.1f ms" % (sc.triangle_count, algorithm, st.get("bvh_stack_depth", -1), min(build_ms), st["bvh_build_gpu_ms"], min(call_ms)))
    assert min(build_ms) <= 15.0, build_ms


@pytest.mark.parametrize("levels", [4, 7, 12])
def test_bounded_lds_stack_gives_the_same_frames(levels):
    """Trees higher than `lds_stack_levels` run k_trace<., ., BOUNDED>: the per-lane LDS stack has that many levels, a ray that
    needs more is void and k_trace_deep traces it again with a full-height stack in global memory. Forced here with tiny
    stacks on ordinary scenes (almost every ray overflows at 4 levels): frames, ray batches and ray counts must be those of
    the unbounded kernel, bit for bit — closest hits and shadow rays, instances, light tracing and connections (the
    visibility rays that splat or fill connection entries), media (segment walks), alpha masks."""
    from stratum_amd.bdpt import BDPT

    cases = [
        (scenes.cornell_box(), [], {}),
        (scenes.cornell_box(), ["connecttoviews", "connecttolightpaths"], {"maxDiffuseVertices": 3}),
        (scenes.forest(n_instances=25, tree_tris=500, tree_kinds=2), ["~defershadowrays"], {}),
        (scenes.spheres_room(), [], {"maxDiffuseVertices": 3}),
        (scenes.cornell_box(fog=_fog()), [], {"maxDiffuseVertices": 3}),
        (scenes.foliage(), ["alphatest"], {"maxDiffuseVertices": 3}),
    ]
    for (sc, cam), flags, args in cases:
        frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
        rays = random_rays(5000, 3, -2.5, 2.5)
        out = {}
        for cap in (None, levels):
            r = BDPT(device=0, args=dict(args, bdptFlag=flags))
            try:
                if cap is not None:
                    r.set_option("lds_stack_levels", cap)
                r.update(sc)
                out[cap] = (r.render(frame, 2, 2), r.trace(rays), r.trace(rays, any_hit=True))
            finally:
                r.close()
        a, b = out[None], out[levels]
        assert np.array_equal(a[0]["radiance"].view(np.uint32), b[0]["radiance"].view(np.uint32)), (sc.name, flags)
        assert np.array_equal(a[0]["visibility"]["instance_primitive_index"], b[0]["visibility"]["instance_primitive_index"])
        assert np.array_equal(a[0]["ray_count"], b[0]["ray_count"])
        for k in (1, 2):
            for f in ("instance_primitive_index", "t", "b1", "b2"):
                assert np.array_equal(a[k][f].view(np.uint32), b[k][f].view(np.uint32)), (sc.name, f)


@pytest.mark.parametrize("levels", [None, 6])
def test_wide_walk_gives_the_frames_of_the_binary_walk(atrium_scene, levels):
    """wide_bvh (on by default for host-built trees): k_trace walks the tree collapsed into 4-wide nodes of 64 bytes with 8-bit
    child planes (bvh.h: WideNode), or (wide_bvh = 3) into 8-wide compressed nodes of 80 bytes whose children are addressed
    by a base and a mask (bvh.h: Wide8Node; the stack then holds 64-bit groups). Every decoded box contains the box it stands
    for and every leaf holds the binary tree's triangles, so the hits — and with them frames and ray counts, bit for bit — are those of the binary walk (wide_bvh = 0):
    merged mesh + instances (atrium), two-level forest, spheres, media segment walks, alpha masks, light tracing and
    connections; with full LDS stacks and with 6-level ones (three pushes per level: almost every ray overflows and is traced
    again by k_trace_deep over the binary tree)."""
    from stratum_amd.bdpt import BDPT

    cases = [
        (atrium_scene, [], {"maxDiffuseVertices": 3}),
        (scenes.cornell_box(), ["connecttoviews", "connecttolightpaths"], {"maxDiffuseVertices": 3}),
        (scenes.forest(n_instances=25, tree_tris=500, tree_kinds=2), ["~defershadowrays"], {}),
        (scenes.spheres_room(), [], {"maxDiffuseVertices": 3}),
        (scenes.cornell_box(fog=_fog()), [], {"maxDiffuseVertices": 3}),
        (scenes.foliage(), ["alphatest"], {"maxDiffuseVertices": 3}),
    ]
    for (sc, cam), flags, args in cases:
        frame = camera.Frame(160, 96, cam["fovy"], cam["eye"], cam["target"])
        out = {}
        for wide in (0, 1, 3):
            r = BDPT(device=0, args=dict(args, bdptFlag=flags))
            try:
                r.set_option("wide_bvh", wide)
                if levels is not None:
                    r.set_option("lds_stack_levels", levels)
                r.update(sc)
                out[wide] = r.render(frame, 1, 2)
                assert r.stats()["bvh_node_bytes"] == {0: 48, 1: 64, 3: 80}[wide], (sc.name, wide)
            finally:
                r.close()
        for wide in (1, 3):
            a, b = out[0], out[wide]
            assert np.array_equal(a["radiance"].view(np.uint32), b["radiance"].view(np.uint32)), (sc.name, flags, wide)
            assert np.array_equal(a["visibility"]["instance_primitive_index"], b["visibility"]["instance_primitive_index"]), (sc.name, wide)
            assert np.array_equal(a["ray_count"], b["ray_count"]), (sc.name, wide)


@pytest.mark.parametrize("levels", [None, 7])
def test_wide_walk_over_gpu_built_trees_and_moved_instances(atrium_scene, levels):
    """The wide form is also made on the device (wide.hip), from the packed nodes as they lie in HBM: for the trees of the GPU
    builder (bvh_builder = 1: PLOC with and without the SAH top, the radix tree) and again after a transforms-only update
    (the top level is new; host- and GPU-built bottom levels). Frames, visibility and ray counts must be those of the
    binary walk over the same tree, and a moved scene must give what a fresh upload of it gives; stats say which nodes
    k_trace walked (64-byte ones)."""
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import rotate_y, translate

    def same(a, b, what):
        assert np.array_equal(a["radiance"].view(np.uint32), b["radiance"].view(np.uint32)), what
        assert np.array_equal(a["visibility"]["instance_primitive_index"], b["visibility"]["instance_primitive_index"]), what
        assert np.array_equal(a["ray_count"], b["ray_count"]), what

    cases = [
        (atrium_scene, [], {"maxDiffuseVertices": 3}),
        (scenes.forest(n_instances=30, tree_tris=700, tree_kinds=2), [], {}),
        (scenes.spheres_room(), [], {"maxDiffuseVertices": 3}),
        (scenes.foliage(), ["alphatest"], {}),
    ]
    for (sc, cam), flags, args in cases:
        frame = camera.Frame(160, 96, cam["fovy"], cam["eye"], cam["target"])
        for builder, algorithm, sah_top in ((1, 1, 64), (1, 1, 0), (1, 0, 0), (0, 1, 64)):
            out = {}
            for wide in (0, 1, 3):
                node_bytes = {0: 48, 1: 64, 3: 80 if builder == 0 else 64}[wide]  # (GPU-built trees get the 4-wide form where the 8-wide one is asked for)
                r = BDPT(device=0, args=dict(args, bdptFlag=flags))
                try:
                    r.set_option("bvh_builder", builder)
                    r.set_option("lbvh_algorithm", algorithm)
                    r.set_option("sah_top", sah_top)
                    r.set_option("wide_bvh", wide)
                    if levels is not None:
                        r.set_option("lds_stack_levels", levels)
                    r.update(sc)
                    out[wide] = [r.render(frame, 1, 2)]
                    if builder == 1 and wide == 3:  # (bottom levels too small for the GPU builder are host-built: a scene of only such meshes gets the 8-wide form)
                        node_bytes = r.stats()["bvh_node_bytes"]
                        assert node_bytes in (64, 80)
                    assert r.stats()["bvh_node_bytes"] == node_bytes, (sc.name, builder, wide)
                    # move every instance that is not part of the merged identity mesh, render, move back
                    ident = np.array([np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]])
                    kinds = sc.instances["packed"][:, 0] & 0xF
                    movable = [int(i) for i in np.nonzero(~ident)[0][:10] if kinds[i] == wire.INSTANCE_TYPE_TRIANGLES]
                    if movable:
                        old = {i: np.vstack([sc.transforms["m"][i], [0, 0, 0, 1]]).astype(np.float64) for i in movable}
                        for k, i in enumerate(movable):
                            sc.set_instance_transform(i, translate((0.11 * ((k % 3) - 1), 0.0, -0.07 * (k % 2))) @ old[i] @ rotate_y(0.2 * k))
                        r.update_transforms(sc)
                        out[wide].append(r.render(frame, 1, 2))
                        assert r.stats()["bvh_node_bytes"] == node_bytes, (sc.name, builder, wide, "after the update")
                        r.update(sc)
                        out[wide].append(r.render(frame, 1, 2))
                        for i in movable:
                            sc.set_instance_transform(i, old[i])
                finally:
                    r.close()
            for wide in (1, 3):
                for k, (a, b) in enumerate(zip(out[0], out[wide])):
                    same(a, b, (sc.name, flags, builder, algorithm, sah_top, wide, k))
                if len(out[wide]) == 3:
                    same(out[wide][1], out[wide][2], (sc.name, "moved scene against its fresh upload", builder, wide))
                    assert not np.array_equal(out[wide][0]["radiance"], out[wide][1]["radiance"]), sc.name


def test_embedded_leaves_give_the_same_frames(atrium_scene):
    """embed_leaves = 1: the host builder puts a leaf's triangles into the node array, in the units right behind the node that
    refers to them (one array, leaf references count its units). A layout experiment (no faster: EXPERIMENTS.md) kept as an
    option; frames, alpha-masked frames and ray batches must not change."""
    from stratum_amd.bdpt import BDPT

    for (sc, cam), flags in ((atrium_scene, []), (scenes.foliage(), ["alphatest"]), (scenes.forest(n_instances=20, tree_tris=400, tree_kinds=2), [])):
        frame = camera.Frame(160, 90, cam["fovy"], cam["eye"], cam["target"])
        rays = random_rays(20000, 8, -6.0, 6.0)
        out = {}
        for embed in (0, 1):
            r = BDPT(device=0, args={"bdptFlag": flags, "maxDiffuseVertices": 3})
            try:
                r.set_option("embed_leaves", embed)
                r.update(sc)
                out[embed] = (r.render(frame, 0, 2), r.trace(rays), r.trace(rays, any_hit=True, alpha_test=bool(flags)))
            finally:
                r.close()
        a, b = out[0], out[1]
        assert np.array_equal(a[0]["radiance"].view(np.uint32), b[0]["radiance"].view(np.uint32))
        assert np.array_equal(a[0]["ray_count"], b[0]["ray_count"])
        for k in (1, 2):
            for f in ("instance_primitive_index", "t", "b1", "b2"):
                assert np.array_equal(a[k][f].view(np.uint32), b[k][f].view(np.uint32)), f


@pytest.mark.parametrize("algorithm", [0, 1])
def test_gpu_lbvh_edge_sizes(algorithm):
    """The device builder at the sizes where it hands over to the host builder (fewer than 64 triangles per mesh), at its
    smallest own sizes (64, 65 triangles: a PLOC run of two rounds' worth), with an odd byte stride mix (16- and 32-bit
    indices) and an identity mesh next to transformed ones: ray batches equal the SAH build's."""
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import SceneBuilder, rotate_y, scale, translate

    def soup(sizes, seed):
        rng = np.random.RandomState(seed)
        b = SceneBuilder("edge")
        m = b.add_material((0.5, 0.5, 0.5))
        e = b.add_emitter((5.0, 5.0, 5.0))
        for k, tris in enumerate(sizes):
            c = rng.uniform(-1, 1, (tris, 1, 3))
            pts = (c + rng.normal(scale=0.2, size=(tris, 3, 3))).reshape(-1, 3)
            mesh = b.add_mesh(pts, None, None, np.arange(tris * 3).reshape(-1, 3), index_stride=2 if k % 2 else 4)
            b.add_instance(mesh, e if k == 0 else m, None if k < 2 else translate(rng.uniform(-1, 1, 3)) @ rotate_y(rng.uniform(0, 6)) @ scale(rng.uniform(0.5, 1.5, 3)))
        return b.build()

    rays = random_rays(30000, 21, -2.5, 2.5)
    for sizes in ([1], [63], [64], [65], [2, 63, 64, 200, 7], [64, 64, 64]):
        sc = soup(sizes, 5 + len(sizes))
        out = {}
        for kind in (0, 1):
            r = BDPT(device=0)
            try:
                r.set_option("bvh_builder", kind)
                r.set_option("lbvh_algorithm", algorithm)
                r.update(sc)
                out[kind] = (r.trace(rays), r.trace(rays, any_hit=True))
            finally:
                r.close()
        for k in (0, 1):
            for f in ("instance_primitive_index", "t", "b1", "b2"):
                assert np.array_equal(out[0][k][f].view(np.uint32), out[1][k][f].view(np.uint32)), (sizes, f)
        assert (out[0][0]["instance_primitive_index"] != wire.MISS).any()


def test_gpu_lbvh_device_and_host_regions():
    """A scene whose bottom levels are split between the two builders in device mode: the forest's shared meshes (>= 64
    triangles: built on the GPU in place) next to tiny meshes (< 64 triangles: host SAH, placed behind the device region
    with their references offset), under a host-built top level — frames and ray batches equal the SAH build's, also
    after instances moved (top level rebuilt through the host copy of the nodes)."""
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import translate

    sc, cam = scenes.forest(n_instances=40, tree_tris=900, tree_kinds=3)
    sc2, _ = scenes.spheres_room()  # small boxes: meshes of 12 triangles, and spheres as top-level entries
    for scene_, cam_ in ((sc, cam), (sc2, scenes.spheres_room()[1])):
        frame = camera.Frame(192, 96, cam_["fovy"], cam_["eye"], cam_["target"])
        rays = random_rays(20000, 4, -3.0, 3.0)
        res = {}
        for kind in (0, 1):
            r = BDPT(device=0, args={"maxDiffuseVertices": 3})
            try:
                r.set_option("bvh_builder", kind)
                r.update(scene_)
                a = (r.render(frame, 1, 2), r.trace(rays))
                kinds = scene_.instances["packed"][:, 0] & 0xF
                ident = np.array([np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in scene_.transforms["m"]])
                movers = np.nonzero((kinds == 0) & ~ident)[0]
                moved = None
                if movers.size:
                    saved = scene_.transforms["m"][movers[0]].copy()
                    m = saved.copy()
                    m[:, 3] += np.float32(0.25)
                    scene_.set_instance_transform(int(movers[0]), m)
                    r.update_transforms(scene_)
                    moved = r.render(frame, 1, 2)
                    scene_.set_instance_transform(int(movers[0]), saved)
                res[kind] = (a, moved)
            finally:
                r.close()
        (a0, m0), (a1, m1) = res[0], res[1]
        assert np.array_equal(a0[0]["radiance"].view(np.uint32), a1[0]["radiance"].view(np.uint32))
        assert np.array_equal(a0[0]["ray_count"], a1[0]["ray_count"])
        for f in ("instance_primitive_index", "t", "b1", "b2"):
            assert np.array_equal(a0[1][f].view(np.uint32), a1[1][f].view(np.uint32)), f
        if m0 is not None:
            assert np.array_equal(m0["radiance"].view(np.uint32), m1["radiance"].view(np.uint32))
            assert not np.array_equal(m0["radiance"], a0[0]["radiance"])


def test_gpu_lbvh_rejects_a_bad_index():
    """The index check moves into the fetch kernel in device mode: a vertex index outside gVertices is still an
    STHIP_ERR_INVALID_ARGUMENT, and the context then has no scene."""
    from stratum_amd import _lib
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.atrium(target_tris=3000)
    good = sc.indices.copy()
    tri_insts = np.nonzero((sc.instances["packed"][:, 0] & 0xF) == 0)[0]
    last = max(tri_insts, key=lambda i: int(sc.instances["packed"][i, 3]))  # the instance whose indices end the buffer
    stride, first_vertex = int(sc.instances["packed"][last, 1] >> 28), int(sc.instances["packed"][last, 2])
    value = 0xFFFF if stride == 2 else 0x7FFFFFFF
    assert first_vertex + value >= sc.vertices.shape[0]
    r = BDPT(device=0)
    try:
        r.set_option("bvh_builder", 1)
        r.update(sc)
        sc.indices = good.copy()
        sc.indices[-stride:] = np.frombuffer(value.to_bytes(stride, "little"), dtype=np.uint8)  # the last index of the last triangle
        with pytest.raises(_lib.StratumHipError, match="vertex index exceeds gVertices"):
            r.update(sc)
        with pytest.raises(_lib.StratumHipError):
            r.render(camera.Frame(32, 16, cam["fovy"], cam["eye"], cam["target"]))
        sc.indices = good
        r.update(sc)  # and the context recovers with a good scene
        r.render(camera.Frame(32, 16, cam["fovy"], cam["eye"], cam["target"]))
    finally:
        r.close()

@pytest.mark.parametrize("flags", [[], ["~raycones"], ["flipnormalmaps", "fliptriangleuvs"], ["~normalmaps"], ["shadingnormalshadowfix"]])
def test_textured_scene(flags):
    """Image values (base colour, roughness/metallic maps, textured emitter), mip selection through ray cones,
    normal maps — software repeat/trilinear sampler on both sides."""
    from oracle import oracle_py
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.textured_box()
    r = BDPT(device=0, args={"bdptFlag": flags, "maxDiffuseVertices": 3})
    try:
        r.update(sc)
        frame = camera.Frame(192, 160, cam["fovy"], cam["eye"], cam["target"])
        got = r.render(frame, 0, 2)
        ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, 2)
        assert np.array_equal(got["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
        assert np.array_equal(got["visibility"]["packed_normal"], ref["visibility"]["packed_normal"])
        assert np.array_equal(got["albedo"].view(np.uint32), ref["albedo"].view(np.uint32))
        assert np.array_equal(got["ray_count"], ref["ray_count"])
        d = rel_l2(got["radiance"], ref["radiance"])
        nd = int((got["radiance"].view(np.uint32) != ref["radiance"].view(np.uint32)).any(axis=-1).sum())
        print("textured %s rel-L2 %.3e, differing pixels %d" % (flags, d, nd))
        assert d <= 1e-4
    finally:
        r.close()


def test_roughness_map_reaching_zero_makes_specular_chains(renderer):
    """A material that is specular only through its texture (metallic 1, roughness constant 0.6 times a map whose dark
    squares are 0): the host must not cap the bounce rounds at gMaxDiffuseVertices + 1 from the constants alone, or
    the radiance of the mirror chains (up to gMaxPathVertices - 1 rays) is lost. Bit-exact ids and ray counts."""
    sc, cam = scenes.textured_box(mirror_map=True)
    got = _compare_frame(sc, cam, [], w=192, h=160, seeds=2, args={"maxPathVertices": 8, "maxDiffuseVertices": 2})
    # the chains beyond gMaxDiffuseVertices + 1 rays exist in this scene: cutting the path length at 4 vertices loses rays
    short = _compare_frame(sc, cam, [], w=192, h=160, seeds=2, args={"maxPathVertices": 4, "maxDiffuseVertices": 2})
    assert int(got["ray_count"][1]) > int(short["ray_count"][1])


# ---- sphere instances / sphere lights / environment maps ----
def _compare_frame(sc, cam, flags, w=176, h=128, seeds=2, args=None):
    from oracle import oracle_py
    from stratum_amd.bdpt import BDPT

    a = {"bdptFlag": flags}
    a.update(args or {})
    r = BDPT(device=0, args=a)
    try:
        r.update(sc)
        frame = camera.Frame(w, h, cam["fovy"], cam["eye"], cam["target"])
        got = r.render(frame, 0, seeds)
        ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, seeds)
        assert np.array_equal(got["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
        assert np.array_equal(got["visibility"]["packed_normal"], ref["visibility"]["packed_normal"])
        assert np.array_equal(got["albedo"].view(np.uint32), ref["albedo"].view(np.uint32))
        assert np.array_equal(got["depth"]["z"].view(np.uint32), ref["depth"]["z"].view(np.uint32))
        assert np.array_equal(got["ray_count"], ref["ray_count"])
        d = rel_l2(got["radiance"], ref["radiance"])
        nd = int((got["radiance"].view(np.uint32) != ref["radiance"].view(np.uint32)).any(axis=-1).sum())
        print("%s %s rel-L2 %.3e, differing pixels %d, rays %s" % (sc.name, flags, d, nd, got["ray_count"]))
        assert np.isfinite(got["radiance"]).all() and got["radiance"][..., :3].mean() > 0.01
        assert d <= 1e-4
        return got
    finally:
        r.close()


def test_trace_contract_with_spheres(renderer):
    """Sphere instances next to triangle meshes: closest hit and occlusion equal the oracle's brute force."""
    from oracle import oracle_py

    sc, _ = scenes.spheres_room()
    renderer.update(sc)
    o = oracle_py.OracleScene(sc)
    rays = random_rays(60000, 4, -1.9, 2.9)
    got = renderer.trace(rays)
    ref, _ = o.trace(rays, brute=True)
    for f in ("instance_primitive_index", "t", "b1", "b2"):
        assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f
    on_sphere = (ref["instance_primitive_index"] >> 16 == 0xFFFF) & (ref["instance_primitive_index"] != wire.MISS)
    assert on_sphere.mean() > 0.03
    rays["tmax"] = 1.2
    got = renderer.trace(rays, any_hit=True)
    ref, _ = o.trace(rays, any_hit=True, brute=True)
    assert np.array_equal(got["instance_primitive_index"], ref["instance_primitive_index"])


@pytest.mark.parametrize("flags", [[], ["uniformspheresampling"], ["~defershadowrays"], ["~nee"], ["~samplebsdfs"], ["shadingnormalshadowfix", "neereservoirs"]])
def test_sphere_instances_and_sphere_lights(flags):
    sc, cam = scenes.spheres_room()
    _compare_frame(sc, cam, flags, args={"maxDiffuseVertices": 3})


@pytest.mark.parametrize("image,emitter", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("flags", [[], ["~mis"], ["sampleenvironmentmapdirectly"]])
def test_environment(image, emitter, flags):
    """Environment emission on misses, environment light sampling (dist2d tables of the lat-long image, or the
    image-less constant environment), and the environment / emitter choice (gEnvironmentSampleProbability)."""
    sc, cam = scenes.environment_scene(image=image, emitter=emitter)
    got = _compare_frame(sc, cam, flags)
    sky = got["visibility"]["instance_primitive_index"] == wire.MISS
    assert sky.mean() > 0.2 and got["radiance"][sky][:, :3].min() > 0.05


def test_environment_errors(renderer):
    from stratum_amd import _lib

    sc, cam = scenes.environment_scene(image=True, emitter=False)
    renderer.update(sc)
    frame = camera.Frame(32, 32, cam["fovy"], cam["eye"], cam["target"])
    renderer.set_flag("samplelightpower")  # reads a table upstream never fills: rejected, never ignored
    with pytest.raises(_lib.StratumHipError, match="sampling flag"):
        renderer.render(frame)
    renderer.set_flag("~samplelightpower")
    sc.distributions = sc.distributions[:-5]  # a table that runs past gDistributions
    renderer.update(sc)
    with pytest.raises(_lib.StratumHipError, match="gDistributions"):
        renderer.render(frame)


def test_packed_tiles_and_assembly(renderer, cornell):
    """The exchange format of the multi-GPU path: each shard's tiles in slot order (STHIP_LAYOUT_SHARD_TILES),
    scattered back by sthip_assemble_tiles, reproduce the unsharded frame bit for bit; the host mirror agrees."""
    import torch

    from stratum_amd import shard

    sc, cam = cornell
    renderer.update(sc)
    W, H, world, seeds = 200, 136, 3, 2  # neither extent is a multiple of the tile size
    frame = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    renderer.set_shard(0, 1)
    full = renderer.render(frame, 0, seeds, aovs=False)["radiance"]
    stride = shard.slot_count(W, H, 0, world, 16, 8)
    gathered = torch.zeros((world, stride, 4), dtype=torch.float32, device="cuda")
    host = []
    try:
        for rank in range(world):
            renderer.set_shard(rank, world, 16, 8)
            assert renderer.shard_slot_count(frame) == shard.slot_count(W, H, rank, world, 16, 8)
            renderer.render(frame, 0, seeds, device_outputs={"radiance": gathered[rank].data_ptr()}, packed_tiles=True)
            host.append(renderer.render(frame, 0, seeds, aovs=False, packed_tiles=True)["radiance"])
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        renderer.assemble_tiles(frame, gathered.data_ptr(), stride, out.data_ptr())
        torch.cuda.synchronize()
    finally:
        renderer.set_shard(0, 1)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), full.view(np.uint32))
    assert np.array_equal(shard.assemble_tiles(host, W, H, 16, 8).view(np.uint32), full.view(np.uint32))



def test_moving_camera_aovs(renderer, cornell):
    """gPrevViews / gPrevInverseViewTransforms of a camera that moved since the last frame: prev-uv, prev_z and dz/dxy
    (the inputs of the temporal reprojection) equal the oracle's."""
    from oracle import oracle_py

    sc, cam = cornell
    renderer.update(sc)
    W, H = 160, 120
    prev = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
    eye = tuple(np.array(cam["eye"]) + np.array([0.07, -0.03, 0.1]))
    frame = camera.Frame(W, H, cam["fovy"], eye, cam["target"], prev=prev)
    got = renderer.render(frame, 5, 1)
    ref = oracle_py.OracleScene(sc).render(frame, renderer.push_constants(frame), renderer.mSamplingFlags, 5, 1)
    assert np.array_equal(got["prev_uv"].view(np.uint32), ref["prev_uv"].view(np.uint32))
    for f in ("z", "prev_z", "dz_dxy"):
        assert np.array_equal(got["depth"][f].view(np.uint32), ref["depth"][f].view(np.uint32)), f
    assert np.array_equal(got["radiance"].view(np.uint32), ref["radiance"].view(np.uint32))
    hit = ref["visibility"]["instance_primitive_index"] != wire.MISS
    uv = (np.stack(np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5), -1) / [W, H]).astype(np.float32)
    moved = np.abs(ref["prev_uv"] - uv).max(-1)
    assert moved[hit].mean() > 2e-3  # the reprojected position really differs from the pixel's own


def test_trace_contract_with_alpha_masks(renderer):
    from oracle import oracle_py

    sc, _ = scenes.foliage()
    renderer.update(sc)
    o = oracle_py.OracleScene(sc)
    rays = random_rays(60000, 6, -2.0, 2.5)
    for flip in (False, True):
        got = renderer.trace(rays, alpha_test=True, flip_uvs=flip)
        ref, _ = o.trace(rays, brute=True, alpha_test=True, flip_uvs=flip)
        for f in ("instance_primitive_index", "t", "b1", "b2"):
            assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), (f, flip)
    solid = renderer.trace(rays)
    ref_solid, _ = o.trace(rays, brute=True)
    assert np.array_equal(solid["instance_primitive_index"], ref_solid["instance_primitive_index"])
    assert (solid["instance_primitive_index"] != got["instance_primitive_index"]).mean() > 0.005
    rays["tmax"] = 3.0
    got = renderer.trace(rays, any_hit=True, alpha_test=True)
    ref, _ = o.trace(rays, any_hit=True, brute=True, alpha_test=True)
    assert np.array_equal(got["instance_primitive_index"], ref["instance_primitive_index"])


@pytest.mark.parametrize("flags", [["alphatest"], [], ["alphatest", "fliptriangleuvs", "~defershadowrays"]])
def test_alpha_masked_foliage(flags):
    sc, cam = scenes.foliage()
    _compare_frame(sc, cam, flags, args={"maxDiffuseVertices": 3})


def test_alpha_masks_with_the_gpu_builder():
    """Scenes with alpha masks go through the GPU builder too: the uvs the traversal's alpha test interpolates are
    filled on the device from the resident leaf triangles (k_fill_tri_shade), whoever built the tree. The frame and the ray
    batches are those of the host-built tree; without the flag the masks do not apply."""
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.foliage()
    frame = camera.Frame(160, 96, cam["fovy"], cam["eye"], cam["target"])
    rays = random_rays(20000, 8, -6.0, 6.0)
    out = {}
    for builder in (0, 1):
        r = BDPT(device=0, args={"bdptFlag": ["alphatest"]})
        try:
            r.set_option("bvh_builder", builder)
            r.update(sc)
            out[builder] = (r.render(frame, 1, 2), r.trace(rays, alpha_test=True), r.trace(rays, any_hit=True, alpha_test=True), r.trace(rays))
        finally:
            r.close()
    a, b = out[0], out[1]
    assert np.array_equal(a[0]["radiance"].view(np.uint32), b[0]["radiance"].view(np.uint32))
    assert np.array_equal(a[0]["visibility"]["instance_primitive_index"], b[0]["visibility"]["instance_primitive_index"])
    assert np.array_equal(a[0]["ray_count"], b[0]["ray_count"])
    for k in (1, 2, 3):
        for f in ("instance_primitive_index", "t", "b1", "b2"):
            assert np.array_equal(a[k][f].view(np.uint32), b[k][f].view(np.uint32)), (k, f)
    assert not np.array_equal(b[1]["instance_primitive_index"], b[3]["instance_primitive_index"])  # the masks do cut something


@pytest.mark.parametrize("flags", [["presamplelights"], ["presamplelights", "~remapthreads", "~defershadowrays"], ["presamplelights", "~samplebsdfs"]])
def test_presampled_lights(flags):
    """ePresampleLights (bdpt.hlsl:84-99, path.hlsli:313-320): NEE picks one of gLightPresampleTileSize points of the
    tile the path index selects; the points are drawn once per seed with rng_init(-1, index)."""
    sc, cam = scenes.cornell_box()
    _compare_frame(sc, cam, flags, seeds=3, args={"lightPresampleTileSize": 64, "lightPresampleTileCount": 16})
    sc, cam = scenes.spheres_room()  # sphere lights keep their solid-angle pdf in the presampled point, as upstream
    _compare_frame(sc, cam, flags, seeds=2)


def test_presampled_lights_with_an_environment_are_rejected(renderer):
    from stratum_amd import _lib

    sc, cam = scenes.environment_scene(image=False, emitter=True)
    renderer.update(sc)
    renderer.set_flag("presamplelights")
    try:
        with pytest.raises(_lib.StratumHipError, match="ePresampleLights with an environment"):
            renderer.render(camera.Frame(32, 32, cam["fovy"], cam["eye"], cam["target"]))
    finally:
        renderer.set_flag("~presamplelights")


@pytest.mark.parametrize("flags", [["neereservoirs"], ["neereservoirs", "presamplelights"], ["neereservoirs", "~defershadowrays"], ["neereservoirs", "~samplebsdfs"]])
def test_nee_reservoirs(flags):
    """eNEEReservoirs without reuse (connect_light_reservoir, path.hlsli:368-486): resampled importance sampling over
    gReservoirM light candidates, fresh or presampled."""
    sc, cam = scenes.cornell_box()
    _compare_frame(sc, cam, flags, seeds=2)
    sc, cam = scenes.spheres_room()
    _compare_frame(sc, cam, flags, seeds=1, args={"maxDiffuseVertices": 3})
    if "presamplelights" not in flags:
        sc, cam = scenes.environment_scene(image=True, emitter=True)
        _compare_frame(sc, cam, flags, seeds=1)


@pytest.mark.parametrize(
    "flags,args",
    [
        (["neereservoirs", "neereservoirreuse"], {"reservoirM": 4}),
        (["neereservoirs", "neereservoirreuse", "jitterhashgridlookups"], {"reservoirM": 2, "reservoirSpatialM": 3}),
        (["neereservoirs", "neereservoirreuse", "presamplelights", "~defershadowrays"], {"reservoirM": 3}),
        (["neereservoirs", "neereservoirreuse"], {"reservoirM": 2, "hashGridBucketCount": 40}),  # cells compete: probing, dropped records
        (["neereservoirs", "neereservoirreuse", "~remapthreads"], {"reservoirM": 1, "reservoirSpatialM": 8, "maxDiffuseVertices": 3}),
    ],
)
def test_nee_reservoir_reuse(flags, args):
    """eNEEReservoirReuse: every view vertex's light reservoir goes into a spatial hash grid, and the next frame's vertices
    resample from the bucket they fall into (path.hlsli:396-439, hashgrid.hlsli). Frames are the seeds of a call: seed s
    reads the grid of seed s - 1. Upstream builds the grid with atomics; under the defined order (appends in path order,
    hashgrid.h) the four-seed frame is the oracle's, bit for bit in ids and ray counts."""
    sc, cam = scenes.cornell_box()
    _compare_frame(sc, cam, flags, w=100, h=76, seeds=4, args=args)


def test_hash_grid_build_paths_agree():
    """The reuse grids are built on the device (hashgrid.hip): in parallel by priority insertion, or — in the rare frame where
    two cells share a 32-bit checksum — by one thread running the serial probe sequence. Both must give the grid the defined
    order gives: the same frames with the serial path forced, with a table so small that cells compete and records drop."""
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(100, 76, cam["fovy"], cam["eye"], cam["target"])
    for flags, args in (
        (["neereservoirs", "neereservoirreuse"], {"reservoirM": 2, "hashGridBucketCount": 40}),
        (["neereservoirs", "neereservoirreuse"], {"reservoirM": 4}),
        (["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "lvcreservoirreuse"], {"lightPathCount": 3000, "hashGridBucketCount": 500}),
    ):
        out = []
        for serial in (0, 1):
            r = BDPT(device=0, args=dict(args, bdptFlag=flags))
            try:
                r.set_option("hashgrid_serial", serial)
                r.update(sc)
                out.append(r.render(frame, 0, 4))
            finally:
                r.close()
        assert np.array_equal(out[0]["radiance"].view(np.uint32), out[1]["radiance"].view(np.uint32)), (flags, args)
        assert np.array_equal(out[0]["ray_count"], out[1]["ray_count"]), (flags, args)


def test_two_views_in_one_frame(renderer, cornell):
    """gViewCount = 2 (one ViewData per eye with its own image rectangle, scene.h:132-137): every output of both halves
    equals the oracle's; pixels outside every view (odd width: the last column) stay untouched."""
    from oracle import oracle_py

    sc, cam = cornell
    renderer.update(sc)
    frame = camera.Frame.stereo(161, 96, cam["fovy"], cam["eye"], cam["target"], eye_separation=0.3)
    got = renderer.render(frame, 2, 2)
    ref = oracle_py.OracleScene(sc).render(frame, renderer.push_constants(frame), renderer.mSamplingFlags, 2, 2)
    for k in ("radiance", "albedo", "prev_uv"):
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
    assert np.array_equal(got["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
    assert np.array_equal(got["depth"]["z"].view(np.uint32), ref["depth"]["z"].view(np.uint32))
    assert np.array_equal(got["ray_count"], ref["ray_count"])
    assert np.all(got["radiance"][:, 160] == 0) and got["radiance"][:, :160, 3].min() == 2
    # the two eyes see the box from different positions
    assert np.abs(got["radiance"][:, :80, :3] - got["radiance"][:, 80:160, :3]).mean() > 1e-3


@pytest.mark.parametrize("flags", [["connecttoviews"], ["connecttoviews", "~nee"], ["connecttoviews", "~mis"], ["connecttoviews", "~samplebsdfs", "~defershadowrays"], ["connecttoviews", "~remapthreads", "presamplelights"]])
def test_light_tracing(flags):
    """eConnectToViews: light subpaths (sample_photons, bdpt.hlsl:101-147) connect their vertices to the camera and splat
    into gLightTraceSamples (quantised integer sums: order-independent), view paths use the BDPT weights
    (path.hlsli:341-351,870-880), add_light_trace adds the two."""
    sc, cam = scenes.cornell_box()
    _compare_frame(sc, cam, flags, w=100, h=76, seeds=2)  # extents that are not multiples of the 8x4 groups
    sc, cam = scenes.spheres_room()
    _compare_frame(sc, cam, flags + ["uniformspheresampling"], w=96, h=64, seeds=1, args={"maxDiffuseVertices": 3})


@pytest.mark.parametrize(
    "flags,args",
    [
        (["connecttolightpaths", "lightvertexcache"], {"lightPathCount": 4000}),
        (["connecttolightpaths", "lightvertexcache", "~defershadowrays"], {"lightPathCount": 7600}),
        (["connecttolightpaths", "lightvertexcache", "~nee"], {"lightPathCount": 3000}),
        (["connecttolightpaths", "lightvertexcache", "lvcreservoirs"], {"lightPathCount": 5000, "reservoirM": 6}),
        (["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "~defershadowrays", "~mis"], {"lightPathCount": 2500, "reservoirM": 3}),
        (["connecttolightpaths", "lightvertexcache", "connecttoviews"], {"lightPathCount": 6000}),
        (["connecttolightpaths", "lightvertexcache"], {"lightPathCount": 1}),  # a cache that may well stay empty
    ],
)
def test_light_vertex_cache(flags, args):
    """eLVC (+ eLVCReservoirs): light subpaths store their vertices in a cache, a view vertex connects to ONE cache entry
    (path.hlsli:491-531,683-800). Upstream allots cache slots with an atomic counter; the order defined here (paths by
    index, a path's vertices in storing order) is one a serial run of upstream produces — under it the frame is the
    oracle's, bit for bit in ids and ray counts. gLightPathCount is the caller's with the cache on (BDPT.cpp:469-470)."""
    sc, cam = scenes.cornell_box()
    a = dict(args, maxDiffuseVertices=3, maxPathVertices=6)
    _compare_frame(sc, cam, flags, w=100, h=76, seeds=2, args=a)


@pytest.mark.parametrize(
    "flags,args",
    [
        (["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "lvcreservoirreuse"], {"lightPathCount": 5000, "reservoirM": 4}),
        (["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "lvcreservoirreuse", "jitterhashgridlookups", "~defershadowrays"], {"lightPathCount": 3000, "reservoirM": 2, "reservoirSpatialM": 3}),
        (["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "lvcreservoirreuse", "neereservoirs", "neereservoirreuse"], {"lightPathCount": 4000, "reservoirM": 2, "hashGridBucketCount": 60}),
        (["connecttolightpaths", "connecttoviews", "neereservoirs", "~defershadowrays"], {"reservoirM": 3}),  # connect_light_reservoir's BDPT weight (path.hlsli:458-465)
    ],
)
def test_lvc_reservoir_reuse(flags, args):
    """eLVCReservoirReuse: connect_lvc's reservoirs go through a hash grid of their own (path.hlsli:727-768), alone and
    together with the NEE grid; four seeds, so three of them read a previous grid."""
    sc, cam = scenes.cornell_box()
    _compare_frame(sc, cam, flags, w=100, h=76, seeds=4, args=dict(args, maxDiffuseVertices=3, maxPathVertices=6))


def test_light_vertex_cache_textured_and_limits(renderer):
    sc, cam = scenes.textured_box()
    _compare_frame(sc, cam, ["connecttolightpaths", "lightvertexcache", "lvcreservoirs"], w=96, h=80, seeds=1, args={"lightPathCount": 3000, "maxDiffuseVertices": 3, "reservoirM": 4})
    # the cache needs at least one storable vertex level, and a sane size
    sc, cam = scenes.cornell_box()
    renderer.update(sc)
    frame = camera.Frame(64, 64, cam["fovy"], cam["eye"], cam["target"])
    renderer.set_flag("connecttolightpaths")
    renderer.set_flag("lightvertexcache")
    old = (renderer.mPushConstants.gMaxDiffuseVertices, renderer.mPushConstants.gLightPathCount)
    try:
        renderer.mPushConstants.gMaxDiffuseVertices = 1
        with pytest.raises(Exception, match="eLVC needs gMaxDiffuseVertices >= 2"):
            renderer.render(frame, 0, 1)
        renderer.mPushConstants.gMaxDiffuseVertices = 2
        renderer.mPushConstants.gLightPathCount = 0
        with pytest.raises(Exception, match="gLightPathCount"):
            renderer.render(frame, 0, 1)
    finally:
        renderer.mPushConstants.gMaxDiffuseVertices, renderer.mPushConstants.gLightPathCount = old
        renderer.set_flag("~connecttolightpaths")
        renderer.set_flag("~lightvertexcache")


def test_light_tracing_textured_and_sharded(renderer):
    from stratum_amd import shard

    sc, cam = scenes.textured_box()
    _compare_frame(sc, cam, ["connecttoviews", "~nee"], w=96, h=80, seeds=1)
    # shards keep the splats that land on their own tiles: the sum over shards is the unsharded frame
    sc, cam = scenes.cornell_box()
    renderer.update(sc)
    renderer.set_flag("connecttoviews")
    try:
        frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
        full = renderer.render(frame, 0, 2, aovs=False)["radiance"]
        total = np.zeros_like(full)
        for rank in range(3):
            renderer.set_shard(rank, 3, 16, 8)
            part = renderer.render(frame, 0, 2, aovs=False)["radiance"]
            assert np.all(part[shard.owner_map(96, 64, 3, 16, 8) != rank] == 0)
            total += part
        assert np.array_equal(total.view(np.uint32), full.view(np.uint32))
    finally:
        renderer.set_shard(0, 1)
        renderer.set_flag("~connecttoviews")


@pytest.mark.parametrize(
    "flags",
    [
        ["connecttolightpaths"],
        ["connecttolightpaths", "connecttoviews"],
        ["connecttolightpaths", "~mis"],
        ["connecttolightpaths", "~nee"],
        ["connecttolightpaths", "connecttoviews", "~defershadowrays", "shadingnormalshadowfix"],
    ],
)
def test_light_path_connections(flags):
    """eConnectToLightPaths without the light vertex cache: light subpaths store their vertices (store_light_vertex,
    path.hlsli:520-531), every view vertex connects to the stored vertices of the light path with its path index
    (connect_light_subpath / connect_light_vertex, path.hlsli:618-680,802-822), contributions are added to gRadiance in
    program order between the vertices' emission terms."""
    sc, cam = scenes.cornell_box()
    _compare_frame(sc, cam, flags, w=100, h=76, seeds=2, args={"maxDiffuseVertices": 4, "maxPathVertices": 7})  # not multiples of 8x4: slots alias / run out
    _compare_frame(sc, cam, flags, w=96, h=64, seeds=1)  # default limits: one stored vertex per light path
    sc, cam = scenes.spheres_room()
    _compare_frame(sc, cam, flags + ["uniformspheresampling"], w=96, h=64, seeds=1, args={"maxDiffuseVertices": 3})


def test_light_path_connections_textured_and_sharded(renderer):
    from stratum_amd import _lib, shard

    sc, cam = scenes.textured_box()  # textures, normal maps (applied again at the stored vertex), specular lobes
    _compare_frame(sc, cam, ["connecttolightpaths"], w=96, h=80, seeds=1, args={"maxDiffuseVertices": 3})
    sc, cam = scenes.cornell_box()
    renderer.update(sc)
    renderer.set_flag("connecttolightpaths")
    renderer.mPushConstants.gMaxDiffuseVertices = 3
    try:
        frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
        full = renderer.render(frame, 0, 2, aovs=False)["radiance"]
        total = np.zeros_like(full)
        for rank in range(3):  # every shard traces all light paths and connects its own pixels
            renderer.set_shard(rank, 3, 16, 8)
            total += renderer.render(frame, 0, 2, aovs=False)["radiance"]
        assert np.array_equal(total.view(np.uint32), full.view(np.uint32))
        renderer.set_shard(0, 1)
        renderer.set_flag("~remapthreads")
        with pytest.raises(_lib.StratumHipError, match="multiple of 8"):
            renderer.render(camera.Frame(100, 64, cam["fovy"], cam["eye"], cam["target"]))
    finally:
        renderer.set_shard(0, 1)
        renderer.set_flag("remapthreads")
        renderer.set_flag("~connecttolightpaths")
        renderer.mPushConstants.gMaxDiffuseVertices = 2


def test_light_tracing_limits(renderer):
    from stratum_amd import _lib

    sc, cam = scenes.environment_scene(image=False, emitter=True)
    renderer.update(sc)
    renderer.set_flag("connecttoviews")
    try:
        with pytest.raises(_lib.StratumHipError, match="light subpaths with an environment"):
            renderer.render(camera.Frame(32, 32, cam["fovy"], cam["eye"], cam["target"]))
    finally:
        renderer.set_flag("~connecttoviews")


# ---- participating media (NanoVDB density grids, delta tracking, phase-function vertices) ----
def _fog():
    import os

    return np.load(os.path.join(os.path.dirname(__file__), "golden", "fog_sphere.npz"))["grid"]


def test_trace_contract_with_volumes(renderer):
    """A volume instance is a top-level entry tested in place (the slabs of its grid's root bounding box in index space,
    intersection.hlsli:93-113): closest hits and occlusion equal the oracle's brute force."""
    from oracle import oracle_py
    from stratum_amd.scene import translate

    sc, _ = scenes.cornell_box(fog=_fog(), fog_transform=translate((0.2, 0.1, -0.1)))
    renderer.update(sc)
    o = oracle_py.OracleScene(sc)
    rays = random_rays(60000, 7, -1.4, 1.4)
    got = renderer.trace(rays)
    ref, _ = o.trace(rays, brute=True)
    for f in ("instance_primitive_index", "t", "b1", "b2"):
        assert np.array_equal(got[f].view(np.uint32), ref[f].view(np.uint32)), f
    on_volume = (ref["instance_primitive_index"] & 0xFFFF) == sc.instances.shape[0] - 1
    assert on_volume.mean() > 0.1
    assert np.array_equal(renderer.trace(rays, any_hit=True)["instance_primitive_index"] != wire.MISS, o.trace(rays, any_hit=True)[0]["instance_primitive_index"] != wire.MISS)


@pytest.mark.parametrize(
    "kwargs,flags,args",
    [
        ({}, [], {"maxDiffuseVertices": 3}),
        ({"anisotropy": 0.6, "density": (6.0, 4.0, 2.0), "albedo": (0.8, 0.9, 1.0)}, [], {"maxDiffuseVertices": 4, "maxPathVertices": 6}),
        ({"anisotropy": -0.3}, ["~nee"], {"maxDiffuseVertices": 4}),
        ({}, ["~samplebsdfs"], {}),
        ({"density": (12.0, 12.0, 12.0)}, ["presamplelights", "~mis"], {"maxDiffuseVertices": 5, "minPathVertices": 2}),
        # without eDeferShadowRays an NEE ray's walk draws from the path's own stream, between the light sample and the BSDF
        # sample of its vertex, and scales both pdfs of the MIS weight (path.hlsli:329-332,866,1011): k_shade walks it itself
        ({}, ["~defershadowrays"], {"maxDiffuseVertices": 3}),
        ({"anisotropy": 0.5, "density": (9.0, 6.0, 3.0)}, ["~defershadowrays", "~mis"], {"maxDiffuseVertices": 4, "maxPathVertices": 6, "minPathVertices": 2}),
        ({"density": (12.0, 12.0, 12.0)}, ["~defershadowrays", "presamplelights", "~samplebsdfs"], {"maxDiffuseVertices": 4}),
        # NEE reservoirs: resampling at surface and medium vertices (there with setup()'s world-space direction in the target,
        # path.hlsli:207-212,391), deferred records and inline walks (:474-485)
        ({}, ["neereservoirs"], {"maxDiffuseVertices": 3, "reservoirM": 4}),
        ({"density": (9.0, 9.0, 9.0)}, ["neereservoirs", "presamplelights", "~samplebsdfs"], {"maxDiffuseVertices": 4, "reservoirM": 3}),
        ({"anisotropy": 0.4, "density": (9.0, 6.0, 3.0)}, ["neereservoirs", "~defershadowrays"], {"maxDiffuseVertices": 4, "reservoirM": 2, "minPathVertices": 2}),
        # light tracing through the media (eConnectToViews): light paths walk and scatter like view paths, every connect_view — from
        # surfaces and from medium vertices — walks its visibility ray itself, in the light path's stream (path.hlsli:533-613)
        ({}, ["connecttoviews"], {"maxDiffuseVertices": 3}),
        ({"anisotropy": 0.5, "density": (9.0, 6.0, 3.0)}, ["connecttoviews", "~defershadowrays"], {"maxDiffuseVertices": 4, "maxPathVertices": 6}),
        ({"density": (12.0, 12.0, 12.0)}, ["connecttoviews", "~mis", "~nee"], {"maxDiffuseVertices": 4}),
        ({}, ["connecttoviews", "neereservoirs", "presamplelights"], {"maxDiffuseVertices": 3, "reservoirM": 2}),
        # ... and the connections to the stored light vertices (eConnectToLightPaths): light vertices inside media
        # (PATH_VERTEX_FLAG_IS_MEDIUM: the phase function with the stored direction), view vertices inside media, every connection's
        # visibility ray walked at once in the view path's stream (path.hlsli:618-680,802-822)
        ({}, ["connecttolightpaths"], {"maxDiffuseVertices": 3}),
        ({"anisotropy": 0.5, "density": (9.0, 6.0, 3.0)}, ["connecttolightpaths", "connecttoviews", "~defershadowrays"], {"maxDiffuseVertices": 4, "maxPathVertices": 6}),
        ({"density": (12.0, 12.0, 12.0)}, ["connecttolightpaths", "~mis", "~nee"], {"maxDiffuseVertices": 4}),
        # ... and to the light vertex cache (eLVC): medium vertices staged and compacted like the others, connect_lvc from surfaces
        # and from medium vertices, the deferred record taking the vertex's shadow-ray slot, reservoirs and their reuse
        ({}, ["connecttolightpaths", "lightvertexcache"], {"maxDiffuseVertices": 3, "lightPathCount": 6000}),
        ({"anisotropy": 0.4}, ["connecttolightpaths", "lightvertexcache", "~defershadowrays", "connecttoviews"], {"maxDiffuseVertices": 4, "lightPathCount": 12288}),
        ({"density": (9.0, 9.0, 9.0)}, ["connecttolightpaths", "lightvertexcache", "lvcreservoirs"], {"maxDiffuseVertices": 3, "lightPathCount": 8000, "reservoirM": 3}),
        ({}, ["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "lvcreservoirreuse", "~defershadowrays"], {"maxDiffuseVertices": 3, "lightPathCount": 9000, "reservoirM": 2, "reservoirSpatialM": 2, "hashGridBucketCount": 20000}),
        # ... with spatial reuse: seeds 1 and 2 look into the grid the seed before them built, from surface and medium vertices alike
        ({"density": (9.0, 9.0, 9.0)}, ["neereservoirs", "neereservoirreuse"], {"maxDiffuseVertices": 3, "reservoirM": 2, "reservoirSpatialM": 3, "hashGridBucketCount": 20000}),
        ({"anisotropy": 0.3}, ["neereservoirs", "neereservoirreuse", "~jitterhashgridlookups", "~defershadowrays", "presamplelights"], {"maxDiffuseVertices": 4, "reservoirM": 3, "reservoirSpatialM": 2, "hashGridBucketCount": 5000}),
    ],
)
def test_media(kwargs, flags, args):
    """A cloud (NanoVDB fog volume) in the Cornell box: volume boundaries, delta tracking, phase-function vertices, NEE
    walks through the medium (medium.hlsli, intersection.hlsli:192-285); every output equals the oracle's."""
    sc, cam = scenes.cornell_box(fog=_fog(), **kwargs)
    got = _compare_frame(sc, cam, flags, w=128, h=96, seeds=3, args=args)
    in_fog = (got["visibility"]["instance_primitive_index"] & 0xFFFF) == sc.instances.shape[0] - 1
    assert in_fog.mean() > 0.01  # first vertices inside the medium (few when the majorant is high: the first null collision ends a walk upstream)


@pytest.mark.parametrize("density", [(300.0, 1.0, 1.0), (1.0, 300.0, 40.0), (2000.0, 2000.0, 2000.0)])
@pytest.mark.parametrize(
    "flags,args",
    [
        ([], {}),
        (["~defershadowrays"], {}),
        (["connecttolightpaths", "lightvertexcache"], {"maxDiffuseVertices": 3, "lightPathCount": 6000}),
        (["neereservoirs", "neereservoirreuse"], {"maxDiffuseVertices": 3, "reservoirM": 2, "reservoirSpatialM": 3, "hashGridBucketCount": 20000}),
    ],
)
def test_media_dense_and_chromatic(density, flags, args):
    """Delta tracking draws a distance for one colour channel and evaluates exp(-majorant t) for all three: with one channel
    300 times denser than another (or all of them very dense) the argument lies far below the domain the arithmetic
    contract's exp once had, where it returned negative and infinite values on both sides alike. Every output equals the
    oracle's, and no radiance is negative or infinite (tests/test_detmath_edges.py checks the oracle's exp itself)."""
    sc, cam = scenes.cornell_box(fog=_fog(), density=density)
    got = _compare_frame(sc, cam, flags, w=64, h=48, seeds=4, args=args)
    rad = got["radiance"][..., :3]
    assert np.isfinite(rad).all() and (rad >= 0).all(), float(np.nanmin(rad))


def test_media_camera_inside_and_moved_volume(renderer):
    from stratum_amd.scene import translate

    sc, cam = scenes.cornell_box(fog=_fog(), fog_transform=translate((0.0, 0.0, 1.6)), density=(2.0, 2.0, 2.0))
    cam = dict(cam, eye=(0.1, 0.0, 1.9))  # inside the cloud's bounding box: gViewMediumInstances
    _compare_frame(sc, cam, [], w=96, h=64, seeds=2, args={"maxDiffuseVertices": 3})
    sc, cam = scenes.textured_box()
    b = sc.builder
    b.add_medium(b.add_volume(_fog()), density_scale=(3, 3, 3), albedo_scale=(0.9, 0.9, 0.9), transform=translate((0.0, -0.2, 0.0)))
    _compare_frame(b.build(), cam, [], w=96, h=80, seeds=2, args={"maxDiffuseVertices": 3})


def test_media_limits(renderer):
    from stratum_amd import _lib

    bad = _fog().copy()
    bad[0] ^= 0xFF  # not a NanoVDB grid any more
    sc, cam = scenes.cornell_box(fog=bad)
    with pytest.raises(_lib.StratumHipError, match="NanoVDB"):
        renderer.update(sc)
    truncated = _fog()[: 672 + 64 + 64 + 4096].copy()  # the header survives, the tree does not: reads outside return zero
    sc, cam = scenes.cornell_box(fog=truncated)
    try:
        renderer.update(sc)
        renderer.render(camera.Frame(32, 32, cam["fovy"], cam["eye"], cam["target"]))
    except _lib.StratumHipError:
        pass

    sc, cam = scenes.cornell_box(fog=_fog())
    renderer.update(sc)
    frame = camera.Frame(32, 32, cam["fovy"], cam["eye"], cam["target"])
    for fs in (("presamplelights", "coherentsampling"),):
        for f in fs:
            renderer.set_flag(f)
        try:
            with pytest.raises(_lib.StratumHipError, match="media"):
                renderer.render(frame)
        finally:
            for f in fs:
                renderer.set_flag("~" + f)


def test_media_stereo_and_long_walks():
    """Two cameras and more diffuse vertices: the walks of earlier vertices' NEE rays are still queued when later
    vertices add theirs (the shadow queue holds up to gMaxDiffuseVertices records per path)."""
    from oracle import oracle_py
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box(fog=_fog(), anisotropy=-0.4, density=(6.0, 4.5, 2.05))
    r = BDPT(device=0, args={"maxDiffuseVertices": 4, "maxPathVertices": 6})
    try:
        r.update(sc)
        frame = camera.Frame.stereo(64, 48, cam["fovy"], cam["eye"], cam["target"], eye_separation=0.2)
        got = r.render(frame, 361, 3)
        ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 361, 3)
        assert np.array_equal(got["radiance"].view(np.uint32), ref["radiance"].view(np.uint32))
        assert np.array_equal(got["ray_count"], ref["ray_count"])
    finally:
        r.close()


def test_randomised_differential():
    """tools/fuzz_parity.py: random scenes x supported flag combinations x limits x frame sizes x views x execution options
    (seeds per pass, split trace launches, packets off, LBVH, sharding), every output against the oracle bit for bit.
    (It found the two defects fixed in its commit: rays of inline NEE with a zero contribution were not counted, and the
    shadow queue overflowed when the walks of several vertices through a medium were alive at once.)"""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    done, rejected, bad = mod.run(cases=250, seed=11)
    assert bad == 0 and done > 150


def test_transforms_only_update(renderer):
    """sthip_scene_update_transforms: instances move, the bottom levels stay in HBM, the top level is rebuilt. Frames equal
    the oracle's on the moved scene and what a full upload gives; when an instance of the merged identity mesh moves the call
    builds the scene again from the copy kept at upload (refused without it: keep_scene = 0)."""
    from oracle import oracle_py
    from stratum_amd import _lib
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import rotate_y, scale, translate

    cases = [
        (scenes.cornell_box(), [(5, translate((0.1, -1.0, 0.45)) @ rotate_y(0.6) @ scale((0.5, 0.7, 0.5))), (6, translate((-0.5, -1.0, -0.2)) @ rotate_y(-0.4) @ scale((0.5, 1.4, 0.5)))], {}),
        (scenes.spheres_room(), None, {"maxDiffuseVertices": 3}),
        (scenes.forest(n_instances=30, tree_tris=600, tree_kinds=2), None, {}),
        (scenes.cornell_box(fog=_fog()), "fog", {"maxDiffuseVertices": 3}),
    ]
    for (sc, cam), moves, args in cases:
        kinds = sc.instances["packed"][:, 0] & 0xF
        if moves is None:  # move every instance that is not part of the merged identity mesh
            ident = np.array([np.array_equal(m, np.eye(4, dtype=np.float32)[:3]) for m in sc.transforms["m"]])
            moves = [(int(i), np.vstack([sc.transforms["m"][i], [0, 0, 0, 1]]).astype(np.float64)) for i in np.nonzero(~ident)[0][:12]]
            moves = [(i, translate((0.07 * ((k % 3) - 1), 0.0 if kinds[i] == wire.INSTANCE_TYPE_TRIANGLES else 0.05, -0.05 * (k % 2))) @ m) for k, (i, m) in enumerate(moves)]
        elif moves == "fog":
            moves = [(sc.instances.shape[0] - 1, translate((0.25, 0.1, -0.2)) @ scale((0.8, 1.1, 0.9)))]
        r = BDPT(device=0, args=args)
        try:
            r.update(sc)
            frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
            before = r.render(frame, 0, 2)["radiance"].copy()
            for i, m in moves:
                sc.set_instance_transform(i, m)
            r.update_transforms(sc)
            got = r.render(frame, 0, 2)
            ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, 2)
            for k in ("radiance", "albedo", "prev_uv"):
                assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (sc.name, k)
            assert np.array_equal(got["visibility"]["instance_primitive_index"], ref["visibility"]["instance_primitive_index"])
            assert np.array_equal(got["ray_count"], ref["ray_count"])
            assert not np.array_equal(before, got["radiance"])
            r.update(sc)  # the full upload of the moved scene gives the same frame
            assert np.array_equal(r.render(frame, 0, 2)["radiance"].view(np.uint32), got["radiance"].view(np.uint32))
        finally:
            r.close()
    # An instance of the merged world-space mesh that moves: the resident tree cannot follow, the call builds the scene again
    # from the copy kept at upload (Scene.cpp:345,435-459: the reference rebuilds whatever is dirty) — with either builder, and
    # the frame is the one a fresh upload of the moved scene gives (and the oracle's). Without the copy it is refused.
    from oracle import oracle_py

    for builder in (0, 1):
        sc, cam = scenes.cornell_box()
        frame = camera.Frame(128, 96, cam["fovy"], cam["eye"], cam["target"])
        r = BDPT(device=0)
        try:
            r.set_option("bvh_builder", builder)
            r.update(sc)
            before = r.render(frame, 0, 2)["radiance"].copy()
            sc.set_instance_transform(0, translate((0.0, 0.1, 0.0)))  # the floor: part of the merged world-space mesh
            r.update_transforms(sc)
            assert r.stats()["full_rebuilds"] == 1
            got = r.render(frame, 0, 2)
            assert not np.array_equal(before, got["radiance"])
            ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, 2)
            assert np.array_equal(got["radiance"].view(np.uint32), ref["radiance"].view(np.uint32)), builder
            assert np.array_equal(got["ray_count"], ref["ray_count"])
            sc.set_instance_transform(0, translate((0.0, 0.0, 0.0)))  # ... and back: the instance is a transformed one now, the top level follows
            r.update_transforms(sc)
            assert np.array_equal(r.render(frame, 0, 2)["radiance"].view(np.uint32), before.view(np.uint32))
        finally:
            r.close()
    sc, cam = scenes.cornell_box()
    r = BDPT(device=0)
    try:
        r.set_option("keep_scene", 0)
        r.update(sc)
        sc.set_instance_transform(0, translate((0.0, 0.1, 0.0)))
        with pytest.raises(_lib.StratumHipError, match="upload the scene again"):
            r.update_transforms(sc)
    finally:
        r.close()


def test_estimators_converge_to_the_same_image(renderer):
    """At sample counts the CPU oracle cannot afford: the unbiased estimator combinations agree on the Cornell box
    (4096 samples per pixel each; mean radiance within 1 %, image within a few % rel-L2 of the default path tracer)."""
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(64, 48, cam["fovy"], cam["eye"], cam["target"])
    images = {}
    for name, flags in (
        ("path tracing, NEE + MIS", []),
        ("NEE without MIS", ["~mis"]),
        ("BSDF sampling only", ["~nee"]),
        ("light tracing + BSDF sampling, MIS", ["connecttoviews", "~nee"]),
        ("light tracing + NEE, uniform weights", ["connecttoviews", "~mis"]),
        ("presampled lights", ["presamplelights"]),
        ("NEE reservoirs", ["neereservoirs"]),
    ):
        r = BDPT(device=0, args={"bdptFlag": flags})
        try:
            r.update(sc)
            images[name] = r.render(frame, 0, 4096, aovs=False)["radiance"][..., :3].astype(np.float64)
        finally:
            r.close()
    ref = images["path tracing, NEE + MIS"]
    for name, img in images.items():
        assert abs(img.mean() / ref.mean() - 1) < 0.01, (name, img.mean() / ref.mean())
        assert np.sqrt(((img - ref) ** 2).sum() / (ref**2).sum()) < (0.08 if "BSDF sampling only" in name else 0.03), name


def test_cache_and_reuse_estimators_stay_close_to_path_tracing(renderer):
    """The estimators whose upstream result depends on scheduling (light vertex cache, reservoir reuse through the hash
    grids) are defined here by an order (paths by index); what must hold whatever the order is that they estimate the same
    image. 1024 samples per pixel on the Cornell box against the default path tracer: mean radiance within 3 % (upstream's
    weights for NEE + connections do not sum to one, and reuse without visibility tests is slightly biased: restated, not
    fixed; 10 % for the cache's reservoir reuse, see below), image within 6 % rel-L2."""
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(64, 48, cam["fovy"], cam["eye"], cam["target"])
    images = {}
    for name, flags, args in (
        ("path tracing, NEE + MIS", [], {}),
        ("NEE reservoirs with reuse", ["neereservoirs", "neereservoirreuse"], {"reservoirM": 4}),
        ("light vertex cache", ["connecttolightpaths", "lightvertexcache", "~defershadowrays"], {"lightPathCount": 64 * 48}),
        ("light vertex cache, reservoirs with reuse", ["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "lvcreservoirreuse", "~defershadowrays"], {"lightPathCount": 64 * 48, "reservoirM": 4}),
    ):
        r = BDPT(device=0, args=dict(args, bdptFlag=flags, maxDiffuseVertices=3))
        try:
            r.update(sc)
            images[name] = r.render(frame, 0, 1024, aovs=False)["radiance"][..., :3].astype(np.float64)
        finally:
            r.close()
    ref = images["path tracing, NEE + MIS"]
    for name, img in images.items():
        print("%-45s mean ratio %.4f rel-L2 %.4f" % (name, img.mean() / ref.mean(), np.sqrt(((img - ref) ** 2).sum() / (ref**2).sum())))
        assert np.isfinite(img).all()
        # connect_lvc's reuse loop weights a vertex taken from a neighbour's reservoir as if it were a fresh uniform pick
        # (target / path_pdf, path.hlsli:748, where the NEE loop has target * W * M, :418): biased upstream, restated here
        tol = 0.10 if "reservoirs with reuse" in name and "cache" in name else 0.03
        assert abs(img.mean() / ref.mean() - 1) < tol, (name, img.mean() / ref.mean())
        assert np.sqrt(((img - ref) ** 2).sum() / (ref**2).sum()) < 0.06, name


def test_treetop_and_packed_nodes_do_not_change_results(atrium_scene):
    """The LDS treetop (bvh_build.h) and the 48-byte packed nodes (bvh.h) only change where a node is read from and how
    wide its box is (conservatively): frames with and without the treetop are bit-identical, on the merged world mesh +
    transformed instances of the atrium and on the two-level forest (treetop through the top level into shared meshes)."""
    from stratum_amd.bdpt import BDPT

    for make, args in ((lambda: atrium_scene, {}), (lambda: scenes.forest(n_instances=60, tree_tris=800), {"maxDiffuseVertices": 4, "maxPathVertices": 6})):
        sc, cam = make()
        frame = camera.Frame(320, 192, cam["fovy"], cam["eye"], cam["target"])
        frames = []
        for treetop in (1, 0):
            r = BDPT(device=0, args=args)
            try:
                r.set_option("treetop", treetop)
                r.update(sc)
                frames.append(r.render(frame, 0, 2))
            finally:
                r.close()
        a, b = frames
        assert np.array_equal(a["radiance"].view(np.uint32), b["radiance"].view(np.uint32))
        assert np.array_equal(a["visibility"]["instance_primitive_index"], b["visibility"]["instance_primitive_index"])
        assert np.array_equal(a["ray_count"], b["ray_count"])


def _cornell_with_a_mirror_and_glass():
    """The Cornell box plus a mirror on the back wall and a pane of glass in front of the blocks (triangles only, no textures:
    the plain k_shade instantiation): specular vertices do not count against the diffuse budget."""
    from stratum_amd.scene import translate

    sc0, cam = scenes.cornell_box()
    b = sc0.builder
    mirror = b.add_material((0.95, 0.95, 0.95), metallic=1.0, roughness=0.0)
    glass = b.add_material((1.0, 1.0, 1.0), transmission=1.0, roughness=0.0, eta=1.5)
    pos, nrm, uv, tri = scenes._quad((-0.7, -0.6, -0.99), (0.7, -0.6, -0.99), (0.7, 0.7, -0.99), (-0.7, 0.7, -0.99), (0, 0, 1))
    b.add_instance(b.add_mesh(pos, nrm, uv, tri), mirror)
    pos, nrm, uv, tri = scenes._quad((-0.8, -0.9, 0.0), (0.8, -0.9, 0.0), (0.8, 0.2, 0.0), (-0.8, 0.2, 0.0), (0, 0, 1))
    b.add_instance(b.add_mesh(pos, nrm, uv, tri), glass, translate((0.0, 0.0, 0.85)))
    return b.build(), cam


def test_culling_finished_paths_in_front_of_k_shade_does_not_change_results(atrium_scene):
    """k_cull_terminal (kernels.h, option "cull_terminal"): in a round where the path or diffuse budget can end, only the
    paths that still have something to do — an emitter was hit, or a specular vertex lets the path go on — are handed to
    k_shade. "answer_last_rays": the ray into a path's last vertex is traced only if it can reach the bounds of an emissive
    instance (aims_at_emitter), and counted either way. Frames and ray counts with and without them are bit-identical, for budgets that end paths by their length, by
    their diffuse vertices, or (mirrors / glass in the scene) leave some of them running; one of them against the oracle."""
    from oracle import oracle_py as orc
    from stratum_amd.bdpt import BDPT

    cases = (
        (lambda: atrium_scene, {}, (320, 192)),
        (lambda: atrium_scene, {"maxDiffuseVertices": 3, "maxPathVertices": 4}, (256, 160)),
        (lambda: atrium_scene, {"maxDiffuseVertices": 4, "maxPathVertices": 9, "minPathVertices": 3}, (256, 160)),
        (scenes.cornell_box, {"maxDiffuseVertices": 1, "maxPathVertices": 6}, (200, 200)),
        (scenes.cornell_box, {"maxDiffuseVertices": 5, "maxPathVertices": 3}, (200, 200)),
        (_cornell_with_a_mirror_and_glass, {"maxDiffuseVertices": 2, "maxPathVertices": 8}, (240, 160)),
    )
    for make, args, (W, H) in cases:
        sc, cam = make()
        frame = camera.Frame(W, H, cam["fovy"], cam["eye"], cam["target"])
        frames, answered = [], []
        for cull, answer in ((1, 1), (0, 0), (1, 0), (0, 1)):
            r = BDPT(device=0, args=args)
            try:
                r.set_option("cull_terminal", cull)
                r.set_option("answer_last_rays", answer)
                r.update(sc)
                frames.append(r.render(frame, 3, 2))
                answered.append(r.stats()["rays_answered"])
            finally:
                r.close()
        a = frames[0]
        for b in frames[1:]:
            assert np.array_equal(a["radiance"].view(np.uint32), b["radiance"].view(np.uint32)), args
            assert np.array_equal(a["ray_count"], b["ray_count"]), args
            assert np.array_equal(a["visibility"]["instance_primitive_index"], b["visibility"]["instance_primitive_index"])
        assert a["radiance"][..., :3].max() > 0
        # last rays that cannot reach an emitter's bounds are answered without a traversal (and only with the option on):
        # most of them where every path ends by its budget, none where the budget never ends a path in these rounds
        assert answered[1] == 0 and answered[2] == 0 and answered[0] == answered[3], answered
        if make is not _cornell_with_a_mirror_and_glass:  # (with specular materials only the path-length budget ends a path for sure)
            assert answered[0] > 0, (args, answered)
    # ... and the culled frame is the oracle's (the last case: mirrors and glass keep some paths alive past the diffuse budget)
    o = orc.OracleScene(sc)
    r = BDPT(device=0, args=args)
    try:
        r.update(sc)
        pc = r.push_constants(frame)
        ref = o.render(frame, pc, r.mSamplingFlags, 3, 2)
    finally:
        r.close()
    assert np.array_equal(a["radiance"].view(np.uint32), ref["radiance"].view(np.uint32))


def test_last_rays_answered_from_the_bounds_of_moving_emitters():
    """aims_at_emitter (kernels.h) with emitters that are instances with a transform — the slab test then runs in the
    instance's object space, as the walk's own tests of its triangles do — next to the ceiling light of the merged mesh; the
    emitters then move (sthip_scene_update_transforms: the bounds are the object-space box and the current inverse transform).
    Frames, AOVs and ray counts are the oracle's bit for bit before and after the move, and the filter answers rays."""
    from oracle import oracle_py
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import rotate_y, scale, translate

    sc0, cam = scenes.cornell_box()
    b = sc0.builder
    glow = b.add_emitter((3.0, 6.0, 9.0))
    pos, nrm, uv, tri = scenes._quad((-0.5, 0.0, 0.5), (0.5, 0.0, 0.5), (0.5, 0.0, -0.5), (-0.5, 0.0, -0.5), (0, 1, 0))
    panel = b.add_mesh(pos, nrm, uv, tri)
    first = b.add_instance(panel, glow, translate((0.55, -0.2, 0.1)) @ rotate_y(0.7) @ scale((0.3, 1.0, 0.5)))
    second = b.add_instance(panel, glow, translate((-0.6, 0.4, -0.5)) @ rotate_y(-1.1) @ scale((0.25, 1.0, 0.25)))
    sc = b.build()
    frame = camera.Frame(160, 120, cam["fovy"], cam["eye"], cam["target"])
    for args in ({}, {"maxDiffuseVertices": 3, "maxPathVertices": 5}):
        r = BDPT(device=0, args=args)
        try:
            r.update(sc)
            for moved in (False, True):
                if moved:
                    sc.set_instance_transform(sc.instances.shape[0] - 2, translate((0.2, 0.3, 0.4)) @ rotate_y(-0.3) @ scale((0.5, 1.0, 0.3)))
                    sc.set_instance_transform(sc.instances.shape[0] - 1, translate((-0.3, -0.5, 0.2)) @ rotate_y(2.0) @ scale((0.3, 1.0, 0.6)))
                    r.update_transforms(sc)
                got = r.render(frame, 1, 2)
                assert r.stats()["rays_answered"] > 0
                ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 1, 2)
                for k in ("radiance", "albedo"):
                    assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (args, moved, k)
                assert np.array_equal(got["ray_count"], ref["ray_count"]), (args, moved)
                r.set_option("answer_last_rays", 0)
                plain = r.render(frame, 1, 2)
                assert r.stats()["rays_answered"] == 0
                r.set_option("answer_last_rays", 1)
                assert np.array_equal(got["radiance"].view(np.uint32), plain["radiance"].view(np.uint32)) and np.array_equal(got["ray_count"], plain["ray_count"])
        finally:
            r.close()


def test_culling_finished_paths_with_spheres_reservoirs_and_an_environment():
    """k_cull_terminal in front of the extended k_shade instantiation (scenes without images: sphere instances and lights, an
    environment, NEE reservoirs): a hit on a sphere is judged by its instance's material like any other, a miss is kept where
    an environment adds the background, NEE reservoirs change what a vertex does but not what a last vertex can add. Last rays
    are not answered there (the filter lives in the plain instantiation). Frames and ray counts are the oracle's and do not
    depend on the options."""
    from oracle import oracle_py
    from stratum_amd.bdpt import BDPT

    cases = (
        (scenes.spheres_room, {}, [], False),
        (scenes.spheres_room, {"maxDiffuseVertices": 3, "maxPathVertices": 5}, ["uniformspheresampling"], False),
        (scenes.cornell_box, {}, ["neereservoirs"], False),
        (lambda: scenes.environment_scene(image=True, emitter=True), {}, [], False),
        (lambda: scenes.environment_scene(image=False, emitter=False), {"maxDiffuseVertices": 1}, [], False),
    )
    for make, args, flags, answers in cases:
        sc, cam = make()
        frame = camera.Frame(128, 96, cam["fovy"], cam["eye"], cam["target"])
        frames, answered = [], []
        for cull, answer in ((1, 1), (0, 0)):
            r = BDPT(device=0, args=dict(args, bdptFlag=flags))
            try:
                r.set_option("cull_terminal", cull)
                r.set_option("answer_last_rays", answer)
                r.update(sc)
                frames.append(r.render(frame, 5, 2))
                answered.append(r.stats()["rays_answered"])
                if cull:
                    ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 5, 2)
            finally:
                r.close()
        a, b = frames
        for k in ("radiance", "albedo"):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (sc.name, flags, k)
        assert np.array_equal(a["ray_count"], b["ray_count"])
        assert np.array_equal(a["radiance"].view(np.uint32), ref["radiance"].view(np.uint32)), (sc.name, flags)
        assert np.array_equal(a["ray_count"], ref["ray_count"])
        assert answered[1] == 0 and (answered[0] > 0) == answers, (sc.name, flags, answered)


def test_a_render_does_not_depend_on_what_a_failed_one_left_in_the_deep_queue(atrium_scene):
    """k_trace_deep leaves the deep queue's control words at zero for the next launch; a call that ended between k_trace and
    k_trace_deep (a failed launch, an early error return) would leave them dirty. sthip_render fills them once per call, so
    every call is self-contained: the frame after such a failure (simulated: option poison_deep_queue) is the frame."""
    from stratum_amd.bdpt import BDPT

    sc, cam = atrium_scene
    frame = camera.Frame(160, 96, cam["fovy"], cam["eye"], cam["target"])
    r = BDPT(device=0, args={"maxDiffuseVertices": 3})
    try:
        r.set_option("lds_stack_levels", 6)  # bounded stacks: nearly every ray goes through the deep queue
        r.update(sc)
        ref = r.render(frame, 1, 2)
        r.set_option("poison_deep_queue", 1)
        got = r.render(frame, 1, 2)
        again = r.render(frame, 1, 2)
    finally:
        r.close()
    for x in (got, again):
        assert np.array_equal(ref["radiance"].view(np.uint32), x["radiance"].view(np.uint32))
        assert np.array_equal(ref["ray_count"], x["ray_count"])


def test_render_halves_its_batch_when_the_device_is_nearly_full():
    """max_paths_in_flight is sized from the device's FREE memory at sthip_create, and a render whose path state does not fit
    beside what else lives on the device retries with half the batch instead of failing (stats: batch_halvings): the frame
    does not depend on how many seeds are traced together. Here another owner (a torch tensor) takes all but ~3 GB after the
    context was sized for an empty device."""
    import torch

    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(1920, 1080, cam["fovy"], cam["eye"], cam["target"])
    seeds = 16
    r = BDPT(device=0)
    try:
        r.update(sc)
        ref = r.render(frame, 0, seeds, aovs=False)
        st = r.stats()
        assert st["seeds_in_flight"] == seeds and st["batch_halvings"] == 0 and st["paths_per_seed"] >= 1920 * 1080
    finally:
        r.close()
    r = BDPT(device=0)  # sized now, while the device is empty
    hog = None
    try:
        r.update(sc)
        torch.cuda.synchronize()
        free, _ = torch.cuda.mem_get_info()
        hog = torch.empty(max(0, free - (3 << 30)), dtype=torch.uint8, device="cuda")
        got = r.render(frame, 0, seeds, aovs=False)
        st = r.stats()
        assert st["batch_halvings"] >= 1 and 1 <= st["seeds_in_flight"] < seeds, st
        again = r.render(frame, 0, seeds, aovs=False)  # the smaller batch stays: no second round of failures
        assert r.stats()["batch_halvings"] == st["batch_halvings"]
        late = BDPT(device=0)  # a context created on the full device starts small (a frame that fits what the first context left: a few hundred MB)
        try:
            late.update(sc)
            small = late.render(camera.Frame(640, 360, cam["fovy"], cam["eye"], cam["target"]), 0, 4, aovs=False)
            assert late.stats()["max_paths_in_flight"] < st["max_paths_in_flight"] * 4 and late.stats()["batch_halvings"] == 0
        finally:
            late.close()
    finally:
        r.close()
        del hog
        torch.cuda.empty_cache()
    assert np.array_equal(ref["radiance"].view(np.uint32), got["radiance"].view(np.uint32))
    assert np.array_equal(ref["radiance"].view(np.uint32), again["radiance"].view(np.uint32))
    assert np.array_equal(ref["ray_count"], got["ray_count"])
    assert small["radiance"].shape == (360, 640, 4)


def test_last_ray_filter_on_ill_conditioned_emitters():
    """answer_last_rays against the plain walk where the filter's box test is least comfortable: emitters with
    zero-area and sliver triangles (a box that is a segment / a point in one axis), a tiny scaled emitter instance (grazing
    rays), and the whole scene at large coordinates (every instance and the camera 4096 units away: the padding terms of the
    slab tests are then dominated by |origin|). The filter holds as long as the origin is within a few scene sizes of the
    scene (the precondition of the hit contract itself): frames and ray counts are identical with it on and off."""
    from stratum_amd.bdpt import BDPT
    from stratum_amd.scene import rotate_y, scale, translate

    def degenerate():
        sc0, cam = scenes.cornell_box()
        b = sc0.builder
        glow = b.add_emitter((5.0, 4.0, 3.0))
        pos = np.array([(-0.3, 0.0, -0.3), (0.3, 0.0, -0.3), (0.3, 0.0, 0.3), (-0.3, 0.0, 0.3),   # a quad ...
                        (0.0, 0.0, 0.0), (0.1, 0.0, 0.0), (0.2, 0.0, 0.0),                           # ... a zero-area triangle (three points on a line) ...
                        (0.5, 0.0, 0.5), (0.5, 0.0, 0.5), (0.5, 0.0, 0.5),                           # ... a point ...
                        (-0.5, 0.0, 0.4), (0.5, 0.0, 0.4), (0.5, 0.0, 0.400001)], np.float32)         # ... and a sliver
        nrm = np.tile(np.array([(0, -1, 0)], np.float32), (pos.shape[0], 1))
        uv = np.zeros((pos.shape[0], 2), np.float32)
        tri = np.array([(0, 2, 1), (0, 3, 2), (4, 5, 6), (7, 8, 9), (10, 11, 12)], np.uint32)
        mesh = b.add_mesh(pos, nrm, uv, tri)
        b.add_instance(mesh, glow, translate((0.1, 0.55, -0.2)) @ rotate_y(0.4))
        b.add_instance(mesh, glow, translate((-0.4, -0.3, 0.3)) @ rotate_y(1.9) @ scale((0.004, 1.0, 0.004)))  # 2 mm across
        return b.build(), cam

    def far_away():
        sc, cam = degenerate()
        T = np.array((4096.0, -2048.0, 1024.0))
        for i in range(sc.instances.shape[0]):
            m = np.vstack([sc.transforms["m"][i], [0, 0, 0, 1]]).astype(np.float64)
            sc.set_instance_transform(i, translate(tuple(T)) @ m)
        return sc, dict(cam, eye=tuple(np.array(cam["eye"]) + T), target=tuple(np.array(cam["target"]) + T))

    for make, args in ((degenerate, {}), (degenerate, {"maxDiffuseVertices": 3, "maxPathVertices": 5}), (far_away, {})):
        sc, cam = make()
        frame = camera.Frame(160, 120, cam["fovy"], cam["eye"], cam["target"])
        out = {}
        for opt in (1, 0):
            r = BDPT(device=0, args=args)
            try:
                r.set_option("answer_last_rays", opt)
                r.update(sc)
                out[opt] = r.render(frame, 0, 6, aovs=False)
                out[opt]["answered"] = r.stats()["rays_answered"]
            finally:
                r.close()
        assert out[1]["answered"] > 0 and out[0]["answered"] == 0, make.__name__
        assert np.array_equal(out[0]["radiance"].view(np.uint32), out[1]["radiance"].view(np.uint32)), (make.__name__, args)
        assert np.array_equal(out[0]["ray_count"], out[1]["ray_count"]), (make.__name__, args)


def _debug_case(sc, cam, mode, flags=(), args=None, view_length=0, light_length=0, seeds=2, w=144, h=96, start=None):
    """One BDPTDebugMode on both sides: gDebugImage (in / out) and the frame, bit for bit."""
    from oracle import oracle_py
    from stratum_amd.bdpt import BDPT

    a = {"bdptFlag": list(flags)}
    a.update(args or {})
    r = BDPT(device=0, args=a)
    try:
        r.mPushConstants.gDebugViewPathLength = view_length
        r.mPushConstants.gDebugLightPathLength = light_length
        r.update(sc)
        frame = camera.Frame(w, h, cam["fovy"], cam["eye"], cam["target"])
        got = r.render(frame, 0, seeds, debug_mode=mode, debug_image=start)
        ref = oracle_py.OracleScene(sc).render(frame, r.push_constants(frame), r.mSamplingFlags, 0, seeds, debug_mode=mode, debug_image=start)
        assert np.array_equal(got["radiance"].view(np.uint32), ref["radiance"].view(np.uint32)), (sc.name, mode, "radiance")
        assert np.array_equal(got["ray_count"], ref["ray_count"]), (sc.name, mode)
        bad = (got["debug"].view(np.uint32) != ref["debug"].view(np.uint32)).any(axis=-1)
        assert not bad.any(), (sc.name, mode, flags, int(bad.sum()), got["debug"][bad][:3], ref["debug"][bad][:3])
        return got
    finally:
        r.close()


def test_debug_modes_of_the_first_hit():
    """BDPTDebugMode -> gDebugImage (bdpt.h:177-193, bdpt.hlsl:161-162,222-223,257-260,294-295, path.hlsli:950): the modes that
    overwrite a pixel with something of the first hit (albedo, is_specular, emission, normals before and after the normal map,
    the reprojection error) or of the last bounce (eDirOut), on a textured scene with normal maps and a mirror, a scene with
    sphere instances, and with a moving camera; pixels whose path never reaches the statement keep what the image held."""
    from stratum_amd import wire as W

    start = np.random.RandomState(5).rand(96, 144, 4).astype(np.float32)
    for make in (scenes.textured_box, lambda: scenes.textured_box(mirror_map=True), scenes.spheres_room, scenes.cornell_box):
        sc, cam = make()
        for mode in (W.DEBUG_ALBEDO, W.DEBUG_SPECULAR, W.DEBUG_EMISSION, W.DEBUG_SHADING_NORMAL, W.DEBUG_GEOMETRY_NORMAL, W.DEBUG_DIR_OUT, W.DEBUG_PREV_UV):
            flags = ["normalmaps"] if "textured" in sc.name else []
            got = _debug_case(sc, cam, mode, flags=flags, start=start)
            assert not np.array_equal(got["debug"], start), (sc.name, mode)
    # a frame without a debug image is the frame with one (the modes only watch)
    sc, cam = scenes.cornell_box()
    plain = _compare_frame(sc, cam, [], w=144, h=96)
    watched = _debug_case(sc, cam, W.DEBUG_ALBEDO)
    assert np.array_equal(plain["radiance"].view(np.uint32), watched["radiance"].view(np.uint32))
    hit = plain["visibility"]["instance_primitive_index"] != wire.MISS  # eAlbedo is the albedo output where something was hit (a miss writes albedo 1 and leaves the debug image alone)
    assert np.array_equal(plain["albedo"][..., :3][hit].view(np.uint32), watched["debug"][..., :3][hit].view(np.uint32)) and not watched["debug"][~hit].any()


def test_debug_modes_that_accumulate():
    """ePathLengthContribution (the unweighted contribution of one (view length, light length) pair: emission found by a path
    of that length, the NEE sample of a vertex — inline shadow rays only, a deferred one adds nothing upstream), eViewTrace-
    Contribution (all unweighted emission), eReservoirWeight (W of unoccluded reservoir samples, added onto what the image
    held), eLightTraceContribution and the view-length-1 pair (light tracing's splats with weight 1; add_light_trace)."""
    from stratum_amd import wire as W

    sc, cam = scenes.cornell_box()
    start = np.random.RandomState(6).rand(96, 144, 4).astype(np.float32)
    total = np.zeros((96, 144, 3), np.float64)
    for view_length in (2, 3, 4):  # emission seen directly, after one bounce, after two
        got = _debug_case(sc, cam, W.DEBUG_PATH_LENGTH_CONTRIBUTION, view_length=view_length, light_length=0, start=start, args={"maxDiffuseVertices": 3, "maxPathVertices": 5})
        assert (got["debug"][..., 3] == 1).all()  # started from (0, 0, 0, 1), not from `start`
        total += got["debug"][..., :3]
    assert total.mean() > 0.01
    for flags in (["~defershadowrays"], ["~defershadowrays", "~mis"], []):  # the NEE sample of the first / second vertex; nothing when deferred
        for view_length in (2, 3):
            got = _debug_case(sc, cam, W.DEBUG_PATH_LENGTH_CONTRIBUTION, flags=flags, view_length=view_length, light_length=1)
            assert (got["debug"][..., :3].sum() > 0) == ("~defershadowrays" in flags), (flags, view_length)
    got = _debug_case(sc, cam, W.DEBUG_VIEW_TRACE_CONTRIBUTION, start=start, args={"maxDiffuseVertices": 3})
    assert got["debug"][..., :3].mean() > 0.01
    for flags in (["neereservoirs", "~defershadowrays"], ["neereservoirs"]):
        got = _debug_case(sc, cam, W.DEBUG_RESERVOIR_WEIGHT, flags=flags, start=start)
        assert (not np.array_equal(got["debug"], start)) == ("~defershadowrays" in flags)
    # light tracing
    for mode, vl, ll in ((W.DEBUG_LIGHT_TRACE_CONTRIBUTION, 0, 0), (W.DEBUG_PATH_LENGTH_CONTRIBUTION, 1, 2), (W.DEBUG_PATH_LENGTH_CONTRIBUTION, 1, 3), (W.DEBUG_VIEW_TRACE_CONTRIBUTION, 0, 0)):
        got = _debug_case(sc, cam, mode, flags=["connecttoviews"], view_length=vl, light_length=ll, start=start, w=128, h=96)
        assert got["debug"][..., :3].mean() > 0
    # ... with gMaxPathVertices = 2 no photon is sampled, yet add_light_trace runs (BDPT.cpp:653,753) over samples nobody wrote
    # this frame (pinned to zero) and overwrites every pixel of the image in these two modes (bdpt.hlsl:335-336)
    for mode, vl in ((W.DEBUG_LIGHT_TRACE_CONTRIBUTION, 0), (W.DEBUG_PATH_LENGTH_CONTRIBUTION, 1)):
        got = _debug_case(sc, cam, mode, flags=["connecttoviews"], args={"maxPathVertices": 2}, view_length=vl, light_length=1, start=start)
        assert not got["debug"][..., :3].any() and (got["debug"][..., 3] == 1).all()
    # light-subpath connections (accumulate_contribution with the light vertex's length, path.hlsli:797,820): the (view, light)
    # pairs with a light length of 2 and more, from the subpath of the same index or one vertex of the cache; connect_lvc's
    # deferred record adds to the radiance only (:781-789)
    for flags, adds in ((["connecttolightpaths"], True), (["connecttolightpaths", "lightvertexcache", "~defershadowrays"], True), (["connecttolightpaths", "lightvertexcache"], False),
                        (["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "~defershadowrays"], True)):
        for vl, ll in ((2, 2), (2, 3), (3, 2)):
            got = _debug_case(sc, cam, W.DEBUG_PATH_LENGTH_CONTRIBUTION, flags=flags, view_length=vl, light_length=ll, start=start, args={"maxDiffuseVertices": 4, "maxPathVertices": 6, "lightPathCount": 5000})
            assert (got["debug"][..., :3].sum() > 0) == adds, (flags, vl, ll)
    # several seeds of a call are upstream's successive frames: the same image as call after call
    a = _debug_case(sc, cam, W.DEBUG_RESERVOIR_WEIGHT, flags=["neereservoirs", "~defershadowrays"], seeds=3, start=start)
    b = start
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0, args={"bdptFlag": ["neereservoirs", "~defershadowrays"]})
    try:
        r.update(sc)
        frame = camera.Frame(144, 96, cam["fovy"], cam["eye"], cam["target"])
        for seed in range(3):
            b = r.render(frame, seed, 1, debug_mode=W.DEBUG_RESERVOIR_WEIGHT, debug_image=b)["debug"]
    finally:
        r.close()
    assert np.array_equal(a["debug"].view(np.uint32), b.view(np.uint32))


def test_debug_modes_of_the_environment():
    """eEnvironmentSampleTest / eEnvironmentSamplePDF (bdpt.hlsl:190-205): nothing is traced; eight environment samples drawn
    from the pixel's stream as spots around the view direction (added to the image), or the pdf of the view direction."""
    from stratum_amd import wire as W
    from test_detmath_edges import check_environment_sample_test_image

    start = np.random.RandomState(7).rand(96, 144, 4).astype(np.float32)
    for image in (True, False):
        sc, cam = scenes.environment_scene(image=image, emitter=True)
        for mode in (W.DEBUG_ENVIRONMENT_SAMPLE_TEST, W.DEBUG_ENVIRONMENT_SAMPLE_PDF):
            for flags in ([], ["sampleenvironmentmapdirectly"]):
                got = _debug_case(sc, cam, mode, flags=flags, start=start)
                assert got["ray_count"][0] == 0 and not got["radiance"][..., :3].any()
                assert np.array_equal(got["debug"][..., 3], start[..., 3]) and not np.array_equal(got["debug"][..., :3], start[..., :3])
                if mode == W.DEBUG_ENVIRONMENT_SAMPLE_TEST:
                    # the spots are 1024 pow(cos, 1024): in [0, 1024] each, the same in the three channels, small (the image
                    # equals the oracle's bit for bit, so the same holds for that one; its own test needs no GPU)
                    check_environment_sample_test_image(got["debug"], start)


def test_bounded_wide8_walk_with_recycled_device_memory():
    """A ray that overflows the bounded LDS stack of the 8-wide walk must stop there (k_trace_deep traces it again): walking on
    with an exit sentinel lost would read world-space groups with an instance's octant — child indices the node does not have,
    and behind the last node whatever the allocation holds. Fresh device memory is zero (an empty node), so the case only shows
    with the heap recycled: STHIP_POISON_ALLOC fills every new buffer (read once per process, hence the child process). The
    case is number 129 of fuzz seed 302: a fog scene with instances, wide_bvh = 3, lds_stack_levels = 6."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_FUZZ_ONLY="129")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), "130", "302"], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "1 cases compared, 0 rejected on both sides, 0 mismatches" in out.stdout


@pytest.mark.gpu
def test_host_outputs_written_in_place():
    """A caller's own host buffers (`host_outputs`: the dict an earlier call returned) are filled in place with what a call with
    fresh buffers returns; a buffer of the wrong size is refused before anything is launched."""
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    r = BDPT(device=0)
    try:
        r.update(sc)
        frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
        fresh = r.render(frame, 3, 2)
        bufs = r.render(frame, 0, 1)
        keep = {k: v for k, v in bufs.items()}
        again = r.render(frame, 3, 2, host_outputs=bufs)
        for k in ("radiance", "albedo", "visibility", "depth", "prev_uv", "ray_count"):
            assert again[k] is keep[k], k
            assert again[k].tobytes() == fresh[k].tobytes(), k
        only = r.render(frame, 4, 1, aovs=False, host_outputs=bufs)
        assert set(only) == {"radiance", "ray_count"} and only["radiance"] is keep["radiance"]
        with pytest.raises(ValueError):
            r.render(camera.Frame(100, 64, cam["fovy"], cam["eye"], cam["target"]), 0, 1, host_outputs=bufs)
    finally:
        r.close()


@pytest.mark.gpu
def test_reuse_grids_persist_between_calls():
    """`reuse_grids_persist`: the hash grids the last seed of a call leaves are what the first seed of the next call looks into
    (upstream's previous frame for a host that renders one frame per call, BDPT.cpp:482-483,621-627). Three calls of one seed
    are then the chain a call of three seeds traces — which the oracle tests pin — frame by frame: the running mean
    (temporal_accumulation.hlsl:118-131) of the three frames, bit for bit, and the same rays. Setting the option again drops the
    grids: that frame is a chain's first (gReservoirSpatialM = 0 upstream)."""
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(96, 72, cam["fovy"], cam["eye"], cam["target"])
    for flags, args in (
        (["neereservoirs", "neereservoirreuse"], {"reservoirM": 2}),
        (["connecttolightpaths", "lightvertexcache", "lvcreservoirs", "lvcreservoirreuse", "~defershadowrays"], {"lightPathCount": 3000, "reservoirM": 2, "maxDiffuseVertices": 3}),
    ):
        r = BDPT(device=0, args=dict(args, bdptFlag=flags))
        try:
            r.update(sc)
            chain = r.render(frame, 4, 3, aovs=False)
            alone = [r.render(frame, 4 + i, 1, aovs=False) for i in range(3)]  # every call a chain of its own
            r.set_option("reuse_grids_persist", 1)
            kept = [r.render(frame, 4 + i, 1, aovs=False) for i in range(3)]
            acc = kept[0]["radiance"].copy()  # k_resolve's running mean: rgb and, in .w, the samples that counted (a non-finite one does not)
            for f in (kept[1]["radiance"], kept[2]["radiance"]):
                nn = acc[..., 3] + f[..., 3]
                with np.errstate(all="ignore"):
                    alpha = np.clip(f[..., 3] / nn, np.float32(0), np.float32(1))[..., None]
                live = acc[..., 3] > 0
                rgb = np.where(live[..., None], acc[..., :3] + alpha * (f[..., :3] - acc[..., :3]), f[..., :3])
                acc = np.concatenate([rgb, np.where(live, nn, f[..., 3])[..., None]], -1).astype(np.float32)
            assert np.array_equal(acc.view(np.uint32), chain["radiance"].view(np.uint32)), flags
            assert np.array_equal(sum(f["ray_count"] for f in kept), chain["ray_count"]), flags
            assert np.array_equal(kept[0]["radiance"], alone[0]["radiance"]) and not np.array_equal(kept[1]["radiance"], alone[1]["radiance"]), flags
            # dropped: by setting the option again, by another table size, by a new scene
            r.set_option("reuse_grids_persist", 1)
            assert np.array_equal(r.render(frame, 6, 1, aovs=False)["radiance"], alone[2]["radiance"]), flags
            r.render(frame, 5, 1, aovs=False)
            r.mPushConstants.gHashGridBucketCount = 150000
            other = r.render(frame, 6, 1, aovs=False)["radiance"]
            r.set_option("reuse_grids_persist", 0)
            assert np.array_equal(other, r.render(frame, 6, 1, aovs=False)["radiance"]), flags
            r.mPushConstants.gHashGridBucketCount = 200000
            r.set_option("reuse_grids_persist", 1)
            r.render(frame, 5, 1, aovs=False)
            r.update(sc)
            assert np.array_equal(r.render(frame, 6, 1, aovs=False)["radiance"], alone[2]["radiance"]), flags
        finally:
            r.close()


def test_an_upload_refused_by_its_check_leaves_the_resident_scene():
    """A call refused by check_scene changes nothing but sthip_last_error: the previous scene still renders the same frame with
    the same rays, from the first hits kept before the refused call (no primary packet is traced again). A failure from the
    build onward leaves no scene, as it always has."""
    import re

    from stratum_amd._lib import StratumHipError
    from stratum_amd.bdpt import BDPT

    sc, cam = scenes.cornell_box()
    frame = camera.Frame(32, 32, cam["fovy"], cam["eye"], cam["target"])
    r = BDPT(device=0)
    try:
        r.update(sc)
        first = {k: v.copy() for k, v in r.render(frame, 0, 1).items()}
        assert r.stats()["rays_primary_packets"] > 0
        bad, _ = scenes.cornell_box()
        bad.lights[0] = bad.instances.shape[0]
        with pytest.raises(StratumHipError, match=re.escape("sthip_scene_upload failed (-1): scene: gLightInstances entry out of range")):
            r.update(bad)
        again = r.render(frame, 0, 1)
        for k in first:
            assert again[k].tobytes() == first[k].tobytes(), k
        assert r.stats()["rays_primary_packets"] == 0
        # the builder refuses an index past vertex_count: that is found after the previous scene was retired
        bad, _ = scenes.cornell_box()
        stride = int(bad.instances["packed"][0, 1] >> 28)
        at = int(bad.instances["packed"][0, 3])
        bad.indices[at : at + stride] = np.frombuffer((0xFFFF if stride == 2 else 0x7FFFFFFF).to_bytes(stride, "little"), dtype=np.uint8)
        with pytest.raises(StratumHipError, match=re.escape("sthip_scene_upload failed (-1): scene: vertex index exceeds gVertices")):
            r.update(bad)
        with pytest.raises(StratumHipError, match=r"sthip_render\w* failed \(-5\)"):
            r.render(frame, 0, 1)
    finally:
        r.close()
