"""The denoiser's filter (sthip_denoise_filter: SVGF variance estimate, a-trous passes, history tap).

The reference of every comparison is tests/cpp/denoise_ref.cpp: a scalar restatement of estimate_variance.hlsl and atrous.hlsl
under the arithmetic contract written at sthip_denoise_desc (include/sthip.h), built here with g++ -O2 -ffp-contract=off. The
first half of this file needs no GPU: the ABI, and known answers of the reference itself. The second half (marked gpu) compares
the device's images with the reference's bit for bit.

Bit for bit means: equal as uint32 (uint16 for RGBA16F) after every NaN has been replaced by one canonical NaN. The sign and
payload of a NaN are no part of the contract — an x86 host makes 0 * inf the negative default NaN, a CDNA device the positive
one — while WHERE a NaN stands is part of it, and is compared.

Known answer for the variance of the a-trous kernel: one pass over a flat region with constant variance multiplies it by
sum(k^2) / sum(k)^2 of the 5x5 kernel = (35/18)^2 / (64/9)^2 = (35/128)^2."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from stratum_amd import _lib, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = wire.FILTER_TYPES if hasattr(wire, "FILTER_TYPES") else ["Atrous", "Box3", "Box5", "Subsampled", "Box3Subsampled", "Box5Subsampled"]


# ---------------------------------------------------------------------------------------------------------------------------
# the reference program
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def ref_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("denoise_ref") / "denoise_ref")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "denoise_ref.cpp")])
    return exe


def views_of(rects):
    v = np.zeros(len(rects), wire.ViewData)
    for k, (x0, y0, x1, y1) in enumerate(rects):
        v[k]["image_min"] = (x0, y0)
        v[k]["image_max"] = (x1, y1)
    return v


def problem(w, h, rects=None, **kw):
    """A flat problem: one instance, normal +z (packed 0: unpacks to (0, 0, 1) exactly), depth 1 without slope, colour 0,
    history length 1, moments 0 — tests overwrite what they are about."""
    vis = np.zeros((h, w), wire.VisibilityInfo)
    depth = np.zeros((h, w), wire.DepthInfo)
    depth["z"] = 1
    p = dict(
        views=views_of(rects or [(0, 0, w, h)]),
        visibility=vis,
        depth=depth,
        instance_index_map=None,
        accum_color=np.zeros((h, w, 4), np.float32),
        accum_moments=np.zeros((h, w, 2), np.float32),
        filter_images=[np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)],
        iterations=1,
        filter_type="Atrous",
        history_tap=0,
        history_limit=0.0,
        variance_boost_length=0.0,
        sigma_luminance_boost=3.0,
    )
    p["accum_color"][..., 3] = 1
    p.update(kw)
    return p


def run_ref(exe, tmp, p, half=False):
    """-> (gFilterImages[0], gFilterImages[1], gAccumColor) of the reference: float32, or float16 with `half` (the colour
    images of `p` then hold half-representable values)."""
    h, w = p["accum_color"].shape[:2]
    imap = p["instance_index_map"]
    hdr = np.zeros(12, np.uint32)
    hdr[0] = np.frombuffer(b"DNR1", np.uint32)[0]
    hdr[1:8] = [w, h, len(p["views"]), 0 if imap is None else len(imap), p["iterations"], wire.FILTER[p["filter_type"]], p["history_tap"]]
    hdr[8:11] = np.array([p["history_limit"], p["variance_boost_length"], p["sigma_luminance_boost"]], np.float32).view(np.uint32)
    fin, fout = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(fin, "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.ascontiguousarray(p["views"], wire.ViewData).tobytes())
        f.write(np.ascontiguousarray(p["visibility"], wire.VisibilityInfo).tobytes())
        f.write(np.ascontiguousarray(p["depth"], wire.DepthInfo).tobytes())
        if imap is not None:
            f.write(np.ascontiguousarray(imap, np.uint32).tobytes())
        for a in (p["accum_color"], p["accum_moments"], p["filter_images"][0], p["filter_images"][1]):
            f.write(np.ascontiguousarray(a).astype(np.float32).tobytes())  # (float16 -> float32 is exact)
    subprocess.check_call([exe, fin, fout] + (["--half"] if half else []))
    out = np.fromfile(fout, np.float16 if half else np.float32).reshape(3, h, w, 4)
    return out[0], out[1], out[2]


def bits(a):
    """The comparison's view of an image: its words, every NaN replaced by one canonical NaN (see the module docstring)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float16:
        u = a.view(np.uint16).copy()
        u[np.isnan(a)] = 0x7E00
    else:
        u = a.view(np.uint32).copy()
        u[np.isnan(a)] = 0x7FC00000
    return u


# ---------------------------------------------------------------------------------------------------------------------------
# ABI (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def test_abi_symbol_descriptor_and_enum(built):
    assert "sthip_denoise_filter" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "sthip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+sthip_denoise_filter\s*\(\s*sthip_ctx\s*\*\s*\w*\s*,\s*const\s+sthip_denoise_desc\s*\*", code)
    assert hasattr(_lib.lib(), "sthip_denoise_filter")
    names = re.findall(r"\bSTHIP_FILTER_(?!TYPE_COUNT)[A-Z0-9_]+", code)
    assert names == ["STHIP_FILTER_ATROUS", "STHIP_FILTER_BOX3", "STHIP_FILTER_BOX5", "STHIP_FILTER_SUBSAMPLED", "STHIP_FILTER_BOX3_SUBSAMPLED", "STHIP_FILTER_BOX5_SUBSAMPLED"]
    assert len(wire.FILTER_TYPES) == 6 and wire.FILTER["Box3"] == 1


def test_wire_descriptor_has_the_headers_size(built, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sthip.h"\nint main(void) { printf("%zu %zu %zu %zu", sizeof(sthip_denoise_desc), offsetof(sthip_denoise_desc, gViews), '
                   "offsetof(sthip_denoise_desc, gFilterImages), offsetof(sthip_denoise_desc, sigma_luminance_boost)); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    size, o_views, o_filter, o_sigma = (int(t) for t in subprocess.check_output([exe]).split())
    D = wire.DenoiseDesc
    assert (C.sizeof(D), D.gViews.offset, D.gFilterImages.offset, D.sigma_luminance_boost.offset) == (size, o_views, o_filter, o_sigma)


# ---------------------------------------------------------------------------------------------------------------------------
# known answers of the reference (no GPU). rtol 1e-5: about 30 additions of 6e-8 each
# ---------------------------------------------------------------------------------------------------------------------------
RTOL = 1e-5


def test_ref_variance_at_or_above_the_history_limit_is_the_pixels_own(ref_exe, tmp_path):
    rng = np.random.RandomState(1)
    p = problem(19, 13, history_limit=4.0)
    p["accum_color"][..., :3] = rng.rand(13, 19, 3)
    p["accum_color"][..., 3] = rng.choice([4.0, 5.0, 100.0], size=(13, 19))
    p["accum_moments"][:] = rng.rand(13, 19, 2)
    f0, _, _ = run_ref(ref_exe, tmp_path, p)
    m = p["accum_moments"]
    assert np.array_equal(f0[..., 3], np.abs(m[..., 1] - m[..., 0] * m[..., 0]))
    assert np.array_equal(f0[..., :3], p["accum_color"][..., :3])


@pytest.mark.parametrize("boost", [0.0, 20.0])
def test_ref_variance_below_the_history_limit_with_uniform_moments(ref_exe, tmp_path, boost):
    p = problem(19, 13, history_limit=100.0, variance_boost_length=boost)
    p["accum_color"][..., :3] = 0.25
    p["accum_moments"][..., 0] = 0.5
    p["accum_moments"][..., 1] = 1.0
    for n in (0.5, 4.0):  # both footprints: 7x7 up to one sample, 5x5 beyond
        p["accum_color"][..., 3] = n
        f0, _, _ = run_ref(ref_exe, tmp_path, p)
        want = 0.75 * (max(1.0, boost / (1 + n)) if boost > 0 else 1.0)
        assert np.allclose(f0[..., 3], want, rtol=RTOL, atol=0)
        assert np.allclose(f0[..., :3], 0.25, rtol=RTOL, atol=0)


def _flat_with_variance(w, h, variance, **kw):
    p = problem(w, h, **kw)
    p["accum_moments"][..., 1] = variance  # history_limit 0: every pixel takes |m.y - m.x^2|
    return p


def test_ref_atrous_reproduces_a_linear_colour_and_shrinks_the_variance(ref_exe, tmp_path):
    w, h = 31, 23
    p = _flat_with_variance(w, h, 2.0, iterations=2)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    r, b = 1 + 0.03 * x, 2 + 0.05 * y
    g = (1.5 - 0.2126 * r - 0.0722 * b) / 0.7152  # luminance 1.5 everywhere
    p["accum_color"][..., 0], p["accum_color"][..., 1], p["accum_color"][..., 2] = r, g, b
    f0, f1, _ = run_ref(ref_exe, tmp_path, p)
    shrink = (35.0 / 128.0) ** 2  # sum(k^2) / sum(k)^2, sum(k) = 64/9, sum(k^2) = (35/18)^2
    inner1 = (slice(2, h - 2), slice(2, w - 2))  # pass 0 (step 1) is whole 2 pixels from the edge
    assert np.allclose(f1[inner1][..., :3], p["accum_color"][inner1][..., :3], rtol=RTOL, atol=0)
    assert np.allclose(f1[inner1][..., 3], 2.0 * shrink, rtol=RTOL, atol=0)
    inner2 = (slice(6, h - 6), slice(6, w - 6))  # pass 1 (step 2) reads whole pixels of pass 0 up to 4 away
    assert np.allclose(f0[inner2][..., :3], p["accum_color"][inner2][..., :3], rtol=RTOL, atol=0)
    assert np.allclose(f0[inner2][..., 3], 2.0 * shrink * shrink, rtol=RTOL, atol=0)


@pytest.mark.parametrize("filter_type", FILTERS)
def test_ref_zero_variance_keeps_a_step_sharp(ref_exe, tmp_path, filter_type):
    w, h = 24, 16
    p = problem(w, h, iterations=3, filter_type=filter_type)
    p["accum_color"][:, :11, :3] = (0.2, 0.3, 0.1)
    p["accum_color"][:, 11:, :3] = (0.9, 0.7, 0.8)
    f0, f1, _ = run_ref(ref_exe, tmp_path, p)
    for img in (f0, f1):
        assert np.allclose(img[..., :3], p["accum_color"][..., :3], rtol=RTOL, atol=0)


def test_ref_a_miss_pixel_passes_through(ref_exe, tmp_path):
    rng = np.random.RandomState(3)
    w, h = 17, 11
    p = _flat_with_variance(w, h, 1.0, iterations=2)
    p["accum_color"][..., :3] = rng.rand(h, w, 3)
    p["depth"]["z"][5, 8] = np.inf
    p["visibility"]["instance_primitive_index"][5, 8] = wire.MISS
    f0, f1, _ = run_ref(ref_exe, tmp_path, p)
    assert np.array_equal(f1[5, 8].view(np.uint32), np.append(p["accum_color"][5, 8, :3], np.float32(1.0)).view(np.uint32))
    assert np.array_equal(f0[5, 8].view(np.uint32), f1[5, 8].view(np.uint32))
    assert not np.array_equal(f1[5, 4], np.append(p["accum_color"][5, 4, :3], np.float32(1.0)))  # (its neighbours are filtered)


def test_ref_taps_stay_inside_their_view(ref_exe, tmp_path):
    w, h = 26, 12
    p = _flat_with_variance(w, h, 4.0, rects=[(0, 0, 13, h), (13, 0, w, h)], iterations=3, filter_type="Box5")
    p["accum_color"][:, :13, :3] = 1.0
    p["accum_color"][:, 13:, :3] = 5.0  # (the variance is large: the luminance weight would let these mix)
    f0, f1, _ = run_ref(ref_exe, tmp_path, p)
    for img in (f0, f1):
        assert np.allclose(img[:, :13, :3], 1.0, rtol=RTOL, atol=0) and np.allclose(img[:, 13:, :3], 5.0, rtol=RTOL, atol=0)
    one = dict(p, views=views_of([(0, 0, w, h)]))
    g0, g1, _ = run_ref(ref_exe, tmp_path, one)
    assert g1[:, 12, 0].min() > 1.2  # with one view over both halves they do mix


def test_ref_history_tap_copies_rgb_and_keeps_alpha(ref_exe, tmp_path):
    rng = np.random.RandomState(5)
    w, h = 15, 9
    p = problem(w, h, history_limit=100.0, history_tap=1)
    p["accum_color"][..., :3] = rng.rand(h, w, 3)
    p["accum_color"][..., 3] = rng.choice([1.0, 2.0, 7.0], size=(h, w))
    p["accum_moments"][:] = rng.rand(h, w, 2)
    f0, _, acc = run_ref(ref_exe, tmp_path, p)
    assert not np.array_equal(f0[..., :3], p["accum_color"][..., :3])  # (the variance pass blurred the colour)
    assert np.array_equal(acc[..., :3].view(np.uint32), f0[..., :3].view(np.uint32))
    assert np.array_equal(acc[..., 3], p["accum_color"][..., 3])
    _, _, untouched = run_ref(ref_exe, tmp_path, dict(p, history_tap=2))  # above `iterations`: never fires
    assert np.array_equal(untouched, p["accum_color"])


@pytest.mark.parametrize("what", ["color_nan", "color_inf", "depth_nan", "depth_inf", "moments_nan", "moments_inf"])
def test_ref_nan_and_inf_stay_within_the_taps_that_see_them(ref_exe, tmp_path, what):
    rng = np.random.RandomState(7)
    w, h = 33, 25
    p = problem(w, h, history_limit=100.0, iterations=1)
    p["accum_color"][..., :3] = 0.5 + rng.rand(h, w, 3)
    p["accum_color"][..., 3] = 2.0
    p["accum_moments"][..., 0] = 1 + rng.rand(h, w)
    p["accum_moments"][..., 1] = 3 + rng.rand(h, w)
    clean = run_ref(ref_exe, tmp_path, p)
    cx, cy = 16, 12
    bad = np.float32(np.nan if what.endswith("nan") else np.inf)
    q = dict(p, accum_color=p["accum_color"].copy(), accum_moments=p["accum_moments"].copy(), depth=p["depth"].copy())
    if what.startswith("color"):
        q["accum_color"][cy, cx, 1] = bad
    elif what.startswith("depth"):
        q["depth"]["z"][cy, cx] = bad
    else:
        q["accum_moments"][cy, cx, 0] = bad
    dirty = run_ref(ref_exe, tmp_path, q)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    # the variance pass reaches 2 pixels (history length 2), the filter's sigma 1 more, its taps at step 1 two more
    far = np.maximum(np.abs(x - cx), np.abs(y - cy)) > 5
    for a, b in zip(clean[:2], dirty[:2]):
        assert np.array_equal(a[far].view(np.uint32), b[far].view(np.uint32))
        assert np.isfinite(b[far]).all()
    assert not np.array_equal(bits(clean[1]), bits(dirty[1]))  # (it does show near the pixel)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the device's images against the reference, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
def synthetic(w=53, h=37, seed=0, half=False):
    """Two views side by side (the right one two rows short: those pixels belong to no view), random colour, moments and guides,
    planted NaN / inf, miss pixels, history lengths on both sides of 1 and of the history limit (4), a non-identity map."""
    rng = np.random.RandomState(seed)
    split = w // 2 + 1
    p = problem(w, h, rects=[(0, 0, split, h), (split, 0, w, h - 2)], history_limit=4.0)
    cd = np.float16 if half else np.float32
    col = np.empty((h, w, 4), np.float32)
    col[..., :3] = rng.rand(h, w, 3) * np.array([2.0, 1.0, 0.5]) + 0.25 * ((np.arange(w) // 6) % 2)[None, :, None]
    col[..., 3] = rng.choice([0.5, 1.0, 2.0, 3.0, 4.0, 9.0], size=(h, w))
    mom = np.empty((h, w, 2), np.float32)
    lum = col[..., :3] @ np.array([0.2126, 0.7152, 0.0722], np.float32)
    mom[..., 0] = lum * (0.8 + 0.4 * rng.rand(h, w))
    mom[..., 1] = mom[..., 0] ** 2 + rng.rand(h, w) * np.where(rng.rand(h, w) < 0.3, 0.0, 0.2)  # (some zero variance)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    inst = ((x // 9) + (y // 11)) % 4
    vis, depth = p["visibility"], p["depth"]
    vis["instance_primitive_index"] = (inst | (rng.randint(0, 50, size=(h, w)) << 16)).astype(np.uint32)
    palette = np.array([[0.0, 0.0], [0.3, 0.1], [-0.6, 0.7], [0.2, -0.9]], np.float32)  # octahedral coordinates; the last two fold (z < 0)
    oct_xy = (palette[((x // 13) + (y // 7)) % 4] + 0.02 * rng.randn(h, w, 2)).astype(np.float16)
    vis["packed_normal"] = oct_xy[..., 0].view(np.uint16).astype(np.uint32) | (oct_xy[..., 1].view(np.uint16).astype(np.uint32) << 16)
    depth["z"] = 2 + 0.05 * x + 0.03 * y + 0.01 * rng.randn(h, w) + 1.5 * (inst == 2)
    depth["prev_z"] = depth["z"]
    depth["dz_dxy"][..., 0] = 0.05 + 0.01 * rng.randn(h, w)
    depth["dz_dxy"][..., 1] = 0.03 + 0.01 * rng.randn(h, w)
    miss = rng.rand(h, w) < 0.04
    vis["instance_primitive_index"][miss] = wire.MISS
    depth["z"][miss] = np.inf
    for k, (yy, xx) in enumerate([(3, 4), (20, 30), (33, 50), (10, 26), (18, 12), (30, 40), (7, 45), (25, 5)]):
        yy, xx = yy % h, xx % w
        bad = np.float32([np.nan, np.inf, -np.inf][k % 3])
        if k < 3:
            col[yy, xx, k % 4] = bad
        elif k < 5:
            depth["z"][yy, xx] = bad
        elif k < 7:
            mom[yy, xx, k % 2] = bad
        else:
            col[yy, xx, 3] = bad
    p["accum_color"] = col.astype(cd)
    p["accum_moments"] = mom
    p["instance_index_map"] = np.array([1, 0, 2, 7], np.uint32)
    p["filter_images"] = [rng.rand(h, w, 4).astype(cd), rng.rand(h, w, 4).astype(cd)]
    return p


def run_gpu(ctx, p):
    from stratum_amd.post import denoise_desc

    keep = []
    d, f0, f1, acc = denoise_desc(p["views"], p["visibility"], p["depth"], p["accum_color"].copy(), p["accum_moments"], p["iterations"], p["filter_type"], p["history_tap"],
                                  p["history_limit"], p["variance_boost_length"], p["sigma_luminance_boost"], p["instance_index_map"], p["filter_images"], keep, ctx.color_dtype)
    ctx._check(_lib.lib().sthip_denoise_filter(ctx._h, C.byref(d)), "sthip_denoise_filter")
    return f0, f1, acc


def assert_same(got, want, what):
    for name, g, r in zip(("gFilterImages[0]", "gFilterImages[1]", "gAccumColor"), got, want):
        assert g.dtype == r.dtype and g.shape == r.shape
        gb, rb = bits(g), bits(r)
        diff = (gb != rb).any(-1)
        print("%s %s: %d of %d pixels differ" % (what, name, diff.sum(), diff.size))
        assert np.array_equal(gb, rb), "%s %s: %d pixels differ, first at (y, x) = %s" % (what, name, diff.sum(), tuple(np.argwhere(diff)[0]))


@pytest.fixture(scope="module")
def gpu_ctx(built):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def gpu_half_ctx(built):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0)
    r.set_half_color_precision(True)
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def _synthetic(half):
    return synthetic(half=half)


@pytest.fixture(scope="module")
def synthetic_reference(ref_exe, tmp_path_factory):
    """The reference's answer for one configuration of the synthetic problem, computed once per configuration."""
    tmp = tmp_path_factory.mktemp("denoise_synthetic")
    cache = {}

    def get(half, **cfg):
        key = (half,) + tuple(sorted(cfg.items()))
        if key not in cache:
            cache[key] = run_ref(ref_exe, tmp, dict(_synthetic(half), **cfg), half)
        return cache[key]

    return get


TAP_AND_BOOST = [(tap, boost) for tap in (0, 1, 2) for boost in (0.0, 6.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("filter_type", FILTERS)
def test_gpu_synthetic_equals_reference(gpu_ctx, synthetic_reference, filter_type, iterations):
    for tap, boost in TAP_AND_BOOST:
        cfg = dict(filter_type=filter_type, iterations=iterations, history_tap=tap, variance_boost_length=boost)
        got = run_gpu(gpu_ctx, dict(_synthetic(False), **cfg))
        assert_same(got, synthetic_reference(False, **cfg), "%s x%d tap %d boost %g" % (filter_type, iterations, tap, boost))


@pytest.mark.gpu
@pytest.mark.parametrize("filter_type,iterations,tap,boost", [("Atrous", 5, 2, 6.0), ("Box3", 2, 1, 0.0), ("Box5Subsampled", 5, 0, 6.0), ("Subsampled", 1, 1, 0.0)])
def test_gpu_synthetic_half_precision_equals_reference(gpu_half_ctx, synthetic_reference, filter_type, iterations, tap, boost):
    cfg = dict(filter_type=filter_type, iterations=iterations, history_tap=tap, variance_boost_length=boost)
    got = run_gpu(gpu_half_ctx, dict(_synthetic(True), **cfg))
    assert got[0].dtype == np.float16
    assert_same(got, synthetic_reference(True, **cfg), "half %s x%d" % (filter_type, iterations))


@pytest.mark.gpu
@pytest.mark.parametrize("block", [0, 1])
def test_gpu_block_shape_does_not_change_results(gpu_ctx, synthetic_reference, block):
    cfg = dict(filter_type="Atrous", iterations=5, history_tap=2, variance_boost_length=6.0)
    gpu_ctx.set_option("denoise_block", block)
    try:
        got = run_gpu(gpu_ctx, dict(_synthetic(False), **cfg))
    finally:
        gpu_ctx.set_option("denoise_block", 0)
    assert_same(got, synthetic_reference(False, **cfg), "block shape %d" % block)


@pytest.mark.gpu
def test_gpu_device_pointer_form(gpu_ctx, ref_exe, tmp_path):
    import torch

    from stratum_amd.post import Denoiser

    p = dict(synthetic(96, 64, seed=4), iterations=4, filter_type="Box5Subsampled", history_tap=3, variance_boost_length=6.0)
    host = run_gpu(gpu_ctx, p)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    t_vis, t_depth, t_map = dev(p["visibility"]), dev(p["depth"]), dev(p["instance_index_map"])
    t_acc, t_mom, t_f0, t_f1 = dev(p["accum_color"]), dev(p["accum_moments"]), dev(p["filter_images"][0]), dev(p["filter_images"][1])
    dn = Denoiser(gpu_ctx, history_limit=p["history_limit"], iterations=4, filter_type="Box5Subsampled", history_tap=3, variance_boost_length=6.0)
    torch.cuda.synchronize()
    dn.device(96, 64, p["views"], t_vis.data_ptr(), t_depth.data_ptr(), t_acc.data_ptr(), t_mom.data_ptr(), t_f0.data_ptr(), t_f1.data_ptr(), t_map.data_ptr(), 4)
    gpu_ctx.stats()  # joins the context's stream
    torch.cuda.synchronize()
    back = lambda t: t.cpu().numpy().view(np.float32).reshape(64, 96, 4)
    got = (back(t_f0), back(t_f1), back(t_acc))
    for g, hst in zip(got, host):
        assert np.array_equal(g.view(np.uint32), hst.view(np.uint32))  # the same bytes as the host form, NaNs included
    assert_same(got, run_ref(ref_exe, tmp_path, p), "device pointers")


def _oracle_frames(n_frames, w=96, h=64):
    """n_frames of the Cornell box from the oracle, one seed per frame, the camera sliding (as tests/test_post.py makes them)."""
    from oracle import oracle_py
    from stratum_amd import camera, scenes

    sc, cam = scenes.cornell_box()
    o = oracle_py.OracleScene(sc)
    frames, outs, prev = [], [], None
    for k in range(n_frames):
        eye = np.array(cam["eye"]) + np.array([0.05, 0.02, 0.0]) * k
        fr = camera.Frame(w, h, cam["fovy"], tuple(eye), cam["target"], prev=prev)
        outs.append(o.render(fr, wire.default_push_constants(w, h, sc.light_count), wire.DEFAULT_SAMPLING_FLAGS, k, 1, threads=4))
        frames.append(fr)
        prev = fr
    return sc, frames, outs


@pytest.mark.gpu
def test_gpu_rendered_frames_through_the_denoiser(gpu_ctx, ref_exe, tmp_path):
    from oracle import oracle_py
    from stratum_amd.post import Denoiser

    _, frames, outs = _oracle_frames(3)
    h, w = 64, 96
    cfg = dict(history_limit=8.0, iterations=4, filter_type="Atrous", history_tap=1, variance_boost_length=4.0, sigma_luminance_boost=3.0)
    dn = Denoiser(gpu_ctx, reprojection=True, demodulate_albedo=True, **cfg)
    vis0 = np.zeros((h, w), wire.VisibilityInfo)
    vis0["instance_primitive_index"] = wire.MISS
    hist = {"accum_color": np.zeros((h, w, 4), np.float32), "accum_moments": np.zeros((h, w, 2), np.float32), "visibility": vis0, "depth": np.zeros((h, w), wire.DepthInfo)}
    for k, (fr, out) in enumerate(zip(frames, outs)):
        got = dn(out, fr.views)
        oc, om = oracle_py.accumulate(out, hist, fr.views, True, True, cfg["history_limit"])
        p = problem(w, h, views=np.ascontiguousarray(fr.views, wire.ViewData), visibility=out["visibility"], depth=out["depth"], accum_color=oc, accum_moments=om, **{k_: v for k_, v in cfg.items()})
        f0, f1, acc = run_ref(ref_exe, tmp_path, p)
        assert_same((dn.filter_images[0], dn.filter_images[1], dn.accumulation.history["accum_color"]), (f0, f1, acc), "frame %d" % k)
        assert got is dn.filter_images[0]  # gFilterImages[iterations % 2]
        hist = {"accum_color": acc, "accum_moments": om, "visibility": out["visibility"], "depth": out["depth"]}  # the tapped colour is the history
    hit = outs[-1]["visibility"]["instance_primitive_index"] != wire.MISS
    assert np.isfinite(got).all() and hit.mean() > 0.5
    # (it does denoise: the filtered frame is smoother than the accumulated one where it sees a surface)
    rough = lambda img: np.abs(np.diff(img[..., :3].astype(np.float64), axis=1))[hit[:, 1:] & hit[:, :-1]].mean()
    assert rough(got) < rough(oc)


@pytest.mark.gpu
def test_gpu_refusals_name_the_field(gpu_ctx):
    from stratum_amd.post import denoise_desc

    p = synthetic(16, 12, seed=2)

    def refused(field, **change):
        keep = []
        d, _, _, _ = denoise_desc(p["views"], p["visibility"], p["depth"], p["accum_color"].copy(), p["accum_moments"], 1, "Box3", 0, 4.0, 0.0, 3.0, p["instance_index_map"], None, keep)
        for k, v in change.items():
            if k.startswith("gFilterImages"):
                d.gFilterImages[int(k[-2])] = v
            else:
                setattr(d, k, v)
        rc = _lib.lib().sthip_denoise_filter(gpu_ctx._h, C.byref(d))
        msg = _lib.lib().sthip_last_error(gpu_ctx._h).decode()
        assert rc == -1, (field, rc)  # STHIP_ERR_INVALID_ARGUMENT
        assert "sthip_denoise_filter" in msg and field in msg, msg

    for name in ("gViews", "gVisibility", "gDepth", "gAccumColor", "gAccumMoments"):
        refused(name, **{name: None})
    refused("gFilterImages[0]", **{"gFilterImages[0]": None})
    refused("gFilterImages[1]", **{"gFilterImages[1]": None})
    refused("iterations", iterations=0)
    refused("iterations", iterations=9)
    refused("filter_type", filter_type=6)
    refused("width", width=0)
    refused("height", height=0)
    refused("width x height", width=1 << 16, height=1 << 15)
    refused("view_count", view_count=0)


# ---- the C++ host: a Denoiser component beside BDPT (tests/cpp/denoise_host.cpp) ----
def _compile_host(src_name, exe):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", src_name), "-L" + os.path.join(ROOT, "stratum_amd"),
                           "-lstratum_hip", "-Wl,-rpath," + os.path.join(ROOT, "stratum_amd")])
    return exe


@pytest.fixture(scope="module")
def cpp_hosts(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("denoise_host")
    return _compile_host("denoise_host.cpp", str(d / "denoise_host")), _compile_host("host_test.cpp", str(d / "host_test"))


def _cornell_description(tmp_path, w=96, h=64):
    from stratum_amd import camera, scenes
    from stratum_amd.scene import dump_description

    sc, cam = scenes.cornell_box()
    fr = camera.Frame(w, h, cam["fovy"], cam["eye"], cam["target"])
    desc = str(tmp_path / "scene.bin")
    dump_description(desc, sc, fr)
    return sc, fr, desc


@pytest.mark.gpu
def test_gpu_cpp_host_with_a_denoiser_equals_the_python_host(cpp_hosts, tmp_path):
    from stratum_amd.bdpt import BDPT
    from stratum_amd.post import Denoiser, Tonemapper

    w, h = 96, 64
    sc, fr, desc = _cornell_description(tmp_path, w, h)
    outp = str(tmp_path / "out.bin")
    run = subprocess.run([cpp_hosts[0], desc, outp, "3", str(wire.TONEMAP["ACES"]), "0.75", "1", "3", str(wire.FILTER["Atrous"]), "1", "8", "4"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("DENOISE HOST OK") and "denoised 1" in run.stdout, run.stdout + run.stderr
    got = np.fromfile(outp, np.float32).reshape(h, w, 4)
    r = BDPT(device=0)
    try:
        r.update(sc)
        r.set_option("reuse_grids_persist", 1)  # (as the C++ host: one frame per call)
        dn = Denoiser(r, history_limit=8, iterations=3, filter_type="Atrous", history_tap=1, variance_boost_length=4)
        tm = Tonemapper(r, "ACES", 0.75, True)
        for seed in range(3):
            out = r.render(fr, seed, 1)
            want = tm(dn(out, fr.views), out["albedo"], modulate_albedo=True)
    finally:
        r.close()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d pixels differ" % (got.view(np.uint32) != want.view(np.uint32)).any(-1).sum()
    assert np.isfinite(got).all() and got[..., :3].max() > 0.05


@pytest.mark.gpu
def test_gpu_cpp_host_without_the_component_is_what_it_was(cpp_hosts, tmp_path):
    w, h = 96, 64
    _, _, desc = _cornell_description(tmp_path, w, h)
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    run = subprocess.run([cpp_hosts[0], desc, a, "1", str(wire.TONEMAP["ACES"]), "0.75", "0"], capture_output=True, text=True)
    assert run.returncode == 0 and "denoised 0" in run.stdout, run.stdout + run.stderr
    run = subprocess.run([cpp_hosts[1], "render", desc, b, "1", str(wire.TONEMAP["ACES"]), "0.75", str(tmp_path / "x.hdr")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("RENDER OK"), run.stdout + run.stderr
    raw = np.fromfile(b, dtype=np.uint8)
    assert np.array_equal(np.fromfile(a, dtype=np.uint8), raw[w * h * 24 + 16 :])  # (host_test writes radiance, visibility, ray counts, then the tone-mapped image)
