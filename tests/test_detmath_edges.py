"""The arithmetic contract (include/sthip_detmath.h) checked from outside it, at and beyond the edges of its domains.

Every GPU test compares a kernel with the CPU oracle, and both sides evaluate exp / log / pow from that one header: a wrong
value in it is wrong on both sides and no parity test sees it. These tests need no GPU. They pin
  * the in-domain bits of exp and log against a float32 numpy restatement of the published Cephes algorithm;
  * the in-domain accuracy against float64;
  * what exp and pow return outside the domain (never negative, never garbage: 0 below, +inf above, NaN for NaN);
  * the call sites that leave the domain: the tonemap gain over the whole exposure range, a frame through dense chromatic
    fog (delta tracking evaluates exp(-majorant_k t) for all three channels from a distance drawn for one of them), and the
    environment sample test image (1024 pow(cos, 1024)).
The delta-tracking segment itself is in tests/test_independent_f64.py."""
import os

import numpy as np

from oracle import oracle_py as orc
from stratum_amd import camera, scenes, wire

F = np.float32
TINY = 2.0**-126  # the smallest positive normal float
FLT_MAX = float(np.finfo(np.float32).max)
STRIDE = 499  # of the strided sweeps over binary32 bit patterns (a prime: every mantissa residue comes up)


def bits(x):
    return int(np.array([x], F).view(np.uint32)[0])


def floats_between(lo, hi, stride=STRIDE):
    """Every stride-th binary32 value from lo to hi (same sign, |lo| <= |hi|), both ends included."""
    a, b = bits(lo), bits(hi)
    assert a <= b
    return np.concatenate([np.arange(a, b, stride, dtype=np.uint64), [b]]).astype(np.uint32).view(F)


def np_expf(x):
    """Cephes expf (Moshier, single precision): n = round(x log2 e), x - n ln 2 with ln 2 split in two constants, a degree-5
    polynomial for e^r - 1 - r, scaled by 2^n through the exponent field. Every operation rounds to float32; none is fused."""
    x = np.asarray(x, F)
    n = np.floor(F(1.44269504088896341) * x + F(0.5))
    r = x - n * F(0.693359375)
    r = r - n * F(-2.12194440e-4)
    z = r * r
    p = F(1.9875691500e-4)
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = p * r + F(c)
    p = p * z + r + F(1.0)
    scale = ((n.astype(np.int64) + 127) << 23).astype(np.uint32).view(F)
    return p * scale


def np_logf(x):
    """Cephes logf: x = m 2^e with m in [sqrt(1/2), sqrt(2)), a degree-8 polynomial in m - 1, e ln 2 added in two parts."""
    u = np.asarray(x, F).view(np.uint32)
    e = ((u >> 23) & 0xFF).astype(np.int64) - 126
    m = ((u & np.uint32(0x007FFFFF)) | np.uint32(0x3F000000)).view(F)
    small = m < F(0.707106781186547524)
    e = np.where(small, e - 1, e)
    m = np.where(small, m + m - F(1.0), m - F(1.0)).astype(F)
    z = m * m
    y = F(7.0376836292e-2)
    for c in (-1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1, 2.0000714765e-1, -2.4999993993e-1, 3.3333331174e-1):
        y = y * m + F(c)
    y = y * m * z
    fe = e.astype(F)
    y = y + F(-2.12194440e-4) * fe
    y = y + F(-0.5) * z
    r = m + y
    return r + F(0.693359375) * fe


def exp_domain():
    return np.concatenate([floats_between(0.0, 88.0), floats_between(-0.0, -87.3)])


def positive_normals():
    return floats_between(TINY, FLT_MAX)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32))


# ---------------------------------------------------------------------------------------------
# inside the domains
# ---------------------------------------------------------------------------------------------
def test_exp_and_log_are_the_published_algorithm_bit_for_bit():
    """What every frame and golden fixture depends on: exp on [-87.3, 88.0] and log of the positive normals are the plain
    Cephes evaluation in float32, to the bit. Making exp total outside that range must not move any of these."""
    x = exp_domain()
    assert x.size > 4_000_000 and x.min() == F(-87.3) and x.max() == F(88.0)
    with np.errstate(all="ignore"):
        assert same_bits(orc.exp(x), np_expf(x))
    x = positive_normals()
    assert x.size > 4_000_000
    assert same_bits(orc.log(x), np_logf(x))


def test_accuracy_inside_the_domains_against_float64():
    """Each bound is 1.5 x the maximum measured for the header on the host over the full range (the sweeps here are strided,
    the true maximum may lie a little above what they find)."""
    x = exp_domain()
    err = np.abs(orc.exp(x) / np.exp(x.astype(np.float64)) - 1).max()
    print("exp: max relative error %.3g" % err)
    assert err < 1.5 * 7.9e-8  # measured 7.9e-8 (0.95 ulp)

    x = positive_normals()
    want = np.log(x.astype(np.float64))
    err = np.abs(orc.log(x) / want - 1)[np.abs(want) > 1e-2].max()
    print("log: max relative error %.3g" % err)
    assert err < 1.5 * 7.8e-8  # measured 7.8e-8

    # the sRGB curve of the tonemapper (post.h rgb_to_srgb1): pow(1.055 c, 1 / 2.4) - 0.055 above the linear toe
    c = floats_between(np.nextafter(F(0.0031308), F(1)), F(FLT_MAX / 1.055))
    got = orc.pow(c * F(1.055), np.full(c.size, 1 / 2.4, F)) - F(0.055)
    want = np.power(1.055 * c.astype(np.float64), 1 / 2.4) - 0.055
    err = np.abs(got / want - 1).max()
    print("srgb: max relative error %.3g" % err)
    assert err < 1.5 * 4.3e-6  # measured 4.3e-6

    # the spot of the environment sample test: 1024 pow(cos, 1024) where it is not yet negligible (every float of the range)
    x = floats_between(0.9187, 1.0, stride=1)
    got = (F(1024) * orc.pow(x, np.full(x.size, 1024, F))).astype(np.float64)
    want = 1024 * np.power(x.astype(np.float64), 1024)
    rel, absolute = np.abs(got / want - 1).max(), np.abs(got - want).max()
    print("spot: max relative error %.3g, absolute %.3g" % (rel, absolute))
    assert rel < 1.5 * 4.1e-6 and absolute < 1.5 * 5.1e-5  # measured 4.1e-6 and 5.1e-5


# ---------------------------------------------------------------------------------------------
# outside them
# ---------------------------------------------------------------------------------------------
def test_exp_outside_its_domain():
    """Below the domain the result is finite and not negative; where e^x is below the smallest normal float (x < -126 ln 2 =
    -87.3365) it is no larger than that float, and exactly +0 once e^x is below half the smallest denormal (x <= -104).
    (Between -87.3365 and -87.3 e^x is still a normal float, up to 1.219e-38 against 2^-126 = 1.1755e-38: there the result
    is held to the accuracy of the domain instead.) Above the domain the result is +inf, and in the last stretch where
    e^x is still finite ([88.0, 88.72]) it is the value or +inf. NaN stays NaN."""
    x = np.concatenate([floats_between(np.nextafter(F(-87.3), F(-100)), -FLT_MAX), F([-87.34, -87.5, -87.68, -87.7, -88, -88.03, -88.5, -95, -103.9, -104, -177, -300, -1e30, -np.inf])])
    got = orc.exp(x)
    assert np.isfinite(got).all() and not np.signbit(got).any()
    normal = x >= F(-126 * np.log(2.0))
    assert 5 < normal.sum() < 0.01 * x.size and np.abs(got[normal] / np.exp(x[normal].astype(np.float64)) - 1).max() < 1.5 * 7.9e-8
    assert (got[~normal] <= F(TINY)).all(), (x[~normal][got[~normal] > F(TINY)][:5], got[~normal][got[~normal] > F(TINY)][:5])
    assert not got[x <= -104].any()
    # no larger than e^x allows either (a denormal is the rounded value, to within one denormal step)
    assert (got.astype(np.float64) <= np.exp(x.astype(np.float64)) + 2.0**-149).all()

    x = floats_between(88.0, 88.72, stride=1)
    got = orc.exp(x)
    assert (got > 0).all()
    fin = np.isfinite(got)
    assert np.abs(got[fin] / np.exp(x[fin].astype(np.float64)) - 1).max() < 1.5 * 7.9e-8 and fin[0]
    assert np.isposinf(got[~fin]).all()
    x = np.concatenate([floats_between(np.nextafter(F(88.73), F(100)), FLT_MAX), F([88.74, 89, 100, 128, 1e30, np.inf])])
    assert np.isposinf(orc.exp(x)).all()

    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], np.uint32).view(F)
    assert np.isnan(orc.exp(nan)).all()


def test_pow_outside_its_domain():
    """pow(a, b) = exp(b log a) with b log a far below -87: a power of a base in [0, 1] lies in [0, 1], and 0 to a power of
    1 or more is +0 (det_logf(0) is about -88.03, a large negative number rather than -inf)."""
    a = np.concatenate([floats_between(0.0, 1.0), F([0.0, 1e-45, 1e-40, TINY, 0.5, 0.9, 0.9187, 0.99999994, 1.0])])
    for b in (1.5, 1024.0, 1e6):
        got = orc.pow(a, np.full(a.size, b, F))
        bad = ~((got >= 0) & (got <= 1))
        assert not bad.any(), (b, a[bad][:5], got[bad][:5])
    b = F([1.0, 1.0000001, 1.1, 1.18, 1.5, 2.0, 2.4, 5.0, 1024.0, 1e6, 3e38])
    got = orc.pow(np.zeros(b.size, F), b)
    assert not got.any() and not np.signbit(got).any(), got


def test_known_answers_outside_the_domains():
    """The inputs at which the unclamped (n + 127) << 23 of exp ran into the sign bit or out of the exponent field. Before
    exp was made total these gave -inf, -6.4e35, -1.56, +6.9e23 and -2.3e-34, and the three powers -1.6e30, 0.999998 and 0.998."""
    table = [  # x, lowest and highest result allowed
        (-88.5, 0.0, TINY),  # e^x = 3.7e-39
        (-95.0, 0.0, TINY),  # 5.5e-42
        (-177.0, 0.0, 0.0),
        (-300.0, 0.0, 0.0),
        (100.0, np.inf, np.inf),
    ]
    got = orc.exp(F([t[0] for t in table]))
    for (x, lo, hi), g in zip(table, got):
        assert lo <= g <= hi and not np.signbit(g), (x, g)
    got = orc.pow(F([0.9, 0.5, 0.0]), F([1024, 1024, 1024]))  # 1.4e-47, 2^-1024, 0: all below half the smallest denormal
    assert not got.any() and not np.signbit(got).any(), got
    # det_logf outside ITS domain is left as it is (every caller tolerates it); pinned so that a change shows:
    # zero and denormals read as 2^-127 times [1, 2) of their mantissa bits, the sign bit is ignored, inf and NaN as 2^128 times the same
    x = np.array([0x00000000, 0x00000001, 0x007FFFFF, 0x80000000, 0xBF800000, 0x7F800000, 0x7FC00000], np.uint32).view(F)
    got = orc.log(x)
    assert same_bits(got, np_logf(x))
    assert got.view(np.uint32).tolist() == [0xC2B00F34, 0xC2B00F34, 0xC2AEAC50, 0xC2B00F34, 0x00000000, 0x42B17218, 0x42B241B1], [hex(v) for v in got.view(np.uint32)]


# ---------------------------------------------------------------------------------------------
# the call sites that leave the domain
# ---------------------------------------------------------------------------------------------
EXPOSURES = (-200.0, -150.0, -127.0, -126.0, 0.0, 126.0, 127.0, 128.0, 200.0)


def test_tonemap_gain_over_the_whole_exposure_range():
    """sthip_tonemap scales by 2^exposure before the curve: Raw without gamma correction shows the gain itself."""
    img = np.ones((1, 2, 4), F)
    img[0, 1, :3] = 3.0
    for exposure in EXPOSURES:
        out, _ = orc.tonemap(img, None, wire.TONEMAP["Raw"], False, False, exposure)
        got = out[..., :3].astype(np.float64)
        assert not np.isnan(got).any() and (got >= 0).all() and not np.signbit(out[..., :3]).any(), (exposure, got)
        for px in range(2):
            value = float(img[0, px, 0])
            want = value * 2.0**exposure
            g = got[0, px]
            if want > FLT_MAX:
                assert np.isposinf(g).all(), (exposure, value, g)
            elif want >= TINY:
                assert np.allclose(g, want, rtol=2e-7, atol=0), (exposure, value, g, want)
            else:
                assert (g <= TINY * value).all(), (exposure, value, g)
    # between the integers the error does not grow with the exposure: the integer part is exact, the fraction f in
    # [-0.5, 0.5] goes through exp(f ln 2): exp's own bound (above), half an ulp of the product (below 0.35: 2^-26) and the
    # float ln 2 (1e-9); measured 1.0e-7. (exp(exposure ln 2) was 3.1e-6 off at 126.)
    rng = np.random.default_rng(5)
    one = np.ones((1, 1, 4), F)
    worst = 0.0
    for exposure in np.concatenate([rng.uniform(-126, 127.9, 1500), np.arange(-126, 128) + 0.5, np.arange(-126, 128) - 0.4999]).astype(F):
        out, _ = orc.tonemap(one, None, wire.TONEMAP["Raw"], False, False, float(exposure))
        worst = max(worst, abs(float(out[0, 0, 0]) / 2.0 ** float(exposure) - 1))
    print("2^exposure: max relative error %.3g" % worst)
    assert worst < 1.5 * 7.9e-8 + 2.0**-26 + 1e-9


def _fog_grid():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "fog_sphere.npz"))["grid"]


def test_frames_through_dense_and_chromatic_fog_have_no_negative_radiance():
    """One dense channel beside two thin ones: a free-flight distance drawn for a thin channel puts exp(-300 t) far below
    the range of exp. With the unclamped exp 1343 of the 3072 pixels of the first frame were negative (down to -7.1e36)."""
    for density in ((300.0, 1.0, 1.0), (1.0, 300.0, 40.0)):
        sc, cam = scenes.cornell_box(fog=_fog_grid(), density=density)
        fr = camera.Frame(64, 48, cam["fovy"], cam["eye"], cam["target"])
        out = orc.OracleScene(sc).render(fr, wire.default_push_constants(64, 48, sc.light_count), wire.DEFAULT_SAMPLING_FLAGS, 0, 16)
        rad = out["radiance"][..., :3]
        bad = ~(np.isfinite(rad) & (rad >= 0)).all(axis=-1)
        assert not bad.any(), (density, int(bad.sum()), float(np.nanmin(rad)))
        in_fog = (out["visibility"]["instance_primitive_index"] & 0xFFFF) == sc.instances.shape[0] - 1
        assert in_fog.sum() > 30 and rad[in_fog].mean() > 0, (density, int(in_fog.sum()))


def check_environment_sample_test_image(debug, start):
    """eEnvironmentSampleTest adds 1024 pow(max(0, cos), 1024) for each of eight environment samples to all three channels:
    at most 1024 per sample (pow of a cosine is at most 1; 1e-5 covers its rounding, measured 4.1e-6), never negative, and
    small spots (below 1 more than 6.7 degrees off the sample), so most pixels gain less than 1."""
    inc = debug[..., :3].astype(np.float64) - start[..., :3].astype(np.float64)
    assert np.isfinite(inc).all() and (inc >= 0).all() and (inc <= 8 * 1024 * (1 + 1e-5)).all(), (float(inc.min()), float(inc.max()))
    # the same eight numbers are added to each channel, onto different start values: each of the eight float32 additions
    # rounds to within half an ulp of a sum that is at most the final value, so two channels differ by at most 2 * 8 * 2^-24 of it
    tol = 16 * 2.0**-24 * debug[..., :3].max(axis=-1).astype(np.float64)
    assert (inc.max(axis=-1) - inc.min(axis=-1) <= tol).all()
    assert (inc.max(axis=-1) < 1).mean() >= 0.5


def test_environment_sample_test_image_on_the_oracle():
    start = np.random.RandomState(7).rand(96, 144, 4).astype(F)
    for image in (True, False):
        sc, cam = scenes.environment_scene(image=image, emitter=True)
        fr = camera.Frame(144, 96, cam["fovy"], cam["eye"], cam["target"])
        pc = wire.default_push_constants(144, 96, sc.light_count)
        pc.gEnvironmentMaterialAddress = sc.environment_address
        for flags in (wire.DEFAULT_SAMPLING_FLAGS, wire.DEFAULT_SAMPLING_FLAGS | wire.flag_mask("eSampleEnvironmentMapDirectly")):
            for begin in (start, None):  # from zeros the three channels are the same sums exactly
                out = orc.OracleScene(sc).render(fr, pc, flags, 0, 1, debug_mode=wire.DEBUG_ENVIRONMENT_SAMPLE_TEST, debug_image=begin)
                base = begin if begin is not None else np.zeros_like(start)
                check_environment_sample_test_image(out["debug"], base)
                assert out["debug"][..., :3].max() > 1  # some pixel looks at a sample
                if begin is None:
                    assert np.array_equal(out["debug"][..., 0], out["debug"][..., 1]) and np.array_equal(out["debug"][..., 0], out["debug"][..., 2])
