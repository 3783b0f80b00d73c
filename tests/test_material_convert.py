"""Material conversion on the device (include/sthip.h: sthip_convert_material; csrc/material_convert.hip): glTF PBR and
diffuse/specular textures to the three Disney material images, the alpha mask and its minimum, and the two roughness kernels
(kernels/material_convert.hlsl).

The reference is the numpy float32 statement of the header's contract below (np_material / np_roughness). It is pinned, bit
for bit, by tests/cpp/material_convert_ref.cpp, a scalar C++ restatement written from the shader; the library must equal it
bit for bit (NaN positions included; payload and sign of a NaN are not part of the contract). oracle/ is not involved.
"""
import ctypes as C
import functools
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stratum_amd import camera, scenes, wire  # noqa: E402
from stratum_amd.scene import ImageValue, SceneBuilder, translate  # noqa: E402

F32 = np.float32
GLTF, DS, A2R, S2R = 0, 1, 2, 3
KIND_NAMES = {GLTF: "GltfPbr", DS: "DiffuseSpecular", A2R: "AlphaToRoughness", S2R: "ShininessToRoughness"}
EXTENTS = [(1, 1), (3, 5), (31, 33), (256, 256)]  # (H, W): 1 texel; 15: only a tail group; 1023: several waves and a 3-texel tail; many blocks


# ---------------------------------------------------------------------------------------------------------------------------
# the contract in numpy float32 (numpy's float32 + - * / and sqrt are the IEEE operations, one rounding each)
# ---------------------------------------------------------------------------------------------------------------------------
def decode(b):
    return np.asarray(b, np.uint8).astype(F32) / F32(255)


def as_float(a):
    return decode(a) if a.dtype == np.uint8 else np.asarray(a, F32)


def saturate(a):
    a = np.asarray(a, F32)
    return np.where(a > 0, np.where(a < 1, a, F32(1)), F32(0)).astype(F32)


def luminance(c):
    return (c[..., 0] * F32(0.2126) + c[..., 1] * F32(0.7152)) + c[..., 2] * F32(0.0722)


def quantise(v):
    return (saturate(v) * F32(255) + F32(0.5)).astype(np.uint32).astype(np.uint8)


def min_alpha_of(a):
    a = np.asarray(a, F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        below = a < 1
    if not below.any():
        return 0xFFFFFFFF
    return int((saturate(a[below]) * F32(4294967296.0)).astype(np.uint64).min())


def np_material(kind, diffuse=None, specular=None, transmittance=None, roughness=None, out8=True):
    """from_gltf_pbr / from_diffuse_specular over (H, W, 4) sources ((H, W) for roughness), uint8 or float32, None = absent."""
    first = next(a for a in (diffuse, specular, transmittance, roughness) if a is not None)
    H, W = first.shape[:2]
    one, zero = np.ones((H, W), F32), np.zeros((H, W), F32)
    d, s, t = (as_float(a) if a is not None else None for a in (diffuse, specular, transmittance))
    data = [np.ones((H, W, 4), F32) for _ in range(3)]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind == GLTF:
            base = d[..., :3] if d is not None else np.ones((H, W, 3), F32)
            data[0][..., :3] = base
            data[1][..., 0] = s[..., 2] if s is not None else one
            data[1][..., 1] = s[..., 1] if s is not None else one
            l = luminance(base)
            data[2][..., 2] = saturate(luminance(t[..., :3]) / np.where(l > 0, l, F32(1))) if t is not None else zero
        else:
            d3 = d[..., :3] if d is not None else np.zeros((H, W, 3), F32)
            s3 = s[..., :3] if s is not None else np.zeros((H, W, 3), F32)
            t3 = t[..., :3] if t is not None else np.zeros((H, W, 3), F32)
            ld, ls, lt = luminance(d3), luminance(s3), luminance(t3)
            den = (ls + ld) + lt
            data[0][..., :3] = ((d3 * ld[..., None] + s3 * ls[..., None]) + t3 * lt[..., None]) / den[..., None]
            if s is not None:
                data[1][..., 0] = saturate(ls / den)
            if roughness is not None:
                data[1][..., 1] = as_float(roughness)
            if t is not None:
                data[2][..., 2] = saturate(lt / den)
    out = [quantise(x) for x in data] if out8 else data
    mask = None
    if d is not None:
        mask = quantise(d[..., 3]) if out8 else d[..., 3].copy()
    return {"output": out, "alpha_mask": mask, "min_alpha": min_alpha_of(d[..., 3]) if d is not None else 0xFFFFFFFF}


def np_roughness(kind, x, out8=True):
    x = as_float(x)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        v = saturate(np.sqrt(x)) if kind == A2R else saturate(np.sqrt(F32(2) / (x + F32(2))))
    return quantise(v) if out8 else v


def same(got, want):
    """Bit equality; for floats NaN stands against NaN whatever its payload."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == F32:
        gn, wn = np.isnan(got), np.isnan(want)
        return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))
    return bool(np.array_equal(got, want))


def assert_material(got, want, what):
    for k in range(3):
        assert same(got["output"][k], want["output"][k]), (what, "gOutput[%d]" % k)
    assert (got["alpha_mask"] is None) == (want["alpha_mask"] is None), what
    if want["alpha_mask"] is not None:
        assert same(got["alpha_mask"], want["alpha_mask"]), (what, "gOutputAlphaMask")
    assert got["min_alpha"] == want["min_alpha"], (what, "gOutputMinAlpha", hex(got["min_alpha"]), hex(want["min_alpha"]))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: seeded random bytes plus planted texels
# ---------------------------------------------------------------------------------------------------------------------------
ALPHAS = ["random", "last", "first", "all255"]


@functools.lru_cache(maxsize=None)
def material_inputs(h, w, src8, alpha="random", seed=0):
    """diffuse, specular, transmittance (h, w, 4) and roughness (h, w). Planted, where the extent has the texel: 5: the rgb of all
    three sources 0 (0 / 0); 6: base luminance 0 with transmittance present (the l > 0 ? l : 1 branch); 7: transmittance
    brighter than the base (saturates to 1). alpha: "last" / "first": 255 everywhere but 17 in that texel; "all255". Float form:
    the decoded bytes, with alpha NaN, -0.5, 1.5, +inf in texels 1..4 and a negative and a > 1 colour in texels 8, 9."""
    rng = np.random.RandomState(1000 * seed + 7 * h + w)
    n = h * w
    d, s, t = (rng.randint(0, 256, size=(n, 4)).astype(np.uint8) for _ in range(3))
    r = rng.randint(0, 256, size=n).astype(np.uint8)
    for a in (d, s, t):
        pick = rng.rand(n, 4)
        a[pick < 0.05] = 0
        a[pick > 0.95] = 255
    if n > 5:
        d[5, :3] = s[5, :3] = t[5, :3] = 0
    if n > 6:
        d[6, :3] = 0
        t[6, :3] = (9, 200, 31)
    if n > 7:
        d[7, :3] = (3, 2, 1)
        t[7, :3] = 255
    if alpha in ("last", "first"):
        d[:, 3] = 255
        d[n - 1 if alpha == "last" else 0, 3] = 17
    elif alpha == "all255":
        d[:, 3] = 255
    if not src8:
        d, s, t, r = decode(d), decode(s), decode(t), decode(r)
        if alpha == "random":
            for i, v in ((1, np.nan), (2, -0.5), (3, 1.5), (4, np.inf)):
                if n > i:
                    d[i, 3] = v
            if n > 9:
                d[8, 0], s[8, 1], t[8, 2] = -0.25, -3.0, -1.0
                d[9, 1], s[9, 2], t[9, 0], r[9] = 7.5, 2.0, 1e30, 1.75
    out = tuple(np.ascontiguousarray(a.reshape(h, w, 4)) for a in (d, s, t)) + (np.ascontiguousarray(r.reshape(h, w)),)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def roughness_input(h, w, src8, seed=0):
    """One channel. Planted: texel 0 = 0 (shininess 0; alpha 0), and in the float form 1e30 (shininess), a negative value (the
    square root is a NaN, which saturates to 0), -2 (2 / 0), 4 (saturates to 1 as an alpha) and a NaN in texels 1..5."""
    rng = np.random.RandomState(2000 * seed + 7 * h + w)
    x = rng.randint(0, 256, size=h * w).astype(np.uint8)
    x[0] = 0
    if not src8:
        x = decode(x) * F32(40.0)
        for i, v in ((1, 1e30), (2, -0.25), (3, -2.0), (4, 4.0), (5, np.nan)):
            if x.size > i:
                x[i] = v
    x = np.ascontiguousarray(x.reshape(h, w))
    x.setflags(write=False)
    return x


def subsets(kind):
    names = ["diffuse", "specular", "transmittance"] + (["roughness"] if kind == DS else [])
    return [c for k in range(1, len(names) + 1) for c in itertools.combinations(names, k)]


def pick(inputs, names):
    return {n: a for n, a in zip(("diffuse", "specular", "transmittance", "roughness"), inputs) if n in names}


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the numpy statement against the C++ restatement of the shader
# ---------------------------------------------------------------------------------------------------------------------------
REF_SRC = os.path.join(ROOT, "tests", "cpp", "material_convert_ref.cpp")


@pytest.fixture(scope="session")
def ref_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("material_convert_ref") / "material_convert_ref")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", exe, REF_SRC])
    return exe


def run_ref(exe, tmp_path, kind, sources, out8, env=None):
    """sources: the dict np_material takes (or {"input": x}); all of one format, as the program expects."""
    arrays = [sources[n] for n in ("diffuse", "specular", "transmittance", "roughness", "input") if sources.get(n) is not None]
    src8 = arrays[0].dtype == np.uint8
    assert all((a.dtype == np.uint8) == src8 for a in arrays)
    h, w = arrays[0].shape[:2]
    use = sum(bit for bit, n in ((1, "diffuse"), (2, "specular"), (4, "transmittance"), (8, "roughness")) if sources.get(n) is not None)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([kind, h * w, use, int(src8), int(out8)], np.uint32).tobytes())
        for a in arrays:
            f.write(a.tobytes())
    subprocess.check_call([exe, fin, fout], env=env)
    raw = np.fromfile(fout, np.uint8)
    dt, size = (np.uint8, 1) if out8 else (F32, 4)
    n = h * w
    if kind >= 2:
        assert raw.size == n * size
        return raw.view(dt).reshape(h, w)
    has_mask = sources.get("diffuse") is not None
    assert raw.size == 3 * n * 4 * size + (n * size if has_mask else 0) + 4
    out = [raw[k * n * 4 * size : (k + 1) * n * 4 * size].view(dt).reshape(h, w, 4) for k in range(3)]
    at = 3 * n * 4 * size
    mask = raw[at : at + n * size].view(dt).reshape(h, w) if has_mask else None
    return {"output": out, "alpha_mask": mask, "min_alpha": int(raw[-4:].view(np.uint32)[0])}


def cpu_cases():
    """Every case the CPU comparison runs: (kind, sources, out8, label)."""
    for kind in (GLTF, DS):
        for src8 in (True, False):
            for out8 in (True, False):
                for alpha in ALPHAS:
                    yield kind, pick(material_inputs(31, 33, src8, alpha), subsets(kind)[-1]), out8, "%s src8=%s out8=%s %s" % (KIND_NAMES[kind], src8, out8, alpha)
                for names in subsets(kind):
                    yield kind, pick(material_inputs(3, 5, src8), names), out8, "%s src8=%s out8=%s %s" % (KIND_NAMES[kind], src8, out8, "+".join(names))
                yield kind, pick(material_inputs(1, 1, src8), subsets(kind)[-1]), out8, "%s 1x1" % KIND_NAMES[kind]
    for kind in (A2R, S2R):
        for src8 in (True, False):
            for out8 in (True, False):
                yield kind, {"input": roughness_input(31, 33, src8)}, out8, "%s src8=%s out8=%s" % (KIND_NAMES[kind], src8, out8)


def test_numpy_statement_equals_the_cpp_restatement_of_the_shader(ref_exe, tmp_path):
    count = 0
    for kind, sources, out8, label in cpu_cases():
        got = run_ref(ref_exe, tmp_path, kind, sources, out8)
        if kind >= 2:
            assert same(np_roughness(kind, sources["input"], out8), got), label
        else:
            assert_material(np_material(kind, out8=out8, **sources), got, label)
        count += 1
    assert count == 2 * 2 * 2 * (4 + 1) + 4 * (7 + 15) + 8


def test_planted_texels_do_what_they_are_planted_for():
    d, s, t, r = material_inputs(31, 33, False)
    g = np_material(GLTF, d, s, t, out8=False)
    ds = np_material(DS, d, s, t, r, out8=False)
    flat = lambda a: a.reshape(-1, a.shape[-1]) if a.ndim == 3 else a.reshape(-1)
    assert np.isnan(flat(ds["output"][0])[5, :3]).all() and flat(ds["output"][1])[5, 0] == 0 and flat(ds["output"][2])[5, 2] == 0  # 0 / 0: NaN kept, saturate(NaN) = 0
    assert np.array_equal(flat(np_material(DS, d, s, t, r)["output"][0])[5], [0, 0, 0, 255])  # ... and a NaN quantises to 0
    assert flat(g["output"][2])[6, 2] == luminance(flat(t)[6, :3]) and 0 < flat(g["output"][2])[6, 2] < 1  # l = 0: divided by 1
    assert flat(g["output"][2])[7, 2] == 1
    mask = flat(g["alpha_mask"])
    assert np.isnan(mask[1]) and mask[2] == F32(-0.5) and mask[3] == F32(1.5) and np.isinf(mask[4])
    assert np.array_equal(flat(np_material(GLTF, d, s, t)["alpha_mask"])[1:5], [0, 0, 255, 255])
    # -0.5 saturates to 0: the minimum is 0, whatever the random bytes hold; NaN, 1.5 and inf take no part
    assert g["min_alpha"] == 0
    assert min_alpha_of(np.array([np.nan, 1.5, np.inf, 1.0], F32)) == 0xFFFFFFFF
    for alpha in ("last", "first"):
        dd = material_inputs(31, 33, True, alpha)[0]
        assert np_material(GLTF, dd)["min_alpha"] == int(F32(17) / F32(255) * F32(4294967296.0)) and (dd[..., 3] != 255).sum() == 1
    assert np_material(GLTF, material_inputs(31, 33, True, "all255")[0])["min_alpha"] == 0xFFFFFFFF
    x = roughness_input(31, 33, False)
    sh, al = np_roughness(S2R, x, False).reshape(-1), np_roughness(A2R, x, False).reshape(-1)
    assert sh[0] == 1 and 0 < sh[1] < 1e-14 and np_roughness(S2R, x).reshape(-1)[1] == 0 and al[2] == 0 and sh[3] == 1 and al[4] == 1 and al[5] == 0 and sh[5] == 0


def test_a_byte_that_passes_through_comes_out_as_it_went_in():
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(quantise(decode(b)), b)
    # ... so the 8-bit GLTF form copies base colour, metallic (b), roughness (g) and alpha
    d, s, t, _ = material_inputs(16, 16, True)
    r = np_material(GLTF, d, s, t)
    assert np.array_equal(r["output"][0][..., :3], d[..., :3]) and np.array_equal(r["alpha_mask"], d[..., 3])
    assert np.array_equal(r["output"][1][..., 0], s[..., 2]) and np.array_equal(r["output"][1][..., 1], s[..., 1])
    assert (r["output"][0][..., 3] == 255).all() and (r["output"][1][..., 2:] == 255).all() and (r["output"][2][..., [0, 1, 3]] == 255).all()


def test_min_alpha_of_every_byte_against_integers():
    for b in range(255):
        # a = RN(b / 255) as a binary32 number, exactly; scaled by 2^32 exactly; truncated
        a = F32(b) / F32(255)
        exact = int(a.astype(np.float64) * 2.0**32)  # (a has 24 significant bits: the product is an integer-valued double)
        assert float(a) * 2.0**32 == exact
        assert min_alpha_of(np.array([1.0, a, 1.0], F32)) == exact, b
        assert abs(exact - (b << 32) / 255) <= 2.0**32 * 2.0**-24  # within the rounding of the decode
    assert min_alpha_of(np.array([1.0], F32)) == 0xFFFFFFFF
    assert min_alpha_of(decode(np.array([254], np.uint8))) < 0xFFFFFFFF


def test_division_free_decode_of_the_kernels_is_the_division(tmp_path):
    """csrc/material_convert.h: decode_unorm8 replaces the IEEE division by a product and a fused correction; all 256 bytes."""
    exe = str(tmp_path / "decode_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "material_convert_decode_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "DECODE bad=0" in out.stdout, out.stdout


def test_ref_under_address_and_undefined_sanitizers(tmp_path):
    """The C++ restatement as a stand-alone program under -fsanitize=address,undefined, over the planted inputs."""
    exe = str(tmp_path / "material_convert_ref_san")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-o", exe, REF_SRC])
    for kind, src8 in itertools.product((GLTF, DS, A2R, S2R), (True, False)):
        sources = {"input": roughness_input(31, 33, src8)} if kind >= 2 else pick(material_inputs(31, 33, src8), subsets(kind)[-1])
        for out8 in (True, False):
            got = run_ref(exe, tmp_path, kind, sources, out8)
            if kind >= 2:
                assert same(np_roughness(kind, sources["input"], out8), got)
            else:
                assert_material(np_material(kind, out8=out8, **sources), got, (kind, src8, out8))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: header, loader, the mirrors' value-only materials
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_loader_and_wire_agree(built, tmp_path):
    from stratum_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sthip.h")).read(), flags=re.S)
    assert re.search(r"int\s+sthip_convert_material\s*\(\s*sthip_ctx\s*\*\s*\w+\s*,\s*const\s+sthip_convert_material_desc\s*\*\s*\w+\s*\)", text)
    assert "sthip_convert_material" in _lib.EXPORTS and hasattr(_lib.lib(), "sthip_convert_material")
    assert _lib.lib().sthip_abi_version() == 11 and "#define STHIP_ABI_VERSION 11" in text
    body = re.search(r"enum\s*\{\s*(STHIP_CONVERT_GLTF_PBR.*?)\}", text, flags=re.S).group(1)
    names = [n.split("=")[0].strip() for n in body.split(",") if n.strip()]
    assert names == ["STHIP_CONVERT_GLTF_PBR", "STHIP_CONVERT_DIFFUSE_SPECULAR", "STHIP_CONVERT_ALPHA_TO_ROUGHNESS", "STHIP_CONVERT_SHININESS_TO_ROUGHNESS", "STHIP_CONVERT_KIND_COUNT"]
    assert [wire.CONVERT[n] for n in ("GltfPbr", "DiffuseSpecular", "AlphaToRoughness", "ShininessToRoughness")] == [GLTF, DS, A2R, S2R]
    src = tmp_path / "size.c"
    fields = [f for f, _ in wire.ConvertMaterialDesc._fields_ if f != "pad_"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sthip.h"\nint main(void) { printf("%zu"' + ' " %zu"' * len(fields) + ', sizeof(sthip_convert_material_desc)'
                   + "".join(", offsetof(sthip_convert_material_desc, %s)" % f for f in fields) + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(wire.ConvertMaterialDesc)] + [getattr(wire.ConvertMaterialDesc, f).offset for f in fields]


def words(a):
    return np.asarray(a, F32).view(np.uint32).tolist()


def test_mirror_value_only_materials_need_no_context():
    b = SceneBuilder()
    lum = lambda c: (F32(c[0]) * F32(0.2126) + F32(c[1]) * F32(0.7152)) + F32(c[2]) * F32(0.0722)
    # glTF: Scene.cpp:165-174
    m = b.make_metallic_roughness_material((0.5, 0.25, 0.125), (0.0, 0.3, 0.7, 0.0), (0.1, 0.2, 0.3), 1.4)
    v = b._materials[m]["values"]["value"]
    assert words(v[0]) == words([0.5, 0.25, 0.125, 0.0])
    assert words(v[1]) == words([0.7, 0.3, 0.0, 0.0])
    assert words(v[2]) == words([0.0, 1.0, lum((0.1, 0.2, 0.3)), 1.4])
    assert (b._materials[m]["values"]["image_index"] == 0xFFFFFFFF).all() and b._materials[m]["alpha_mask_index"] == 0xFFFFFFFF
    assert b.min_alpha(m) is None and not b.alpha_test(m) and b._images == [] and b._images1 == []
    # diffuse / specular: Scene.cpp:213-225
    d, s, t = np.array([0.5, 0.25, 0.125], F32), np.array([0.1, 0.2, 0.05], F32), np.array([0.0, 0.3, 0.1], F32)
    m = b.make_diffuse_specular_material(d, s, 0.35, t, 1.3)
    ld, ls, lt = lum(d), lum(s), lum(t)
    den = (ld + ls) + lt
    v = b._materials[m]["values"]["value"]
    assert words(v[0]) == words(list(((d * ld + s * ls) + t * lt) / den) + [0.0])
    assert words(v[1]) == words([ls / den, 0.35, 0.0, 0.0])
    assert words(v[2]) == words([0.0, 1.0, lt / den, 1.3])
    # the emission branch of both: Scene.cpp:158-164,206-212
    e = np.array([2.0, 3.0, 4.0], F32)
    glow = np.full((2, 2, 4), 200, np.uint8)
    for m in (b.make_metallic_roughness_material((0.5, 0.5, 0.5), emission=ImageValue(e, glow)), b.make_diffuse_specular_material((0.5, 0.5, 0.5), (0.1, 0.1, 0.1), 0.2, emission=e)):
        v = b._materials[m]["values"]["value"]
        assert words(v[0]) == words(list(e / lum(e)) + [lum(e)]) and words(v[1]) == [0] * 4 and words(v[2]) == [0] * 4  # eta = 0
    assert len(b._images) == 1 and b._materials[m - 1]["values"]["image_index"][0] == 0 and b._materials[m]["values"]["image_index"][0] == 0xFFFFFFFF
    # the roughness values
    assert words(b.alpha_to_roughness(0.25).value) == words([0.5]) and b.alpha_to_roughness(0.25).image is None
    assert words(b.shininess_to_roughness(30.0).value) == words([np.sqrt(F32(2) / F32(32))])
    # an image without a context cannot be converted
    with pytest.raises(ValueError):
        b.make_metallic_roughness_material(ImageValue((1, 1, 1), glow))


def test_alpha_test_is_min_alpha_below_half():
    b = SceneBuilder()
    m = [b.add_material((1, 1, 1)) for _ in range(3)]
    b._min_alpha[m[0]], b._min_alpha[m[1]] = 0x7FFFFFFE, 0x7FFFFFFF
    assert b.alpha_test(m[0]) and not b.alpha_test(m[1]) and not b.alpha_test(m[2])  # Material.hpp:19: < 0xFFFFFFFF / 2; absent: false
    assert b.min_alpha(m[2]) is None


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: bit-equal to the numpy statement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0)
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def expected_material(kind, h, w, src8, out8, alpha, names):
    return np_material(kind, out8=out8, **pick(material_inputs(h, w, src8, alpha), names))


def device_material(ctx, kind, sources, out8, offset=0):
    """The device form through torch buffers: sources up, outputs pre-filled with 0xAB, min_alpha pre-filled with 0. offset: bytes
    every image starts beyond its allocation (4: an image that is not 16-byte aligned)."""
    import torch

    from stratum_amd import _lib

    first = next(iter(sources.values()))
    h, w = first.shape[:2]
    n = h * w

    def up(a):
        t = torch.empty(a.nbytes + offset, dtype=torch.uint8, device="cuda")
        t[offset:].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        return t

    def room(nbytes):
        return torch.full((nbytes + offset,), 0xAB, dtype=torch.uint8, device="cuda")

    d = wire.ConvertMaterialDesc()
    d.kind, d.width, d.height, d.device_ptrs, d.output_format = kind, w, h, 1, int(out8)
    keep = []
    for name, field, fmt in (("diffuse", "gDiffuse", "diffuse_format"), ("specular", "gSpecular", "specular_format"), ("transmittance", "gTransmittance", "transmittance_format"),
                             ("roughness", "gRoughness", "roughness_format"), ("input", "gInput", "input_format")):
        if sources.get(name) is not None:
            keep.append(up(sources[name]))
            setattr(d, field, keep[-1].data_ptr() + offset)
            setattr(d, fmt, int(sources[name].dtype == np.uint8))
    size = 1 if out8 else 4
    dt = np.uint8 if out8 else F32
    back = lambda t, shape: t[offset:].cpu().numpy().view(dt).reshape(shape)
    if kind >= 2:
        rw = room(n * size)
        d.gRoughnessRW = rw.data_ptr() + offset
        torch.cuda.synchronize()
        ctx._check(_lib.lib().sthip_convert_material(ctx._h, C.byref(d)), "sthip_convert_material")
        torch.cuda.synchronize()
        return {"roughness": back(rw, (h, w))}
    outs = [room(n * 4 * size) for _ in range(3)]
    for k in range(3):
        d.gOutput[k] = outs[k].data_ptr() + offset
    mask = room(n * size) if sources.get("diffuse") is not None else None
    if mask is not None:
        d.gOutputAlphaMask = mask.data_ptr() + offset
    min_alpha = torch.zeros(1, dtype=torch.int32, device="cuda")
    d.gOutputMinAlpha = min_alpha.data_ptr()
    torch.cuda.synchronize()
    ctx._check(_lib.lib().sthip_convert_material(ctx._h, C.byref(d)), "sthip_convert_material")
    torch.cuda.synchronize()
    return {"output": [back(t, (h, w, 4)) for t in outs], "alpha_mask": back(mask, (h, w)) if mask is not None else None, "min_alpha": int(min_alpha.cpu().numpy().view(np.uint32)[0])}


def run_material(ctx, form, kind, sources, out8):
    if form == "device":
        return device_material(ctx, kind, sources, out8)
    return ctx.convert_material(KIND_NAMES[kind], output_format=int(out8), **sources)  # (its gOutputMinAlpha is pre-filled with 0 too)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("out8", [True, False], ids=["out8", "outf"])
@pytest.mark.parametrize("src8", [True, False], ids=["src8", "srcf"])
@pytest.mark.parametrize("kind", [GLTF, DS], ids=["gltf", "diffspec"])
def test_gpu_material_kinds_equal_numpy(ctx, kind, src8, out8, form):
    """All sources present, at every extent; at 33 x 31 and 256 x 256 with the minimum alpha in the last texel, in the first, and
    nowhere (gOutputMinAlpha, pre-filled with 0 by the caller, comes back 0xFFFFFFFF and the mask is all 255 / 1.0)."""
    names = subsets(kind)[-1]
    for h, w in EXTENTS:
        for alpha in ALPHAS if h * w > 15 else ["random"]:
            got = run_material(ctx, form, kind, pick(material_inputs(h, w, src8, alpha), names), out8)
            assert_material(got, expected_material(kind, h, w, src8, out8, alpha, names), (h, w, alpha))
            if alpha == "all255":
                assert got["min_alpha"] == 0xFFFFFFFF and (got["alpha_mask"] == (255 if out8 else 1)).all()
            if alpha in ("last", "first"):
                assert got["min_alpha"] == int(F32(17) / F32(255) * F32(4294967296.0))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("out8", [True, False], ids=["out8", "outf"])
@pytest.mark.parametrize("src8", [True, False], ids=["src8", "srcf"])
@pytest.mark.parametrize("kind", [A2R, S2R], ids=["alpha", "shininess"])
def test_gpu_roughness_kinds_equal_numpy(ctx, kind, src8, out8, form):
    for h, w in EXTENTS:
        x = roughness_input(h, w, src8)
        if form == "device":
            got = device_material(ctx, kind, {"input": x}, out8)["roughness"]
        else:
            got = ctx.convert_material(KIND_NAMES[kind], input=x, output_format=int(out8))["roughness"]
        assert same(got, np_roughness(kind, x, out8)), (h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("formats", ["bytes", "floats"])
@pytest.mark.parametrize("kind", [GLTF, DS], ids=["gltf", "diffspec"])
def test_gpu_every_subset_of_sources(ctx, kind, formats, form):
    """The 7 and 15 subsets of present sources at 33 x 31: an absent source is upstream's gUseX = false."""
    src8 = out8 = formats == "bytes"
    assert len(subsets(kind)) == (7 if kind == GLTF else 15)
    for names in subsets(kind):
        got = run_material(ctx, form, kind, pick(material_inputs(31, 33, src8), names), out8)
        assert_material(got, expected_material(kind, 31, 33, src8, out8, "random", names), names)
        assert (got["alpha_mask"] is None) == ("diffuse" not in names)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [GLTF, DS], ids=["gltf", "diffspec"])
def test_gpu_mixed_source_formats_and_unaligned_images(ctx, kind):
    """A format byte per source: bytes and floats side by side give what each gives alone; device images aligned to 4 bytes
    only (not 16) take the one-texel path of the 8-bit kernel and give the same bytes."""
    b = material_inputs(31, 33, True)
    fb = tuple(decode(a) for a in b)
    names = subsets(kind)[-1]
    for mix in ((b[0], fb[1], b[2], fb[3]), (fb[0], b[1], fb[2], b[3])):
        for out8 in (True, False):
            for form in ("host", "device"):
                got = run_material(ctx, form, kind, pick(mix, names), out8)
                assert_material(got, np_material(kind, out8=out8, **pick(b, names)), ("mixed", out8, form))
    got = device_material(ctx, kind, pick(b, names), True, offset=4)
    assert_material(got, expected_material(kind, 31, 33, True, True, "random", names), "offset 4")


@pytest.mark.gpu
def test_gpu_a_second_call_with_a_smaller_extent(ctx):
    for kind in (GLTF, DS):
        names = subsets(kind)[-1]
        for h, w in ((256, 256), (3, 5)):
            got = ctx.convert_material(KIND_NAMES[kind], **pick(material_inputs(h, w, True), names))
            assert_material(got, expected_material(kind, h, w, True, True, "random", names), (h, w))
    for h, w in ((256, 256), (3, 5)):
        x = roughness_input(h, w, True)
        assert same(ctx.convert_material("ShininessToRoughness", input=x)["roughness"], np_roughness(S2R, x))


@pytest.mark.gpu
def test_gpu_refusals_name_the_field(ctx):
    from stratum_amd import _lib

    L = _lib.lib()
    d8, s8, t8, r8 = (np.array(a) for a in material_inputs(3, 5, True))
    out = [np.zeros((3, 5, 4), np.uint8) for _ in range(3)]
    mask, min_alpha, rough = np.zeros((3, 5), np.uint8), np.zeros(1, np.uint32), np.zeros((3, 5), np.uint8)

    def desc(kind):
        d = wire.ConvertMaterialDesc()
        d.kind, d.width, d.height, d.output_format = kind, 5, 3, 1
        d.diffuse_format = d.specular_format = d.transmittance_format = d.roughness_format = d.input_format = 1
        d.gDiffuse, d.gSpecular, d.gTransmittance, d.gRoughness, d.gInput = (a.ctypes.data for a in (d8, s8, t8, r8, r8))
        for k in range(3):
            d.gOutput[k] = out[k].ctypes.data
        d.gOutputAlphaMask, d.gOutputMinAlpha, d.gRoughnessRW = mask.ctypes.data, min_alpha.ctypes.data, rough.ctypes.data
        return d

    def refused(d, field):
        rc = L.sthip_convert_material(ctx._h, C.byref(d))
        msg = L.sthip_last_error(ctx._h).decode()
        assert rc == -1 and field in msg and "sthip_convert_material" in msg, (field, rc, msg)

    for kind in (GLTF, DS, A2R, S2R):
        assert L.sthip_convert_material(ctx._h, C.byref(desc(kind))) == 0, kind
    d = desc(4)
    refused(d, "kind")
    for kind in (GLTF, A2R):
        d = desc(kind)
        d.width = 0
        refused(d, "width")
        d = desc(kind)
        d.height = 0
        refused(d, "height")
        d = desc(kind)
        d.width, d.height = 1 << 15, (1 << 15) + 1  # more than 2^30 texels: refused before anything is touched
        refused(d, "width x height")
        d = desc(kind)
        d.output_format = 2
        refused(d, "output_format")
    for kind in (GLTF, DS):
        for field in ("diffuse_format", "specular_format", "transmittance_format") + (("roughness_format",) if kind == DS else ()):
            d = desc(kind)
            setattr(d, field, 2)
            refused(d, field)
        d = desc(kind)
        d.gDiffuse = d.gSpecular = d.gTransmittance = d.gRoughness = None
        refused(d, "no source")
        for k in range(3):
            d = desc(kind)
            d.gOutput[k] = None
            refused(d, "gOutput[%d]" % k)
        d = desc(kind)
        d.gOutputMinAlpha = None
        refused(d, "gOutputMinAlpha")
        d = desc(kind)
        d.gOutputAlphaMask = None
        refused(d, "gOutputAlphaMask")
        d.gDiffuse = None  # ... which is only needed with gDiffuse
        assert L.sthip_convert_material(ctx._h, C.byref(d)) == 0
    d = desc(GLTF)  # gRoughness is no source of the glTF kind
    d.gDiffuse = d.gSpecular = d.gTransmittance = None
    refused(d, "no source")
    for kind in (A2R, S2R):
        d = desc(kind)
        d.input_format = 3
        refused(d, "input_format")
        d = desc(kind)
        d.gInput = None
        refused(d, "gInput")
        d = desc(kind)
        d.gRoughnessRW = None
        refused(d, "gRoughnessRW")
    assert L.sthip_convert_material(ctx._h, None) == -1 and L.sthip_convert_material(None, C.byref(desc(GLTF))) == -1


@pytest.mark.gpu
def test_gpu_poisoned_allocations_give_the_same_bytes(built):
    """The host form once more in a fresh child process with STHIP_POISON_ALLOC (read once per process): the staged output
    buffers start as 0x7F bytes, so a texel the kernels do not write shows."""
    if os.environ.get("STHIP_MATERIAL_CONVERT_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_MATERIAL_CONVERT_POISON_CHILD="1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "(kinds_equal_numpy and host) or (every_subset and host)"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout


# ---------------------------------------------------------------------------------------------------------------------------
# GPU, end to end: a converted material renders what the numpy-converted images render
# ---------------------------------------------------------------------------------------------------------------------------
def quad_sources(opaque):
    """16 x 16 RGBA8 glTF sources for a card. The base colour's alpha is a checker of 0 and 255 (holes), or with `opaque` 255 and
    a few texels of 200 (min_alpha above a half: the material is opaque and loses its mask)."""
    rng = np.random.RandomState(77)
    base, mr, tr = (rng.randint(0, 256, size=(16, 16, 4)).astype(np.uint8) for _ in range(3))
    yy, xx = np.mgrid[0:16, 0:16]
    base[..., 3] = np.where(((yy // 4) + (xx // 4)) % 2 == 0, 255, 200 if opaque else 0)
    tr[..., :3] //= 4
    return base, mr, tr


def quad_scene(opaque, context):
    """A floor, a card with the glTF material over it and a light. context: a BDPT — the material comes from
    SceneBuilder.make_metallic_roughness_material; None — the numpy-converted arrays are attached by add_image /
    set_material_images / set_material_alpha_mask to a material with the same values."""
    base, mr, tr = quad_sources(opaque)
    values = dict(base_color=(0.9, 0.8, 0.7), metallic_roughness=(0.0, 0.6, 0.4, 0.0), transmission=(0.2, 0.2, 0.2), eta=1.45)
    b = SceneBuilder("converted card")
    floor = b.add_material((0.6, 0.6, 0.6), roughness=0.5)
    if context is not None:
        card = b.make_metallic_roughness_material(ImageValue(values["base_color"], base), ImageValue(values["metallic_roughness"], mr), ImageValue(values["transmission"], tr), values["eta"],
                                                  context=context)
        assert b.alpha_test(card) == (not opaque)
    else:
        want = np_material(GLTF, base, mr, tr)
        lum = (F32(0.2) * F32(0.2126) + F32(0.2) * F32(0.7152)) + F32(0.2) * F32(0.0722)
        card = b.add_material(values["base_color"], emission=0.0, metallic=0.4, roughness=0.6, anisotropic=0.0, subsurface=0.0, clearcoat=0.0, clearcoat_gloss=1.0, transmission=lum, eta=1.45)
        b.set_material_images(card, *[b.add_image(im) for im in want["output"]])
        assert (want["min_alpha"] < 0xFFFFFFFF // 2) == (not opaque)
        if not opaque:
            b.set_material_alpha_mask(card, b.add_image1(want["alpha_mask"]))
    light = b.add_emitter((17.0, 12.0, 4.0))

    def quad(p0, p1, p2, p3, n, mat, transform=None):
        pos, nrm, uv, tri = scenes._quad(p0, p1, p2, p3, n)
        b.add_instance(b.add_mesh(pos, nrm, uv, tri), mat, transform)

    quad((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1), (0, 1, 0), floor)
    quad((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (0, 0, 1), floor)
    quad((-0.6, 0, 0.6), (0.6, 0, 0.6), (0.6, 0, -0.6), (-0.6, 0, -0.6), (0, 1, 0), card, translate((0.0, -0.3, 0.0)))
    quad((-0.3, 0.9, -0.3), (0.3, 0.9, -0.3), (0.3, 0.9, 0.3), (-0.3, 0.9, 0.3), (0, -1, 0), light)
    return b.build(), {"eye": (0.0, 0.6, 3.5), "target": (0.0, -0.3, 0.0), "fovy": np.radians(40.0)}


def render_scene(sc, cam, flags):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0, args={"bdptFlag": list(flags)})
    try:
        r.update(sc)
        out = r.render(camera.Frame(64, 64, cam["fovy"], cam["eye"], cam["target"]), 0, 2)
        return {k: np.array(v, copy=True) for k, v in out.items() if isinstance(v, np.ndarray)}
    finally:
        r.close()


@pytest.mark.gpu
def test_gpu_a_converted_material_renders_the_frame_of_the_numpy_converted_images(ctx):
    frames = {}
    for opaque in (False, True):
        made, cam = quad_scene(opaque, ctx)
        attached, _ = quad_scene(opaque, None)
        assert made.materials.tobytes() == attached.materials.tobytes()
        assert len(made.images) == 3 and all(a.dtype == np.uint8 and np.array_equal(a, b) for a, b in zip(made.images, attached.images))
        assert len(made.images1) == len(attached.images1) == (0 if opaque else 1)  # opaque by min_alpha: the mask is dropped
        assert all(np.array_equal(a, b) for a, b in zip(made.images1, attached.images1))
        for alpha_test in (True, False):
            flags = ["alphatest" if alpha_test else "~alphatest"]
            a, b = render_scene(made, cam, flags), render_scene(attached, cam, flags)
            for k in ("radiance", "albedo", "visibility", "depth", "prev_uv", "ray_count"):
                assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (opaque, alpha_test, k)
            assert a["radiance"][..., :3].any()
            frames[opaque, alpha_test] = a["radiance"]
    # the comparison discriminates: the holes show only with the test on and only in the material that kept its mask
    assert not np.array_equal(frames[False, True], frames[False, False])
    assert np.array_equal(frames[True, True], frames[True, False])


# ---------------------------------------------------------------------------------------------------------------------------
# the C++ host (stratum_amd/host/stratum_hip.hpp: Scene::make_*_material, Scene::shininess_to_roughness)
# ---------------------------------------------------------------------------------------------------------------------------
MATERIAL_CONVERT_HOST = os.path.join(ROOT, "tests", "cpp", "material_convert_host")


@pytest.fixture(scope="module")
def material_convert_host(built):
    src = os.path.join(ROOT, "tests", "cpp", "material_convert_host.cpp")
    deps = [src, os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp"), os.path.join(ROOT, "include", "sthip.h")]
    if not os.path.exists(MATERIAL_CONVERT_HOST) or os.path.getmtime(MATERIAL_CONVERT_HOST) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", MATERIAL_CONVERT_HOST, src, "-L" + os.path.join(ROOT, "stratum_amd"), "-lstratum_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "stratum_amd")])
    return MATERIAL_CONVERT_HOST


def host_image(image, alpha_texel=None, alpha=0):
    """The bytes tests/cpp/material_convert_host.cpp fills its 9 x 7 sources with."""
    i = np.arange(63, dtype=np.uint64)[:, None]
    c = np.arange(4, dtype=np.uint64)[None, :]
    im = ((i * 37 + c * 101 + image * 59 + (i * i) % 251) & 0xFF).astype(np.uint8)
    if alpha_texel is not None:
        im[:, 3] = 255
        im[alpha_texel, 3] = alpha
    return np.ascontiguousarray(im.reshape(7, 9, 4))


def test_cpp_host_builds_and_prints_its_usage(material_convert_host):
    out = subprocess.run([material_convert_host], capture_output=True, text=True)
    assert out.returncode == 2 and "usage: material_convert_host" in out.stderr


@pytest.mark.gpu
def test_gpu_cpp_host_equals_the_python_mirror(ctx, material_convert_host, tmp_path):
    outp = str(tmp_path / "out.bin")
    run = subprocess.run([material_convert_host, outp], capture_output=True, text=True)
    assert run.returncode == 0 and "CONVERTED" in run.stdout, run.stdout + run.stderr
    raw = np.fromfile(outp, np.uint8)
    n, at = 63, 0

    def take(count):
        nonlocal at
        at += count
        return raw[at - count : at]

    transmission = ImageValue((0.1, 0.2, 0.3), host_image(2))
    shininess = (np.arange(63, dtype=np.uint32) * 11 + 7).astype(np.uint8).reshape(7, 9)
    b1, b2 = SceneBuilder(), SceneBuilder()
    m1 = b1.make_metallic_roughness_material(ImageValue((0.5, 0.25, 0.75), host_image(0, 5, 40)), ImageValue((0.0, 0.3, 0.7, 0.0), host_image(1)), transmission, 1.4, context=ctx)
    roughness = b2.shininess_to_roughness(ImageValue(30.0, shininess), context=ctx)
    m2 = b2.make_diffuse_specular_material(ImageValue((0.6, 0.5, 0.4), host_image(3, 3, 200)), ImageValue((0.2, 0.2, 0.2), host_image(4)), roughness, transmission, 1.5, context=ctx)
    for b, m, masked in ((b1, m1, True), (b2, m2, False)):
        record = take(72)
        assert record.tobytes() == b._materials[m].tobytes(), "the stored material record"
        assert int(take(4).view(np.uint32)[0]) == b.min_alpha(m) and int(take(4).view(np.uint32)[0]) == int(masked) and b.alpha_test(m) == masked
        for k in range(3):
            assert np.array_equal(take(n * 4), b._images[int(b._materials[m]["values"]["image_index"][k])].reshape(-1)), k
        if masked:
            assert np.array_equal(take(n), b._images1[0].reshape(-1))
        assert len(b._images1) == int(masked)
    assert take(4).tobytes() == roughness.value.tobytes() and np.array_equal(take(n), roughness.image.reshape(-1))
    assert at == raw.size
    assert b1.min_alpha(m1) == int(F32(40) / F32(255) * F32(4294967296.0))
