"""Source texel formats (include/sthip.h: sthip_texel_format, sthip_decode_texels; csrc/texel_decode.h, texel_decode.hip): sRGB,
one to four channels, 16-bit unorm, binary32 and BC1-BC5, decoded on the device on the way in, alone and as the sources of
sthip_convert_material.

The reference is the numpy float32 statement of the header's contract below (np_decode). It is pinned, bit for bit, by
tests/cpp/texel_decode_ref.cpp, a scalar C++ restatement written from the header; the library must equal it bit for bit. The one
thing numpy cannot state is det_powf: the sRGB curve of a value is taken from that program (its `srgb` mode), the divisions are
numpy's own. Any 64- or 128-bit word is a valid block, so the fixtures are made here from a seed. oracle/ is not involved.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stratum_amd import wire  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_material_convert as mc  # noqa: E402  (the numpy statement of the conversion, and its inputs)

F32 = np.float32
T = wire.TEXEL_FORMATS
LINEAR = [n for n, v in T.items() if 16 <= v < 32 or v < 2]
BLOCK = [n for n, v in T.items() if v >= 32]
FORMATS = LINEAR + BLOCK
EXTENTS = [(7, 5), (4, 4), (1, 1), (5, 67)]  # (H, W): partial blocks on both axes; one block; one texel; 335 texels: two workgroups, groups and singles, rows no multiple of 4
DESTINATIONS = [("rgba32f", 0, None), ("rgba8", 1, None), ("r32f", 0, 1), ("r8", 1, 2), ("r32f_a", 0, 3), ("r8_r", 1, 0)]  # (id, dst_format, channel)

REF_SRC = os.path.join(ROOT, "tests", "cpp", "texel_decode_ref.cpp")
CXX_FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall"]


@functools.lru_cache(maxsize=None)
def ref_program(sanitized=False):
    d = tempfile.mkdtemp(prefix="texel_decode_ref")
    exe = os.path.join(d, "texel_decode_ref_san" if sanitized else "texel_decode_ref")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall"] if sanitized else CXX_FLAGS
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-o", exe, REF_SRC])
    return exe


def run_program(exe, mode, payload):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(payload)
        subprocess.check_call([exe, mode, fin, fout])
        return np.fromfile(fout, F32)


_SRGB_KNOWN = {}


def srgb_curve(c):
    """The contract's sRGB curve of float32 values, through det_powf of the C++ program (each distinct value asked once)."""
    c = np.ascontiguousarray(c, F32)
    bits = c.view(np.uint32).reshape(-1)
    missing = np.array(sorted(set(np.unique(bits).tolist()) - set(_SRGB_KNOWN)), np.uint32)
    if missing.size:
        got = run_program(ref_program(), "srgb", missing.tobytes())
        _SRGB_KNOWN.update(zip(missing.tolist(), got.view(np.uint32).tolist()))
    return np.array([_SRGB_KNOWN[b] for b in bits.tolist()], np.uint32).view(F32).reshape(c.shape)


def ref_decode(name, data, w, h, exe=None):
    out = run_program(exe or ref_program(), "decode", np.array([T[name], w, h], np.uint32).tobytes() + np.ascontiguousarray(data).tobytes())
    return out.reshape(h, w, 4)


# ---------------------------------------------------------------------------------------------------------------------------
# the contract in numpy float32 (numpy's float32 division is the IEEE operation, one rounding)
# ---------------------------------------------------------------------------------------------------------------------------
def ratio(num, den):
    return np.asarray(num).astype(F32) / F32(den)


def np_colour_block(b, t, bc1):
    """b: (n, 8) bytes of each texel's colour block, t: (n,) the texel in it. Returns (n, 3)."""
    b = b.astype(np.uint32)
    c0, c1 = b[:, 0] | b[:, 1] << 8, b[:, 2] | b[:, 3] << 8
    bits = b[:, 4] | b[:, 5] << 8 | b[:, 6] << 16 | b[:, 7] << 24
    index = (bits >> (2 * t).astype(np.uint32)) & 3
    four = (c0 > c1) if bc1 else np.ones(len(b), bool)
    out = np.zeros((len(b), 3), F32)
    for k, (shift, mask, top) in enumerate(((11, 31, 31), (5, 63, 63), (0, 31, 31))):
        e0, e1 = (c0 >> shift) & mask, (c1 >> shift) & mask
        v4 = np.where(index == 2, ratio(2 * e0 + e1, 3 * top), ratio(e0 + 2 * e1, 3 * top))
        v3 = np.where(index == 2, ratio(e0 + e1, 2 * top), F32(0))
        out[:, k] = np.where(index == 0, ratio(e0, top), np.where(index == 1, ratio(e1, top), np.where(four, v4, v3)))
    return out


def np_rgtc_block(b, t):
    b = b.astype(np.uint64)
    r0, r1 = b[:, 0], b[:, 1]
    bits = np.zeros(len(b), np.uint64)
    for k in range(6):
        bits |= b[:, 2 + k] << np.uint64(8 * k)
    i = ((bits >> (3 * t).astype(np.uint64)) & np.uint64(7)).astype(np.int64)
    r0, r1 = r0.astype(np.int64), r1.astype(np.int64)
    eight = ratio((8 - i) * r0 + (i - 1) * r1, 1785)
    six = np.where(i < 6, ratio((6 - i) * r0 + (i - 1) * r1, 1275), np.where(i == 6, F32(0), F32(1)))
    return np.where(i == 0, ratio(r0, 255), np.where(i == 1, ratio(r1, 255), np.where(r0 > r1, eight, six))).astype(F32)


def np_decode(name, data, w, h):
    """(h, w, 4) float32: the decode of include/sthip.h. data: the image's bytes (uint8, flat)."""
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    block, channels, size, srgb = wire.texel_format_info(name)
    assert data.size == wire.texel_image_bytes(name, w, h)
    out = np.zeros((h * w, 4), F32)
    out[:, 3] = 1
    if not block:
        if size == 1:
            v = data.reshape(h * w, channels).astype(F32) / F32(255)
        elif size == 2:
            two = data.reshape(h * w, channels, 2).astype(np.uint32)
            v = (two[..., 0] | two[..., 1] << 8).astype(F32) / F32(65535)
        else:
            v = data.view(F32).reshape(h * w, channels)
        out[:, :channels] = v
    else:
        y, x = np.divmod(np.arange(h * w), w)
        b = data.reshape(-1, block)[(y // 4) * ((w + 3) // 4) + x // 4]
        t = 4 * (y % 4) + x % 4
        v = T[name]
        if v in (T["BC1_RGB"], T["BC1_RGB_SRGB"]):
            out[:, :3] = np_colour_block(b, t, True)
        elif v in (T["BC2"], T["BC2_SRGB"]):
            out[:, :3] = np_colour_block(b[:, 8:], t, False)
            out[:, 3] = ratio((b[np.arange(h * w), t // 2] >> (4 * (t % 2)).astype(np.uint8)) & 15, 15)
        elif v in (T["BC3"], T["BC3_SRGB"]):
            out[:, :3] = np_colour_block(b[:, 8:], t, False)
            out[:, 3] = np_rgtc_block(b[:, :8], t)
        elif v == T["BC4_UNORM"]:
            out[:, 0] = np_rgtc_block(b, t)
        else:
            out[:, 0], out[:, 1] = np_rgtc_block(b[:, :8], t), np_rgtc_block(b[:, 8:], t)
    if srgb:
        out[:, :3] = srgb_curve(out[:, :3])
    return out.reshape(h, w, 4)


def quantise(v):
    return mc.quantise(v)


def to_destination(rgba, dst_format, channel):
    v = rgba if channel is None else rgba[..., channel]
    return quantise(v) if dst_format else np.ascontiguousarray(v, F32)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def image_bytes(name, w, h, seed=0):
    """Seeded random bytes of the image's size (any word is a valid block); binary32 formats: finite values in [-0.5, 1.5]
    with a NaN and an infinity planted where there is room."""
    rng = np.random.RandomState(977 * seed + 31 * T[name] + 7 * h + w)
    n = wire.texel_image_bytes(name, w, h)
    if name.endswith("32F"):
        v = rng.uniform(-0.5, 1.5, n // 4).astype(F32)
        if v.size > 8:
            v[3], v[5] = np.nan, np.inf
        data = v.view(np.uint8)
    else:
        data = rng.randint(0, 256, n).astype(np.uint8)
    data = np.array(data)
    data.setflags(write=False)
    return data


def every_byte_image(name):
    """16 x 16: linear 8-bit formats hold every byte value in every channel; the others random bytes."""
    block, channels, size, _ = wire.texel_format_info(name)
    if not block and size == 1:
        data = np.repeat(np.arange(256, dtype=np.uint8), channels)
        for k in range(1, channels):
            data[k::channels] = np.roll(np.arange(256, dtype=np.uint8), 37 * k)  # (a permutation per channel: channels differ)
        return data
    return image_bytes(name, 16, 16, seed=3)


@functools.lru_cache(maxsize=None)
def expected(name, w, h, every=False):
    data = every_byte_image(name) if every else image_bytes(name, w, h)
    return data, np_decode(name, data, w, h)


def same(got, want):
    return mc.same(got, want)


def block_of(c0, c1, indices):
    """A colour block from two 16-bit endpoints and sixteen 2-bit indices."""
    bits = sum(int(i) << (2 * t) for t, i in enumerate(indices))
    return np.array([c0 & 255, c0 >> 8, c1 & 255, c1 >> 8] + [(bits >> (8 * k)) & 255 for k in range(4)], np.uint8)


def rgtc_of(r0, r1, indices):
    bits = sum(int(i) << (3 * t) for t, i in enumerate(indices))
    return np.array([r0, r1] + [(bits >> (8 * k)) & 255 for k in range(6)], np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_formats_named_here_are_all_the_header_builds():
    assert len(FORMATS) == 2 + 14 + 8 and sorted(T.values()) == [0, 1] + [v for v in range(16, 40) if v not in (19, 31)]


def test_numpy_statement_equals_the_cpp_restatement():
    count = 0
    for name in FORMATS:
        for h, w in EXTENTS + [(16, 16)]:
            data, want = expected(name, w, h, every=(h, w) == (16, 16))
            assert same(ref_decode(name, data, w, h), want), (name, h, w)
            count += 1
    assert count == 24 * 5


def test_planted_blocks_do_what_they_are_planted_for():
    idx = [0, 1, 2, 3] * 4
    r = lambda e: F32(e) / F32(31)
    g = lambda e: F32(e) / F32(63)
    hi, lo = (31 << 11) | (10 << 5) | 3, (2 << 11) | (50 << 5) | 30
    four = np_decode("BC1_RGB", block_of(hi, lo, idx), 4, 4)[0]
    assert np.array_equal(four[0], [r(31), g(10), r(3), 1]) and np.array_equal(four[1], [r(2), g(50), r(30), 1])
    assert np.array_equal(four[2], [F32(64) / F32(93), F32(70) / F32(189), F32(36) / F32(93), 1])
    assert np.array_equal(four[3], [F32(35) / F32(93), F32(110) / F32(189), F32(63) / F32(93), 1])
    three = np_decode("BC1_RGB", block_of(lo, hi, idx), 4, 4)[0]  # c0 < c1
    assert np.array_equal(three[2], [F32(33) / F32(62), F32(60) / F32(126), F32(33) / F32(62), 1]) and np.array_equal(three[3], [0, 0, 0, 1])
    equal = np_decode("BC1_RGB", block_of(hi, hi, idx), 4, 4)[0]  # c0 == c1: the three-colour rule too
    assert np.array_equal(equal[2], [F32(62) / F32(62), F32(20) / F32(126), F32(6) / F32(62), 1]) and np.array_equal(equal[3], [0, 0, 0, 1])
    # BC2 and BC3 always take the four-colour rule, whatever the endpoints' order
    for name, head in (("BC2", np.zeros(8, np.uint8)), ("BC3", rgtc_of(0, 0, [0] * 16))):
        v = np_decode(name, np.concatenate([head, block_of(lo, hi, idx)]), 4, 4)[0]
        assert np.array_equal(v[2, :3], [F32(35) / F32(93), F32(110) / F32(189), F32(63) / F32(93)]) and np.array_equal(v[3, :3], [F32(64) / F32(93), F32(70) / F32(189), F32(36) / F32(93)])
    # BC2 alpha: all 16 nibbles, texel t holds nibble t
    nibbles = np.array([(2 * k) | ((2 * k + 1) << 4) for k in range(8)], np.uint8)
    a = np_decode("BC2", np.concatenate([nibbles, block_of(hi, lo, idx)]), 4, 4)[..., 3].reshape(-1)
    assert np.array_equal(a, np.arange(16).astype(F32) / F32(15))
    # BC4: every index 0..7 in the three orders of the endpoints
    order = list(range(8)) * 2
    big = np_decode("BC4_UNORM", rgtc_of(200, 40, order), 4, 4)[..., 0].reshape(-1)[:8]
    assert np.array_equal(big, [F32(200) / F32(255), F32(40) / F32(255)] + [F32((8 - i) * 200 + (i - 1) * 40) / F32(1785) for i in range(2, 8)])
    small = np_decode("BC4_UNORM", rgtc_of(40, 200, order), 4, 4)[..., 0].reshape(-1)[:8]
    assert np.array_equal(small, [F32(40) / F32(255), F32(200) / F32(255)] + [F32((6 - i) * 40 + (i - 1) * 200) / F32(1275) for i in range(2, 6)] + [0, 1])
    equal = np_decode("BC4_UNORM", rgtc_of(77, 77, order), 4, 4)[..., 0].reshape(-1)[:8]
    assert np.array_equal(equal, [F32(77) / F32(255)] * 2 + [F32(5 * 77) / F32(1275)] * 4 + [0, 1])
    one = np_decode("BC4_UNORM", rgtc_of(200, 40, order), 4, 4)
    assert (one[..., 1:3] == 0).all() and (one[..., 3] == 1).all()
    # BC5: the halves are independent
    two = np_decode("BC5_UNORM", np.concatenate([rgtc_of(200, 40, order), rgtc_of(40, 200, order[::-1])]), 4, 4)
    assert np.array_equal(two[..., 0].reshape(-1)[:8], big) and np.array_equal(two[..., 1].reshape(-1)[:8], small[::-1]) and (two[..., 2] == 0).all() and (two[..., 3] == 1).all()
    # a partial block: texels beyond the extent change nothing that is read
    b = np.array(image_bytes("BC3", 4, 4))
    whole = np_decode("BC3", b, 4, 4)
    assert np.array_equal(np_decode("BC3", b, 3, 2), whole[:2, :3])
    # absent channels
    assert np.array_equal(np_decode("RG16_UNORM", np.array([0xFF, 0xFF, 0x01, 0x00], np.uint8), 1, 1)[0, 0], [1, F32(1) / F32(65535), 0, 1])
    # sRGB: colour only, alpha linear
    v = np_decode("RGBA8_SRGB", np.array([128, 128, 128, 128], np.uint8), 1, 1)[0, 0]
    assert v[3] == F32(128) / F32(255) and v[0] == v[1] == v[2] and 0.2158 < v[0] < 0.2159


SRGB_MEASURED_ERROR = 4.52e-7  # measured on the CPU, at byte 31 (det_powf = det_expf(2.4 * det_logf(x)): the error of the logarithm times 2.4 |ln x|); printed by the test above


def test_srgb_curve_of_every_byte_against_float64():
    b = np.arange(256)
    c = b.astype(F32) / F32(255)
    got = srgb_curve(c).astype(np.float64)
    x = b / 255.0
    exact = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
    rel = np.abs(got[1:] - exact[1:]) / exact[1:]
    print("sRGB curve, 256 bytes: largest relative error %.3e at byte %d" % (rel.max(), 1 + rel.argmax()))
    assert got[0] == 0 and got[255] == 1
    assert rel.max() < 1.5 * SRGB_MEASURED_ERROR  # (the margin tests/test_detmath_edges.py gives det_powf)
    assert (np.diff(got) > 0).all()  # monotonic
    # continuous across 0.04045: byte 10 is the last on the line, byte 11 the first on the power; the step between them is the
    # step of their neighbours, not a jump
    assert c[10] <= F32(0.04045) < c[11]
    assert got[10] - got[9] < got[11] - got[10] < got[12] - got[11] and (got[11] - got[10]) < 1.2 * (got[10] - got[9])



def test_unorm8_into_an_8bit_destination_is_the_identity():
    for name in ("R8_UNORM", "RG8_UNORM", "RGB8_UNORM", "RGBA8_UNORM"):
        data = every_byte_image(name)
        channels = wire.texel_format_info(name)[1]
        got = quantise(np_decode(name, data, 16, 16))
        assert np.array_equal(got[..., :channels].reshape(-1), data), name
        for k in range(channels):
            assert sorted(got[..., k].reshape(-1).tolist()) == list(range(256))
        assert (got[..., channels:3] == 0).all() and (channels == 4 or (got[..., 3] == 255).all())


def test_header_loader_and_wire_agree(built, tmp_path):
    from stratum_amd import _lib

    raw = open(os.path.join(ROOT, "include", "sthip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+sthip_decode_texels\s*\(\s*sthip_ctx\s*\*\s*\w+\s*,\s*const\s+sthip_decode_texels_desc\s*\*\s*\w+\s*\)", text)
    assert "sthip_decode_texels" in _lib.EXPORTS and hasattr(_lib.lib(), "sthip_decode_texels")
    assert _lib.lib().sthip_abi_version() == 11 and "#define STHIP_ABI_VERSION 11" in text
    body = re.search(r"enum\s+sthip_texel_format\s*\{(.*?)\}", text, flags=re.S).group(1)
    enum = {n.strip(): int(v) for n, v in (e.split("=") for e in body.split(",") if e.strip())}
    for name, value in list(wire.TEXEL_FORMATS.items()) + list(wire.TEXEL_UNSUPPORTED.items()):
        assert enum["STHIP_TEXEL_" + name] == value, name
    assert enum["STHIP_TEXEL_RGBA8_UNORM_"] == 19 and enum["STHIP_TEXEL_RGBA32F_"] == 31 and enum["STHIP_TEXEL_FIRST"] == 16 and enum["STHIP_TEXEL_END"] == 40
    assert all(v < 2 or v >= 16 for v in enum.values())  # 2 .. 15 stay no format ...
    assert "2 .. 15 stay no format" in raw  # ... in the header's wording
    src = tmp_path / "size.c"
    fields = [f for f, _ in wire.DecodeTexelsDesc._fields_ if f != "pad_"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sthip.h"\nint main(void) { printf("%zu %zu"' + ' " %zu"' * len(fields) + ', sizeof(sthip_convert_material_desc), sizeof(sthip_decode_texels_desc)'
                   + "".join(", offsetof(sthip_decode_texels_desc, %s)" % f for f in fields) + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(wire.ConvertMaterialDesc), C.sizeof(wire.DecodeTexelsDesc)] + [getattr(wire.DecodeTexelsDesc, f).offset for f in fields]


def test_ref_under_address_and_undefined_sanitizers():
    """The C++ restatement as a stand-alone program under -fsanitize=address,undefined, every format, partial blocks."""
    exe = ref_program(sanitized=True)
    for name in FORMATS:
        for h, w in ((7, 5), (1, 1)):
            data, want = expected(name, w, h)
            assert same(ref_decode(name, data, w, h, exe), want), (name, h, w)
    c = np.arange(256).astype(F32) / F32(255)
    assert np.array_equal(run_program(exe, "srgb", c.tobytes()), srgb_curve(c))


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_the_header_the_kernels_compile_equals_numpy_on_the_host(tmp_path, sanitized):
    """csrc/texel_decode.h as a stand-alone host program (tests/cpp/texel_decode_host_check.cpp), plain and under
    -fsanitize=address,undefined with the image in an allocation of exactly its size: every format, every extent."""
    exe = str(tmp_path / "texel_decode_host_check")
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall"] if sanitized else CXX_FLAGS
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "texel_decode_host_check.cpp")])
    for name in FORMATS:
        for h, w in EXTENTS + [(16, 16)]:
            data, want = expected(name, w, h, every=(h, w) == (16, 16))
            fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([T[name], w, h], np.uint32).tobytes() + data.tobytes())
            subprocess.check_call([exe, fin, fout])
            assert same(np.fromfile(fout, F32).reshape(h, w, 4), want), (name, h, w)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: bit-equal to the numpy statement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0)
    yield r
    r.close()


def device_decode(ctx, name, data, w, h, dst_format, channel, offset=0, dst_offset=0):
    """The device form through torch buffers; the destination is pre-filled with 0xAB. offset: bytes the source starts beyond
    its (256-byte aligned) allocation."""
    import torch

    from stratum_amd import _lib

    src = torch.empty(data.size + offset, dtype=torch.uint8, device="cuda")
    src[offset:].copy_(torch.from_numpy(np.array(data)))
    size = (1 if channel is not None else 4) * (1 if dst_format else 4)
    dst = torch.full((w * h * size + dst_offset,), 0xAB, dtype=torch.uint8, device="cuda")
    d = wire.DecodeTexelsDesc()
    d.src_format, d.width, d.height, d.device_ptrs, d.dst_format = T[name], w, h, 1, dst_format
    d.dst_channels, d.channel = (4, 0) if channel is None else (1, channel)
    d.src, d.dst = src.data_ptr() + offset, dst.data_ptr() + dst_offset
    torch.cuda.synchronize()
    ctx._check(_lib.lib().sthip_decode_texels(ctx._h, C.byref(d)), "sthip_decode_texels")
    torch.cuda.synchronize()
    return dst[dst_offset:].cpu().numpy().view(np.uint8 if dst_format else F32).reshape((h, w, 4) if channel is None else (h, w))


def run_decode(ctx, form, name, data, w, h, dst_format, channel):
    if form == "device":
        return device_decode(ctx, name, data, w, h, dst_format, channel)
    return ctx.decode_texels(wire.TexelImage(data, name, w, h), dst_format=dst_format, channel=channel)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("destination", DESTINATIONS, ids=[d[0] for d in DESTINATIONS])
def test_gpu_decode_texels_equals_numpy(ctx, destination, form):
    """Every format into this destination, at every extent and on the 16 x 16 image of every byte value."""
    _, dst_format, channel = destination
    for name in FORMATS:
        for h, w in EXTENTS + [(16, 16)]:
            data, want = expected(name, w, h, every=(h, w) == (16, 16))
            got = run_decode(ctx, form, name, data, w, h, dst_format, channel)
            assert same(got, to_destination(want, dst_format, channel)), (name, h, w)


@pytest.mark.gpu
def test_gpu_unorm8_into_8bit_gives_the_source_bytes(ctx):
    for name in ("R8_UNORM", "RG8_UNORM", "RGB8_UNORM", "RGBA8_UNORM"):
        data = every_byte_image(name)
        channels = wire.texel_format_info(name)[1]
        for form in ("host", "device"):
            got = run_decode(ctx, form, name, data, 16, 16, 1, None)
            assert np.array_equal(got[..., :channels].reshape(-1), data), (name, form)
            for k in range(channels):
                assert np.array_equal(run_decode(ctx, form, name, data, 16, 16, 1, k).reshape(-1), data[k::channels]), (name, form, k)


@pytest.mark.gpu
def test_gpu_sources_and_destinations_at_their_minimum_alignment(ctx):
    """A device source offset by its natural alignment only (1 byte for an 8-bit linear image: the four-texel path is declined;
    8 or 16 for blocks) and a destination offset by one texel give the same values."""
    for name in FORMATS:
        block, channels, size, _ = wire.texel_format_info(name)
        step = block or size
        data, want = expected(name, 67, 5)
        for dst_format, channel in ((1, None), (0, None), (1, 2), (0, 0)):
            texel = (1 if channel is not None else 4) * (1 if dst_format else 4)
            got = device_decode(ctx, name, data, 67, 5, dst_format, channel, offset=step, dst_offset=texel)
            assert same(got, to_destination(want, dst_format, channel)), (name, dst_format, channel)


@pytest.mark.gpu
def test_gpu_decode_refusals_name_the_field_and_write_nothing(ctx):
    import torch

    from stratum_amd import _lib

    L = _lib.lib()
    data = np.array(image_bytes("BC3", 8, 8))
    out = np.full((8, 8, 4), 0xAB, np.uint8)

    def desc():
        d = wire.DecodeTexelsDesc()
        d.src_format, d.width, d.height, d.device_ptrs, d.dst_format, d.dst_channels, d.channel = T["BC3"], 8, 8, 0, 1, 4, 0
        d.src, d.dst = data.ctypes.data, out.ctypes.data
        return d

    def refused(d, field, code=-1):
        rc = L.sthip_decode_texels(ctx._h, C.byref(d))
        msg = L.sthip_last_error(ctx._h).decode()
        assert rc == code and field in msg and "sthip_decode_texels" in msg, (field, rc, msg)
        assert (out == 0xAB).all()

    for field, value in (("width", 0), ("height", 0), ("dst_format", 2), ("dst_channels", 3), ("dst_channels", 0), ("src", None), ("dst", None)):
        d = desc()
        setattr(d, field, value)
        refused(d, field)
    d = desc()
    d.width, d.height = 1 << 15, (1 << 15) + 1
    refused(d, "width x height")
    for value in list(range(2, 16)) + [40, 47, 54, 55, 80, 255, 1 << 16]:
        d = desc()
        d.src_format = value
        refused(d, "src_format")
    for name, value in wire.TEXEL_UNSUPPORTED.items():
        d = desc()
        d.src_format = value
        refused(d, "src_format %d" % value, code=-4)
    d = desc()
    d.src_format = wire.TEXEL_UNSUPPORTED["BC7_UNORM"]
    refused(d, "BC7_UNORM", code=-4)
    d = desc()
    d.src_format = wire.TEXEL_UNSUPPORTED["R8_SNORM"]
    refused(d, "SNORM", code=-4)
    d = desc()
    d.dst_channels, d.channel = 1, 4
    refused(d, "channel")
    # device pointers that are not naturally aligned
    src = torch.zeros(data.size + 64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(8 * 8 * 16 + 64, dtype=torch.uint8, device="cuda")
    for name, src_off, dst_format, dst_off, field in (("BC3", 8, 1, 0, "src"), ("BC1_RGB", 4, 1, 0, "src"), ("RGB16_UNORM", 1, 1, 0, "src"), ("R32F", 2, 1, 0, "src"),
                                                     ("BC3", 0, 1, 2, "dst"), ("BC3", 0, 0, 8, "dst")):
        d = desc()
        d.src_format, d.device_ptrs, d.dst_format = T[name], 1, dst_format
        d.src, d.dst = src.data_ptr() + src_off, dst.data_ptr() + dst_off
        refused(d, field)
    assert int(dst.max().item()) == 0
    assert L.sthip_decode_texels(ctx._h, None) == -1 and L.sthip_decode_texels(None, C.byref(desc())) == -1
    assert L.sthip_decode_texels(ctx._h, C.byref(desc())) == 0 and not (out == 0xAB).all()


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the same formats as sources of sthip_convert_material
# ---------------------------------------------------------------------------------------------------------------------------
GLTF, DS, A2R, S2R = mc.GLTF, mc.DS, mc.A2R, mc.S2R
MIXES = {  # a format per source: diffuse, specular, transmittance, roughness
    "gltf_srgb": ("RGBA8_SRGB", "RGB8_UNORM", "RGBA8_UNORM", "R8_UNORM"),
    "blocks": ("BC3_SRGB", "BC1_RGB", "BC5_UNORM", "BC4_UNORM"),
    "wide": ("RGBA16_UNORM", "RGB32F", "BC2_SRGB", "RG16_UNORM"),
    "narrow": ("BC2", "RG8_SRGB", "RGB8_SRGB", "RGBA8_SRGB"),  # (a one-channel source in a four-channel format: channel 0)
}
SOURCE_NAMES = ("diffuse", "specular", "transmittance", "roughness")
ALPHA_FORMATS = ("RGBA8_SRGB", "RGBA8_UNORM", "RGBA16_UNORM", "BC2", "BC3", "BC2_SRGB", "BC3_SRGB")


def plant_alpha(name, data, w, h, alpha):
    """all255: every alpha 1; one_below: one texel just below 1; zero: one texel 0. Formats without alpha are left alone."""
    data = np.array(data)
    if name not in ALPHA_FORMATS or alpha == "random":
        return data
    n = w * h
    texel = min(5, n - 1)
    if name in ("RGBA8_SRGB", "RGBA8_UNORM"):
        data[3::4] = 255
        if alpha != "all255":
            data[4 * texel + 3] = 254 if alpha == "one_below" else 0
    elif name == "RGBA16_UNORM":
        data[6::8] = data[7::8] = 255
        if alpha != "all255":
            data[8 * texel + 6 : 8 * texel + 8] = (0xFE, 0xFF) if alpha == "one_below" else (0, 0)
    else:
        blocks = data.reshape(-1, 16)
        y, x = divmod(texel, w)
        b, t = (y // 4) * ((w + 3) // 4) + x // 4, 4 * (y % 4) + x % 4
        if name.startswith("BC2"):
            blocks[:, :8] = 255
            if alpha != "all255":
                blocks[b, t // 2] = (0xFF & ~(0xF << (4 * (t % 2)))) | ((14 if alpha == "one_below" else 0) << (4 * (t % 2)))
        else:
            blocks[:, :8] = rgtc_of(255, 254, [0] * 16)  # r0 > r1, every index 0: alpha 1
            if alpha != "all255":
                blocks[b, :8] = rgtc_of(255, 254 if alpha == "one_below" else 0, [int(k == t) for k in range(16)])
    return data


@functools.lru_cache(maxsize=None)
def convert_case(kind, mix, w, h, names, alpha):
    """(sources in their formats, numpy-decoded float sources)."""
    given, floats = {}, {}
    for name, fmt in zip(SOURCE_NAMES, MIXES[mix]):
        if name not in names:
            continue
        data = plant_alpha(fmt, image_bytes(fmt, w, h, seed=11 + SOURCE_NAMES.index(name)), w, h, alpha if name == "diffuse" else "random")
        rgba = np_decode(fmt, data, w, h)
        given[name] = (fmt, data)
        floats[name] = np.ascontiguousarray(rgba[..., 0]) if name == "roughness" else rgba
    return given, floats


def run_convert(ctx, form, kind, given, w, h, out8, offset=0):
    """sthip_convert_material with sources in texel formats (given: name -> (format by name or number, bytes)). Host form, or device form through torch buffers whose images start
    `offset` bytes (a multiple of 16) beyond their allocations."""
    from stratum_amd import _lib

    if form == "device":
        import torch

    n = w * h
    d = wire.ConvertMaterialDesc()
    d.kind, d.width, d.height, d.device_ptrs, d.output_format = kind, w, h, int(form == "device"), int(out8)
    keep = []
    fields = {"diffuse": ("gDiffuse", "diffuse_format"), "specular": ("gSpecular", "specular_format"), "transmittance": ("gTransmittance", "transmittance_format"),
              "roughness": ("gRoughness", "roughness_format"), "input": ("gInput", "input_format")}
    for name, (fmt, data) in given.items():
        data = np.array(data)
        if form == "device":
            t = torch.empty(data.size + offset, dtype=torch.uint8, device="cuda")
            t[offset:].copy_(torch.from_numpy(data))
            keep.append(t)
            setattr(d, fields[name][0], t.data_ptr() + offset)
        else:
            keep.append(data)
            setattr(d, fields[name][0], data.ctypes.data)
        setattr(d, fields[name][1], wire.texel_format(fmt))
    size, dt = (1, np.uint8) if out8 else (4, F32)

    def room(nbytes):
        if form == "device":
            return torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
        return np.full(nbytes, 0xAB, np.uint8)

    address = lambda b: b.data_ptr() if form == "device" else b.ctypes.data
    back = lambda b, shape: (b.cpu().numpy() if form == "device" else b).view(dt).reshape(shape)
    if kind >= 2:
        rw = room(n * size)
        d.gRoughnessRW = address(rw)
        ctx._check(_lib.lib().sthip_convert_material(ctx._h, C.byref(d)), "sthip_convert_material")
        if form == "device":
            torch.cuda.synchronize()
        return back(rw, (h, w))
    outs = [room(n * 4 * size) for _ in range(3)]
    for k in range(3):
        d.gOutput[k] = address(outs[k])
    mask = room(n * size) if "diffuse" in given else None
    if mask is not None:
        d.gOutputAlphaMask = address(mask)
    min_alpha = room(4)
    d.gOutputMinAlpha = address(min_alpha)
    if form == "device":
        torch.cuda.synchronize()
    ctx._check(_lib.lib().sthip_convert_material(ctx._h, C.byref(d)), "sthip_convert_material")
    if form == "device":
        torch.cuda.synchronize()
    word = (min_alpha.cpu().numpy() if form == "device" else min_alpha).view(np.uint32)[0]
    return {"output": [back(t, (h, w, 4)) for t in outs], "alpha_mask": back(mask, (h, w)) if mask is not None else None, "min_alpha": int(word)}


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("mix", sorted(MIXES))
@pytest.mark.parametrize("kind", [GLTF, DS], ids=["gltf", "diffspec"])
def test_gpu_material_kinds_with_sources_in_texel_formats(ctx, kind, mix, form):
    """Mixed formats, every subset of sources, 8-bit and float outputs, at 67 x 5 and 5 x 7: the numpy conversion of the
    numpy-decoded floats, bit for bit; alpha planted as all 1, one texel just below 1 and one texel 0."""
    count = 0
    for h, w in ((5, 67), (7, 5)):
        for names in mc.subsets(kind):
            for out8 in (True, False):
                for alpha in ("random", "all255", "one_below", "zero") if names == mc.subsets(kind)[-1] else ("random",):
                    count += 1
                    given, floats = convert_case(kind, mix, w, h, names, alpha)
                    want = mc.np_material(kind, out8=out8, **floats)
                    got = run_convert(ctx, form, kind, given, w, h, out8)
                    mc.assert_material(got, want, (mix, h, w, names, out8, alpha))
                    if "diffuse" in names and MIXES[mix][0] in ALPHA_FORMATS:
                        if alpha == "all255":
                            assert got["min_alpha"] == 0xFFFFFFFF
                        if alpha == "zero":
                            assert got["min_alpha"] == 0
                        if alpha == "one_below":
                            assert 0xF0000000 < got["min_alpha"] < 0xFFFFFFFF or MIXES[mix][0].startswith("BC2")
    assert count == 2 * 2 * ((7 if kind == GLTF else 15) + 3)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("kind", [A2R, S2R], ids=["alpha", "shininess"])
def test_gpu_roughness_kinds_with_an_input_in_a_texel_format(ctx, kind, form):
    """gInput in any format: channel 0 is taken, as a Texture2D<float> read does."""
    for fmt in FORMATS:
        if fmt in ("RGBA32F", "RGBA8_UNORM"):  # (0 and 1 are R32F and R8_UNORM for a one-channel source: the existing suite)
            continue
        for h, w in ((5, 67), (7, 5)):
            data, rgba = expected(fmt, w, h)
            for out8 in (True, False):
                got = run_convert(ctx, form, kind, {"input": (fmt, data)}, w, h, out8)
                with np.errstate(invalid="ignore"):
                    assert same(got, mc.np_roughness(kind, np.ascontiguousarray(rgba[..., 0]), out8)), (fmt, h, w, out8)


@pytest.mark.gpu
def test_gpu_formats_0_and_1_are_unchanged(ctx):
    """One case of each existing kind through the existing numpy statement, and format 19 / 31 (the same texels by their new
    names) give the same bytes as 1 / 0."""
    for kind in (GLTF, DS):
        names = mc.subsets(kind)[-1]
        for src8 in (True, False):
            sources = mc.pick(mc.material_inputs(31, 33, src8), names)
            want = mc.np_material(kind, out8=True, **sources)
            mc.assert_material(ctx.convert_material(mc.KIND_NAMES[kind], **sources), want, (kind, src8))
            four, one = (19, 16) if src8 else (31, 28)
            given = {n: (four if n != "roughness" else one, np.ascontiguousarray(a).view(np.uint8).reshape(-1)) for n, a in sources.items()}
            mc.assert_material(run_convert(ctx, "host", kind, given, 33, 31, True), want, (kind, src8, "by the new names"))
    x = mc.roughness_input(31, 33, True)
    assert same(ctx.convert_material("AlphaToRoughness", input=x)["roughness"], mc.np_roughness(A2R, x))


@pytest.mark.gpu
def test_gpu_convert_refusals_with_texel_formats(ctx):
    from stratum_amd import _lib

    import torch

    L = _lib.lib()
    given, _ = convert_case(GLTF, "blocks", 5, 7, ("diffuse", "specular"), "random")
    out = [np.full((7, 5, 4), 0xAB, np.uint8) for _ in range(3)]
    mask, min_alpha = np.full((7, 5), 0xAB, np.uint8), np.full(1, 0xABABABAB, np.uint32)
    keep = {n: np.array(data) for n, (_, data) in given.items()}

    def desc():
        d = wire.ConvertMaterialDesc()
        d.kind, d.width, d.height, d.output_format = GLTF, 5, 7, 1
        d.diffuse_format, d.specular_format = T["BC3_SRGB"], T["BC1_RGB"]
        d.gDiffuse, d.gSpecular = keep["diffuse"].ctypes.data, keep["specular"].ctypes.data
        for k in range(3):
            d.gOutput[k] = out[k].ctypes.data
        d.gOutputAlphaMask, d.gOutputMinAlpha = mask.ctypes.data, min_alpha.ctypes.data
        return d

    def refused(d, field, code=-1):
        rc = L.sthip_convert_material(ctx._h, C.byref(d))
        msg = L.sthip_last_error(ctx._h).decode()
        assert rc == code and field in msg and "sthip_convert_material" in msg, (field, rc, msg)
        assert all((o == 0xAB).all() for o in out) and (mask == 0xAB).all() and min_alpha[0] == 0xABABABAB

    for value in (2, 15, 40, 47, 80, 255):
        d = desc()
        d.specular_format = value
        refused(d, "specular_format")
    d = desc()
    d.diffuse_format = wire.TEXEL_UNSUPPORTED["BC7_SRGB"]
    refused(d, "BC7_SRGB", code=-4)
    d = desc()
    d.diffuse_format = wire.TEXEL_UNSUPPORTED["R8_SNORM"]
    refused(d, "diffuse_format", code=-4)
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d = desc()
    d.device_ptrs = 1
    d.gDiffuse, d.gSpecular = t.data_ptr() + 8, t.data_ptr() + 1024  # a BC3 image needs 16 bytes
    for k in range(3):
        d.gOutput[k] = t.data_ptr() + 2048 + 256 * k
    d.gOutputAlphaMask, d.gOutputMinAlpha = t.data_ptr() + 3072, t.data_ptr() + 3584
    refused(d, "gDiffuse")
    d.gDiffuse, d.gSpecular = t.data_ptr(), t.data_ptr() + 1024 + 4  # a BC1 image 8
    refused(d, "gSpecular")
    assert int(t.max().item()) == 0
    assert L.sthip_convert_material(ctx._h, C.byref(desc())) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [GLTF, DS], ids=["gltf", "diffspec"])
def test_gpu_the_wide_srgb_path_equals_the_generic_path(ctx, kind):
    """gDiffuse RGBA8_SRGB with the other sources RGBA8_UNORM and 8-bit outputs: 16-byte aligned images take k_material_bytes
    four texels per lane, images offset by 4 bytes its one-texel lanes, and the same bytes under their 1-byte aligned names
    (19, 16) offset by 1 byte the generic kernel. All three give the numpy statement's bytes."""
    for h, w in ((5, 67), (7, 5), (16, 16)):
        for alpha in ("random", "all255", "one_below", "zero"):
            d = plant_alpha("RGBA8_SRGB", every_byte_image("RGBA8_SRGB") if h == 16 else image_bytes("RGBA8_SRGB", w, h, seed=21), w, h, alpha)
            s, t, r = (np.array(image_bytes(f, w, h, seed=22 + k)) for k, f in enumerate(("RGBA8_UNORM", "RGBA8_UNORM", "R8_UNORM")))
            floats = {"diffuse": np_decode("RGBA8_SRGB", d, w, h), "specular": np_decode("RGBA8_UNORM", s, w, h), "transmittance": np_decode("RGBA8_UNORM", t, w, h)}
            wide = {"diffuse": ("RGBA8_SRGB", d), "specular": (1, s), "transmittance": (1, t)}
            generic = {"diffuse": ("RGBA8_SRGB", d), "specular": (19, s), "transmittance": (19, t)}
            if kind == DS:
                floats["roughness"] = np_decode("R8_UNORM", r, w, h)[..., 0].copy()
                wide["roughness"], generic["roughness"] = (1, r), (16, r)
            want = mc.np_material(kind, out8=True, **floats)
            for label, given, offset in (("wide", wide, 0), ("one texel per lane", wide, 4), ("generic", generic, 1), ("host", wide, None)):
                got = run_convert(ctx, "host" if offset is None else "device", kind, given, w, h, True, offset=offset or 0)
                mc.assert_material(got, want, (label, h, w, alpha))
            if kind == GLTF:  # the alpha byte and the mask pass through; the base colour byte is the table's
                assert np.array_equal(got["alpha_mask"].reshape(-1), d[3::4])
                assert np.array_equal(got["output"][0][..., :3].reshape(-1, 3), quantise(srgb_curve(ratio(d.reshape(-1, 4)[:, :3], 255))))


# ---------------------------------------------------------------------------------------------------------------------------
# GPU, end to end: the hosts
# ---------------------------------------------------------------------------------------------------------------------------
def asset_images():
    """16 x 16: an sRGB8 base colour (alpha a checker of 0 and 255), an RGBA8 metallic/roughness image, an RGB8 normal map
    (a bumpy field around +z) and an sRGB8 emission image."""
    rng = np.random.RandomState(91)
    base, mr, emission = (rng.randint(0, 256, size=(16, 16, 4)).astype(np.uint8) for _ in range(3))
    yy, xx = np.mgrid[0:16, 0:16]
    base[..., 3] = np.where(((yy // 4) + (xx // 4)) % 2 == 0, 255, 0)
    normal = np.stack([128 + 60 * np.sin(xx), 128 + 60 * np.cos(yy), np.full((16, 16), 230.0)], axis=-1).astype(np.uint8)
    return base, mr, np.ascontiguousarray(normal), emission


def asset_scene(context, raw, colour="RGBA8_SRGB"):
    """A floor, a card with the glTF material and the normal map, and an emissive quad with an emission image. raw: the images
    as TexelImages in the asset's formats; else as the numpy-decoded float arrays. colour: the format the base colour and the
    emission bytes are taken for."""
    from stratum_amd import scenes
    from stratum_amd.scene import ImageValue, SceneBuilder, TexelImage, translate

    base, mr, normal, emission = asset_images()
    if raw:
        base_i, normal_i, emission_i = TexelImage(base, colour, 16, 16), TexelImage(normal, "RGB8_UNORM", 16, 16), TexelImage(emission, colour, 16, 16)
    else:
        base_i, normal_i, emission_i = (np_decode(f, a.reshape(-1), 16, 16) for f, a in (("RGBA8_SRGB", base), ("RGB8_UNORM", normal), ("RGBA8_SRGB", emission)))
    b = SceneBuilder("asset card")
    floor = b.add_material((0.6, 0.6, 0.6), roughness=0.5)
    card = b.make_metallic_roughness_material(ImageValue((0.9, 0.8, 0.7), base_i), ImageValue((0.0, 0.6, 0.4, 0.0), mr), context=context)
    b.set_material_images(card, bump_image=b.add_image(normal_i, context=context), bump_strength=1.0)
    light = b.make_metallic_roughness_material((1.0, 1.0, 1.0), emission=ImageValue((17.0, 12.0, 4.0), emission_i), context=context)
    assert b.alpha_test(card)

    def quad(p0, p1, p2, p3, n, mat, transform=None):
        pos, nrm, uv, tri = scenes._quad(p0, p1, p2, p3, n)
        b.add_instance(b.add_mesh(pos, nrm, uv, tri), mat, transform)

    quad((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1), (0, 1, 0), floor)
    quad((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (0, 0, 1), floor)
    quad((-0.6, 0, 0.6), (0.6, 0, 0.6), (0.6, 0, -0.6), (-0.6, 0, -0.6), (0, 1, 0), card, translate((0.0, -0.3, 0.0)))
    quad((-0.3, 0.9, -0.3), (0.3, 0.9, -0.3), (0.3, 0.9, 0.3), (-0.3, 0.9, 0.3), (0, -1, 0), light)
    return b.build(), {"eye": (0.0, 0.6, 3.5), "target": (0.0, -0.3, 0.0), "fovy": np.radians(40.0)}


@pytest.mark.gpu
def test_gpu_an_asset_in_its_own_formats_renders_the_frame_of_the_numpy_decoded_images(ctx):
    """64 x 64, one sample, level 0 only (no ray cones: an 8-bit resident image then gives what its decoded floats give, the
    contract of the resident formats): bit for bit."""
    from stratum_amd import camera
    from stratum_amd.bdpt import BDPT

    made, cam = asset_scene(ctx, True)
    attached, _ = asset_scene(ctx, False)
    assert made.materials.tobytes() == attached.materials.tobytes()
    assert len(made.images) == len(attached.images) == 5 and len(made.images1) == len(attached.images1) == 1
    kinds = [a.dtype for a in made.images]
    assert kinds == [np.uint8] * 4 + [F32]  # the three material images; the RGB8 normal map stays bytes; the sRGB emission image is binary32
    for a, b in zip(made.images + made.images1, attached.images + attached.images1):
        assert same(mc.as_float(a), mc.as_float(b))
    too_bright, _ = asset_scene(ctx, True, colour="RGBA8_UNORM")  # what handing the sRGB bytes over as unorm gives: another frame
    frames = []
    for sc in (made, attached, too_bright):
        r = BDPT(device=0, args={"bdptFlag": ["~raycones", "normalmaps", "alphatest"]})
        try:
            r.update(sc)
            out = r.render(camera.Frame(64, 64, cam["fovy"], cam["eye"], cam["target"]), 0, 1)
            frames.append({k: np.array(v, copy=True) for k, v in out.items() if isinstance(v, np.ndarray)})
        finally:
            r.close()
    for k in ("radiance", "albedo", "visibility", "depth"):
        assert np.array_equal(np.ascontiguousarray(frames[0][k]).view(np.uint8), np.ascontiguousarray(frames[1][k]).view(np.uint8)), k
    assert frames[0]["radiance"][..., :3].any()
    assert not np.array_equal(frames[0]["radiance"], frames[2]["radiance"]) and frames[2]["radiance"][..., :3].sum() > frames[0]["radiance"][..., :3].sum()


TEXEL_FORMATS_HOST = os.path.join(ROOT, "tests", "cpp", "texel_formats_host")


@pytest.fixture(scope="module")
def texel_formats_host(built):
    src = os.path.join(ROOT, "tests", "cpp", "texel_formats_host.cpp")
    deps = [src, os.path.join(ROOT, "stratum_amd", "host", "stratum_hip.hpp"), os.path.join(ROOT, "include", "sthip.h")]
    if not os.path.exists(TEXEL_FORMATS_HOST) or os.path.getmtime(TEXEL_FORMATS_HOST) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", TEXEL_FORMATS_HOST, src, "-L" + os.path.join(ROOT, "stratum_amd"), "-lstratum_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "stratum_amd")])
    return TEXEL_FORMATS_HOST


def host_texels(image, channels, alpha_texel=None, alpha=0):
    """The bytes tests/cpp/texel_formats_host.cpp fills its 9 x 7 sources with."""
    i = np.arange(63 * channels, dtype=np.uint64)
    data = ((i * 29 + image * 71 + (i * i) % 241) & 0xFF).astype(np.uint8)
    if alpha_texel is not None:
        data[3::4] = 255
        data[4 * alpha_texel + 3] = alpha
    return data


def test_cpp_host_builds_and_prints_its_usage(texel_formats_host):
    out = subprocess.run([texel_formats_host], capture_output=True, text=True)
    assert out.returncode == 2 and "usage: texel_formats_host" in out.stderr


@pytest.mark.gpu
def test_gpu_cpp_host_equals_the_python_mirror(ctx, texel_formats_host, tmp_path):
    from stratum_amd.scene import ImageValue, SceneBuilder, TexelImage

    outp = str(tmp_path / "out.bin")
    run = subprocess.run([texel_formats_host, outp], capture_output=True, text=True)
    assert run.returncode == 0 and "DECODED" in run.stdout, run.stdout + run.stderr
    raw = np.fromfile(outp, np.uint8)
    n, at = 63, 0

    def take(count):
        nonlocal at
        at += count
        return raw[at - count : at]

    b1, b2 = SceneBuilder(), SceneBuilder()
    metallic_roughness = ImageValue((0.0, 0.3, 0.7, 0.0), TexelImage(host_texels(1, 3), "RGB8_UNORM", 9, 7))
    m1 = b1.make_metallic_roughness_material(ImageValue((0.5, 0.25, 0.75), TexelImage(host_texels(0, 4, 5, 40), "RGBA8_SRGB", 9, 7)), metallic_roughness, eta=1.4, context=ctx)
    b1.set_material_images(m1, bump_image=b1.add_image(TexelImage(host_texels(2, 3), "RGB8_UNORM", 9, 7), context=ctx))
    m2 = b2.make_metallic_roughness_material((0.0, 0.0, 0.0), metallic_roughness, eta=1.4, emission=ImageValue((2.0, 1.5, 1.0), TexelImage(host_texels(3, 4), "RGBA8_SRGB", 9, 7)), context=ctx)
    assert take(72).tobytes() == b1._materials[m1].tobytes(), "the stored material record: values and image handles"
    assert int(take(4).view(np.uint32)[0]) == b1.min_alpha(m1) == int(F32(40) / F32(255) * F32(4294967296.0)) and b1.alpha_test(m1)
    for k in range(3):
        assert np.array_equal(take(n * 4), b1._images[k].reshape(-1)), k
    assert np.array_equal(take(n), b1._images1[0].reshape(-1))
    bump = b1._images[int(b1._materials[m1]["bump_index"])]
    assert bump.dtype == np.uint8 and np.array_equal(take(n * 4), bump.reshape(-1))
    assert np.array_equal(bump[..., :3].reshape(-1), host_texels(2, 3)) and (bump[..., 3] == 255).all()
    assert take(72).tobytes() == b2._materials[m2].tobytes()
    emission = b2._images[0]
    assert emission.dtype == F32 and take(n * 16).tobytes() == emission.tobytes()
    assert same(emission, np_decode("RGBA8_SRGB", host_texels(3, 4), 9, 7))
    assert at == raw.size


@pytest.mark.gpu
def test_gpu_poisoned_allocations_give_the_same_values(built):
    """The host forms once more in a fresh child process with STHIP_POISON_ALLOC (read once per process): the staged buffers
    start as 0x7F bytes, so a texel the kernels do not write shows."""
    if os.environ.get("STHIP_TEXEL_FORMATS_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="0x7F", STHIP_TEXEL_FORMATS_POISON_CHILD="1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                          "(decode_texels_equals_numpy and host and (rgba8 or r32f_a)) or (texel_formats and host and blocks)"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout
