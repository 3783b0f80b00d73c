"""The reuse hash grid on its own (include/sthip.h: sthip_build_hash_grid; csrc/hashgrid.hip, and the records chain around it in
csrc/api.hip: build_hash_grid): the device build against the serial probe rule csrc/hashgrid.h defines, stated in Python
integers by tests/hashgrid_ref.py. Every comparison is of whole integer arrays and exact: there are no tolerances here.

The frame tests (test_gpu_parity.py: test_hash_grid_build_paths_agree, test_nee_reservoir_reuse, test_lvc_reservoir_reuse) see
the grid through pixels, at sizes where the special pass of hashgrid.hip, the overflow of its list, a displaced cell that runs
out of its window, padding keys in the sorts and stale scratch are reached by luck or never. Here each has a key set of its own,
and the info struct says which path the device took."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hashgrid_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTED = R.directed_cases()
BY_NAME = {c.name: c for c in DIRECTED}
assert len(BY_NAME) == len(DIRECTED)
TABLE = ("checksums", "counters", "indices", "dest")


# ---------------------------------------------------------------- CPU: the reference, the cases, the header ----------------
def table(buckets, entries):
    t = np.zeros(buckets, np.uint32)
    for slot, value in entries.items():
        t[slot] = value
    return t


def test_reference_equals_hand_written_tables():
    """Three directed cases worked out by hand from the probe rule, so that a wrong reference cannot quietly agree with a wrong
    kernel."""
    # a filler at 20, X = (20, c) is pushed to 21, Y = (21, c) finds c there and joins: X Y X Y Y share slot 21 in append order
    c = 0xC0FFEE
    got = R.build(BY_NAME["twins_1_lower_filled"].keys, 100)
    assert np.array_equal(got["checksums"], table(132, {20: 500, 21: c}))
    assert np.array_equal(got["counters"], table(132, {20: 1, 21: 5}))
    assert np.array_equal(got["indices"], np.array([0] * 21 + [1] + [6] * 110, np.uint32))
    assert got["dest"].tolist() == [0, 1, 2, 3, 4, 5]
    assert (got["special_cells"], got["dropped"], got["away"], got["merged"]) == (2, 0, True, True)
    # one home, 40 checksums twice: the first 32 hold the window, the other 8 are dropped both times
    got = R.build(BY_NAME["one_bucket_40_checksums"].keys, 1)
    assert np.array_equal(got["checksums"], np.array([100 + i for i in range(32)] + [0], np.uint32))
    assert np.array_equal(got["counters"], np.array([2] * 32 + [0], np.uint32))
    assert np.array_equal(got["indices"], np.array([2 * i for i in range(33)], np.uint32))
    assert got["dest"].tolist() == [2 * i for i in range(32)] + [R.DROPPED] * 8 + [2 * i + 1 for i in range(32)] + [R.DROPPED] * 8
    assert (got["special_cells"], got["dropped"], got["away"], got["merged"]) == (0, 16, True, False)
    # S = (30, c) and its twin (35, c) first, then five ordinary cells of the homes 30 .. 34: they stack up behind S and the last
    # one steps over the twin
    c = 0x5EC1A1
    got = R.build(BY_NAME["special_displaces_cascade"].keys, 100)
    assert np.array_equal(got["checksums"], table(132, {30: c, 31: 800, 32: 801, 33: 802, 34: 803, 35: c, 36: 804}))
    assert np.array_equal(got["counters"], table(132, {s: 2 for s in range(30, 37)}))
    assert np.array_equal(got["indices"], np.array([0] * 30 + [0, 2, 4, 6, 8, 10, 12] + [14] * 95, np.uint32))
    first = [0, 10, 2, 4, 6, 8, 12]
    assert got["dest"].tolist() == first + [d + 1 for d in first]
    assert (got["special_cells"], got["dropped"], got["away"], got["merged"]) == (2, 0, True, False)


def test_directed_cases_classify_as_intended():
    """What each case is FOR, by the reference's own derivation from the keys: the special counts, the drops, and 1024 / 1025
    special cells on either side of the list's bound."""
    for case in DIRECTED:
        ref = R.build(case.keys, case.bucket_count)
        assert len(case.keys) <= case.slots and len(case.keys) <= 5000, case
        if case.specials is not None:
            assert ref["special_cells"] == case.specials, case
        if case.drops is True:
            assert ref["dropped"] > 0, case
        elif case.drops is not None:
            assert ref["dropped"] == case.drops, case
        if case.away is not None:
            assert ref["away"] == case.away, case
        if case.merged is not None:
            assert ref["merged"] == case.merged, case
    at, over = R.build(BY_NAME["special_list_1024"].keys, BY_NAME["special_list_1024"].bucket_count), R.build(BY_NAME["special_list_1025"].keys, BY_NAME["special_list_1025"].bucket_count)
    assert at["special_cells"] == R.SPECIAL_MAX and over["special_cells"] == R.SPECIAL_MAX + 1
    for d in (1, 31, 32, 33):  # 31 is special, 32 is not; with nothing between them both twins keep a slot of their own
        for earlier in ("lower", "higher"):
            ref = R.build(BY_NAME["twins_%d_%s_empty" % (d, earlier)].keys, 100)
            assert ref["special_cells"] == (2 if d < 32 else 0) and ref["checksums"][20] == ref["checksums"][20 + d] == 0xC0FFEE
            assert np.count_nonzero(ref["checksums"]) == 2
    # the displaced cell of "displaced_cell_runs_out_of_window" is dropped, not parked: its window [10, 42) is full of earlier cells
    ref = R.build(BY_NAME["displaced_cell_runs_out_of_window"].keys, 100)
    assert ref["slot_of"][-2:] == [None, None] and (ref["checksums"][10:42] != 0).all() and 999 not in ref["checksums"].tolist()
    # the special cell of "special_window_full_dropped" and its later append have no slot
    case = BY_NAME["special_window_full_dropped"]
    ref = R.build(case.keys, 100)
    assert [k for k, key in enumerate(case.keys) if key == (30, 0x5EC1A1)] == [k for k, s in enumerate(ref["slot_of"]) if s is None and case.keys[k][1] == 0x5EC1A1]


def test_generated_slice_covers_the_paths():
    """The 300 generated key sets, classified by the reference from the keys alone. Conditions on the committed seeds."""
    cases = list(R.generated_cases())
    assert len(cases) == 300
    special = away = merged = drops = 0
    for case in cases:
        ref = R.build(case.keys, case.bucket_count)
        assert len(case.keys) <= case.slots
        special += ref["special_cells"] > 0
        away += bool(ref["away"])
        merged += bool(ref["merged"])
        drops += ref["dropped"] > 0
    print("generated slice: %d with special cells, %d with a cell away from its home, %d with a merge, %d with drops" % (special, away, merged, drops))
    assert special >= 60 and away >= 50 and merged >= 25 and drops >= 5


def test_bucket_index_restatement_conversions():
    """The conversions of hashgrid_bucket_index as the reference states them (csrc/hashgrid.h: hg_f2i_sat, hg_f2u_sat)."""
    F = np.float32
    assert [R.f2i_sat(F(v)) for v in (2.5, -2.5, -0.5, 3e9, -3e9, np.nan, np.inf, -np.inf, 2147483520.0)] == [2, -2, 0, 0x7FFFFFFF, -0x80000000, 0, 0x7FFFFFFF, -0x80000000, 2147483520]
    assert [R.f2u_sat(F(v)) for v in (2.5, -2.5, 0.0, -0.0, 5e9, np.nan, np.inf, 4294967040.0)] == [2, 0, 0, 0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 4294967040]
    # uint -> float to nearest EVEN: 2^24 + 1 is a tie and goes down, 2^24 + 3 is a tie and goes up; 0xFFFFFFFF rounds to 2^32
    assert R.u2f(16777217) == F(16777216.0) and R.u2f(16777219) == F(16777220.0) and R.u2f(0xFFFFFFFF) == F(4294967296.0)
    assert R.bucket_index((0.0, 0.0, 0.0), 0.25, 1)[0] == 0 and R.bucket_index((0.1, 0.2, 0.3), 0.25, 40)[1] >= 1
    # a point exactly on a cell border belongs to the cell above it; -0.0 to cell 0
    assert R.bucket_index((0.5, 0.0, 0.0), 0.25, 1000) == R.bucket_index((0.74, 0.2, 0.1), 0.25, 1000) != R.bucket_index((0.49, 0.0, 0.0), 0.25, 1000)
    assert R.bucket_index((-0.0, 0.0, 0.0), 0.25, 1000) == R.bucket_index((0.1, 0.0, 0.0), 0.25, 1000)


def test_bucket_index_hashes_equal_the_oracles(built):
    """The two hashes of the restatement, and only those, against the oracle's orc_xxhash32 / orc_pcg."""
    from oracle import oracle_py as orc

    rng = np.random.RandomState(5)
    for v in [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF] + [int(x) for x in rng.randint(0, 2**32, 500, dtype=np.uint64)]:
        assert orc.lib().orc_xxhash32(v) == R.xxhash32(v) and orc.lib().orc_pcg(v) == R.pcg(v), hex(v)


def test_header_documents_the_entry(built):
    from stratum_amd import _lib, wire

    raw = open(os.path.join(ROOT, "include", "sthip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+sthip_build_hash_grid\s*\(\s*sthip_ctx\s*\*\s*\w+\s*,\s*const\s+sthip_hash_grid_desc\s*\*\s*\w+\s*,\s*sthip_hash_grid_info\s*\*\s*\w+\s*\)", text)
    assert "sthip_build_hash_grid" in _lib.EXPORTS and hasattr(_lib.lib(), "sthip_build_hash_grid")
    assert "#define STHIP_ABI_VERSION 11" in text
    body = re.search(r"typedef struct sthip_hash_grid_desc \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in wire.HashGridDesc._fields_] and body.split()[:2] == ["uint32_t", "struct_size;"]
    body = re.search(r"typedef struct sthip_hash_grid_info \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in wire.HashGridInfo._fields_]
    doc = " ".join(raw[raw.index("the reuse hash grid on its own") : raw.index("typedef struct sthip_hash_grid_desc")].replace("*", " ").split())
    for words in ("Refused with STHIP_ERR_INVALID_ARGUMENT before anything is touched", "bucket_count outside (0, 2^28]", "count > slots", "a home >= bucket_count", "a checksum of 0",
                  "a NULL", "struct_size that is not sizeof(sthip_hash_grid_desc)", '"hashgrid_serial" applying as it does in a render', "DROPS the grids kept for the next render",
                  "0xFFFFFFFF for a dropped append", "more than 1024 special cells"):
        assert words in doc, words


def test_wire_structs_have_the_headers_layout(tmp_path):
    from stratum_amd import wire

    fields = [f for f, _ in wire.HashGridDesc._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sthip.h"\nint main(void) { printf("%zu %zu"' + ' " %zu"' * len(fields) + ", sizeof(sthip_hash_grid_desc), sizeof(sthip_hash_grid_info)"
                   + "".join(", offsetof(sthip_hash_grid_desc, %s)" % f for f in fields) + "); return 0; }\n")
    exe = str(tmp_path / "size")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(wire.HashGridDesc), C.sizeof(wire.HashGridInfo)] + [getattr(wire.HashGridDesc, f).offset for f in fields]


# ---------------------------------------------------------------- GPU ------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from stratum_amd.bdpt import BDPT

    r = BDPT(device=0)  # a context and no scene
    yield r
    r.close()


_REFS = {}


def reference(case):
    """Computed once per case, shared by the tests that need it, and never written to."""
    if case.name not in _REFS:
        ref = R.build(case.keys, case.bucket_count)
        for name in TABLE:
            ref[name].setflags(write=False)
        _REFS[case.name] = ref
    return _REFS[case.name]


def check_keys_case(ctx, case, report=True):
    """Both build paths of a key set against the reference; with "hashgrid_serial" 0 the info struct against what the reference
    derived from the keys, so that a case aimed at a path is known to have taken it."""
    ref = reference(case)
    keys = np.array(case.keys, np.uint32).reshape(-1, 2)
    for serial in (0, 1):
        ctx.set_option("hashgrid_serial", serial)
        try:
            got = ctx.build_hash_grid(case.bucket_count, keys=keys, slots=case.slots)
        finally:
            ctx.set_option("hashgrid_serial", 0)
        if report:
            print("%s (count %d, slots %d, bucket_count %d), hashgrid_serial %d: device reports %d special cells, serial rebuild %d, %d dropped"
                  % (case.name, len(case.keys), case.slots, case.bucket_count, serial, got["special_cells"], got["serial_rebuild"], got["dropped"]))
        assert got["count"] == len(case.keys)
        for name in TABLE:
            same = np.array_equal(got[name], ref[name])
            assert same, "%s, hashgrid_serial %d: %s differs at %s" % (case.name, serial, name, np.flatnonzero(got[name] != ref[name])[:8] if got[name].shape == ref[name].shape else "(shape)")
        assert got["dropped"] == ref["dropped"]
        if serial:
            assert got["serial_rebuild"] == 1
        else:
            assert got["special_cells"] == ref["special_cells"], case.name
            assert got["serial_rebuild"] == (1 if ref["special_cells"] > R.SPECIAL_MAX else 0), case.name


STALE_SEQUENCE = ("special_list_1025", "ten_appends_40_buckets", "special_list_1024")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in DIRECTED])
def test_gpu_directed_keys(ctx, name):
    check_keys_case(ctx, BY_NAME[name])


@pytest.mark.gpu
def test_gpu_stale_scratch_sequence(ctx):
    """owner, the control words and the special list live behind the table and are reused from call to call and from a larger
    grid to a smaller one: the overflowing list, then ten appends in a 40-bucket table, then the full list."""
    for name in STALE_SEQUENCE:
        check_keys_case(ctx, BY_NAME[name])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", R.GENERATED_SEEDS)
def test_gpu_generated_keys(ctx, seed):
    for case in R.generated_cases(seeds=(seed,)):
        check_keys_case(ctx, case, report=False)


@pytest.mark.gpu
def test_gpu_refusals(ctx):
    """Refused on the host before anything is touched: the outputs keep the caller's bytes."""
    from stratum_amd import wire

    L = ctx._lib
    keep = []

    def desc(key_list=((3, 7), (4, 9)), **kw):
        d = wire.HashGridDesc()
        keys = np.array(key_list, np.uint32).reshape(-1, 2)
        d.struct_size, d.form, d.bucket_count, d.count, d.slots = C.sizeof(d), 0, 40, keys.shape[0], 8
        out = [np.full(72, 0xAB, np.uint32) for _ in range(4)]
        d.keys, d.checksums, d.counters, d.indices, d.dest = [a.ctypes.data for a in [keys] + out]
        for k, v in kw.items():
            setattr(d, k, v)
        keep.append((keys, out))
        return d, out

    def refused(text, **kw):
        d, out = desc(**kw)
        info = wire.HashGridInfo(count=77)
        rc = L.sthip_build_hash_grid(ctx._h, C.byref(d), C.byref(info))
        msg = L.sthip_last_error(ctx._h).decode()
        assert rc == -1 and "sthip_build_hash_grid" in msg and text in msg, (kw, rc, msg)
        assert info.count == 77 and all((a == 0xAB).all() for a in out)

    refused("struct_size", struct_size=C.sizeof(wire.HashGridDesc) - 8)
    refused("form", form=3)
    refused("bucket_count", bucket_count=0)
    refused("bucket_count", bucket_count=(1 << 28) + 1)
    refused("slots", slots=0)
    refused("count", count=9)
    refused("home bucket", key_list=[(3, 7), (40, 9)])
    refused("checksum of 0", key_list=[(3, 7), (4, 0)])
    for field in ("keys", "checksums", "counters", "indices", "dest"):
        refused(field, **{field: None})
    for form in (1, 2):
        rec = np.zeros((8, 6, 4), np.float32)
        big = np.zeros(8 * 6 * 4, np.uint32)
        full = dict(form=form, records=rec.ctypes.data, compacted_keys=big.ctypes.data, data=big.ctypes.data)
        for field in ("records", "compacted_keys", "data"):
            refused(field, **dict(full, **{field: None}))
    d, _ = desc()
    assert L.sthip_build_hash_grid(ctx._h, None, C.byref(wire.HashGridInfo())) == -1 and L.sthip_build_hash_grid(ctx._h, C.byref(d), None) == -1
    assert L.sthip_build_hash_grid(None, C.byref(d), C.byref(wire.HashGridInfo())) == -1
    info = wire.HashGridInfo()
    assert L.sthip_build_hash_grid(ctx._h, C.byref(d), C.byref(info)) == 0 and info.count == 2  # (the descriptor the refusals vary is a good one)


# ---- records form ----
SPECIAL_POSITIONS = [
    (np.nan, 0.0, 0.0), (0.0, np.nan, np.nan), (np.inf, 0.0, 0.0), (-np.inf, np.inf, 0.0), (1e30, 0.0, 0.0), (-1e30, 1e30, -1e30), (-0.0, -0.0, -0.0), (0.0, 0.0, 0.0),
    (-0.25, -0.5, -0.75), (-0.26, -0.01, -100.3), (0.25, 0.5, 0.75), (0.5, 0.5, 0.5), (-0.5, 0.25, 1.0), (3e9, -3e9, 2147483648.0), (2147483520.0, -2147483648.0, 0.3),
]  # NaN, +/-inf, +/-1e30, -0.0, negative coordinates, coordinates exactly on a cell border (cell sizes 0.25 * 2^k), beyond the int32 range
BIG_CELLS = (16777216.0, 3e9, 1e30, 4294967296.0)  # cell_size + (float)hash rounds differently: the hash's low bits, or all of it, are lost


def make_records(slots, lvc, staged, seed, special=False):
    """`slots` append records of random, distinct payload bits; the staged ones (a boolean mask) with a position on a small lattice
    and a cell size that is a power of two times the minimum radius, or (special) the positions and sizes no scene produces."""
    rng = np.random.RandomState(seed)
    rec = 6 if lvc else 4
    bits = rng.randint(0, 2**32, (slots, rec, 4), dtype=np.uint64).astype(np.uint32)
    bits[:, rec - 1, 3] = np.arange(slots) * 2 + 1  # (distinct whatever the draw)
    records = bits.view(np.float32)
    cell_at = (0, 3) if lvc else (2, 3)
    for s in range(slots):
        if not staged[s]:
            bits[(s,) + cell_at] = 0  # a hole: everything else of it stays random, and must not arrive anywhere
            continue
        if special:
            records[s, 0, :3] = SPECIAL_POSITIONS[s % len(SPECIAL_POSITIONS)]
            sizes = (0.25, 0.5, 0.1) + BIG_CELLS
            records[(s,) + cell_at] = sizes[(s // len(SPECIAL_POSITIONS)) % len(sizes)]
        else:
            radius = (0.25, 0.1)[rng.randint(2)]  # (0.25: lattice points lie exactly on cell borders)
            records[s, 0, :3] = rng.randint(-3, 4, 3) * np.float32(0.25) + (0 if rng.randint(2) else np.float32(0.01))
            records[(s,) + cell_at] = np.float32(radius) * np.float32(2 ** rng.randint(0, 4))
    return records


def hole_patterns(slots):
    idx = np.arange(slots)
    return {"none": idx < 0, "all": idx >= 0, "first": idx == 0, "last": idx == slots - 1, "alternating": idx % 2 == 1, "run_across_256": (idx >= 250) & (idx < 263)}


def check_records_case(ctx, records, bucket_count, lvc, label):
    ref = R.build_records(records, bucket_count, lvc)
    for serial in (0, 1):
        ctx.set_option("hashgrid_serial", serial)
        try:
            got = ctx.build_hash_grid(bucket_count, records=records, lvc=lvc)
        finally:
            ctx.set_option("hashgrid_serial", 0)
        print("%s, hashgrid_serial %d: %d of %d staged, device reports %d special cells, serial rebuild %d, %d dropped" % (label, serial, got["count"], records.shape[0], got["special_cells"], got["serial_rebuild"], got["dropped"]))
        assert got["count"] == ref["count"], label
        assert np.array_equal(got["keys"], ref["keys"]), "%s: keys differ at %s" % (label, np.flatnonzero((got["keys"] != ref["keys"]).any(1))[:8])
        for name in TABLE:
            assert np.array_equal(got[name], ref[name]), (label, serial, name)
        assert np.array_equal(got["data"].view(np.uint32), ref["data"]), (label, serial, "data")  # (NaN payloads: as bits)
        assert got["dropped"] == ref["dropped"]
        if not serial:
            assert got["special_cells"] == ref["special_cells"] and got["serial_rebuild"] == (1 if ref["special_cells"] > R.SPECIAL_MAX else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nee", "lvc"])
@pytest.mark.parametrize("pattern", ["none", "all", "first", "last", "alternating", "run_across_256"])
def test_gpu_records_hole_patterns(ctx, kind, pattern):
    slots = 700
    records = make_records(slots, kind == "lvc", hole_patterns(slots)[pattern], seed=len(pattern) + (100 if kind == "lvc" else 0))
    check_records_case(ctx, records, 40, kind == "lvc", "%s records, %s staged" % (kind, pattern))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nee", "lvc"])
def test_gpu_records_4097_slots(ctx, kind):
    """The largest stage of this file: 4097 slots, three of four staged, a table small enough that appends are dropped."""
    slots = 4097
    records = make_records(slots, kind == "lvc", np.arange(slots) % 4 != 2, seed=9)
    check_records_case(ctx, records, 33, kind == "lvc", "%s records, 4097 slots" % kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["nee", "lvc"])
def test_gpu_records_positions_no_scene_produces(ctx, kind):
    """NaN, +/-inf, +/-1e30, -0.0, negative coordinates, coordinates exactly on a cell border, and cell sizes at which
    cell_size + (float)hash rounds the hash away: the saturating conversions of hashgrid_bucket_index, word for word."""
    slots = len(SPECIAL_POSITIONS) * 7 + 3
    records = make_records(slots, kind == "lvc", np.arange(slots) % 11 != 10, seed=3, special=True)
    check_records_case(ctx, records, 100, kind == "lvc", "%s records, positions no scene produces" % kind)


@pytest.mark.gpu
def test_gpu_a_render_after_the_entry_starts_without_a_kept_grid(built, cornell):
    """The entry builds in the buffers a render keeps its grids in and drops the kept grids: with "reuse_grids_persist" the frame
    after it is the frame of a context that dropped them itself, and not the frame that looks into the kept grid."""
    from stratum_amd import camera
    from stratum_amd.bdpt import BDPT

    sc, cam = cornell
    frame = camera.Frame(96, 64, cam["fovy"], cam["eye"], cam["target"])
    frames = {}
    for mode in ("kept", "dropped", "entry"):
        r = BDPT(device=0, args=dict(bdptFlag=["neereservoirs", "neereservoirreuse"], reservoirM=2))
        try:
            r.set_option("reuse_grids_persist", 1)
            r.update(sc)
            r.render(frame, 4, 1, aovs=False)
            if mode == "entry":
                check_keys_case(r, BY_NAME["ten_appends_40_buckets"], report=False)
            elif mode == "dropped":
                r.set_option("reuse_grids_persist", 1)  # (setting it drops the kept grids)
            frames[mode] = r.render(frame, 5, 1, aovs=False)["radiance"].copy()
        finally:
            r.close()
    assert np.array_equal(frames["entry"].view(np.uint32), frames["dropped"].view(np.uint32))
    assert not np.array_equal(frames["kept"], frames["dropped"])  # (the second frame does look into a kept grid)


@pytest.mark.gpu
def test_gpu_stale_scratch_with_poisoned_allocations(built):
    """The stale-scratch sequence once more in a fresh child process with STHIP_POISON_ALLOC (read once per process): owner, the
    control words, the special list and the sort buffers start as 0x7F bytes, so a word read before it is written shows."""
    if os.environ.get("STHIP_HASH_GRID_POISON_CHILD"):
        return  # (this is the child)
    env = dict(os.environ, STHIP_POISON_ALLOC="127", STHIP_HASH_GRID_POISON_CHILD="1")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "stale_scratch_sequence"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and " passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
