"""The reuse hash grid as csrc/hashgrid.h DEFINES it, in Python integers (no GPU, no oracle, no library): what
sthip_build_hash_grid must give, word for word. Also what decides which path of csrc/hashgrid.hip a key set takes, derived
from the keys alone, the directed key sets of tests/test_hash_grid.py, and the generator of its generated slice.

The definition: the appends take effect in append order. Append k = (home, checksum) probes the slots home .. home + 31 of a
table of bucket_count + 32 slots as the earlier appends left it: the first empty slot is claimed, the first slot holding the
checksum is joined, otherwise the append is dropped. counters = appends per slot, indices = their exclusive prefix sum in
slot order, dest[k] = indices[slot] + the rank of k among the slot's appends in append order; 0xFFFFFFFF for a dropped one."""
import random

import numpy as np

WINDOW = 32
DROPPED = 0xFFFFFFFF
SPECIAL_MAX = 1024  # hashgrid.hip's HG_SPECIAL_MAX: more special cells than this and one thread rebuilds the table serially
M32 = 0xFFFFFFFF
F32 = np.float32


def special_cells(keys):
    """The distinct (home, checksum) cells that have another cell with the same checksum and a home fewer than 32 away."""
    homes = {}
    for home, checksum in set((int(h), int(c)) for h, c in keys):
        homes.setdefault(checksum, []).append(home)
    n = 0
    for hs in homes.values():
        hs.sort()
        for i, h in enumerate(hs):
            if (i > 0 and h - hs[i - 1] < WINDOW) or (i + 1 < len(hs) and hs[i + 1] - h < WINDOW):
                n += 1
    return n


def build(keys, bucket_count):
    """keys: a sequence of (home, checksum). Returns the table, dest and what the keys alone say about the paths taken."""
    buckets = bucket_count + WINDOW
    checksums, cell_of, members = [0] * buckets, [None] * buckets, [[] for _ in range(buckets)]
    slot_of = []
    merged = False
    for k, (home, checksum) in enumerate((int(h), int(c)) for h, c in keys):
        assert 0 <= home < bucket_count and 0 < checksum <= M32, (k, home, checksum)
        slot = None
        for i in range(home, home + WINDOW):
            if checksums[i] == 0:
                checksums[i], cell_of[i] = checksum, (home, checksum)
                slot = i
                break
            if checksums[i] == checksum:
                slot = i
                merged = merged or cell_of[i] != (home, checksum)
                break
        slot_of.append(slot)
        if slot is not None:
            members[slot].append(k)
    counters = [len(m) for m in members]
    indices, total = [], 0
    for c in counters:
        indices.append(total)
        total += c
    dest = [DROPPED] * len(slot_of)
    for slot, m in enumerate(members):
        for rank, k in enumerate(m):
            dest[k] = indices[slot] + rank
    return {
        "checksums": np.array(checksums, np.uint32),
        "counters": np.array(counters, np.uint32),
        "indices": np.array(indices, np.uint32),
        "dest": np.array(dest, np.uint32).reshape(-1),
        "slot_of": slot_of,
        "special_cells": special_cells(keys),
        "dropped": sum(1 for s in slot_of if s is None),
        "away": any(c is not None and c[0] != i for i, c in enumerate(cell_of)),  # a cell that sits away from its home
        "merged": merged,  # an append joined a slot that a different cell claimed
        "kept": total,
    }


# ---- hashgrid_bucket_index (csrc/hashgrid.h, hashgrid.hlsli:15-21) a third time: numpy float32 and Python integers ----
def xxhash32(p):  # rng.hlsli:6-15
    h = (p + 374761393) & M32
    h = (668265263 * (((h << 17) | (h >> 15)) & M32)) & M32
    h = (2246822519 * (h ^ (h >> 15))) & M32
    h = (3266489917 * (h ^ (h >> 13))) & M32
    return h ^ (h >> 16)


def pcg(v):  # rng.hlsli:17-21
    state = (v * 747796405 + 2891336453) & M32
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
    return ((word >> 22) ^ word) & M32


def f2i_sat(f):
    """float32 -> int32 as the hardware converts: saturating, NaN to 0, towards zero."""
    if f >= F32(2147483648.0):
        return 0x7FFFFFFF
    if f <= F32(-2147483648.0):
        return -0x80000000
    return int(f) if f == f else 0


def f2u_sat(f):
    """float32 -> uint32 as the hardware converts: NaN and negatives to 0, too large to 0xFFFFFFFF, towards zero."""
    if not (f > F32(0)):
        return 0
    if f >= F32(4294967296.0):
        return M32
    return int(f)


def u2f(u):
    """uint32 -> float32, to nearest even (the integer is exact as a double, which rounds once)."""
    return F32(float(u))


def bucket_index(pos, cell_size, bucket_count):
    """(home bucket, checksum) of a position (three float32) and a cell size (float32)."""
    cell_size = F32(cell_size)
    with np.errstate(all="ignore"):
        p = [f2i_sat(F32(np.floor(F32(F32(x) / cell_size)) + F32(0.5))) & M32 for x in pos]
        checksum = xxhash32(f2u_sat(F32(cell_size + u2f(xxhash32((p[2] + xxhash32((p[1] + xxhash32(p[0])) & M32)) & M32)))))
        home = pcg(f2u_sat(F32(cell_size + u2f(pcg((p[2] + pcg((p[1] + pcg(p[0])) & M32)) & M32))))) % bucket_count
    return home, max(1, checksum)


def build_records(records, bucket_count, lvc):
    """The records form: `records` a (slots, 4, 4) float32 array of NEE appends (staged when word 3 of float4 2, the cell size, is
    not zero as bits) or, with lvc, (slots, 6, 4) of LVC appends (word 3 of float4 0). Compaction in order, the keys, the build,
    and the scattered data (3 resp. 5 float4 per record; records the build did not place are zero)."""
    bits = records.view(np.uint32)
    staged = [s for s in range(records.shape[0]) if bits[s, 0 if lvc else 2, 3] != 0]
    keys = [bucket_index(records[s, 0, :3], records[s, 0 if lvc else 2, 3], bucket_count) for s in staged]
    out = build(keys, bucket_count)
    data = np.zeros((records.shape[0], 5 if lvc else 3, 4), np.uint32)
    for k, s in enumerate(staged):
        d = int(out["dest"][k])
        if d == DROPPED:
            continue
        r = bits[s]
        if lvc:
            data[d] = r[1:6]
        else:
            data[d, 0] = (r[0, 3], r[1, 0], r[1, 1], r[1, 2])
            data[d, 1] = (r[2, 0], r[2, 1], r[2, 2], r[3, 3])
            data[d, 2] = (r[3, 0], r[3, 1], r[3, 2], r[1, 3])
    out.update(count=len(staged), keys=np.array(keys, np.uint32).reshape(-1, 2), data=data)
    return out


# ---- the directed key sets: each the smallest that reaches its path ----
class Case:
    """name, bucket_count, keys, slots, and what the case is FOR, as conditions on what the reference derives from the keys:
    specials (exact count, or None), drops (exact count, True for "some", or None)."""

    def __init__(self, name, bucket_count, keys, slots=None, specials=None, drops=None, away=None, merged=None):
        self.name, self.bucket_count, self.keys = name, bucket_count, [(int(h), int(c)) for h, c in keys]
        self.slots = max(len(self.keys), 1) if slots is None else slots
        self.specials, self.drops, self.away, self.merged = specials, drops, away, merged

    def __repr__(self):
        return self.name


def _pick(rng, seq):
    return seq[int(rng.random() * len(seq))]  # (random() is the one stream Python promises to keep)


def _random_keys(rng, bucket_count, appends, alphabet, pool):
    checksums = [1 + int(rng.random() * M32) for _ in range(alphabet)]
    cells = [(int(rng.random() * bucket_count), _pick(rng, checksums)) for _ in range(pool)]
    return [_pick(rng, cells) for _ in range(appends)]


def _twice(cells):
    """Every cell appended twice: all the first appends in order, then the second ones in order."""
    return list(cells) + list(cells)


def special_bound_case(cells_wanted):
    """Exactly `cells_wanted` (1024 or 1025) special cells: pairs 5 apart with one checksum per pair, 40 slots from pair to pair
    (1025: the last group is a chain of three), every cell appended twice, the order shuffled with a fixed seed."""
    pairs, triple = (cells_wanted // 2, 0) if cells_wanted % 2 == 0 else ((cells_wanted - 3) // 2, 1)
    cells = []
    for i in range(pairs + triple):
        cells += [(40 * i, 1000 + i), (40 * i + 5, 1000 + i)]
    if triple:
        cells.append((40 * (pairs + triple - 1) + 10, 1000 + pairs + triple - 1))
    keys = _twice(cells)
    rng = random.Random(20240 + cells_wanted)
    for i in range(len(keys) - 1, 0, -1):  # (a shuffle from random() alone: the one stream Python promises to keep)
        j = int(rng.random() * (i + 1))
        keys[i], keys[j] = keys[j], keys[i]
    return Case("special_list_%d" % cells_wanted, 40 * (pairs + triple) + 40, keys, specials=cells_wanted, drops=0)


STALE_SMALL = Case("ten_appends_40_buckets", 40, [(3, 7), (3, 9), (4, 7), (3, 7), (39, 5), (39, 6), (4, 9), (38, 5), (3, 9), (39, 5)], specials=6, drops=0)


def directed_cases():
    cases = []
    add = lambda *a, **k: cases.append(Case(*a, **k))
    # sizes
    add("count0_slots1", 40, [], slots=1, specials=0, drops=0)
    add("count0_slots300", 40, [], slots=300, specials=0, drops=0)
    add("count1", 40, [(17, 0x12345678)], specials=0, drops=0)
    for n in (1, 255, 256, 257, 4096, 4097):
        add("count_eq_slots_%d" % n, 300, _random_keys(random.Random(n), 300, n, 1000, 400))
    add("slots4097_count4096", 300, _random_keys(random.Random(11), 300, 4096, 1000, 400), slots=4097)
    add("slots4097_count1", 300, [(299, 77)], slots=4097, specials=0, drops=0)
    # one cell
    add("one_cell_5000", 40, [(7, 0xDEADBEEF)] * 5000, specials=0, drops=0, away=False)
    # full windows
    add("one_bucket_40_checksums", 1, _twice([(0, 100 + i) for i in range(40)]), specials=0, drops=16, away=True)
    add("five_buckets_80_cells", 5, _twice([(i % 5, 100 + i) for i in range(80)]), specials=0, drops=2 * (80 - 36), away=True)  # (the windows of the homes 0 .. 4 end at slot 35)
    add("descending_homes_crowded", 100, _twice([(h, 1000 + 2 * h + j) for h in range(60, 19, -1) for j in (0, 1)]), specials=0, drops=True, away=True)
    # a later cell L (home 10) may claim a slot of its window before the earlier cells arrive; they displace it down a chain
    # that runs to the end of its window [10, 42): 20 cells of home 0 hold 0..19, 30 cells of home 12 hold 20..43 (6 dropped)
    add("displaced_cell_runs_out_of_window", 100, [(0, 100 + i) for i in range(20)] + [(12, 200 + i) for i in range(30)] + [(10, 999), (10, 999)], specials=0, drops=6 + 2, away=True)
    # same checksum, two cells d apart
    for d in (1, 31, 32, 33):
        for earlier in ("lower", "higher"):
            x, y = (20, 0xC0FFEE), (20 + d, 0xC0FFEE)
            first, second = (x, y) if earlier == "lower" else (y, x)
            near = 2 if d < WINDOW else 0
            add("twins_%d_%s_empty" % (d, earlier), 100, [first, second, first, second, second], specials=near, drops=0, away=False, merged=False)
            fillers = [(20 + i, 500 + i) for i in range(d)]  # the slots [20, 20 + d) go to earlier cells
            add("twins_%d_%s_filled" % (d, earlier), 100, fillers + [first, second, first, second, second], specials=near, drops=0 if d < WINDOW else 2 if earlier == "lower" else 3,
                merged=d < WINDOW)
    # three cells in a chain, 20 apart, one checksum: A-C are not near, all three are special
    chain = [(20, 0xABCDEF), (40, 0xABCDEF), (60, 0xABCDEF)]
    for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        cells = [chain[i] for i in order]
        name = "chain_" + "".join("ABC"[i] for i in order)
        add(name + "_empty", 100, _twice(cells), specials=3, drops=0, away=False, merged=False)
        fillers = [(h, 700 + h) for h in list(range(20, 40)) + list(range(41, 60))]  # A is pushed onto B's home: whichever of the two comes later joins the other
        add(name + "_filled", 100, fillers + _twice(cells), specials=3, drops=0, merged=True)
    # a special cell S that displaces later ordinary cells (its twin sits out of the way)
    s = (30, 0x5EC1A1)
    add("special_displaces_cascade", 100, _twice([s, (35, 0x5EC1A1)] + [(30 + i, 800 + i) for i in range(5)]), specials=2, drops=0, away=True)
    add("special_displaces_one_out_of_window", 100, _twice([s, (5, 0x5EC1A1)] + [(30 + i, 800 + i) for i in range(31)] + [(30, 899)]), specials=2, drops=2, away=True)
    add("special_window_full_dropped", 100, _twice([(20, 0x5EC1A1)] + [(30 + i, 800 + i) for i in range(32)] + [s, (30, 899)]), specials=2, drops=4)
    # the special list at its bound
    cases.append(special_bound_case(1024))
    cases.append(special_bound_case(1025))
    # checksum values: 1 and 0xFFFFFFFF, the latter at the largest home of its table next to the padding keys of the sort
    add("checksums_1_and_ffffffff", 64, _twice([(63, M32), (0, 1), (63, 1), (0, M32), (10, 1), (20, M32)]), slots=300, specials=4, drops=0)
    add("checksum_ffffffff_pair_at_the_end", 64, _twice([(63, M32), (60, M32), (62, 5)]), slots=257, specials=2, drops=0)
    cases.append(STALE_SMALL)
    return cases


# ---- the generated slice: 300 key sets from committed seeds ----
GENERATED_SEEDS = (4, 5, 6)
GENERATED_PER_SEED = 100


def generated_cases(seeds=GENERATED_SEEDS, per_seed=GENERATED_PER_SEED):
    for seed in seeds:
        rng = random.Random(seed)
        for i in range(per_seed):
            bucket_count = _pick(rng, (1, 2, 5, 33, 40, 100, 300))
            appends = _pick(rng, (0, 1, 2, 10, 50, 200, 600))
            alphabet = _pick(rng, (1, 2, 3, 8, 1000))
            pool = _pick(rng, (1, 3, 20, 100, 400))
            keys = _random_keys(rng, bucket_count, appends, alphabet, pool)
            slots = max(1, appends + _pick(rng, (0, 0, 1, 7, 300)))
            yield Case("generated_%d_%d" % (seed, i), bucket_count, keys, slots=slots)
