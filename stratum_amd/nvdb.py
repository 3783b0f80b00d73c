"""A NanoVDB 32.3.3 float grid (FogVolume, background 0) from a dense box of binary32 values: the numpy statement of the
contract of include/sthip.h (sthip_build_volume), which csrc/volume_build.hip equals byte for byte. numpy only, no GPU: a host
without a device makes the grids of gVolumes[] with it (SceneBuilder.add_dense_volume).

Layout (the published format, the constants media.h and bvh_build.cpp read by): GridData 672 B, TreeData 64 B, the root (64 B)
with its tiles (32 B each), then all upper nodes (270 400 B), all lower nodes (33 856 B), all leaves (2 144 B), breadth first.
Root tiles ascend by signed tile coordinate (x, then y, then z); the nodes of a level follow their parents' order and then
the child index. Nothing is pruned: a full constant leaf stays a leaf."""
import numpy as np

MAGIC = 0x304244566F6E614E
VERSION = 0x04000C03  # 32.3.3
FLAGS = 0x26  # bounding boxes, min/max, breadth first
GRID_BYTES, TREE_BYTES, ROOT_BYTES, TILE_BYTES, UPPER_BYTES, LOWER_BYTES, LEAF_BYTES = 672, 64, 64, 32, 270400, 33856, 2144
MAX_BYTES, MAX_TILES = 0xFFFFFFF0, 65536

GRID = np.dtype(
    [("magic", "<u8"), ("checksum", "<u8"), ("version", "<u4"), ("flags", "<u4"), ("grid_index", "<u4"), ("grid_count", "<u4"), ("grid_size", "<u8"), ("name", "S256"),
     ("matf", "<f4", 9), ("invmatf", "<f4", 9), ("vecf", "<f4", 3), ("taperf", "<f4"), ("matd", "<f8", 9), ("invmatd", "<f8", 9), ("vecd", "<f8", 3), ("taperd", "<f8"),
     ("world_bbox", "<f8", 6), ("voxel_size", "<f8", 3), ("grid_class", "<u4"), ("grid_type", "<u4"), ("blind_offset", "<i8"), ("blind_count", "<u4"), ("pad", "u1", 20)]
)
TREE = np.dtype([("node_offset", "<u8", 4), ("node_count", "<u4", 3), ("tile_count", "<u4", 3), ("voxel_count", "<u8")])  # offsets: leaf, lower, upper, root
ROOT = np.dtype([("bbox", "<i4", 6), ("table_size", "<u4"), ("background", "<f4"), ("min", "<f4"), ("max", "<f4"), ("ave", "<f4"), ("stddev", "<f4"), ("pad", "u1", 16)])
TILE = np.dtype([("key", "<u8"), ("child", "<i8"), ("state", "<u4"), ("value", "<f4"), ("pad", "u1", 8)])


def _internal(log2dim):
    n = 1 << (3 * log2dim)
    return np.dtype([("bbox", "<i4", 6), ("flags", "<u8"), ("value_mask", "u1", n // 8), ("child_mask", "u1", n // 8), ("min", "<f4"), ("max", "<f4"), ("ave", "<f4"), ("stddev", "<f4"),
                     ("pad", "u1", 16), ("table", "<i8", n)])


UPPER, LOWER = _internal(5), _internal(4)
LEAF = np.dtype([("bbox_min", "<i4", 3), ("bbox_dif", "u1", 3), ("flags", "u1"), ("value_mask", "u1", 64), ("min", "<f4"), ("max", "<f4"), ("ave", "<f4"), ("stddev", "<f4"), ("values", "<f4", 512)])
assert (GRID.itemsize, TREE.itemsize, ROOT.itemsize, TILE.itemsize, UPPER.itemsize, LOWER.itemsize, LEAF.itemsize) == (GRID_BYTES, TREE_BYTES, ROOT_BYTES, TILE_BYTES, UPPER_BYTES, LOWER_BYTES, LEAF_BYTES)


def _groups(keys):
    """First index of each run of equal rows of `keys` (n, 3), and the run every row belongs to."""
    new = np.ones(len(keys), bool)
    new[1:] = (keys[1:] != keys[:-1]).any(axis=1)
    return np.flatnonzero(new), np.cumsum(new) - 1


def _reduce(first, lo, hi, mn, mx):
    """Boxes and min/max of the runs that begin at `first`."""
    return np.minimum.reduceat(lo, first, axis=0), np.maximum.reduceat(hi, first, axis=0), np.minimum.reduceat(mn, first), np.maximum.reduceat(mx, first)


def dense_to_nanovdb(dense, origin=(0, 0, 0), voxel_size=1.0, translation=(0.0, 0.0, 0.0), name=""):
    """The grid's bytes (uint8 array). dense[x, y, z] is the voxel at index coordinate origin + (x, y, z); a voxel is active
    iff its value != 0. ValueError for what sthip_build_volume refuses."""
    dense = np.ascontiguousarray(dense, dtype=np.float32)
    if dense.ndim != 3 or min(dense.shape) < 1:
        raise ValueError("dense must be a [nx, ny, nz] array with every extent >= 1")
    origin = np.asarray(origin, dtype=np.int64).reshape(3)
    dims = np.asarray(dense.shape, dtype=np.int64)
    vs, tr = float(voxel_size), np.asarray(translation, dtype=np.float64).reshape(3)
    if not (np.isfinite(vs) and vs > 0):
        raise ValueError("voxel_size must be finite and positive")
    if not np.isfinite(tr).all():
        raise ValueError("translation must be finite")
    if (origin < -(2**31)).any() or (origin + dims - 1 > 2**31 - 1).any():
        raise ValueError("the box leaves int32")
    name_bytes = name.encode("utf-8") if isinstance(name, str) else bytes(name or b"")
    if len(name_bytes) > 255 or b"\0" in name_bytes:
        raise ValueError("name must be at most 255 bytes without a NUL")
    if not np.isfinite(dense).all():
        raise ValueError("a value is NaN or infinite")
    if not (dense != 0).any():
        raise ValueError("no active voxel")

    # ---- the 8^3 bricks of the leaf lattice the box touches ----
    l0 = origin >> 3
    ln = ((origin + dims - 1) >> 3) - l0 + 1
    padded = np.zeros(tuple(8 * ln), np.float32)
    off = origin - 8 * l0
    padded[off[0] : off[0] + dims[0], off[1] : off[1] + dims[1], off[2] : off[2] + dims[2]] = dense
    bricks = padded.reshape(ln[0], 8, ln[1], 8, ln[2], 8).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 8, 8, 8)
    act = bricks != 0
    count = act.reshape(len(bricks), -1).sum(axis=1)
    keep = np.flatnonzero(count > 0)
    lc = np.stack(np.unravel_index(keep, tuple(ln)), axis=1).astype(np.int64) + l0  # leaf coordinates (index >> 3)
    # breadth-first order: the upper node (tile coordinate), the lower node in it, the leaf in that: each x-major, so the
    # order is lexicographic in (index >> 12, index >> 7, index >> 3) per level
    order = np.lexsort((lc[:, 2], lc[:, 1], lc[:, 0], lc[:, 2] >> 4, lc[:, 1] >> 4, lc[:, 0] >> 4, lc[:, 2] >> 9, lc[:, 1] >> 9, lc[:, 0] >> 9))
    keep, lc = keep[order], lc[order]
    values, act, count = bricks[keep].copy(), act[keep], count[keep]
    values[~act] = 0.0  # (-0.0f is inactive and reads back as +0)
    n_leaf = len(keep)

    leaves = np.zeros(n_leaf, LEAF)
    lo, hi = np.zeros((n_leaf, 3), np.int64), np.zeros((n_leaf, 3), np.int64)
    for axis in range(3):
        along = act.any(axis=tuple(a for a in (1, 2, 3) if a != axis + 1))  # (n, 8)
        lo[:, axis] = along.argmax(axis=1)
        hi[:, axis] = 7 - along[:, ::-1].argmax(axis=1)
    leaves["bbox_dif"] = hi - lo
    lo += 8 * lc
    hi += 8 * lc
    leaves["bbox_min"] = lo
    leaves["flags"] = 2
    leaves["value_mask"] = np.packbits(act.reshape(n_leaf, 512), axis=1, bitorder="little")
    leaf_min = np.where(act, values, np.float32(np.inf)).reshape(n_leaf, -1).min(axis=1)
    leaf_max = np.where(act, values, np.float32(-np.inf)).reshape(n_leaf, -1).max(axis=1)
    leaves["min"], leaves["max"] = leaf_min, leaf_max
    leaves["values"] = values.reshape(n_leaf, 512)

    # ---- lower nodes, upper nodes, root tiles: runs of equal parent coordinate in the order above ----
    low_first, low_of_leaf = _groups(lc >> 4)
    low_c = (lc >> 4)[low_first]
    low_lo, low_hi, low_min, low_max = _reduce(low_first, lo, hi, leaf_min, leaf_max)
    up_first, up_of_low = _groups(low_c >> 5)
    up_c = (low_c >> 5)[up_first]
    up_lo, up_hi, up_min, up_max = _reduce(up_first, low_lo, low_hi, low_min, low_max)
    n_low, n_up = len(low_first), len(up_first)
    if n_up > MAX_TILES:
        raise ValueError("more than 65536 root tiles")
    root_off = GRID_BYTES + TREE_BYTES
    up_off = root_off + ROOT_BYTES + TILE_BYTES * n_up
    low_off = up_off + UPPER_BYTES * n_up
    leaf_off = low_off + LOWER_BYTES * n_low
    total = leaf_off + LEAF_BYTES * n_leaf
    if total > MAX_BYTES:
        raise ValueError("the grid has more than 0xFFFFFFF0 bytes")

    def internal(dtype, bits, n, first_lo, first_hi, mn, mx, child_c, parent_of_child, self_off, self_bytes, child_off, child_bytes):
        nodes = np.zeros(n, dtype)
        nodes["bbox"][:, :3], nodes["bbox"][:, 3:] = first_lo, first_hi
        nodes["flags"] = 2
        nodes["min"], nodes["max"] = mn, mx
        mask = (1 << bits) - 1
        slot = ((child_c[:, 0] & mask) << (2 * bits)) | ((child_c[:, 1] & mask) << bits) | (child_c[:, 2] & mask)
        child = np.arange(len(child_c), dtype=np.int64)
        nodes["table"][parent_of_child, slot] = (child_off + child_bytes * child) - (self_off + self_bytes * parent_of_child)  # relative to the node itself
        bitsarr = np.zeros((n, 1 << (3 * bits)), np.uint8)
        bitsarr[parent_of_child, slot] = 1
        nodes["child_mask"] = np.packbits(bitsarr, axis=1, bitorder="little")
        return nodes

    lowers = internal(LOWER, 4, n_low, low_lo, low_hi, low_min, low_max, lc, low_of_leaf, low_off, LOWER_BYTES, leaf_off, LEAF_BYTES)
    uppers = internal(UPPER, 5, n_up, up_lo, up_hi, up_min, up_max, low_c, up_of_low, up_off, UPPER_BYTES, low_off, LOWER_BYTES)

    tiles = np.zeros(n_up, TILE)
    t = (up_c & 0xFFFFF).astype(np.uint64)  # ((uint32)index >> 12: 20 bits per axis)
    tiles["key"] = t[:, 2] | (t[:, 1] << np.uint64(21)) | (t[:, 0] << np.uint64(42))
    tiles["child"] = up_off + UPPER_BYTES * np.arange(n_up, dtype=np.int64) - root_off  # relative to the root
    root = np.zeros(1, ROOT)
    bmin, bmax = up_lo.min(axis=0), up_hi.max(axis=0)
    root["bbox"][0, :3], root["bbox"][0, 3:] = bmin, bmax
    root["table_size"] = n_up
    root["min"], root["max"] = up_min.min(), up_max.max()

    tree = np.zeros(1, TREE)
    tree["node_offset"][0] = [leaf_off - GRID_BYTES, low_off - GRID_BYTES, up_off - GRID_BYTES, root_off - GRID_BYTES]
    tree["node_count"][0] = [n_leaf, n_low, n_up]
    tree["voxel_count"] = int(count.sum())

    g = np.zeros(1, GRID)
    g["magic"], g["checksum"], g["version"], g["flags"], g["grid_count"], g["grid_size"] = MAGIC, 0xFFFFFFFFFFFFFFFF, VERSION, FLAGS, 1, total
    g["name"] = name_bytes
    inv = 1.0 / vs
    for k in (0, 4, 8):
        g["matf"][0, k], g["invmatf"][0, k], g["matd"][0, k], g["invmatd"][0, k] = np.float32(vs), np.float32(inv), vs, inv
    g["vecf"][0], g["vecd"][0], g["taperf"], g["taperd"] = tr.astype(np.float32), tr, 1.0, 1.0
    g["world_bbox"][0, :3] = bmin.astype(np.float64) * vs + tr
    g["world_bbox"][0, 3:] = (bmax + 1).astype(np.float64) * vs + tr
    g["voxel_size"][0] = vs
    g["grid_class"], g["grid_type"] = 2, 1  # FogVolume, float
    out = np.concatenate([x.view(np.uint8).reshape(-1) for x in (g, tree, root, tiles, uppers, lowers, leaves)])
    assert out.size == total
    return out


def grid_info(grid_bytes):
    """What sthip_volume_info carries, read from a grid's bytes: sizes, boxes, min/max and the node counts."""
    b = np.ascontiguousarray(grid_bytes, dtype=np.uint8).reshape(-1)
    g = b[:GRID_BYTES].view(GRID)[0]
    tree = b[GRID_BYTES : GRID_BYTES + TREE_BYTES].view(TREE)[0]
    r0 = GRID_BYTES + int(tree["node_offset"][3])
    root = b[r0 : r0 + ROOT_BYTES].view(ROOT)[0]
    return {
        "bytes": int(b.size),
        "bbox_min": root["bbox"][:3].copy(),
        "bbox_max": root["bbox"][3:].copy(),
        "world_bbox": g["world_bbox"].copy(),
        "min": float(root["min"]),
        "max": float(root["max"]),
        "active_voxels": int(tree["voxel_count"]),
        "leaf_count": int(tree["node_count"][0]),
        "lower_count": int(tree["node_count"][1]),
        "upper_count": int(tree["node_count"][2]),
        "root_tiles": int(root["table_size"]),
    }
