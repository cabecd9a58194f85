"""numpy restatement of the region edits (vrc_fill_boxes / vrc_write_regions, include/vrc.h): the operations applied IN INDEX
ORDER to a dense material grid int8[z][y][x] -- the block vrc_read_regions returns for the whole scene --, each clipped to the
grid in Python integers (lo + size never wraps), each testing the WHERE_* flags against the grid as the operations before it left
it.  An operation that touches no voxel of the grid is skipped and counted.  Also the expansion of a batch into the single-voxel
batch vrc_set_voxels takes, the bricks a batch touches, and the random batches the tests share.  The test oracle of
tests/test_region_edits_cpu.py and tests/test_voxel_region_edits_gpu.py.  Not a test file."""
import numpy as np

WHERE_EMPTY, WHERE_SOLID, SKIP_ZERO = 1, 2, 4
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _clip(lo, size, dims_xyz):
    """the in-scene part [a, b) of the box, per axis, in Python integers; None when it is empty"""
    a = [max(int(l), 0) for l in lo]
    b = [min(int(l) + int(s), int(d)) for l, s, d in zip(lo, size, dims_xyz)]
    return (a, b) if all(x < y for x, y in zip(a, b)) else None


def _allowed(cur, flags):
    if flags & WHERE_EMPTY:
        return cur == 0
    if flags & WHERE_SOLID:
        return cur != 0
    return np.ones(cur.shape, bool)


def fill(grid_zyx, lo, size, materials, flags=0):
    """(grid after the batch, skipped, voxels_changed): lo (n, 3), size (n, 3) or one triple, materials (n,); grid_zyx is not
    modified."""
    assert flags in (0, WHERE_EMPTY, WHERE_SOLID)
    before = np.asarray(grid_zyx, dtype=np.int8)
    g = before.copy()
    lo = np.asarray(lo, dtype=np.int64).reshape(-1, 3)
    size = np.broadcast_to(np.asarray(size, dtype=np.int64), lo.shape)
    m = np.broadcast_to(np.asarray(materials, dtype=np.int64), (len(lo),))
    assert (size >= 1).all() and ((m >= -128) & (m <= 127)).all()
    dims = g.shape[::-1]
    skipped = 0
    for l, s, v in zip(lo, size, m):                        # one by one on purpose: the order is the specification
        c = _clip(l, s, dims)
        if c is None:
            skipped += 1
            continue
        (ax, ay, az), (bx, by, bz) = c
        view = g[az:bz, ay:by, ax:bx]
        view[_allowed(view, flags)] = v
    return g, skipped, int(np.count_nonzero(g != before))


def paste(grid_zyx, lo, data, flags=0):
    """(grid after the batch, skipped, voxels_changed): lo (n, 3), data int8 (n, sz, sy, sx), the shape read_regions returns."""
    assert flags & ~7 == 0 and flags & 3 != 3
    before = np.asarray(grid_zyx, dtype=np.int8)
    g = before.copy()
    lo = np.asarray(lo, dtype=np.int64).reshape(-1, 3)
    data = np.asarray(data)
    assert data.dtype == np.int8 and data.ndim == 4 and len(data) == len(lo)
    size = data.shape[:0:-1]
    dims = g.shape[::-1]
    skipped = 0
    for l, block in zip(lo, data):
        c = _clip(l, size, dims)
        if c is None:
            skipped += 1
            continue
        (ax, ay, az), (bx, by, bz) = c
        lx, ly, lz = (int(v) for v in l)
        src = block[az - lz:bz - lz, ay - ly:by - ly, ax - lx:bx - lx]
        view = g[az:bz, ay:by, ax:bx]
        ok = _allowed(view, flags)
        if flags & SKIP_ZERO:
            ok &= src != 0
        view[ok] = src[ok]
    return g, skipped, int(np.count_nonzero(g != before))


def expand_fill(lo, size, materials, dims_xyz):
    """(positions (k, 3) int32, materials (k,) int32): the in-scene voxels of every box, operation by operation -- the batch
    that gives vrc_set_voxels the same result as a fill with flags = 0."""
    lo = np.asarray(lo, dtype=np.int64).reshape(-1, 3)
    size = np.broadcast_to(np.asarray(size, dtype=np.int64), lo.shape)
    m = np.broadcast_to(np.asarray(materials, dtype=np.int64), (len(lo),))
    ps, ms = [np.zeros((0, 3), np.int32)], [np.zeros(0, np.int32)]
    for l, s, v in zip(lo, size, m):
        c = _clip(l, s, dims_xyz)
        if c is None:
            continue
        (ax, ay, az), (bx, by, bz) = c
        z, y, x = np.meshgrid(np.arange(az, bz), np.arange(ay, by), np.arange(ax, bx), indexing="ij")
        ps.append(np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.int32))
        ms.append(np.full(ps[-1].shape[0], v, np.int32))
    return np.concatenate(ps), np.concatenate(ms)


def expand_paste(lo, data, dims_xyz):
    """expand_fill for pasted blocks (flags = 0: every byte is written, zeros included)."""
    lo = np.asarray(lo, dtype=np.int64).reshape(-1, 3)
    data = np.asarray(data)
    size = data.shape[:0:-1]
    ps, ms = [np.zeros((0, 3), np.int32)], [np.zeros(0, np.int32)]
    for l, block in zip(lo, data):
        c = _clip(l, size, dims_xyz)
        if c is None:
            continue
        (ax, ay, az), (bx, by, bz) = c
        lx, ly, lz = (int(v) for v in l)
        z, y, x = np.meshgrid(np.arange(az, bz), np.arange(ay, by), np.arange(ax, bx), indexing="ij")
        ps.append(np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.int32))
        ms.append(block[az - lz:bz - lz, ay - ly:by - ly, ax - lx:bx - lx].reshape(-1).astype(np.int32))
    return np.concatenate(ps), np.concatenate(ms)


def brick_corners(lo, size, dims_xyz):
    """(k, 3): the lowest voxel of every map-aligned 8^3 brick that the in-scene part of an operation overlaps, each once --
    bricks_touched is their number, and edit_replay.touched_nodes of them gives the growth bound's counts."""
    lo = np.asarray(lo, dtype=np.int64).reshape(-1, 3)
    size = np.broadcast_to(np.asarray(size, dtype=np.int64), lo.shape)
    bricks = set()
    for l, s in zip(lo, size):
        c = _clip(l, s, dims_xyz)
        if c is None:
            continue
        (ax, ay, az), (bx, by, bz) = c
        for z in range(az >> 3, ((bz - 1) >> 3) + 1):
            for y in range(ay >> 3, ((by - 1) >> 3) + 1):
                for x in range(ax >> 3, ((bx - 1) >> 3) + 1):
                    bricks.add((8 * x, 8 * y, 8 * z))
    return np.array(sorted(bricks), dtype=np.int64).reshape(-1, 3)


def random_fills(rng, dim, n=40, materials=(5, 6, 7, -3, -128, 127)):
    """(lo (n, 3) int32, size (n, 3) int32, materials (n,) int32) for a dim^3 scene.  Every batch holds: boxes that overlap
    earlier boxes with another material (the order decides), boxes partly and wholly outside, negative corners, the box at
    lo = INT32_MIN with size INT32_MAX (it ends at -1: wholly outside) and one from INT32_MIN + 2 (it covers voxel 0 of every
    axis), a box that starts inside and has size INT32_MAX, clears (material 0) and negative materials."""
    assert n >= 16
    lo = rng.integers(0, dim, size=(n, 3))
    size = rng.integers(1, max(dim // 2, 2) + 1, size=(n, 3))
    m = rng.choice(np.asarray(materials), size=n)
    m[rng.random(n) < 0.3] = 0                                   # clears
    for i in range(4, n, 5):                                     # overlap an earlier box, shifted by a voxel, other material
        j = int(rng.integers(0, i))
        lo[i], size[i] = lo[j] + rng.integers(-1, 2, size=3), size[j]
        m[i] = -3 if m[j] != -3 else 0
    lo[1] = rng.integers(-dim, 0, size=3)                        # negative corner, reaches inside
    size[1] = -lo[1] + rng.integers(1, dim // 2 + 1, size=3)
    lo[2], size[2] = [dim - 1, -3, dim // 2], [5, 5, dim]        # partly outside on every axis
    lo[3], size[3] = [dim, 0, 0], [4, 4, 4]                      # wholly outside: touches the face
    lo[5], size[5] = [0, -9, 0], [dim, 9, dim]                   # wholly outside: ends at -1
    lo[6], size[6] = [INT32_MIN] * 3, [INT32_MAX] * 3            # ends at -1
    lo[7], size[7], m[7] = [INT32_MIN + 2] * 3, [INT32_MAX] * 3, -128
    lo[8], size[8], m[8] = [dim // 2, 0, dim - 1], [INT32_MAX, 1, INT32_MAX], 127
    m[9], m[10] = 0, -3
    return lo.astype(np.int32), size.astype(np.int32), m.astype(np.int32)


def random_pastes(rng, dim, n=12, size=None, zeros=0.5, materials=(5, 6, 7, -3, -128, 127)):
    """(lo (n, 3) int32, data int8 (n, sz, sy, sx)): random blocks of one odd, non-cubic size, about `zeros` of their bytes 0,
    at corners inside, overlapping each other, with negative coordinates, partly outside and (blocks 2 and 3) wholly outside."""
    assert n >= 6
    if size is None:
        size = (max(dim // 2 + 1, 2), max(dim // 4 + 1, 1), max(dim // 3 + 2, 2))
    sx, sy, sz = size
    data = rng.choice(np.asarray(materials, dtype=np.int8), size=(n, sz, sy, sx))
    data[rng.random(data.shape) < zeros] = 0
    lo = rng.integers(-2, dim, size=(n, 3))
    lo[0] = [-(sx // 2), -(sy // 2), -(sz // 2)]
    lo[1] = lo[0] + 1                                            # overlaps block 0
    lo[2] = [dim, 0, 0]
    lo[3] = [0, INT32_MIN, 0]
    lo[4] = [dim - 1, dim - 1, dim - 1]
    lo[5] = [INT32_MAX, 3, 3]                                    # lo + size passes 2^31
    return lo.astype(np.int32), data
