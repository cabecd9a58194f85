"""numpy and Python-integer restatement of the shape fills (vrc_fill_shapes, include/vrc.h): balls and axis-aligned cylinders
applied IN INDEX ORDER to a dense material grid int8[z][y][x], each clipped to the grid in Python integers (c + h and c - r never
wrap), each testing the WHERE_* flags against the grid as the operations before it left it.  Membership is the header's:

    ball                 (x - cx)^2 + (y - cy)^2 + (z - cz)^2 <= r^2                                   (h = 0)
    cylinder along a     c_a <= v_a < c_a + h, and the squared distance over the other two axes <= r^2   (kind = 1 + a, h >= 1)

A shape with no voxel in the grid is skipped and counted.  Also the expansion of a batch into the single-voxel batch
vrc_set_voxels takes, the bricks a batch touches -- by brute force over that expansion, not by the closed form of
csrc/shape_span.hpp --, and the random batches the tests share.  The test oracle of tests/test_shape_fills_cpu.py,
tests/test_voxel_shape_fills_gpu.py and tests/shape_audit_case.py.  Not a test file."""
import numpy as np

WHERE_EMPTY, WHERE_SOLID = 1, 2
BALL, CYLINDER_X, CYLINDER_Y, CYLINDER_Z = 0, 1, 2, 3
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
MAX_RADIUS = 2 ** 30


def dims3(dims):
    return (int(dims),) * 3 if np.ndim(dims) == 0 else tuple(int(d) for d in dims)


def valid(shape, material):
    kind, _, _, _, r, h = (int(v) for v in shape)
    return (0 <= kind <= 3 and 0 <= r <= MAX_RADIUS and (h == 0 if kind == BALL else h >= 1) and -128 <= int(material) <= 127)


def _voxels(shape, dims_xyz):
    """(lo, mask): the clipped bounding box's lowest voxel (x, y, z) and the shape's voxels inside it as bool[z][y][x]; None when
    the shape has no voxel in the scene"""
    kind, r, h = int(shape[0]), int(shape[4]), int(shape[5])
    c = [int(v) for v in shape[1:4]]
    lo, hi = [], []
    for a in range(3):
        a0, a1 = (c[a], c[a] + h) if kind == 1 + a else (c[a] - r, c[a] + r + 1)
        lo.append(max(a0, 0))
        hi.append(min(a1, dims_xyz[a]))
    if any(l >= u for l, u in zip(lo, hi)):
        return None
    # inside the clipped box |d| <= r on every radial axis: the squares are at most 2^60 and int64 holds their sum
    d2 = np.zeros((hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]), np.int64)
    for a in range(3):
        if kind == 1 + a:
            continue
        d = np.arange(lo[a], hi[a], dtype=np.int64) - c[a]
        d2 += (d * d).reshape([-1 if k == 2 - a else 1 for k in range(3)])
    mask = d2 <= r * r
    return (lo, mask) if mask.any() else None


def fill_shapes(grid_zyx, shapes, materials, flags=0):
    """(grid after the batch, skipped, voxels_changed): shapes (n, 6) = kind, cx, cy, cz, r, h; materials (n,) or one value;
    grid_zyx is not modified."""
    assert flags in (0, WHERE_EMPTY, WHERE_SOLID)
    before = np.asarray(grid_zyx, dtype=np.int8)
    g = before.copy()
    shapes = np.asarray(shapes, dtype=np.int64).reshape(-1, 6)
    m = np.broadcast_to(np.asarray(materials, dtype=np.int64), (len(shapes),))
    dims = g.shape[::-1]
    skipped = 0
    for s, v in zip(shapes, m):                              # one by one on purpose: the order is the specification
        assert valid(s, v), (s, v)
        got = _voxels(s, dims)
        if got is None:
            skipped += 1
            continue
        (x, y, z), mask = got
        view = g[z:z + mask.shape[0], y:y + mask.shape[1], x:x + mask.shape[2]]
        if flags & WHERE_EMPTY:
            mask = mask & (view == 0)
        if flags & WHERE_SOLID:
            mask = mask & (view != 0)
        view[mask] = v
    return g, skipped, int(np.count_nonzero(g != before))


def expand_shapes(shapes, materials, dims_xyz):
    """(positions (k, 3) int32, materials (k,) int32): the in-scene voxels of every shape, operation by operation -- the batch
    that gives vrc_set_voxels the same result as fill_shapes with flags = 0."""
    dims = dims3(dims_xyz)
    shapes = np.asarray(shapes, dtype=np.int64).reshape(-1, 6)
    m = np.broadcast_to(np.asarray(materials, dtype=np.int64), (len(shapes),))
    ps, ms = [np.zeros((0, 3), np.int32)], [np.zeros(0, np.int32)]
    for s, v in zip(shapes, m):
        got = _voxels(s, dims)
        if got is None:
            continue
        lo, mask = got
        zyx = np.argwhere(mask)
        ps.append((zyx[:, ::-1] + np.array(lo)).astype(np.int32))
        ms.append(np.full(len(zyx), v, np.int32))
    return np.concatenate(ps), np.concatenate(ms)


def brick_corners(shapes, dims_xyz, log2=3):
    """(k, 3): the lowest voxel of every map-aligned brick (8^3 unless log2 says otherwise) that holds at least one in-scene voxel
    of a shape, each once, sorted -- bricks_touched is their number."""
    p, _ = expand_shapes(shapes, np.zeros(len(np.asarray(shapes).reshape(-1, 6)), np.int64), dims_xyz)
    if not len(p):
        return np.zeros((0, 3), np.int64)
    return np.unique((p.astype(np.int64) >> log2) << log2, axis=0)


def batch(dims, k=0):
    """batch k of the scene `dims`: the one the GPU tests send and tests/test_shape_fills_cpu.py holds the input conditions of"""
    return random_shapes(np.random.default_rng(1700 + 10 * sum(dims3(dims)) + k), dims)


def random_shapes(rng, dims, n=28, materials=(5, 6, 7, -3, -128, 127)):
    """(shapes (n, 6) int32, materials (n,) int32) for a scene of `dims` (one number or (dx, dy, dz)).  Every batch holds all four
    kinds; every r of {0, 1, 7, 8, 9}; shapes around one centre with different materials (the order decides); clears and negative
    materials; centres outside the scene that reach in; shapes wholly outside, one of them with a bounding box that is not; the
    ball at (-2^30 + 3, 4, 4) with r = 2^30, a thin cap at x <= 3; a cylinder from INT32_MAX - 1 with h = INT32_MAX (c + h passes
    2^31); one from INT32_MIN with h = INT32_MAX (it ends at -1) and one from INT32_MIN + 2 (it covers coordinate 0 alone); a
    Z-cylinder with r = 0, a one-voxel column through brick (8, 8, *) where the scene has one -- a brick the bounding box of the
    ball before it holds and the ball does not."""
    assert n >= 24
    dx, dy, dz = dims3(dims)
    d = np.array([dx, dy, dz], np.int64)
    s = np.zeros((n, 6), np.int64)
    s[:, 0] = rng.integers(0, 4, size=n)
    s[:, 1:4] = rng.integers(0, d, size=(n, 3))
    s[:, 4] = rng.choice(np.array([0, 1, 7, 8, 9]), size=n)
    s[:, 5] = rng.integers(1, max(int(d.max()) // 2, 1) + 2, size=n)
    m = rng.choice(np.asarray(materials, dtype=np.int64), size=n)
    m[rng.random(n) < 0.3] = 0
    mid = d // 2
    for i, (kind, r) in enumerate(((BALL, 0), (CYLINDER_X, 1), (CYLINDER_Y, 7), (CYLINDER_Z, 8), (BALL, 9))):
        s[i, 0], s[i, 4] = kind, r
    s[5], m[5] = [BALL, 2, 2, 2, 8, 0], 6                        # its box holds brick (8, 8, 8), the ball does not
    s[6], m[6] = [CYLINDER_Z, min(9, dx - 1), min(9, dy - 1), 0, 0, dz], -3
    s[7], m[7] = [BALL, *mid, 7, 0], 7                           # three around one centre: the order decides
    s[8], m[8] = [CYLINDER_X, mid[0] - 3, mid[1], mid[2], 1, 7], 0
    s[9], m[9] = [BALL, *mid, 1, 0], -128
    s[10], m[10] = [BALL, -3, mid[1], mid[2], 7, 0], 127         # centres outside that reach in
    s[11], m[11] = [CYLINDER_Y, mid[0], -5, mid[2], 1, 9], 5
    s[12] = [BALL, dx + 20, 0, 0, 9, 0]                          # wholly outside
    s[13], m[13] = [BALL, -6, -6, -6, 9, 0], 7                   # its box reaches (3, 3, 3); its nearest voxel is at 108 > 81
    s[14], m[14] = [BALL, -2 ** 30 + 3, 4, 4, 2 ** 30, 0], 5
    s[15] = [CYLINDER_X, INT32_MAX - 1, mid[1], mid[2], 7, INT32_MAX]
    s[16] = [CYLINDER_Y, mid[0], INT32_MIN, mid[2], 8, INT32_MAX]
    s[17], m[17] = [CYLINDER_Z, mid[0], mid[1], INT32_MIN + 2, 1, INT32_MAX], -3
    s[18], m[18] = [BALL, *rng.integers(0, d), 9, 0], 0          # a crater
    m[19] = -3
    s[s[:, 0] == BALL, 5] = 0
    return s.astype(np.int32), m.astype(np.int32)
