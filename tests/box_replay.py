"""numpy restatement of a box query (vrc_box_intersection, include/vrc.h): the range rule, the clipping and rejection flags,
counts, corners and the Morton-ordered, truncated list, from a dense material grid (the frame's index, branch rule and
materials) or, for device-built shell terrains, from the procedural columns (vrc.shell_column).  The test oracle of
tests/test_box_queries_*.py.  Not a test file.

Counts come from a summed-volume table, corners from binary searches on it, lists from the scene's counted voxels sorted by
Morton key once and filtered by range; every max_voxels is a prefix of one full list."""
import numpy as np

F = np.float32
ANY, TRUNCATED, CLIPPED, REJECTED = 1, 2, 4, 8
LIMIT = F(2.0 ** 30)


def morton_key(xyz):
    """Key bit 3k = x bit k, 3k + 1 = y bit k, 3k + 2 = z bit k (the tree's child-slot order at every level)."""
    v = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    key = np.zeros(len(v), dtype=np.int64)
    for k in range(21):
        for a in range(3):
            key |= ((v[:, a] >> k) & 1) << (3 * k + a)
    return key


def box_ranges(boxes, map_dim):
    """Per box: clipped lo, hi (n, 3) int64 ([lo, hi) per axis, lo >= hi on an axis = nothing to examine), the flags
    (CLIPPED / REJECTED) and the rejected mask."""
    b = np.ascontiguousarray(boxes, dtype=F).reshape(-1, 6)
    o, m = b[:, :3], b[:, 3:]
    dims = np.asarray(map_dim, dtype=np.int64).reshape(3)
    with np.errstate(all="ignore"):
        e = (o + m).astype(F)                                 # o + m rounded to float32
        rej = (~np.isfinite(b).all(axis=1) | (m < 0).any(axis=1) | ~(np.abs(o) < LIMIT).all(axis=1)
               | ~(np.abs(e) < LIMIT).all(axis=1))
        lo = np.where(rej[:, None], 0, np.floor(np.where(np.isfinite(o), o, 0))).astype(np.int64)
        hi = np.where(rej[:, None], 0, np.ceil(np.where(np.isfinite(e), e, 0))).astype(np.int64)
    hi = np.maximum(hi, lo + 1)
    clipped = ((lo < 0) | (hi > dims)).any(axis=1) & ~rej
    lo_c, hi_c = np.maximum(lo, 0), np.minimum(hi, dims)
    lo_c[rej] = 0
    hi_c[rej] = 0
    flags = np.where(rej, REJECTED, 0) | np.where(clipped, CLIPPED, 0)
    return lo_c, hi_c, flags.astype(np.int32), rej


def brute_overlap(boxes, map_dim):
    """The range rule restated as an overlap test, voxel by voxel (small maps, a few boxes): voxel v counts on an axis when
    [v, v + 1) shares a point with [o, e), e = o + m in float32 -- for e > o that is v < e and v + 1 > o, for e = o the voxel
    holding o."""
    b = np.ascontiguousarray(boxes, dtype=F).reshape(-1, 6)
    dims = np.asarray(map_dim, dtype=np.int64).reshape(3)
    out = []
    for row in b:
        o, m = row[:3], row[3:]
        with np.errstate(all="ignore"):
            e = (o + m).astype(F)
        if (not np.isfinite(row).all() or (m < 0).any() or (np.abs(o) >= LIMIT).any() or (np.abs(e) >= LIMIT).any()):
            out.append(None)
            continue
        axes = []
        for a in range(3):
            v = np.arange(dims[a], dtype=np.float64)
            if e[a] == o[a]:                                 # (m = 0, or o + m rounded back to o)
                sel = v == np.floor(np.float64(o[a]))
            else:
                sel = (v < np.float64(e[a])) & (v + 1 > np.float64(o[a]))
            axes.append(np.nonzero(sel)[0])
        out.append(axes)
    return out


class GridReplay:
    """A scene given as its materials on a dense grid, mat[x, y, z] (the frame's hit test: the array branch's bytes, or the
    tree's materials -- the attachments, 5 without them)."""

    def __init__(self, mat_xyz, stopping_only=False):
        mat = np.asarray(mat_xyz)
        self.dims = np.array(mat.shape, dtype=np.int64)
        cnt = ((mat == 5) | (mat == 6)) if stopping_only else (mat != 0)
        sat = np.zeros(tuple(self.dims + 1), dtype=np.int64)
        sat[1:, 1:, 1:] = cnt.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
        self.sat = sat
        xyz = np.argwhere(cnt)
        key = morton_key(xyz)
        order = np.argsort(key, kind="stable")
        self.xyz, self.key = xyz[order], key[order]
        self.mat = mat[tuple(self.xyz.T)].astype(np.int32) if len(self.xyz) else np.zeros(0, np.int32)

    def count(self, lo, hi):
        s = self.sat
        x0, y0, z0 = lo.T
        x1, y1, z1 = hi.T
        return (s[x1, y1, z1] - s[x0, y1, z1] - s[x1, y0, z1] - s[x1, y1, z0]
                + s[x0, y0, z1] + s[x0, y1, z0] + s[x1, y0, z0] - s[x0, y0, z0])

    def query(self, boxes, max_voxels=0):
        """(records (n, 8) int32, counts (n,) int64, voxels (n, max_voxels, 4) int32 with -1 past each box's entries, or None)."""
        lo, hi, flags, rej = box_ranges(boxes, self.dims)
        n = len(lo)
        lo = np.minimum(lo, self.dims)
        hi = np.maximum(hi, lo)                                   # empty ranges count 0
        counts = self.count(lo, hi)
        counts[rej] = 0
        rec = np.full((n, 8), -1, dtype=np.int32)
        has = counts > 0
        # corners: per axis the first / last slab of the range holding a counted voxel (binary search on the table)
        for a in range(3):
            for side in (0, 1):
                L, H = lo[:, a].copy(), hi[:, a] - 1
                while True:
                    act = has & (L < H)
                    if not act.any():
                        break
                    mid = (L + H) // 2
                    l2, h2 = lo.copy(), hi.copy()
                    if side == 0:
                        h2[:, a] = mid + 1
                        found = self.count(l2, h2) > 0
                        H = np.where(act & found, mid, H)
                        L = np.where(act & ~found, mid + 1, L)
                    else:
                        l2[:, a] = mid + 1
                        found = self.count(l2, h2) > 0
                        L = np.where(act & found, mid + 1, L)
                        H = np.where(act & ~found, mid, H)
                rec[has, 1 + 3 * side + a] = L[has]
        f = flags | np.where(has, ANY, 0)
        if max_voxels > 0:
            f |= np.where(counts > max_voxels, TRUNCATED, 0)
        rec[:, 0] = f
        rec[:, 7] = np.minimum(counts, max_voxels)
        vox = None
        if max_voxels > 0:
            vox = np.full((n, max_voxels, 4), -1, dtype=np.int32)
            for i in np.nonzero(has)[0]:
                lst = self.first_voxels(lo[i], hi[i], min(int(counts[i]), max_voxels))
                vox[i, :len(lst)] = lst
        return rec, counts.astype(np.int64), vox

    def first_voxels(self, lo, hi, k):
        """The first k counted voxels of the range in Morton order, (k, 4) = x, y, z, material."""
        i0 = np.searchsorted(self.key, morton_key(lo)[0])
        i1 = np.searchsorted(self.key, morton_key(hi - 1)[0], side="right")
        got = []
        have = 0
        step = max(4096, 8 * k)
        for s in range(i0, i1, step):
            xyz = self.xyz[s: min(s + step, i1)]
            sel = ((xyz >= lo) & (xyz < hi)).all(axis=1)
            idx = np.nonzero(sel)[0][: k - have] + s
            got.append(np.concatenate([self.xyz[idx], self.mat[idx, None]], axis=1))
            have += len(idx)
            if have >= k:
                break
        return np.concatenate(got).astype(np.int32) if got else np.zeros((0, 4), np.int32)


def grid_xyz(grid, dim):
    """A scene's flat grid (index x + dim * (y + dim * z)) as mat[x, y, z]."""
    return np.asarray(grid, dtype=np.int8).reshape(dim, dim, dim).transpose(2, 1, 0)


def column_replay(boxes, depth, columns):
    """Counts and corners of boxes on a device-built shell terrain: column (x, y) is solid for lo <= z <= hi, material 5.
    columns: callable (x, y) -> (lo, hi).  Returns (records (n, 8), counts (n,)) without list fields ([7] = 0)."""
    dim = 1 << depth
    lo, hi, flags, rej = box_ranges(boxes, (dim,) * 3)
    n = len(lo)
    rec = np.full((n, 8), -1, dtype=np.int32)
    counts = np.zeros(n, dtype=np.int64)
    for i in range(n):
        if rej[i] or (lo[i] >= hi[i]).any():
            continue
        xs, ys = np.arange(lo[i, 0], hi[i, 0]), np.arange(lo[i, 1], hi[i, 1])
        X, Y = np.meshgrid(xs, ys, indexing="ij")
        LH = np.array([[columns(int(x), int(y)) for x, y in zip(X.ravel(), Y.ravel())]], dtype=np.int64).reshape(-1, 2)
        z0 = np.maximum(LH[:, 0], lo[i, 2])
        z1 = np.minimum(LH[:, 1] + 1, hi[i, 2])
        w = np.maximum(z1 - z0, 0)
        counts[i] = int(w.sum())
        if counts[i]:
            sel = w > 0
            rec[i, 1:4] = [X.ravel()[sel].min(), Y.ravel()[sel].min(), z0[sel].min()]
            rec[i, 4:7] = [X.ravel()[sel].max(), Y.ravel()[sel].max(), (z1[sel] - 1).max()]
    rec[:, 0] = flags | np.where(counts > 0, ANY, 0)
    rec[:, 7] = 0
    return rec, counts


def column_list(lo, hi, columns, k):
    """The first k voxels (Morton order) of a small box on a shell terrain, (k, 4) with material 5."""
    pts = []
    for x in range(lo[0], hi[0]):
        for y in range(lo[1], hi[1]):
            c0, c1 = columns(x, y)
            for z in range(max(c0, lo[2]), min(c1 + 1, hi[2])):
                pts.append((x, y, z))
    if not pts:
        return np.zeros((0, 4), np.int32)
    p = np.array(pts, dtype=np.int64)
    p = p[np.argsort(morton_key(p), kind="stable")][:k]
    return np.concatenate([p, np.full((len(p), 1), 5)], axis=1).astype(np.int32)


def random_boxes(rng, n, dim):
    """Seeded boxes of every kind the query must handle: extents 0 .. dim, fractional and integer origins, boxes partly and
    wholly outside, zero extents (planes, lines, points), and a few rejected ones."""
    o = rng.uniform(-0.25 * dim, 1.1 * dim, size=(n, 3))
    ext = dim * rng.uniform(0, 1, size=(n, 3)) ** 3
    kind = rng.integers(0, 8, size=n)
    o[kind == 1] = np.floor(o[kind == 1])                      # integer origins
    ext[kind == 2] = np.floor(ext[kind == 2])                  # integer extents
    z = kind == 3
    ext[z, rng.integers(0, 3, size=int(z.sum()))] = 0.0        # a zero extent
    ext[kind == 4] = 0.0                                       # a point
    ext[kind == 5] = rng.uniform(0, 3, size=(int((kind == 5).sum()), 3))   # small
    o[kind == 6] = rng.uniform(0, dim, size=(int((kind == 6).sum()), 3))   # inside
    b = np.concatenate([o, ext], axis=1).astype(F)
    bad = rng.choice(n, size=max(1, n // 100), replace=False)
    b[bad[0::4], 3] = F(-1.0)
    b[bad[1::4], 1] = F(np.nan)
    b[bad[2::4], 5] = F(np.inf)
    b[bad[3::4], 0] = F(2.0 ** 30)
    return b
