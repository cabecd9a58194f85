"""numpy restatement of a swept-box query (vrc_sweep_boxes, include/vrc.h): the start test, the event loop in float32 (every
event time from the current integer bound), the stops and the rejections, on a dense material grid (box_replay.GridReplay) or,
for device-built shell terrains, on the procedural columns (ColumnScene).  The test oracle of tests/test_sweep_queries_*.py.
Not a test file.

The sweeps of a batch advance in lock step, one event per pass, so a pass is a handful of array operations; a scene only has
to count the counted voxels of clipped ranges (count) and name the first one in Morton order (first)."""
import numpy as np

import box_replay as br

F = np.float32
HIT, START_SOLID, CLIPPED, REJECTED, EVENT_CAP, LEFT_MAP = 1, 2, 4, 8, 16, 32
LIMIT = br.LIMIT


class GridScene:
    """A dense material grid mat[x, y, z] (box_replay.GridReplay: the summed-volume table and the Morton-sorted voxels)."""

    def __init__(self, mat_xyz, stopping_only=False):
        self.g = br.GridReplay(mat_xyz, stopping_only)
        self.dims = self.g.dims

    def count(self, lo, hi):
        return self.g.count(lo, hi)

    def first(self, lo, hi):
        return self.g.first_voxels(lo, hi, 1)[0]


class ColumnScene:
    """A device-built shell terrain of 2^depth: column (x, y) is solid for lo <= z <= hi, material 5 (columns: callable
    (x, y) -> (lo, hi), e.g. vrc.shell_column).  For a few sweeps of small faces: it asks for every column of a range."""

    def __init__(self, depth, columns):
        self.dims = np.array([1 << depth] * 3, dtype=np.int64)
        self.columns = columns

    def count(self, lo, hi):
        out = np.zeros(len(lo), dtype=np.int64)
        for i in range(len(lo)):
            for x in range(lo[i, 0], hi[i, 0]):
                for y in range(lo[i, 1], hi[i, 1]):
                    c0, c1 = self.columns(int(x), int(y))
                    out[i] += max(0, min(c1 + 1, hi[i, 2]) - max(c0, lo[i, 2]))
        return out

    def first(self, lo, hi):
        return br.column_list(lo, hi, self.columns, 1)[0]


def sweep_ranges(sweeps):
    """o, e, d (n, 3) float32 (zeroed where rejected), the start lo, hi (n, 3) int64, and the rejected mask."""
    s = np.ascontiguousarray(sweeps, dtype=F).reshape(-1, 9)
    o, m, d = s[:, :3].copy(), s[:, 3:6], s[:, 6:].copy()
    with np.errstate(all="ignore"):
        e = (o + m).astype(F)                                   # o + m rounded to float32
        od, ed = (o + d).astype(F), (e + d).astype(F)
        rej = (~np.isfinite(s).all(axis=1) | (m < 0).any(axis=1) | ~(np.abs(o) < LIMIT).all(axis=1) | ~(np.abs(e) < LIMIT).all(axis=1)
               | ~(np.abs(od) < LIMIT).all(axis=1) | ~(np.abs(ed) < LIMIT).all(axis=1))
    o[rej] = 0
    e[rej] = 0
    d[rej] = 0
    lo = np.floor(o).astype(np.int64)
    hi = np.maximum(np.ceil(e).astype(np.int64), lo + 1)
    return o, e, d, lo, hi, rej


def sweep_replay(scene, sweeps, max_events=0, trace=None):
    """records (n, 8) int32.  trace: a dict that receives 'min_width' (n,), the smallest hi - lo any axis had, per sweep."""
    o, e, d, lo, hi, rej = sweep_ranges(sweeps)
    n = len(o)
    dims = np.asarray(scene.dims, dtype=np.int64)
    cap = int(max_events) if max_events > 0 else int(2 * dims.sum() + 64)
    rec = np.zeros((n, 8), dtype=np.int32)
    rec[:, 3:6] = -1
    flags = np.where(rej, REJECTED, 0).astype(np.int64)
    t = np.zeros(n, dtype=F)
    t_last = np.zeros(n, dtype=F)
    events = np.zeros(n, dtype=np.int64)
    clipped = ((lo < 0) | (hi > dims)).any(axis=1) & ~rej
    width = (hi - lo).min(axis=1)

    def clip(l, h):
        cl = np.minimum(np.maximum(l, 0), dims)
        return cl, np.maximum(np.minimum(h, dims), cl)

    # the start test
    cl, ch = clip(lo, hi)
    solid = ~rej & (scene.count(cl, ch) > 0)
    for i in np.nonzero(solid)[0]:
        rec[i, 3:7] = scene.first(cl[i], ch[i])
    flags[solid] |= START_SOLID
    active = ~rej & ~solid
    t[active] = F(1.0)
    rows = np.arange(n)
    while active.any():
        idx = rows[active]
        L, H, D = lo[idx], hi[idx], d[idx]
        left = (((H <= 0) & (D <= 0)) | ((L >= dims) & (D >= 0))).any(axis=1)
        flags[idx[left]] |= LEFT_MAP
        active[idx[left]] = False
        idx = idx[~left]
        if not len(idx):
            continue
        L, H, D, O, E = lo[idx], hi[idx], d[idx], o[idx], e[idx]
        k = len(idx)
        bt = np.zeros(k, dtype=F)
        code = np.full(k, -1, dtype=np.int64)
        with np.errstate(all="ignore"):
            for lead in (0, 1):                                  # trailing x y z, then leading x y z: the first strictly smallest
                for a in range(3):
                    da = D[:, a]
                    if lead:
                        pos = ((H[:, a]).astype(F) - E[:, a]) / da
                        neg = (O[:, a] - (L[:, a]).astype(F)) / (-da)
                    else:
                        pos = ((L[:, a] + 1).astype(F) - O[:, a]) / da
                        neg = (E[:, a] - (H[:, a] - 1).astype(F)) / (-da)
                    tt = np.where(da > 0, pos, neg).astype(F)
                    take = (da != 0) & ((code < 0) | (tt < bt))
                    bt = np.where(take, tt, bt).astype(F)
                    code = np.where(take, 4 * lead + a, code)
        free = (code < 0) | ~(bt < F(1.0))
        active[idx[free]] = False
        capped = ~free & (events[idx] == cap)
        flags[idx[capped]] |= EVENT_CAP
        t[idx[capped]] = t_last[idx[capped]]
        active[idx[capped]] = False
        go = ~free & ~capped
        idx, L, H, D, bt, code = idx[go], L[go], H[go], D[go], bt[go], code[go]
        if not len(idx):
            continue
        k = len(idx)
        events[idx] += 1
        t_last[idx] = bt
        axis, lead = code & 3, (code >> 2).astype(bool)
        r = np.arange(k)
        fwd = D[r, axis] > 0
        tr = ~lead
        lo[idx[tr & fwd], axis[tr & fwd]] += 1
        hi[idx[tr & ~fwd], axis[tr & ~fwd]] -= 1
        # leading: the slab of the layer entered, the other axes' current ranges, clipped to the map
        layer = np.where(fwd, H[r, axis], L[r, axis] - 1)
        sl, sh = np.maximum(L, 0), np.minimum(H, dims)
        sl[r, axis] = layer
        sh[r, axis] = layer + 1
        empty = (layer < 0) | (layer >= dims[axis]) | (sl >= sh).any(axis=1)
        test = lead & ~empty
        hit = np.zeros(k, dtype=bool)
        if test.any():
            hit[test] = scene.count(sl[test], sh[test]) > 0
        for j in np.nonzero(hit)[0]:
            i = idx[j]
            rec[i, 3:7] = scene.first(sl[j], sh[j])
            rec[i, 1] = -(axis[j] + 1) if fwd[j] else axis[j] + 1
            flags[i] |= HIT
            t[i] = bt[j]
            active[i] = False
        ext = lead & ~hit
        hi[idx[ext & fwd], axis[ext & fwd]] += 1
        lo[idx[ext & ~fwd], axis[ext & ~fwd]] -= 1
        clipped[idx] |= ((lo[idx] < 0) | (hi[idx] > dims)).any(axis=1)
        width[idx] = np.minimum(width[idx], (hi[idx] - lo[idx]).min(axis=1))
    flags[clipped] |= CLIPPED
    rec[:, 0] = flags
    rec[:, 2] = t.view(np.int32)
    rec[:, 7] = events
    if trace is not None:
        trace["min_width"] = width
    return rec


def random_sweeps(rng, n, dim):
    """Seeded sweeps of every kind the query must handle: tiny, player- and face-sized boxes, boxes larger than the map, starts
    outside, axis-aligned, diagonal, zero and subnormal displacement components, integer origins and extents, rejected ones."""
    o = rng.uniform(0, dim, size=(n, 3))
    ext = rng.uniform(0, 3, size=(n, 3))
    d = rng.normal(0, 0.15 * dim, size=(n, 3))
    kind = rng.integers(0, 12, size=n)
    k = kind == 0
    ext[k] = rng.uniform(0, 0.5, size=(int(k.sum()), 3))                       # tiny
    k = kind == 1
    ext[k] = (0.6, 0.6, 1.8)                                                   # player-sized, falling
    d[k, 2] = -2 * np.abs(d[k, 2])
    k = kind == 2
    ext[k] = rng.uniform(4, min(dim, 24), size=(int(k.sum()), 3))              # face-sized, half of them falling
    d[k, 2] = np.where(rng.integers(0, 2, size=int(k.sum())) == 0, d[k, 2], -2 * np.abs(d[k, 2]))
    k = kind == 3
    ext[k] = rng.uniform(dim, 1.5 * dim, size=(int(k.sum()), 3))               # larger than the map
    o[k] = rng.uniform(-0.75 * dim, 0.25 * dim, size=(int(k.sum()), 3))
    d[k] *= 0.1
    k = kind == 4
    o[k] = rng.uniform(-0.5 * dim, 1.5 * dim, size=(int(k.sum()), 3))          # starting anywhere, outside included
    d[k] = rng.normal(0, 0.6 * dim, size=(int(k.sum()), 3))
    k = np.nonzero(kind == 5)[0]
    keep = rng.integers(0, 3, size=len(k))                                     # axis-aligned
    for a in range(3):
        d[k[keep != a], a] = 0.0
    k = kind == 6
    d[k] = np.sign(d[k]) * np.abs(d[k][:, :1])                                 # diagonal
    k = kind == 7
    o[k] = np.floor(o[k])                                                      # integer origins and extents: resting contacts
    ext[k] = np.floor(ext[k]) + 1
    d[k] = np.round(d[k] * 0.2)
    k = np.nonzero(kind == 8)[0]
    ext[k, rng.integers(0, 3, size=len(k))] = 0.0                              # a plane; every other one a point
    ext[k[::2]] = 0.0
    k = np.nonzero(kind == 9)[0]
    d[k, rng.integers(0, 3, size=len(k))] = 0.0                                # a zero component; some do not move at all
    d[k[::3]] = 0.0
    k = np.nonzero(kind == 10)[0]
    d[k] *= 0.02                                                               # short moves
    s = np.concatenate([o, ext, d], axis=1).astype(F)
    k = np.nonzero(kind == 11)[0]
    s[k, 6 + rng.integers(0, 3, size=len(k))] = F(1e-41)                       # a subnormal component
    s[k[::2], 6] = F(-3e-39)
    bad = rng.choice(n, size=max(6, n // 60), replace=False)
    s[bad[0::6], 3] = F(-1.0)
    s[bad[1::6], 1] = F(np.nan)
    s[bad[2::6], 7] = F(np.inf)
    s[bad[3::6], 0] = F(2.0 ** 30)
    s[bad[4::6], 8] = F(-2.0 ** 30)
    s[bad[5::6], 6] = F(np.nan)
    return s
