"""The cases and the oracle of tests/test_terrain_edits_*.py: scene edits, compaction and face extraction on the device-built
shell terrains of depth 10, 12 and 14, where a brick coordinate has 7, 9 and 11 bits and 7, 9 and 11 levels lie above the bricks.
Everything a GPU test expects is computed here, without a GPU, from the procedural columns (vrc.shell_column) and the numpy
replays (edit_replay, region_replay, voxel_replay, face_replay); nothing here reads a device.  Not a test file.

A case works on a few WINDOWS: boxes of 48 x 48 x 64 voxels whose content before the edits is voxel_replay.column_region.  The
in-scene part of every edit of a case lies inside a window's CORE, the 16 x 16 x 32 voxels in its middle, so the 16 voxels of
margin on every side read back the untouched sibling bricks and the untouched children of the touched ancestors two levels above
the bricks.  A window's content after a batch is the replay applied to the window with shifted coordinates; the voxels of a window
that lie outside the map stay 0.  (Every operation of the three calls treats a voxel by that voxel's own content and the
operations before it, so replaying a window alone is replaying the scene there.)  The counts (skipped, voxels_changed,
bricks_touched, descriptors_added) are the whole scene's: 72 words per touched brick, 16 per touched node above, 1 for the root.

The windows of a depth: `central`, around the column (dim/2, dim/2) at the terrain's surface, its core across x = dim/2 and
y = dim/2 (every bit of the brick key flips between neighbouring bricks; four children of the root); `midair`, around
(dim/2, dim/2, dim/2), empty before the edits (new paths from the root down in all eight children of the root; left out where the
shell reaches it); `far`, whose core lies across x, y = dim - 1 and runs past the map (every high bit set; clipped and skipped
edits); `near`, whose core starts at negative coordinates; `random`, at a seeded place.

The batches of a depth, by name: set05, setmix, setmix2 (vrc_set_voxels: about 1500 edits over all the windows, a tenth of them
repeating an earlier position, a twentieth outside the map with the ends of int32 among them, half of them clears; the materials
{0, 5}, and {0, 5, 6, 7, -3} twice); fill, fill_empty, fill_solid (vrc_fill_boxes: the same 12 boxes of 1 to 40 voxels per axis
under the three `where` modes -- a pillar across the dim/2 planes on the central surface, a box across all three dim/2 planes in
mid-air, boxes that hang over the map's edges, one wholly outside); paste, paste_skip0 (vrc_write_regions: one block of
13 x 9 x 21 per window, one that overlaps the first, one wholly outside)."""
import functools
from types import SimpleNamespace

import numpy as np

import edit_replay as er
import face_replay as fr
import region_replay as rg
import voxel_replay as vr
import voxel_raycaster_amd as vrc

DEPTHS = (10, 12, 14)
CORE = np.array([16, 16, 32], np.int64)
MARGIN = 16
WINDOW = CORE + 2 * MARGIN                                     # 48 x 48 x 64
BLOCK = (13, 9, 21)                                            # the pasted blocks, x y z
CHUNK = (13, 9, 24)                                            # the face chunks of the pristine tree
CONTROL = (32, 32, 48)
MIXED = (5, 6, 7, -3)
I = np.int32
BATCHES = ("set05", "setmix", "setmix2", "fill", "fill_empty", "fill_solid", "paste", "paste_skip0")
FLAGS = {"fill": 0, "fill_empty": rg.WHERE_EMPTY, "fill_solid": rg.WHERE_SOLID, "paste": 0, "paste_skip0": rg.SKIP_ZERO}


@functools.lru_cache(maxsize=None)
def columns(depth):
    """(x, y) -> (lo, hi) of vrc.shell_column at the suite's seed, remembered"""
    return functools.lru_cache(maxsize=None)(lambda x, y: vrc.shell_column(depth, x, y))


def _surface(depth, x, y):
    dim = 1 << depth
    return columns(depth)(int(np.clip(x, 0, dim - 1)), int(np.clip(y, 0, dim - 1)))[1]


def _apart(lo_a, size_a, lo_b, size_b):
    return bool(((lo_a + size_a <= lo_b) | (lo_b + size_b <= lo_a)).any())


@functools.lru_cache(maxsize=None)
def windows(depth):
    """the windows of a depth: name, lo (the window's lowest voxel), core_lo, before int8[64][48][48], inside (the window's voxels
    that lie in the map)"""
    dim, h = 1 << depth, 1 << (depth - 1)
    cores = [("central", (h - 7, h - 9, _surface(depth, h, h) - 14)),
             ("midair", (h - 9, h - 7, h - 15)),
             ("far", (dim - 13, dim - 13, _surface(depth, dim - 1, dim - 1) - 14)),
             ("near", (-3, -3, _surface(depth, 0, 0) - 14))]
    rng = np.random.default_rng(1000 + depth)
    while True:
        x, y = (int(v) for v in rng.integers(64, dim - 128, size=2))
        if all(max(abs(x - c[0]), abs(y - c[1])) > 128 for _, c in cores):
            break
    cores.append(("random", (x, y, _surface(depth, x + 8, y + 8) - 14 - int(rng.integers(0, 5)))))
    out = []
    for name, c in cores:
        core_lo = np.array(c, np.int64)
        lo = core_lo - MARGIN
        before = vr.column_region(depth, lo, WINDOW, columns(depth))
        if name == "midair" and before.any():
            continue
        ax = [(np.arange(lo[a], lo[a] + WINDOW[a]) >= 0) & (np.arange(lo[a], lo[a] + WINDOW[a]) < dim) for a in range(3)]
        inside = ax[2][:, None, None] & ax[1][None, :, None] & ax[0][None, None, :]
        out.append(SimpleNamespace(name=name, lo=lo, core_lo=core_lo, before=before, inside=inside))
    for i, a in enumerate(out):
        assert WINDOW[0] <= 48 and WINDOW[1] <= 48 and WINDOW[2] <= 64
        for b in out[:i]:
            assert _apart(a.lo, WINDOW, b.lo, WINDOW), (a.name, b.name)
    return tuple(out)


def window(depth, name):
    return next(w for w in windows(depth) if w.name == name)


def window_lo(depth):
    return np.array([w.lo for w in windows(depth)], I)


# ---------------------------------------------------------------------------- the batches
def _set_batch(depth, seed, materials, n=1500):
    dim, ws = 1 << depth, windows(depth)
    rng = np.random.default_rng(seed)
    core = np.array([w.core_lo for w in ws])[rng.integers(0, len(ws), size=n)]
    p = core + rng.integers(0, CORE, size=(n, 3))
    dup = np.nonzero(rng.random(n) < 0.10)[0]                   # (duplicates and outsiders as edit_replay.random_batch makes them)
    dup = dup[dup > 0]
    p[dup] = p[(rng.random(len(dup)) * dup).astype(np.int64)]
    far = np.array([-1, dim, dim + 7, -9, 2 ** 31 - 1, -2 ** 31])
    for i in np.nonzero(rng.random(n) < 0.05)[0]:
        p[i, rng.integers(0, 3)] = far[rng.integers(0, len(far))]
    m = np.where(rng.random(n) < 0.5, 0, rng.choice(np.asarray(materials), size=n))
    return p.astype(I), m.astype(I)


def _fill_batch(depth):
    dim, h = 1 << depth, 1 << (depth - 1)
    rng = np.random.default_rng(3000 + depth)
    ws = windows(depth)
    c, f, n = window(depth, "central"), window(depth, "far"), window(depth, "near")
    top = int(c.core_lo[2] + CORE[2])
    s = _surface(depth, h, h)
    boxes = [((dim - 6, dim - 9, int(f.core_lo[2]) + 9), (40, 30, 12), 7),              # hangs over the map's edge on x and y
             ((dim, dim - 4, int(f.core_lo[2]) + 3), (5, 5, 5), 5),                     # wholly outside: skipped
             ((-35, -20, int(n.core_lo[2]) + 8), (40, 25, 9), 0)]                       # from negative coordinates; a clear
    if any(w.name == "midair" for w in ws):
        boxes.append(((h - 3, h - 4, h - 5), (9, 7, 11), 5))                            # across all three dim/2 planes
    k = 0
    while len(boxes) < 10:
        w = ws[k % len(ws)]
        k += 1
        lo = w.core_lo + rng.integers(0, CORE - 1, size=3)
        size = np.minimum(rng.integers(1, 41, size=3), w.core_lo + CORE - lo)
        # (the first round gives every window a box that is not a clear)
        m = MIXED[k % len(MIXED)] if k <= len(ws) else int(rng.choice([0, 0, 5, 6, 7, -3]))
        boxes.append((tuple(int(v) for v in lo), tuple(int(v) for v in size), m))
    # the pillar, across x = dim/2 and y = dim/2, of a material that stops a ray (the undo frames look at its top), behind the
    # boxes that could repaint it; then a clear that digs into its foot and into the surface
    boxes += [((h - 5, h - 4, s - 2), (10, 9, top - (s - 2)), 6), ((h - 2, h - 3, s - 6), (3, 5, 9), 0)]
    return (np.array([b[0] for b in boxes], I), np.array([b[1] for b in boxes], I), np.array([b[2] for b in boxes], I))


def _paste_batch(depth):
    rng = np.random.default_rng(4000 + depth)
    ws = windows(depth)
    room = CORE - np.array(BLOCK) + 1
    lo = [w.core_lo + rng.integers(0, room, size=3) for w in ws]
    for k, w in enumerate(ws):
        if w.name == "near":
            lo[k][:2] = w.core_lo[:2]                           # starts at negative x and y
        if w.name == "far":
            lo[k][:2] = w.core_lo[:2] + room[:2] - 1            # ends past the map on x and y
    # one more overlaps the first window's block (the order decides), the last one lies wholly outside: skipped
    lo.append(np.clip(lo[0] + rng.integers(-2, 3, size=3), ws[0].core_lo, ws[0].core_lo + room - 1))
    lo.append(np.array([(1 << depth) + 2, 5, lo[0][2]]))
    data = rng.choice(np.array(MIXED, np.int8), size=(len(lo), BLOCK[2], BLOCK[1], BLOCK[0]))
    data[rng.random(data.shape) < 0.5] = 0
    return np.array(lo, I), data


@functools.lru_cache(maxsize=None)
def batch(depth, name):
    """(kind, arguments of the call, flags): kind is set_voxels, fill_boxes or write_regions"""
    if name.startswith("set"):
        args = _set_batch(depth, 2000 + 10 * depth + BATCHES.index(name), (5,) if name == "set05" else MIXED)
        out = ("set_voxels", args, 0)
    elif name.startswith("fill"):
        out = ("fill_boxes", _fill_batch(depth), FLAGS[name])
    elif name == "undo":
        return ("write_regions", undo_batch(depth), 0)
    else:
        out = ("write_regions", _paste_batch(depth), FLAGS[name])
    _assert_inside_cores(depth, out)
    return out


def _boxes_of(b):
    """(lo, size) (n, 3) int64 of the operations of a batch"""
    kind, args, _ = b
    lo = np.asarray(args[0], np.int64).reshape(-1, 3)
    if kind == "set_voxels":
        return lo, np.ones_like(lo)
    return lo, np.broadcast_to(np.asarray(args[1].shape[:0:-1] if kind == "write_regions" else args[1], np.int64), lo.shape)


def _assert_inside_cores(depth, b):
    dim = 1 << depth
    for lo, size in zip(*_boxes_of(b)):
        c = rg._clip(lo, size, (dim,) * 3)
        if c is not None:
            assert any((np.array(c[0]) >= w.core_lo).all() and (np.array(c[1]) <= w.core_lo + CORE).all() for w in windows(depth)), (lo, size)


def expanded(depth, name):
    """the vrc_set_voxels batch that gives the result of a fill or a paste with flags = 0"""
    kind, args, flags = batch(depth, name)
    assert flags == 0
    dims = (1 << depth,) * 3
    return rg.expand_fill(*args, dims) if kind == "fill_boxes" else rg.expand_paste(*args, dims)


def undo_batch(depth):
    """the vrc_write_regions call that puts every window back as it was"""
    return window_lo(depth), np.stack([w.before for w in windows(depth)])


# ---------------------------------------------------------------------------- the oracle
def touched_bricks(depth, b):
    """(k, 3) the lowest voxels of the bricks the in-scene part of a batch touches, and the number of skipped operations"""
    dim = 1 << depth
    lo, size = _boxes_of(b)
    if b[0] == "set_voxels":
        ok = ((lo >= 0) & (lo < dim)).all(axis=1)
        return np.unique(lo[ok] >> 3 << 3, axis=0), int((~ok).sum())
    skipped = sum(rg._clip(l, s, (dim,) * 3) is None for l, s in zip(lo, size))
    return rg.brick_corners(lo, size, (dim,) * 3), int(skipped)


def apply(depth, w, current, b):
    """(the window after the batch, the voxels it changed there)"""
    dim = 1 << depth
    kind, args, flags = b
    if kind == "set_voxels":
        p = np.asarray(args[0], np.int64)
        ok = ((p >= 0) & (p < dim)).all(axis=1)
        after = er.replay(current, p[ok] - w.lo, args[1][ok])[0]
    elif kind == "fill_boxes":
        after = rg.fill(current, np.asarray(args[0], np.int64) - w.lo, args[1], args[2], flags)[0]
    else:
        after = rg.paste(current, np.asarray(args[0], np.int64) - w.lo, args[1], flags)[0]
    after[~w.inside] = 0
    return after, int(np.count_nonzero(after != current))


@functools.lru_cache(maxsize=None)
def expected(depth, names):
    """The batches `names` (a tuple) sent one after the other to a pristine tree: per batch grids (the windows afterwards), the
    four counts of the whole scene, changed (per window) and the touched bricks"""
    dim = 1 << depth
    grids = [w.before for w in windows(depth)]
    out = []
    for name in names:
        b = batch(depth, name)
        done = [apply(depth, w, g, b) for w, g in zip(windows(depth), grids)]
        grids = [d[0] for d in done]
        changed = sum(d[1] for d in done)
        corners, skipped = touched_bricks(depth, b)
        bricks, above = er.touched_nodes(corners, dim)
        counts = dict(skipped=skipped, voxels_changed=changed, bricks_touched=bricks if changed else 0,
                      descriptors_added=72 * bricks + 16 * above + 1 if changed else 0)
        out.append(SimpleNamespace(name=name, grids=grids, counts=counts, changed=[d[1] for d in done], corners=corners))
    return out


def brick_keys(corners):
    """the brick keys of touched_bricks' corners, one bit at a time"""
    keys = []
    for x, y, z in (np.asarray(corners, np.int64) >> 3):
        keys.append(sum(((int(x) >> k & 1) << 3 * k) | ((int(y) >> k & 1) << 3 * k + 1) | ((int(z) >> k & 1) << 3 * k + 2) for k in range(21)))
    return keys


def points_of(depth, b):
    """the positions a batch names (set_voxels) or a sample of the positions its operations cover, (n, 3) int32"""
    lo, size = _boxes_of(b)
    if b[0] == "set_voxels":
        return np.asarray(b[1][0], I)
    rng = np.random.default_rng(len(lo) + depth)
    return np.concatenate([l + rng.integers(0, s, size=(40, 3)) for l, s in zip(lo, size)]).astype(I)


def read_points(depth, grids, p):
    """the materials of the positions p in the windows `grids`; every in-map position must lie in a window"""
    dim = 1 << depth
    p = np.asarray(p, np.int64)
    out = np.zeros(len(p), I)
    found = ~((p >= 0) & (p < dim)).all(axis=1)
    for w, g in zip(windows(depth), grids):
        q = p - w.lo
        here = ((q >= 0) & (q < WINDOW)).all(axis=1) & ~found
        out[here] = g[q[here, 2], q[here, 1], q[here, 0]]
        found |= here
    assert found.all()
    return out


@functools.lru_cache(maxsize=None)
def control(depth):
    """(lo (32, 3), the blocks of CONTROL voxels there, points above, in and below the shells, their materials): places away from
    every window, which no case touches"""
    dim = 1 << depth
    rng = np.random.default_rng(5000 + depth)
    lo = []
    while len(lo) < 32:
        x, y = (int(v) for v in rng.integers(0, dim - 32, size=2))
        c = np.array([x, y, _surface(depth, x + 16, y + 16) - int(rng.integers(8, 40))], np.int64)
        if all(_apart(c, np.array(CONTROL), w.lo, WINDOW) for w in windows(depth)):
            lo.append(c)
    lo = np.array(lo, I)
    blocks = np.stack([vr.column_region(depth, c, CONTROL, columns(depth)) for c in lo])
    pts = []
    for x, y, _ in lo[:16]:
        c0, c1 = columns(depth)(int(x), int(y))
        pts += [(x, y, z) for z in (c0 - 1, c0, (c0 + c1) // 2, c1, c1 + 1, 0, dim - 1, dim, -1)]
    pts = np.array(pts, I)
    col = [columns(depth)(int(x), int(y)) for x, y, _ in pts]
    want = np.array([5 if (c0 <= z <= c1 and 0 <= z < dim) else 0 for (c0, c1), (_, _, z) in zip(col, pts)], I)
    for p in pts:
        assert all(_apart(p.astype(np.int64), np.ones(3, np.int64), w.lo, WINDOW) for w in windows(depth))
    return lo, blocks, pts, want


# ---------------------------------------------------------------------------- faces
@functools.lru_cache(maxsize=None)
def chunks(depth):
    """lo (24, 3) of the face chunks of the pristine tree: 12 at coordinates >= dim/2, 4 across the map's edges and corners"""
    dim, h = 1 << depth, 1 << (depth - 1)
    rng = np.random.default_rng(6000 + depth)
    xy = np.concatenate([rng.integers(0, h - 13, size=(12, 2)), rng.integers(h, dim - 13, size=(12, 2))])
    xy[:2] = [(-7, h // 3), (0, 0)]
    xy[12:14] = [(dim - 5, dim - 4), (dim - 13, h + 3)]
    z = [_surface(depth, x + 6, y + 4) - int(rng.integers(4, 20)) for x, y in xy]
    return np.column_stack([xy, z]).astype(I)


def chunk_faces(depth, no_map_edge):
    return fr.column_regions(depth, chunks(depth), CHUNK, columns(depth), no_map_edge)


def core_lo(depth):
    return np.array([w.core_lo for w in windows(depth)], I)


def core_faces(depth, grids, no_map_edge, stopping_only):
    """(counts, faces) of vrc_extract_faces of every window's core, the one-voxel apron read from the same window"""
    lists = []
    for w, g in zip(windows(depth), grids):
        a, b = MARGIN - 1, MARGIN + CORE + 1
        block = g[a:b[2], a:b[1], a:b[0]].transpose(2, 1, 0)
        lists.append(fr.block_faces(block, w.core_lo, 1 << depth, no_map_edge, stopping_only))
    return fr.packed(lists)


# ---------------------------------------------------------------------------- the undo frames' camera
def pillar_camera(depth):
    """(cam_dir, cam_pos): the suite's direction (inclination 2.0, azimuth pi/2: along +y, downwards), the centre ray into the
    top of the fill batch's pillar, from 20 voxels of y away: what the frame sees of the scene is the pillar or,
    without it, the ground under it.  The line of sight is empty in the window before the edits."""
    h = 1 << (depth - 1)
    w = window(depth, "central")
    top = int(w.core_lo[2] + CORE[2])                           # the pillar ends at top - 1
    d = np.array([0.0, np.sin(2.0), np.cos(2.0)])
    target = np.array([h + 0.37, h + 0.41, top - 1.5])
    pos = target - d * (20 / d[1])
    for t in np.linspace(0.0, 1.0, 200):
        q = np.floor(pos + (target - pos) * t).astype(np.int64) - w.lo
        assert (q >= 0).all() and (q < WINDOW).all() and w.before[q[2], q[1], q[0]] == 0, (depth, t, q)
    return np.array([2.0, 1.5708], np.float32), pos.astype(np.float32)


def first_stop(depth, grid):
    """((x, y, z), material) of the first voxel of material 5 or 6 -- those stop a ray -- that the centre ray of pillar_camera
    meets in the central window `grid`, or None where it leaves the window first"""
    w = window(depth, "central")
    _, pos = pillar_camera(depth)
    d = np.array([0.0, np.sin(2.0), np.cos(2.0)])
    for t in np.arange(0.0, 100.0, 0.01):
        q = np.floor(pos.astype(np.float64) + d * t).astype(np.int64) - w.lo
        if not ((q >= 0).all() and (q < WINDOW).all()):
            return None
        if grid[q[2], q[1], q[0]] in (5, 6):
            return tuple(int(v) for v in q + w.lo), int(grid[q[2], q[1], q[0]])
    return None
