"""numpy float32 restatement of a ray query (vrc_cast_rays, include/vrc.h): the set-up of ray_setup without the table rotation,
the step loop t += dt * mask (the mask is 0 / 1: a select, exact) and the stop rule on a dense material grid, vectorised over rays.
The test oracle of tests/test_ray_queries_*.py.  Not a test file."""
import numpy as np

F = np.float32
HIT, LEFT_MAP, STEP_CAP, REJECTED = 1, 2, 4, 8


def c_div2(v):
    """C's int / 2 (truncates toward zero)."""
    return np.where(v < 0, -((-v) // 2), v // 2)


def origin_bias(origins, descriptors, root_index, dim, enabled=True):
    """The octree bias of ray_caster_kernel.cl:342-354 for a camera at each origin (what frame_setup_kernel computes), via the
    oracle's get_oct_vox: (sub_oct_pos - voxel) * resolution / 2 per axis."""
    from oracle import orc
    o = np.asarray(origins, dtype=F).reshape(-1, 3)
    out = np.zeros((len(o), 3), dtype=np.int64)
    if not enabled:
        return out
    cache = {}
    for k, p in enumerate(np.floor(o).astype(np.int64)):
        key = tuple(int(x) for x in p)
        if key not in cache:
            ts = orc.get_oct_vox(key, descriptors, root_index, dim)
            cache[key] = c_div2((np.array(ts.sub_oct_pos[:3], dtype=np.int64) - np.array(key)) * int(ts.resolution))
        out[k] = cache[key]
    return out


def replay(rays, materials, map_dim, max_steps=0, as_pixel=False, bias=None):
    """rays (n, 6) float32; materials: the grid the ray reads, flat, index x + dx * (y + dz * z) (the reference's array-branch
    index; an index past the array reads 0); for the SVO branch the tree's materials (5 where it is solid without attachments).
    bias: (n, 3) or (3,) ints added to t (AS_PIXEL), None = 0.  Returns the (n, 8) int32 records."""
    r = np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)
    n = len(r)
    as_pixel = bool(as_pixel)
    dims = np.asarray(map_dim, dtype=np.int64).reshape(3)
    mat = np.ascontiguousarray(materials).reshape(-1)
    o, d = r[:, :3], r[:, 3:]
    rec = np.zeros((n, 8), dtype=np.int32)
    rec[:, :3] = -1
    finite = np.isfinite(r).all(axis=1)
    zero = d == 0
    rej = ~finite | zero.all(axis=1) | (as_pixel & zero.any(axis=1))
    rec[rej, 5] = REJECTED
    with np.errstate(all="ignore"):
        s = np.sign(d).astype(np.int64)
        fl = np.floor(o)
        v = np.where(np.isfinite(fl), fl, 0).astype(np.int64)
        dt = np.abs(F(1) / d)
        t = (dt * (o - fl)) * -(s.astype(F))
        t = t + dt * F(-1) * np.where(t < 0, F(-1), F(0))
        if not as_pixel:
            t = np.where(dt == np.inf, F(np.inf), t)
        b = np.zeros((n, 3), dtype=np.int64) if bias is None else np.broadcast_to(np.asarray(bias, dtype=np.int64), (n, 3))
        t = (t + b.astype(F)).astype(F)
    cap = int(max_steps) if max_steps > 0 else 3 * int(dims.max()) + 3
    dist = np.zeros(n, dtype=np.int64)
    m_last = np.zeros(n, dtype=F)
    fm_last = np.zeros(n, dtype=np.int64)
    status = np.where(rej, REJECTED, 0)
    active = np.nonzero(~rej)[0]
    mincl = lambda a, b: np.where(b < a, b, a)
    with np.errstate(all="ignore"):
        while active.size:
            tt, dd = t[active], dt[active]
            m_last[active] = np.fmin(np.fmin(tt[:, 0], tt[:, 1]), tt[:, 2])
            f = np.stack([tt[:, 0] <= mincl(tt[:, 1], tt[:, 2]), tt[:, 1] <= mincl(tt[:, 2], tt[:, 0]),
                          tt[:, 2] <= mincl(tt[:, 0], tt[:, 1])], axis=1)
            t[active] = np.where(f, tt + dd, tt)
            v[active] += s[active] * f
            fm_last[active] = f[:, 0] | (f[:, 1].astype(np.int64) << 1) | (f[:, 2].astype(np.int64) << 2)
            vv = v[active]
            out = ((vv < 0) | (vv >= dims)).any(axis=1)
            status[active[out]] = LEFT_MAP
            inside = active[~out]
            vi = v[inside]
            idx = vi[:, 0] + dims[0] * (vi[:, 1] + dims[2] * vi[:, 2])
            val = np.where(idx < mat.size, mat[np.minimum(idx, mat.size - 1)], 0)
            hit = (val == 5) | (val == 6)
            status[inside[hit]] = HIT
            rec[inside[hit], 3] = val[hit]
            go = inside[~hit]
            dist[go] += 1
            capped = go[dist[go] >= cap]
            status[capped] = STEP_CAP
            active = go[dist[go] < cap]
    h = status == HIT
    rec[h, 0:3] = v[h]
    rec[h, 4] = fm_last[h]
    rec[:, 5] = status
    rec[~rej, 6] = dist[~rej]
    rec[~rej, 7] = m_last[~rej].view(np.int32)
    return rec


def oracle_records(rays, *, scene, descriptors, root_index, using_octree, max_steps=0, as_pixel=False, attachment_lookup=None,
                   attachments=None, atlas=None):
    """Each ray rendered as a 1 x 1 frame of the CPU oracle (camera at the origin, a one-entry viewport table holding the
    direction, trig (0, 1, 0, 1) -- the identity for non-zero components --, shadow_rays = 0): fields 0-4 and 6 of its hit
    record.  Field 6 of a mirror hit is the frame's count after the bounce."""
    from oracle import orc
    r = np.asarray(rays, dtype=F).reshape(-1, 6)
    dim = scene["dim"]
    md = scene.get("map_dim", (dim, dim, dim))
    cap = int(max_steps) if max_steps > 0 else 3 * max(md) + 3
    out = np.zeros((len(r), 8), dtype=np.int32)
    trig = np.array([0, 1, 0, 1], dtype=F)
    for k, ray in enumerate(r):
        vp = np.zeros((1, 1, 4), dtype=F)
        vp[0, 0, :3] = ray[3:]
        _, hits, _ = orc.raycast(width=1, height=1, cam_dir=(0.0, 0.0), cam_pos=tuple(ray[:3]), lights=scene["lights"],
                                 atlas=atlas, tile_dim=(16, 16), descriptors=descriptors, root_index=root_index, octree_dim=dim,
                                 using_octree=using_octree, grid=scene.get("grid"), map_dim=md, max_distance=cap, shadow_rays=0,
                                 viewport=vp, trig=trig, no_bias=0 if as_pixel else 1, attachment_lookup=attachment_lookup,
                                 attachments=attachments)
        out[k] = hits[0, 0]
    return out


def random_rays(rng, n, dim, kinds=("unit", "long", "tiny", "zero1", "zero2", "negzero")):
    """Seeded rays with origins inside [0, dim)^3 and directions of every kind the query must handle: unit vectors, components
    > 1, components < 1e-3, exactly 0 on one and on two axes, and -0."""
    o = rng.uniform(0.0, dim, size=(n, 3)).astype(F)
    o = np.minimum(o, F(np.nextafter(F(dim), F(0))))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kind = rng.integers(0, len(kinds), size=n)
    for k, name in enumerate(kinds):
        sel = kind == k
        cnt = int(sel.sum())
        if not cnt:
            continue
        ax = rng.integers(0, 3, size=cnt)
        rows = np.nonzero(sel)[0]
        if name == "long":
            d[rows] *= rng.uniform(1.5, 40.0, size=(cnt, 1))
        elif name == "tiny":
            d[rows, ax] = rng.uniform(1e-7, 9e-4, size=cnt) * rng.choice([-1, 1], size=cnt)
        elif name == "zero1":
            d[rows, ax] = 0.0
        elif name == "zero2":
            d[rows, ax] = 0.0
            d[rows, (ax + 1) % 3] = 0.0
        elif name == "negzero":
            d[rows, ax] = -0.0
    return np.concatenate([o, d.astype(F)], axis=1).astype(F)


def entry_param(rays, iterations, as_pixel=False, bias=None):
    """Field 7 from a step count alone (trees too large for a dense grid): min(t) before the increment of iteration
    `iterations` (1-based) of the occupancy-free recurrence -- dist + 1 for a hit or an exit, dist for the step cap."""
    r = np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)
    n = len(r)
    it = np.asarray(iterations, dtype=np.int64).reshape(n)
    empty = np.zeros(1, np.int8)
    big = 1 << 20
    # the replay on an empty map that holds every map a test builds, with the cap at `iterations`: its field 7 is what is asked for
    out = np.zeros(n, dtype=np.int32)
    for k in np.unique(it):
        sel = np.nonzero(it == k)[0]
        if k <= 0:
            continue
        rr = r[sel]
        b = None if bias is None else np.broadcast_to(np.asarray(bias, dtype=np.int64), (n, 3))[sel]
        out[sel] = replay(rr, empty, (big, big, big), max_steps=int(k), as_pixel=as_pixel, bias=b)[:, 7]
    return out
