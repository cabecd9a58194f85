"""GPU suite (-m gpu): maps of 2^3, 4^3, 8^3 and 16^3 voxels through every query family and the frame kernels.  The boundary
accepts them (log2_dim >= 1), but no query test used a map below 16^3, so no test reached

* the region read's branch for trees shallower than a brick (resolve_row<2> / resolve_row<1> from the root),
* the box walk starting at the root with r == n,
* a 2^3 map, whose root is itself the bottom-level descriptor (the attachments are looked up at root_index),
* trees below depth 5 (no coarse table by default) with an explicit coarse_log2: 1 at 8^3, 2 at 16^3.

Random maps (density 0.3, materials 5, 6, 1, -3), an all-solid and an all-empty map (Generate gives the single word 0xff000001
for an empty 2^3 map, a childless root otherwise; validate accepts both), the SVO branch with and without attachments and the
array branch; and all 256 maps of 2^3 voxels on one handle.  Every comparison is exact, against the numpy replays
(voxel_replay, box_replay, sweep_replay, ray_replay) and, for frames, the oracle."""
import functools
import gc

import numpy as np
import pytest

import box_replay as br
import ray_replay
import scenes
import sweep_replay as sr
import voxel_raycaster_amd as vrc
import voxel_replay as vr
from oracle import orc
from test_box_queries_gpu import _caster, _derive
from test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu
I, F = np.int32, np.float32
W, H = 64, 48
DIMS = (2, 4, 8, 16)
MAPS = ("random", "solid", "empty")
# name -> (using_octree, settings, attachments)
CONFIGS = {"svo-attached": (0, (), True), "svo-plain": (0, (), False), "array": (1, (), True),
           "svo-coarse1": (0, (("coarse_log2", 1),), True), "svo-coarse2": (0, (("coarse_log2", 2),), True)}


def _cases():
    out = []
    for dim in DIMS:
        for kind in MAPS:
            for config in CONFIGS:
                if (config == "svo-coarse1" and dim != 8) or (config == "svo-coarse2" and dim != 16):
                    continue
                out.append((dim, kind, config))
    return out


@functools.lru_cache(maxsize=None)
def _map(dim, kind):
    if kind == "solid":
        return np.full(dim ** 3, 5, np.int8)
    if kind == "empty":
        return np.zeros(dim ** 3, np.int8)
    rng = np.random.default_rng(400 + dim)
    g = rng.choice(np.array([0, 5, 6, 1, -3], np.int8), size=dim ** 3, p=[0.7, 0.15, 0.07, 0.04, 0.04])
    assert 0 < np.count_nonzero(g) < g.size and (dim == 2 or len(set(g.tolist())) == 5)
    return g


def _scene(dim, kind):
    lights = np.array([[0.01, 0.01, 0.01, 0.2, dim * 0.8, dim * 0.2, dim * 0.9, -1, -1, -1.5]], dtype=F)
    return dict(dim=dim, grid=_map(dim, kind), cam_pos=(dim * 0.5 + 0.37, -1.59, dim * 0.45 + 0.29), cam_dir=(2.0, 1.5708), lights=lights)


class Case:
    def __init__(self, dim, kind, config, atlas):
        self.dim, self.kind, self.config, self.atlas = dim, kind, config, atlas
        self.using_octree, self.settings, self.attached = CONFIGS[config]
        self.s = _scene(dim, kind)
        self.g = self.s["grid"]
        self.o = vrc.Octree.Generate(self.g, dim)
        if kind == "empty":
            assert self.o.descriptor_buffer.tolist() == [0xff000001]
        if dim == 2:
            assert self.o.descriptor_buffer.size == 1 and self.o.root_index == 0
        if self.attached:
            self.o.attach_materials_from_grid(self.g)
        mat = br.grid_xyz(self.g, dim)
        self.mat = mat if self.attached else np.where(mat != 0, 5, 0).astype(np.int8)
        self.tag = f"{dim}^3 {kind} {config}"
        self.c = _caster(self.s, atlas, using_octree=self.using_octree, settings=self.settings, octree=self.o)
        self.structures()

    def structures(self):
        """Which derived structures the handle built: a table only where coarse_log2 asks for one (trees below depth 5 get none
        by default), and the empty boxes exactly where the table is."""
        m = self.c.memory_usage2()
        want = {"svo-coarse1": 1, "svo-coarse2": 2}.get(self.config, 0)
        assert m["coarse_log2"] == want and (m["coarse_bytes"] > 0) == (want > 0), (self.tag, m)
        assert (m["box_bytes"] > 0) == (want > 0) and m["note"] == "", (self.tag, m)
        return want


@pytest.fixture(scope="module", params=_cases(), ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}")
def case(request, atlas):
    k = Case(*request.param, atlas)
    yield k
    del k.c
    gc.collect()


def test_points(case):
    """Every voxel and two layers of outside points around the map."""
    ax = np.arange(-2, case.dim + 2)
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(I)
    got = case.c.get_voxels(pts)
    want = vr.points(case.mat, pts)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (case.tag, pts[bad[:4]], got[bad[:4]], want[bad[:4]])
    assert np.count_nonzero(got) == np.count_nonzero(case.mat)


def test_regions(case):
    dim, c = case.dim, case.c
    for lo, size in (((0, 0, 0), (dim,) * 3), ((-3, -3, -3), (dim + 6,) * 3)):
        got = c.read_regions(np.array([lo], I), size)
        assert np.array_equal(got, vr.regions(case.mat, [lo], size)), (case.tag, lo, size)
    rng = np.random.default_rng(dim + 31)
    for k in range(20):                                         # 100 regions: 20 sizes (1 .. 12 per axis), 5 corners each
        size = tuple(int(v) for v in rng.integers(1, 13, size=3))
        lo = rng.integers(-10, dim + 3, size=(5, 3)).astype(I)
        got = c.read_regions(lo, size)
        want = vr.regions(case.mat, lo, size)
        bad = np.nonzero((got != want).any(axis=(1, 2, 3)))[0]
        assert bad.size == 0, (case.tag, size, lo[bad[:3]], np.argwhere(got[bad[0]] != want[bad[0]])[:4])


def test_boxes(case):
    boxes = br.random_boxes(np.random.default_rng(case.dim + 37), 500, case.dim)
    whole = np.array([[0, 0, 0, case.dim, case.dim, case.dim], [-1, -1, -1, case.dim + 2, case.dim + 2, case.dim + 2]], F)
    boxes = np.concatenate([whole, boxes]).astype(F)
    any_hit = 0
    for stopping in (False, True):
        full = br.GridReplay(case.mat, stopping).query(boxes, 64)
        for maxv in (0, 64):
            rec, cnt, vox = case.c.box_intersection(boxes, max_voxels=maxv, stopping_only=stopping)
            er, ec, ev = _derive(full, maxv)
            bad = np.nonzero((rec != er).any(1) | (cnt != ec))[0]
            assert bad.size == 0, (case.tag, stopping, maxv, bad[:4], rec[bad[:2]], er[bad[:2]], cnt[bad[:2]], ec[bad[:2]], boxes[bad[:2]])
            if maxv:
                badl = np.nonzero((vox != ev).any(axis=(1, 2)))[0]
                assert badl.size == 0, (case.tag, stopping, maxv, badl[:4], boxes[badl[:2]])
            any_hit += int((rec[:, 0] & br.ANY).sum())
        if not stopping:
            assert cnt[0] == cnt[1] == np.count_nonzero(case.mat)
    assert (any_hit > 0) == (case.kind != "empty")


def small_sweeps(rng, n, dim):
    """Sweeps for maps down to 2^3 (sweep_replay.random_sweeps draws face-sized boxes from uniform(4, min(dim, 24))): origins
    in [-2, dim + 1], extents in [0, dim], displacements in [-2 dim, 2 dim]; a quarter with integer origins and extents, some
    axis-aligned, some that do not move, a few rejected."""
    o = rng.uniform(-2, dim + 1, size=(n, 3))
    ext = rng.uniform(0, dim, size=(n, 3)) * rng.uniform(0, 1, size=(n, 1))
    d = rng.uniform(-2 * dim, 2 * dim, size=(n, 3))
    kind = rng.integers(0, 8, size=n)
    k = kind == 0
    o[k], ext[k], d[k] = np.floor(o[k]), np.floor(ext[k]), np.round(d[k])
    k = kind == 1
    o[k], ext[k] = np.floor(o[k]), np.floor(ext[k]) + 1
    k = np.nonzero(kind == 2)[0]
    keep = rng.integers(0, 3, size=len(k))
    for a in range(3):
        d[k[keep != a], a] = 0.0
    k = np.nonzero(kind == 3)[0]
    ext[k] = 0.0
    d[k[::4]] = 0.0
    k = kind == 4
    o[k] = rng.uniform(0, dim, size=(int(k.sum()), 3))
    ext[k] = rng.uniform(0, 0.5, size=(int(k.sum()), 3))
    s = np.concatenate([o, ext, d], axis=1).astype(F)
    bad = rng.choice(n, size=8, replace=False)
    s[bad[0::4], 3] = F(-1.0)
    s[bad[1::4], 1] = F(np.nan)
    s[bad[2::4], 7] = F(np.inf)
    s[bad[3::4], 0] = F(2.0 ** 30)
    return s


def test_sweeps(case):
    sweeps = small_sweeps(np.random.default_rng(case.dim + 41), 500, case.dim)
    flags = 0
    for stopping in (False, True):
        scene = sr.GridScene(case.mat, stopping)
        for cap in (0, 3):
            want = sr.sweep_replay(scene, sweeps, max_events=cap)
            got = case.c.sweep_boxes(sweeps, max_events=cap, stopping_only=stopping)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (case.tag, stopping, cap, len(bad), bad[:4], got[bad[:3]], want[bad[:3]], sweeps[bad[:3]])
            flags |= int(np.bitwise_or.reduce(got[:, 0]))
    assert flags & sr.CLIPPED and flags & sr.LEFT_MAP and flags & sr.REJECTED, (case.tag, flags)
    assert bool(flags & sr.HIT) == (case.kind != "empty") and bool(flags & sr.START_SOLID) == (case.kind != "empty"), (case.tag, flags)
    assert case.dim == 2 or flags & sr.EVENT_CAP, (case.tag, flags)


def test_rays(case):
    dim = case.dim
    rays = ray_replay.random_rays(np.random.default_rng(dim + 43), 500, dim)
    rays[:50, :3] = np.floor(rays[:50, :3])
    bias = ray_replay.origin_bias(rays[:, :3], case.o.descriptor_buffer, case.o.root_index, dim)
    seen = set()
    for as_pixel in (False, True):
        for max_steps in (0, 2):
            got = case.c.cast_rays(rays, max_steps=max_steps, as_pixel=as_pixel)
            want = ray_replay.replay(rays, case.mat.transpose(2, 1, 0).reshape(-1), (dim,) * 3, max_steps=max_steps, as_pixel=as_pixel,
                                     bias=bias if as_pixel else None)
            bad = np.nonzero((got != want).any(1))[0]
            assert bad.size == 0, (case.tag, as_pixel, max_steps, bad[:4], got[bad[:2]], want[bad[:2]], rays[bad[:2]])
            seen |= set(got[:, 5].tolist())
    assert (vrc.RAY_HIT in seen) == (case.kind != "empty") and vrc.RAY_LEFT_MAP in seen and vrc.RAY_REJECTED in seen, (case.tag, seen)


def test_frames(case):
    """64x48 frames from inside the map, from outside it and from a voxel centre: the exact kernel and mode B (SVO branch), each on
    a handle of its own."""
    dim = case.dim
    kw = dict(attachment_lookup=case.o.attachment_lookup, attachments=case.o.attachment_buffer) if case.attached and not case.using_octree else {}
    table = case.structures()
    li = np.zeros((8, 10), dtype=F)
    li[:1] = case.s["lights"][:1]
    for mode in ((0,) if case.using_octree else (0, 1)):
        c = _caster(case.s, case.atlas, using_octree=case.using_octree, octree=case.o,
                    settings=case.settings + ((("stepping_mode", 1),) if mode else ()))
        assert c.create_viewport(W, H), c.last_error()
        for cam_pos, cam_dir in (((dim * 0.5 + 0.37, dim * 0.25 + 0.41, dim * 0.45 + 0.29), (2.0, 1.5708)),
                                 ((dim * 0.5 + 0.37, -1.59, dim * 0.45 + 0.29), (1.7, 1.5708)),
                                 ((-2.25, dim + 1.5, dim + 0.75), (2.1, -0.7)),
                                 ((dim // 2 + 0.5, dim // 2 - 0.5, dim - 0.5), (2.4, 0.9))):
            direction, position = np.array(cam_dir, F), np.array(cam_pos, F)
            assert c.assign_camera(direction, position) and c.validate() and c.compute(), c.last_error()
            oimg, ohits, octr = orc.raycast(width=W, height=H, cam_dir=direction, cam_pos=position, lights=li, atlas=case.atlas,
                                            tile_dim=(16, 16), descriptors=case.o.descriptor_buffer, root_index=case.o.root_index,
                                            octree_dim=dim, using_octree=case.using_octree, grid=case.g, max_distance=3 * dim,
                                            stepping_mode=mode, coarse_log2=table if mode else -1, **kw)
            try:
                assert_same(c.read_image(), c.read_hits(), c.counters(), oimg, ohits, octr)
            except AssertionError as e:
                raise AssertionError(f"{case.tag} mode {mode} camera {cam_pos}: {e}") from None
        del c


def test_all_256_maps_of_two_cubed(atlas):
    """One handle, re-assigned and re-validated per occupancy pattern (material 5; pattern 0 is the empty map)."""
    ax = np.arange(-1, 3)
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(I)
    edges = [(a, b) for a in range(3) for b in range(3) if a < b]
    boxes = np.array([[x0, y0, z0, x1 - x0, y1 - y0, z1 - z0] for x0, x1 in edges for y0, y1 in edges for z0, z1 in edges], F)
    assert len(boxes) == 27 and len(pts) == 64
    c = _caster(_scene(2, "empty"), atlas)
    for p in range(256):
        g = np.array([5 if p >> k & 1 else 0 for k in range(8)], np.int8)           # index x + 2 * (y + 2 * z) = slot
        o = vrc.Octree.Generate(g, 2)
        assert o.descriptor_buffer.tolist() == [0xff000001 | (p << 16)] and o.root_index == 0
        assert c.assign_octree(o) and c.validate(), (p, c.last_error())
        mat = br.grid_xyz(g, 2)
        assert np.array_equal(c.get_voxels(pts), vr.points(mat, pts)), p
        assert np.array_equal(c.read_regions(np.full((1, 3), -1, I), (4, 4, 4)), vr.regions(mat, [[-1, -1, -1]], (4, 4, 4))), p
        rec, cnt, vox = c.box_intersection(boxes, max_voxels=8)
        er, ec, ev = br.GridReplay(mat).query(boxes, 8)
        assert np.array_equal(rec, er) and np.array_equal(cnt, ec) and np.array_equal(vox, ev), p
