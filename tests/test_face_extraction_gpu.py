"""GPU suite (-m gpu): the exposed voxel faces of the resident scene (vrc_extract_faces / vrc_extract_faces_device,
csrc/face_extract.hip).

Every comparison is exact, counts and lists in order, against the numpy replay (tests/face_replay.py): whole maps, whole maps
with an apron and random regions of every size class and alignment, under all four flag combinations and in four
configurations, and the SVO branch with attachments is the array branch; tiles partition the whole map's set; a truncated list
is a prefix and leaves the rest of the buffer alone; maps of 2^3, 4^3 and 8^3 voxels and all 256 maps of 2^3; solid leaves above
the bottom; device-built shell terrains and re-laid-out trees (far pointers); the scene after edits and after compaction; the
replay fed with the region read; a non-cubic array map and corners at the ends of int32; 512 chunks of a 256^3 terrain in one
call; the device path, group handles, a frame in flight, argument errors and released staging."""
import ctypes as C
import gc

import numpy as np
import pytest

import box_replay as br
import face_replay as fr
import leaftree
import relayout as rl
import scenes
import voxel_raycaster_amd as vrc
from test_box_queries_gpu import CONFIGS, _caster
from test_voxel_reads_gpu import _random_regions

pytestmark = pytest.mark.gpu
I = np.int32
SENTINEL = -77
FLAGS = [(False, False), (True, False), (False, True), (True, True)]         # (no_map_edge, stopping_only)


def _same(got, want, tag):
    """(counts, faces, ...) of a call against the replay's (counts, faces)."""
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, (tag, "counts", bad[:4], got[0][bad[:4]], want[0][bad[:4]])
    assert got[1].shape == want[1].shape, (tag, got[1].shape, want[1].shape)
    rows = np.nonzero((got[1] != want[1]).any(axis=1))[0]
    assert rows.size == 0, (tag, "faces", rows[:4], got[1][rows[:4]], want[1][rows[:4]])


def _check(c, mat, lo, size, tag, flags=FLAGS, cache=None):
    """All flag combinations of one batch against the replay; returns the calls' results.  cache: a dict that keeps the replay's
    answers for the handles that follow (the caller keeps `mat` alive)."""
    out = []
    for no_edge, stopping in flags:
        got = c.extract_faces(lo, size, no_map_edge=no_edge, stopping_only=stopping)
        key = (mat.ctypes.data, np.asarray(lo).tobytes(), tuple(int(v) for v in size), no_edge, stopping)
        want = cache.get(key) if cache is not None else None
        if want is None:
            want = fr.regions(mat, lo, size, no_edge, stopping)
            if cache is not None:
                cache[key] = want
        _same(got, want, (tag, size, no_edge, stopping))
        info = got[2]
        assert info["faces_total"] == info["faces_written"] == got[0].sum() == len(got[1]) and not info["truncated"], (tag, info)
        out.append(got[:2])
    return out


def _check_scene(c, mat, dim, regions, tag, cache=None):
    out = _check(c, mat, np.zeros((1, 3), I), (dim,) * 3, tag, cache=cache)
    out += _check(c, mat, np.full((1, 3), -3, I), (dim + 6,) * 3, tag, cache=cache)
    for size, lo in regions:
        out += _check(c, mat, lo, size, tag, cache=cache)
    return out


@pytest.mark.parametrize("make", scenes.ALL, ids=lambda m: m.__name__)
def test_small_scenes_equal_the_replay(atlas, make):
    s = dict(make())
    dim = s["dim"]
    grid = rl.with_materials(s["grid"], dim)
    s["grid"] = grid
    mat = br.grid_xyz(grid, dim)
    plain = np.where(mat != 0, 5, 0).astype(np.int8)
    regions = _random_regions(np.random.default_rng(dim + 29), dim)
    results, cache = {}, {}
    for name, using_octree, settings, attached in CONFIGS:
        tree = vrc.Octree.Generate(grid, dim)
        if attached:
            tree = tree.attach_materials_from_grid(grid)
        c = _caster(s, atlas, using_octree=using_octree, settings=settings, octree=tree)
        results[name] = _check_scene(c, mat if attached else plain, dim, regions, name, cache)
        del c
    assert sum(len(f) for _, f in results["array"]) > 0
    for a, b in zip(results["svo-attached"], results["array"]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _tiles(dim, edge, shift):
    g = np.arange(-edge, dim, edge)
    lo = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.array(shift)
    assert (lo.min(axis=0) <= 0).all() and (lo.max(axis=0) + edge >= dim).all()
    return lo.astype(I)


def test_tiles_partition_the_map(atlas):
    s = dict(scenes.random_sparse(32, density=0.3))
    dim = s["dim"]
    s["grid"] = rl.with_materials(s["grid"], 7)
    mat = br.grid_xyz(s["grid"], dim)
    tree = vrc.Octree.Generate(s["grid"], dim).attach_materials_from_grid(s["grid"])
    for using_octree in (0, 1):
        c = _caster(s, atlas, using_octree=using_octree, octree=tree)
        for no_edge, stopping in ((False, False), (True, True)):
            _, whole, _ = c.extract_faces(np.zeros((1, 3), I), (dim,) * 3, no_map_edge=no_edge, stopping_only=stopping)
            want = {tuple(r) for r in whole.tolist()}
            assert len(want) == len(whole) > 5000
            for edge, shift in ((8, (0, 0, 0)), (8, (3, 5, 1)), (11, (2, 0, 7))):
                lo = _tiles(dim, edge, shift)
                got = c.extract_faces(lo, (edge,) * 3, no_map_edge=no_edge, stopping_only=stopping)
                _same(got, fr.regions(mat, lo, (edge,) * 3, no_edge, stopping), (using_octree, edge, shift))
                assert len(got[1]) == len(whole) and {tuple(r) for r in got[1].tolist()} == want, (using_octree, edge, shift)
        del c


def test_truncation(atlas):
    torch = pytest.importorskip("torch")
    s = scenes.floor_pillars()
    dim = s["dim"]
    mat = np.where(br.grid_xyz(s["grid"], dim) != 0, 5, 0).astype(np.int8)
    c = _caster(s, atlas)
    lo = _tiles(dim, 11, (3, 5, 1))
    counts, faces = fr.regions(mat, lo, (11, 11, 11))
    total = len(faces)
    assert total > 1000
    tl = torch.from_numpy(lo).to("cuda:0")
    for capacity in (0, 1, total - 1, total, total + 5):
        # the host call: the written prefix, and the caller's memory behind it as it was
        buf = np.full((total + 8, 4), SENTINEL, I)
        cnt = np.full(len(lo), SENTINEL, np.int64)
        info = vrc.FacesInfo()
        info.struct_size = C.sizeof(vrc.FacesInfo)
        size = np.array([11, 11, 11], I)
        rc = vrc.lib.vrc_extract_faces(c._h, lo.ctypes.data_as(C.POINTER(C.c_int32)), len(lo), size.ctypes.data_as(C.POINTER(C.c_int32)),
                                       capacity, 0, cnt.ctypes.data_as(C.POINTER(C.c_int64)),
                                       buf.ctypes.data_as(C.POINTER(C.c_int32)) if capacity else None, C.byref(info))
        assert rc == 0, c.last_error()
        # ... and the device call into a sentinel-filled tensor
        # (at a 16-byte-aligned address and 4 bytes behind one: the list need only be 4-byte aligned)
        results = [(cnt, buf, info.as_dict())]
        for offset in (0, 1):
            flat = torch.full((4 * (total + 8) + 4,), SENTINEL, dtype=torch.int32, device="cuda:0")
            dbuf = flat[offset:offset + 4 * (total + 8)]
            assert dbuf.data_ptr() % 16 == 4 * offset
            dcnt = torch.full((len(lo),), SENTINEL, dtype=torch.int64, device="cuda:0")
            dinfo = c.extract_faces_device(tl.data_ptr(), len(lo), (11, 11, 11), dcnt.data_ptr(), dbuf.data_ptr() if capacity else 0, capacity)
            got_all = flat.cpu().numpy()
            assert (got_all[:offset] == SENTINEL).all() and (got_all[offset + 4 * (total + 8):] == SENTINEL).all()
            results.append((dcnt.cpu().numpy(), dbuf.cpu().numpy().reshape(-1, 4), dinfo))
        written = min(total, capacity)
        for got_cnt, got, inf in results:
            assert np.array_equal(got_cnt, counts), capacity
            assert np.array_equal(got[:written], faces[:written]) and (got[written:] == SENTINEL).all(), capacity
            assert inf["faces_total"] == total and inf["faces_written"] == written and inf["truncated"] == int(total > capacity), (capacity, inf)
            assert inf["seconds"] > 0
    # the wrapper with a given capacity returns the written prefix
    got = c.extract_faces(lo, (11, 11, 11), capacity=total - 1)
    assert np.array_equal(got[1], faces[:total - 1]) and got[2]["truncated"] == 1


def _small_map(dim, kind):
    if kind == "solid":
        return np.full(dim ** 3, 5, np.int8)
    if kind == "empty":
        return np.zeros(dim ** 3, np.int8)
    rng = np.random.default_rng(400 + dim)
    return rng.choice(np.array([0, 5, 6, 1, -3], np.int8), size=dim ** 3, p=[0.6, 0.2, 0.1, 0.05, 0.05])


def _small_scene(dim, grid):
    lights = np.array([[0.01, 0.01, 0.01, 0.2, dim * 0.8, dim * 0.2, dim * 0.9, -1, -1, -1.5]], dtype=np.float32)
    return dict(dim=dim, grid=grid, cam_pos=(dim * 0.5 + 0.37, -1.59, dim * 0.45 + 0.29), cam_dir=(2.0, 1.5708), lights=lights)


@pytest.mark.parametrize("dim", [2, 4, 8])
def test_smallest_trees(atlas, dim):
    """Trees shallower than a brick (the brick at the origin holds the whole map) and the tree that is one brick."""
    rng = np.random.default_rng(dim)
    regions = [((dim,) * 3, np.zeros((1, 3), I)), ((dim + 6,) * 3, np.full((1, 3), -3, I))]
    regions += [(tuple(int(v) for v in rng.integers(1, 12, size=3)), rng.integers(-9, dim + 3, size=(12, 3)).astype(I)) for _ in range(8)]
    faces = 0
    for kind in ("random", "solid", "empty"):
        grid = _small_map(dim, kind)
        mat = br.grid_xyz(grid, dim)
        for name, using_octree, attached in (("svo-attached", 0, True), ("svo-plain", 0, False), ("array", 1, True)):
            tree = vrc.Octree.Generate(grid, dim)
            if attached:
                tree = tree.attach_materials_from_grid(grid)
            c = _caster(_small_scene(dim, grid), atlas, using_octree=using_octree, octree=tree)
            m = mat if attached else np.where(mat != 0, 5, 0).astype(np.int8)
            for size, lo in regions:
                faces += sum(len(f) for _, f in _check(c, m, lo, size, (dim, kind, name)))
            if kind == "solid":
                assert c.extract_faces(np.zeros((1, 3), I), (dim,) * 3)[0].tolist() == [6 * dim * dim]
                assert c.extract_faces(np.zeros((1, 3), I), (dim,) * 3, no_map_edge=True)[0].tolist() == [0]
            del c
    assert faces > 100


def test_all_256_maps_of_two_cubed(atlas):
    """One handle, re-assigned per occupancy pattern; every pattern through one batched call of all 64 corners of a 3^3 region."""
    ax = np.arange(-2, 2)
    lo = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(I)
    c = _caster(_small_scene(2, np.zeros(8, np.int8)), atlas)
    for p in range(256):
        g = np.array([5 if p >> k & 1 else 0 for k in range(8)], np.int8)
        assert c.assign_octree(vrc.Octree.Generate(g, 2)) and c.validate(), (p, c.last_error())
        mat = br.grid_xyz(g, 2)
        for no_edge in (False, True):
            _same(c.extract_faces(lo, (3, 3, 3), no_map_edge=no_edge), fr.regions(mat, lo, (3, 3, 3), no_edge), (p, no_edge))


def test_solid_leaves_above_the_bottom(atlas):
    depth, dim = 5, 32
    cubes = [(0, 0, 0, 4), (8, 8, 8, 8), (4, 0, 0, 2), (16, 16, 0, 4), (20, 4, 6, 2)]
    rng = np.random.default_rng(5)
    desc, root, grid = leaftree.leaf_octree(rng.integers(0, dim, size=(300, 3)), cubes, depth)
    mat = br.grid_xyz(grid, dim)
    s = dict(scenes.floor_pillars(dim))
    s["grid"] = grid
    regions = _random_regions(rng, dim, total=200)
    for settings in ((), (("coarse_log2", 0),)):
        c = _caster(s, atlas, octree=vrc.Octree(desc, root, dim), settings=settings)
        whole = _check_scene(c, mat, dim, regions, settings)[0][1]
        for x, y, z, k in cubes:                                   # cubes of 5, and no face inside one
            v = whole[:, :3] - np.array([x, y, z])
            own = ((v >= 0) & (v < k)).all(axis=1)
            assert own.any() and (whole[own, 3] >> 8 == 5).all()
            assert not ((v > 0) & (v < k - 1)).all(axis=1).any()
        del c


@pytest.mark.parametrize("depth", [7, 8])
def test_shell_terrains_equal_the_columns(atlas, depth):
    import bench
    sc = bench.device_scene_header(depth)
    s = dict(dim=sc["dim"], cam_dir=sc["cam_dir"], cam_pos=sc["cam_pos"], lights=sc["lights"])
    c = _caster(s, atlas, device_tree=depth)
    dim = 1 << depth
    rng = np.random.default_rng(depth)
    cols = {}

    def column(x, y):
        if (x, y) not in cols:
            cols[(x, y)] = vrc.shell_column(depth, x, y)
        return cols[(x, y)]

    size = (13, 9, 24)
    xy = rng.integers(0, dim - 13, size=(24, 2))
    xy[:4] = [(-7, 50), (dim - 5, dim - 4), (0, 0), (dim - 13, 3)]            # across the map's edges and at its corners
    hi = np.array([column(int(np.clip(x + 6, 0, dim - 1)), int(np.clip(y + 4, 0, dim - 1)))[1] for x, y in xy])
    lo = np.stack([xy[:, 0], xy[:, 1], hi - rng.integers(4, 20, size=24)], axis=1).astype(I)
    lo = np.concatenate([lo, [[5, 5, dim - 10], [9, 40, -20]]]).astype(I)     # the map's top and its bottom
    total = 0
    for no_edge in (False, True):
        got = c.extract_faces(lo, size, no_map_edge=no_edge)
        _same(got, fr.column_regions(depth, lo, size, column, no_edge), (depth, no_edge))
        total += len(got[1])
    assert total > 24 * 13 * 9
    del c
    gc.collect()


@pytest.mark.parametrize("make", [scenes.floor_pillars, scenes.random_sparse], ids=lambda m: m.__name__)
def test_relaid_trees(atlas, make):
    """Far pointers, a root in the middle of the array and filler words between the blocks (tests/relayout.py)."""
    s = dict(make())
    dim = s["dim"]
    g = rl.with_materials(s["grid"], dim)
    s["grid"] = g
    mat = br.grid_xyz(g, dim)
    o = vrc.Octree.Generate(g, dim, layout=2).attach_materials_from_grid(g)
    regions = _random_regions(np.random.default_rng(dim + 3), dim, total=100)
    cache = {}
    for far in (0.5, 1.0):
        d2, r2, l2 = rl.relayout(o.descriptor_buffer, o.root_index, dim, np.random.default_rng(dim + int(10 * far)), far, o.attachment_lookup)
        assert r2 != 0
        o2 = vrc.Octree(d2, r2, dim)
        o2.attachment_lookup, o2.attachment_buffer = l2, o.attachment_buffer
        for settings in ((), (("coarse_log2", 0),)):
            c = _caster(s, atlas, octree=o2, settings=settings)
            _check_scene(c, mat, dim, regions, (far, settings), cache)
            del c


def test_after_edits_and_compaction(atlas):
    s = dict(scenes.random_sparse(64, density=0.1))
    dim = s["dim"]
    g = rl.with_materials(s["grid"], 9)
    s["grid"] = g
    cur = br.grid_xyz(g, dim).copy()                                # mat[x, y, z]
    c = _caster(s, atlas, octree=vrc.Octree.Generate(g, dim).attach_materials_from_grid(g))
    rng = np.random.default_rng(77)
    regions = _random_regions(rng, dim, total=100)
    pts = rng.integers(-2, dim + 2, size=(600, 3)).astype(I)
    mats = rng.choice(np.array([0, 0, 5, 6, 1, -3], I), size=600)
    c.set_voxels(pts, mats)
    for p, m in zip(pts, mats):
        if ((p >= 0) & (p < dim)).all():
            cur[tuple(p)] = m
    _check_scene(c, cur, dim, regions, "set_voxels")
    lo = np.array([[4, 4, 4], [30, -3, 20], [50, 50, 50], [10, 40, 0]], I)
    size = np.array([[9, 17, 5], [8, 8, 8], [20, 20, 20], [3, 3, 30]], I)
    fill = np.array([6, 0, 5, -3], I)
    c.fill_boxes(lo, size, fill)
    for a, e, m in zip(lo, size, fill):
        a0, a1 = np.clip(a, 0, dim), np.clip(a + e, 0, dim)
        cur[a0[0]:a1[0], a0[1]:a1[1], a0[2]:a1[2]] = m
    before = _check_scene(c, cur, dim, regions, "fill_boxes")
    info = c.compact_octree()
    assert info["n_descriptors"] < info["descriptors_before"]
    after = _check_scene(c, cur, dim, regions, "compacted")
    for a, b in zip(before, after):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_replay_fed_with_the_region_read(atlas):
    """A mesher's other route: read every region with its one-voxel apron, extract on the host.  The same faces."""
    s = dict(scenes.random_sparse())
    dim = s["dim"]
    s["grid"] = rl.with_materials(s["grid"], 4)
    tree = vrc.Octree.Generate(s["grid"], dim).attach_materials_from_grid(s["grid"])
    c = _caster(s, atlas, octree=tree)
    rng = np.random.default_rng(15)
    size = np.array([13, 8, 21])
    lo = rng.integers(-10, dim + 3, size=(60, 3)).astype(I)
    blocks = c.read_regions(lo - 1, size + 2)
    for no_edge, stopping in FLAGS:
        lists = [fr.block_faces(b.transpose(2, 1, 0), corner, dim, no_edge, stopping) for b, corner in zip(blocks, lo)]
        got = c.extract_faces(lo, size, no_map_edge=no_edge, stopping_only=stopping)
        _same(got, fr.packed(lists), (no_edge, stopping))
    assert len(got[1]) > 100


def test_non_cubic_map_and_far_corners(atlas):
    """The array branch on a 16 x 8 x 4 map read by the frame's index (y stride dz, so rows alias; sides that are no multiple of a
    brick), and corners at the ends of int32: they own nothing and the corner arithmetic does not wrap."""
    from gpu_helpers import configure
    from test_voxel_reads_gpu import _frame_index_materials
    rng = np.random.default_rng(33)
    dx, dy, dz = 16, 8, 4
    mp = rng.choice(np.array([0, 0, 5, 6, 1, -2], np.int8), size=dx * dy * dz)
    s = dict(scenes.axis_aligned(16))
    c = vrc.CLCaster()
    assert c.init(0)
    li = np.zeros((8, 10), dtype=np.float32)
    li[:1] = s["lights"][:1]
    configure(c, 16, atlas, s["cam_dir"], s["cam_pos"], li, 96, 64)
    assert c.overwrite_setting("using_octree", 1)
    assert c.assign_octree(vrc.Octree.Generate(np.asarray(s["grid"], np.int8), 16)) and c.assign_map(mp, (dx, dy, dz))
    assert c.validate(), c.last_error()
    mat = _frame_index_materials(mp, dx, dy, dz)
    faces = sum(len(f) for _, f in _check(c, mat, np.full((1, 3), -2, I), (dx + 4, dy + 4, dz + 4), "non-cubic"))
    for size in ((5, 3, 2), (8, 8, 8), (1, 1, 1), (16, 8, 4)):
        lo = np.stack([rng.integers(-6, d + 3, size=30) for d in (dx, dy, dz)], axis=1).astype(I)
        faces += sum(len(f) for _, f in _check(c, mat, lo, size, "non-cubic"))
    assert faces > 1000
    big = 2 ** 31 - 1
    far = np.array([[big - 8, 0, 0], [-big - 1, -big - 1, 0], [0, big, 0], [0, 0, -big - 1], [0, 0, 0]], I)
    counts, listed, _ = c.extract_faces(far, (9, 9, 9))
    assert counts[:4].tolist() == [0, 0, 0, 0] and counts[4] == len(listed) > 0
    _same((counts, listed), fr.regions(mat, far, (9, 9, 9)), "far corners")


def test_batched_chunks_of_a_terrain(atlas):
    s = scenes.terrain256()
    dim = s["dim"]
    grid = np.asarray(s["grid"], np.int8)
    mat = br.grid_xyz(grid, dim)
    tree = vrc.Octree.Generate(grid, dim).attach_materials_from_grid(grid)
    c = _caster(s, atlas, octree=tree)
    g = np.arange(0, dim, 32)
    lo = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(I)
    assert len(lo) == 512
    for shift, no_edge in (((0, 0, 0), True), ((3, 5, 1), False)):
        corners = lo + np.array(shift, I)
        got = c.extract_faces(corners, (32, 32, 32), no_map_edge=no_edge)
        _same(got, fr.regions(mat, corners, (32, 32, 32), no_edge), shift)
        assert len(got[1]) > dim * dim


def test_device_path(atlas):
    torch = pytest.importorskip("torch")
    s = dict(scenes.random_sparse())
    dim = s["dim"]
    s["grid"] = rl.with_materials(s["grid"], 4)
    tree = vrc.Octree.Generate(s["grid"], dim).attach_materials_from_grid(s["grid"])
    c = _caster(s, atlas, octree=tree)
    rng = np.random.default_rng(8)
    dev_before = torch.cuda.current_device()
    for size, n in (((8, 8, 8), 40), ((13, 5, 9), 40), ((dim, dim, dim), 1), ((1, 1, 1), 9)):
        lo = (np.zeros((1, 3), I) if n == 1 else rng.integers(-10, dim + 3, size=(n, 3)).astype(I))
        for no_edge, stopping in FLAGS:
            counts, faces, _ = c.extract_faces(lo, size, no_map_edge=no_edge, stopping_only=stopping)
            tl = torch.from_numpy(lo).to("cuda:0")
            tc = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device="cuda:0")
            info = c.extract_faces_device(tl.data_ptr(), n, size, tc.data_ptr(), no_map_edge=no_edge, stopping_only=stopping)      # count only
            assert info["faces_total"] == len(faces) and info["faces_written"] == 0
            tf = torch.full((len(faces) + 1, 4), SENTINEL, dtype=torch.int32, device="cuda:0")
            info = c.extract_faces_device(tl.data_ptr(), n, size, tc.data_ptr(), tf.data_ptr(), len(faces), no_map_edge=no_edge, stopping_only=stopping)
            assert info["faces_written"] == len(faces) and not info["truncated"]
            got_c, got_f = tc.cpu().numpy(), tf.cpu().numpy()
            assert np.array_equal(got_c[:n], counts) and got_c[n] == SENTINEL
            assert np.array_equal(got_f[:-1], faces) and (got_f[-1] == SENTINEL).all()
    # misaligned pointers are refused
    raw = torch.zeros(256, dtype=torch.int8, device="cuda:0")
    size3 = np.array([2, 2, 2], I)
    sp = size3.ctypes.data_as(C.POINTER(C.c_int32))
    p = raw.data_ptr()
    assert p % 8 == 0
    call = lambda d_lo, d_counts, d_faces, cap: vrc.lib.vrc_extract_faces_device(c._h, C.c_void_p(d_lo), 1, sp, cap, 0, C.c_void_p(d_counts),
                                                                                  C.c_void_p(d_faces), None)
    assert call(p + 2, p + 64, p + 128, 4) == 1 and "aligned" in c.last_error()
    assert call(p, p + 68, p + 128, 4) == 1
    assert call(p, p + 64, p + 130, 4) == 1
    assert call(p, p + 64, p + 130, 0) == 0                         # (a count-only call does not look at faces)
    assert call(p, p + 64, p + 128, 4) == 0
    assert torch.cuda.current_device() == dev_before


def test_group_handle_equals_a_single_handle(atlas):
    torch = pytest.importorskip("torch")
    s = scenes.floor_pillars()
    dim = s["dim"]
    rng = np.random.default_rng(12)
    lo = rng.integers(-10, dim + 3, size=(50, 3)).astype(I)
    single = _caster(s, atlas)
    dev_before = torch.cuda.current_device()
    group = _caster(s, atlas, group=[0, 0])
    for batch, size in ((lo, (9, 8, 7)), (np.zeros((1, 3), I), (dim,) * 3)):
        a, b = group.extract_faces(batch, size), single.extract_faces(batch, size)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[1]) > 0
    assert torch.cuda.current_device() == dev_before


def test_extraction_between_async_and_sync_leaves_the_frame(atlas):
    s = scenes.terrain256()
    dim = s["dim"]
    ref = _caster(s, atlas)
    assert ref.compute()
    img0, hits0, ctr0, k0 = ref.read_image().copy(), ref.read_hits().copy(), ref.counters(), ref.last_kernel()
    c = _caster(s, atlas)
    rng = np.random.default_rng(5)
    lo = rng.integers(-10, dim, size=(300, 3)).astype(I)
    assert c.timing_reset()
    assert c.compute_async()
    got = c.extract_faces(lo, (16, 16, 16))
    assert c.sync()
    assert np.array_equal(c.read_image().view(np.uint32), img0.view(np.uint32))
    assert np.array_equal(c.read_hits(), hits0) and c.counters() == ctr0 and c.last_kernel() == k0
    assert c.timing()[0] == 1
    mat = np.where(br.grid_xyz(s["grid"], dim) != 0, 5, 0).astype(np.int8)
    _same(got, fr.regions(mat, lo, (16, 16, 16)), "in flight")
    _same(c.extract_faces(lo, (16, 16, 16)), got, "again")


def test_argument_errors_and_released_staging(atlas):
    s = scenes.floor_pillars()
    dim = s["dim"]
    c = _caster(s, atlas)
    lib = vrc.lib
    lo = np.array([[0, 0, 0], [5, 5, 0], [40, 0, 0], [-3, -3, -3]], I)
    size = np.array([8, 8, 8], I)
    cnt = np.full(4, SENTINEL, np.int64)
    out = np.full((64, 4), SENTINEL, I)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    cp = cnt.ctypes.data_as(C.POINTER(C.c_int64))
    info = vrc.FacesInfo()
    info.struct_size = C.sizeof(vrc.FacesInfo)
    f = lib.vrc_extract_faces
    assert f(None, ip(lo), 4, ip(size), 64, 0, cp, ip(out), None) == 1
    assert f(c._h, None, 4, ip(size), 64, 0, cp, ip(out), None) == 1
    assert f(c._h, ip(lo), 4, None, 64, 0, cp, ip(out), None) == 1
    assert f(c._h, ip(lo), 4, ip(size), 64, 0, None, ip(out), None) == 1
    assert f(c._h, ip(lo), 4, ip(size), 64, 0, cp, None, None) == 1 and "null faces" in c.last_error()
    assert f(c._h, ip(lo), -1, ip(size), 64, 0, cp, ip(out), None) == 1 and "n = -1" in c.last_error()
    for bad in ([0, 8, 8], [8, -1, 8], [8, 8, 0]):
        assert f(c._h, ip(lo), 4, ip(np.array(bad, I)), 64, 0, cp, ip(out), None) == 1 and "size" in c.last_error()
    assert f(c._h, ip(lo), 4, ip(size), -1, 0, cp, ip(out), None) == 1 and "capacity" in c.last_error()
    assert f(c._h, ip(lo), 4, ip(size), 64, 4, cp, ip(out), None) == 1 and "flag" in c.last_error()
    unset = vrc.FacesInfo()
    assert f(c._h, ip(lo), 4, ip(size), 64, 0, cp, ip(out), C.byref(unset)) == 1 and "struct_size" in c.last_error()
    assert f(c._h, ip(lo), 1 << 40, ip(size), 64, 0, cp, ip(out), None) == 6                   # n x bricks per region > 2^31 - 1
    assert f(c._h, ip(lo), 4, ip(np.array([2 ** 31 - 1] * 3, I)), 64, 0, cp, ip(out), None) == 6
    assert f(c._h, ip(lo), 4, ip(size), 1 << 60, 0, cp, ip(out), None) == 6                    # capacity * 16 overflows size_t
    assert lib.vrc_extract_faces_device(c._h, ip(lo), 4, ip(size), 64, 0, cp, ip(out), None) == 1   # pageable host memory is not device memory
    assert (cnt == SENTINEL).all() and (out == SENTINEL).all()                                  # nothing was launched
    assert f(c._h, ip(lo), 0, ip(size), 0, 0, cp, None, C.byref(info)) == 0 and info.faces_total == 0
    assert lib.vrc_extract_faces_device(c._h, None, 0, ip(size), 0, 0, None, None, None) == 0
    assert (cnt == SENTINEL).all()
    mat = br.grid_xyz(s["grid"], dim)
    want = fr.regions(mat, lo, size)
    assert f(c._h, ip(lo), 4, ip(size), 64, 0, cp, ip(out), C.byref(info)) == 0, c.last_error()
    assert np.array_equal(cnt, want[0]) and info.faces_total == len(want[1]) > 64 and info.truncated == 1 and info.faces_written == 64
    assert np.array_equal(out, want[1][:64])
    short = vrc.FacesInfo()
    short.struct_size = 8                                           # an older caller's struct: only its 8 bytes are written
    assert f(c._h, ip(lo), 4, ip(size), 64, 0, cp, ip(out), C.byref(short)) == 0
    assert short.struct_size == 8 and short.truncated == 1 and short.faces_total == 0
    # release_viewport frees staging and scratch (and un-validates the handle): the next call grows them again
    before = c.extract_faces(np.zeros((1, 3), I), (dim,) * 3)
    assert c.release_viewport()
    assert f(c._h, ip(lo), 4, ip(size), 64, 0, cp, ip(out), None) == 2
    assert c.create_viewport(96, 64) and c.validate(), c.last_error()
    _same(c.extract_faces(np.zeros((1, 3), I), (dim,) * 3), before, "regrown")
    fresh = vrc.CLCaster()
    assert fresh.init(0)
    assert f(fresh._h, ip(lo), 4, ip(size), 64, 0, cp, ip(out), None) == 2 and "validate" in fresh.last_error()
    assert c.release_octree()
    assert f(c._h, ip(lo), 4, ip(size), 64, 0, cp, ip(out), None) == 2
