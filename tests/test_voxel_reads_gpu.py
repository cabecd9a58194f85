"""GPU suite (-m gpu): voxel reads against the resident scene (vrc_get_voxels / vrc_read_regions and their _device variants,
csrc/voxel_read.hip).

Every comparison is exact.  Whole maps, whole maps with an apron, random regions of every size class and alignment and every
voxel as a point equal the numpy replay (tests/voxel_replay.py) in four configurations, and the SVO branch with attachments is
the array branch; 512 chunks of a 256^3 terrain come back in one call, aligned and shifted; solid leaves above the bottom read
as cubes of 5; device-built shell terrains (far pointers) equal the procedural columns; a read feeds vrc_build_dense_grid and
the rebuilt tree is the same tree; the non-zero voxels of a region are the box query's list; the device path writes exactly its
n V bytes at any alignment; group handles, a frame in flight, argument errors and released staging behave as the header says."""
import ctypes as C
import gc

import numpy as np
import pytest

import box_replay as br
import leaftree
from relayout import with_materials as _with_materials
import scenes
import voxel_raycaster_amd as vrc
import voxel_replay as vr
from test_box_queries_gpu import CONFIGS, _caster

pytestmark = pytest.mark.gpu
I = np.int32
SENTINEL = -77


def _size_classes(rng, n_random):
    """Region sizes 1 .. 21 per axis: 1, 7, 8 and 9 on every axis, mixed triples of them, then random ones."""
    fixed = [(1, 1, 1), (7, 7, 7), (8, 8, 8), (9, 9, 9), (1, 8, 9), (9, 7, 1), (8, 1, 7), (21, 21, 21), (16, 2, 13)]
    return fixed + [tuple(int(v) for v in rng.integers(1, 22, size=3)) for _ in range(n_random)]


def _random_regions(rng, dim, total=300):
    """[(size, lo (k, 3))]: `total` regions in batches of one size; lo from -10 to dim + 2, odd and even, some wholly outside."""
    sizes = _size_classes(rng, 11)
    per = total // len(sizes)
    out = []
    for size in sizes:
        lo = rng.integers(-10, dim + 3, size=(per, 3))
        lo[0] = (lo[0] // 2) * 2                                   # an even and an odd corner in every batch
        lo[1] = (lo[1] // 2) * 2 + 1
        lo[2] = (-10, dim + 2, 3)                                  # wholly outside
        out.append((size, lo.astype(I)))
    assert sum(len(lo) for _, lo in out) == total
    return out


def _all_points(dim, rng, outside=200):
    g = np.arange(dim)
    inside = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    out = rng.integers(-12, dim + 12, size=(4 * outside, 3))
    out = out[((out < 0) | (out >= dim)).any(axis=1)][:outside - 4]
    far = np.array([[2 ** 31 - 1, 0, 0], [-2 ** 31, 1, 1], [0, -1, 0], [0, 0, dim]])
    return np.concatenate([inside, out, far]).astype(I)


def _check_scene(c, mat, dim, regions, pts, tag):
    whole = c.read_regions(np.zeros((1, 3), I), (dim,) * 3)
    assert np.array_equal(whole, vr.regions(mat, [[0, 0, 0]], (dim,) * 3)), tag
    apron = c.read_regions(np.full((1, 3), -3, I), (dim + 6,) * 3)
    assert np.array_equal(apron, vr.regions(mat, [[-3, -3, -3]], (dim + 6,) * 3)), tag
    got = []
    for size, lo in regions:
        r = c.read_regions(lo, size)
        want = vr.regions(mat, lo, size)
        bad = np.nonzero((r != want).any(axis=(1, 2, 3)))[0]
        assert bad.size == 0, (tag, size, lo[bad[:3]], np.argwhere(r[bad[0]] != want[bad[0]])[:4])
        got.append(r)
    p = c.get_voxels(pts)
    want = vr.points(mat, pts)
    bad = np.nonzero(p != want)[0]
    assert bad.size == 0, (tag, pts[bad[:4]], p[bad[:4]], want[bad[:4]])
    return whole, apron, got, p


@pytest.mark.parametrize("make", scenes.ALL, ids=lambda m: m.__name__)
def test_small_scenes_equal_the_replay(atlas, make):
    s = dict(make())
    dim = s["dim"]
    grid = _with_materials(s["grid"], dim)
    s["grid"] = grid
    mat = br.grid_xyz(grid, dim)
    plain = np.where(mat != 0, 5, 0).astype(np.int8)
    rng = np.random.default_rng(dim + 29)
    regions = _random_regions(rng, dim)
    pts = _all_points(dim, rng)
    results = {}
    for name, using_octree, settings, attached in CONFIGS:
        tree = vrc.Octree.Generate(grid, dim)
        if attached:
            tree = tree.attach_materials_from_grid(grid)
        c = _caster(s, atlas, using_octree=using_octree, settings=settings, octree=tree)
        results[name] = _check_scene(c, mat if attached else plain, dim, regions, pts, name)
        del c
    a, b = results["svo-attached"], results["array"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


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
    for shift in ((0, 0, 0), (3, 5, 1)):
        corners = lo + np.array(shift, I)
        got = c.read_regions(corners, (32, 32, 32))
        assert got.shape == (512, 32, 32, 32)
        assert np.array_equal(got, vr.regions(mat, corners, (32, 32, 32))), shift
    assert np.count_nonzero(got) > dim * dim


def test_solid_leaves_above_the_bottom(atlas):
    depth = 5
    dim = 1 << depth
    cubes = [(0, 0, 0, 4), (8, 8, 8, 8), (4, 0, 0, 2), (16, 16, 0, 4), (20, 4, 6, 2)]
    rng = np.random.default_rng(5)
    desc, root, grid = leaftree.leaf_octree(rng.integers(0, dim, size=(300, 3)), cubes, depth)
    mat = br.grid_xyz(grid, dim)
    s = dict(scenes.floor_pillars(dim))
    s["grid"] = grid
    regions = _random_regions(rng, dim, total=200)
    pts = _all_points(dim, rng)
    for settings in ((), (("coarse_log2", 0),)):
        c = _caster(s, atlas, octree=vrc.Octree(desc, root, dim), settings=settings)
        whole = _check_scene(c, mat, dim, regions, pts, settings)[0]
        for x, y, z, k in cubes:
            assert (whole[0, z:z + k, y:y + k, x:x + k] == 5).all()
        del c


@pytest.mark.parametrize("depth", [12, 14])
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

    size = (32, 32, 48)
    xy = rng.integers(0, dim - 32, size=(64, 2))
    xy[:4] = [(-7, 100), (dim - 20, dim - 9), (0, 0), (dim - 32, 3)]          # across the map's edges and at its corners
    hi = np.array([column(int(np.clip(x + 16, 0, dim - 1)), int(np.clip(y + 16, 0, dim - 1)))[1] for x, y in xy])
    surface = np.stack([xy[:, 0], xy[:, 1], hi - rng.integers(8, 40, size=64)], axis=1)
    sky = np.stack([xy[:8, 0], xy[:8, 1], np.full(8, dim - 30)], axis=1)      # the top 30 layers and 18 above the map
    c_lo = np.array([column(int(np.clip(x, 0, dim - 1)), int(np.clip(y, 0, dim - 1)))[0] for x, y in xy[:8]])
    below = np.stack([xy[:8, 0], xy[:8, 1], c_lo - 60], axis=1)
    lo = np.concatenate([surface, sky, below]).astype(I)
    got = c.read_regions(lo, size)
    solid = 0
    for i, corner in enumerate(lo):
        want = vr.column_region(depth, corner, size, column)
        assert np.array_equal(got[i], want), (i, corner, np.argwhere(got[i] != want)[:4])
        solid += int(np.count_nonzero(want))
    assert solid > 64 * 32 * 32 // 2
    # points on the same columns: the shell, one voxel above and below it, the map's floor and ceiling
    pts = []
    for x, y in xy[4:36]:
        c0, c1 = column(int(x), int(y))
        pts += [(x, y, z) for z in (c0 - 1, c0, (c0 + c1) // 2, c1, c1 + 1, 0, dim - 1, dim, -1)]
    pts = np.array(pts, I)
    want = np.array([5 if (column(int(x), int(y))[0] <= z <= column(int(x), int(y))[1] and 0 <= z < dim) else 0 for x, y, z in pts], I)
    assert np.array_equal(c.get_voxels(pts), want)
    del c
    gc.collect()


def _built_from_grid(grid, depth, atlas, s):
    c = vrc.CLCaster()
    assert c.init(0)
    dim = 1 << depth
    info = c.build_dense_grid(depth, grid, attachments=True)
    assert info["n_descriptors"] > 0
    li = np.zeros((8, 10), dtype=np.float32)
    li[:1] = s["lights"][:1]
    from gpu_helpers import configure
    configure(c, dim, atlas, s["cam_dir"], s["cam_pos"], li, 96, 64)
    assert c.validate(), c.last_error()
    return c


def test_round_trip_through_build_dense_grid(atlas):
    s = scenes.random_sparse()
    dim, depth = s["dim"], 6
    grid = np.asarray(s["grid"], np.int8).copy()
    rng = np.random.default_rng(21)
    solid = np.nonzero(grid)[0]
    grid[rng.choice(solid, size=solid.size // 10, replace=False)] = 6
    a = _built_from_grid(grid, depth, atlas, s)
    first = a.read_regions(np.zeros((1, 3), I), (dim,) * 3)
    assert np.array_equal(first.reshape(-1), grid)
    assert set(np.unique(first).tolist()) == {0, 5, 6}
    b = _built_from_grid(first.reshape(-1), depth, atlas, s)
    assert np.array_equal(a.read_descriptors(), b.read_descriptors())
    second = b.read_regions(np.zeros((1, 3), I), (dim,) * 3)
    assert second.tobytes() == first.tobytes()


def _frame_index_materials(mp, dx, dy, dz):
    """mat[x, y, z] of a dense map read by the frame's index x + dx * (y + dz * z); an index past the array is 0."""
    x, y, z = np.meshgrid(np.arange(dx), np.arange(dy), np.arange(dz), indexing="ij")
    idx = x + dx * (y + dz * z)
    return np.where(idx < mp.size, mp[np.minimum(idx, mp.size - 1)], 0).astype(np.int8)


def _check_against_box_query(c, dims, rng, n=200):
    lo = np.stack([rng.integers(-3, d + 2, size=n) for d in dims], axis=1).astype(I)
    ext = rng.integers(1, 7, size=(n, 3)).astype(I)
    boxes = np.concatenate([lo, ext], axis=1).astype(np.float32)
    rec, cnt, vox = c.box_intersection(boxes, max_voxels=6 ** 3)
    assert not (rec[:, 0] & (vrc.BOX_TRUNCATED | vrc.BOX_REJECTED)).any()
    nonzero = 0
    for i in range(n):
        r = c.read_regions(lo[i:i + 1], ext[i])[0]
        z, y, x = np.nonzero(r)
        mine = {(int(a + lo[i, 0]), int(b + lo[i, 1]), int(d + lo[i, 2]), int(r[d, b, a])) for a, b, d in zip(x, y, z)}
        listed = {tuple(int(v) for v in e) for e in vox[i, :rec[i, 7]]}
        assert rec[i, 7] == cnt[i] and mine == listed, (i, boxes[i], sorted(mine ^ listed)[:4])
        nonzero += len(mine)
    assert nonzero > n


def test_regions_agree_with_the_box_query(atlas):
    rng = np.random.default_rng(33)
    # a non-cubic dense map in the array branch: y stride dz, so rows alias and the last rows read past the array's rows
    dx, dy, dz = 16, 8, 4
    mp = rng.choice(np.array([0, 0, 5, 6, 1, -2], np.int8), size=dx * dy * dz)
    s = dict(scenes.axis_aligned(16))
    c = vrc.CLCaster()
    assert c.init(0)
    from gpu_helpers import configure
    li = np.zeros((8, 10), dtype=np.float32)
    li[:1] = s["lights"][:1]
    configure(c, 16, atlas, s["cam_dir"], s["cam_pos"], li, 96, 64)
    assert c.overwrite_setting("using_octree", 1)
    assert c.assign_octree(vrc.Octree.Generate(np.asarray(s["grid"], np.int8), 16)) and c.assign_map(mp, (dx, dy, dz))
    assert c.validate(), c.last_error()
    _check_against_box_query(c, (dx, dy, dz), rng)
    mat = _frame_index_materials(mp, dx, dy, dz)
    assert np.array_equal(c.read_regions(np.full((1, 3), -2, I), (dx + 4, dy + 4, dz + 4)), vr.regions(mat, [[-2, -2, -2]], (dx + 4, dy + 4, dz + 4)))
    g = np.stack(np.meshgrid(np.arange(-1, dx + 1), np.arange(-1, dy + 1), np.arange(-1, dz + 1), indexing="ij"), axis=-1).reshape(-1, 3)
    assert np.array_equal(c.get_voxels(g), vr.points(mat, g))
    # ... and the SVO branch with materials
    s = dict(scenes.random_sparse())
    s["grid"] = _with_materials(s["grid"], 3)
    tree = vrc.Octree.Generate(s["grid"], s["dim"]).attach_materials_from_grid(s["grid"])
    _check_against_box_query(_caster(s, atlas, octree=tree), (s["dim"],) * 3, rng)


def test_device_path(atlas):
    torch = pytest.importorskip("torch")
    s = dict(scenes.random_sparse())
    dim = s["dim"]
    s["grid"] = _with_materials(s["grid"], 4)
    tree = vrc.Octree.Generate(s["grid"], dim).attach_materials_from_grid(s["grid"])
    c = _caster(s, atlas, octree=tree)
    rng = np.random.default_rng(8)
    dev_before = torch.cuda.current_device()
    for size, n in (((8, 8, 8), 40), ((13, 5, 9), 40), ((dim, dim, dim), 1), ((1, 1, 1), 9)):
        lo = (np.zeros((1, 3), I) if n == 1 else rng.integers(-10, dim + 3, size=(n, 3)).astype(I))
        host = c.read_regions(lo, size)
        total = host.size
        tl = torch.from_numpy(lo).to("cuda:0")
        for offset in (0, 1):                                  # offset 1: the base pointer is odd
            buf = torch.full((total + offset + 16,), SENTINEL, dtype=torch.int8, device="cuda:0")
            out = buf[offset:]
            assert out.data_ptr() % 2 == offset
            assert c.read_regions_device(tl.data_ptr(), n, size, out.data_ptr(), total), c.last_error()
            got = buf.cpu().numpy()
            assert np.array_equal(got[offset:offset + total], host.reshape(-1)), (size, offset)
            assert (got[:offset] == SENTINEL).all() and (got[offset + total:] == SENTINEL).all()
    # no sentinel survives inside n V even where the scene is empty: a region in the sky
    buf = torch.full((8 * 8 * 8 + 1,), SENTINEL, dtype=torch.int8, device="cuda:0")
    tl = torch.tensor([[3, 3, dim + 40]], dtype=torch.int32, device="cuda:0")
    assert c.read_regions_device(tl.data_ptr(), 1, (8, 8, 8), buf.data_ptr(), 512)
    got = buf.cpu().numpy()
    assert (got[:512] == 0).all() and got[512] == SENTINEL
    pts = _all_points(dim, rng)[::7].copy()
    tp = torch.from_numpy(pts).to("cuda:0")
    vals = torch.full((len(pts) + 1,), SENTINEL, dtype=torch.int32, device="cuda:0")
    assert c.get_voxels_device(tp.data_ptr(), len(pts), vals.data_ptr()), c.last_error()
    v = vals.cpu().numpy()
    assert np.array_equal(v[:-1], c.get_voxels(pts)) and v[-1] == SENTINEL
    # misaligned 4-byte pointers are refused; the region output may have any alignment (above)
    raw = torch.zeros(64, dtype=torch.int8, device="cuda:0")
    assert vrc.lib.vrc_get_voxels_device(c._h, C.c_void_p(raw.data_ptr() + 1), 2, C.c_void_p(vals.data_ptr())) == 1
    assert vrc.lib.vrc_get_voxels_device(c._h, C.c_void_p(tp.data_ptr()), 2, C.c_void_p(raw.data_ptr() + 2)) == 1
    size3 = np.array([2, 2, 2], I)
    assert vrc.lib.vrc_read_regions_device(c._h, C.c_void_p(raw.data_ptr() + 2), 1, size3.ctypes.data_as(C.POINTER(C.c_int32)),
                                           C.c_void_p(raw.data_ptr() + 32), 8) == 1
    assert torch.cuda.current_device() == dev_before


def test_group_handle_equals_a_single_handle(atlas):
    torch = pytest.importorskip("torch")
    s = scenes.floor_pillars()
    dim = s["dim"]
    rng = np.random.default_rng(12)
    lo = rng.integers(-10, dim + 3, size=(50, 3)).astype(I)
    pts = _all_points(dim, rng)
    single = _caster(s, atlas)
    dev_before = torch.cuda.current_device()
    group = _caster(s, atlas, group=[0, 0])
    assert np.array_equal(group.read_regions(lo, (9, 8, 7)), single.read_regions(lo, (9, 8, 7)))
    assert np.array_equal(group.read_regions(np.zeros((1, 3), I), (dim,) * 3), single.read_regions(np.zeros((1, 3), I), (dim,) * 3))
    assert np.array_equal(group.get_voxels(pts), single.get_voxels(pts))
    assert torch.cuda.current_device() == dev_before


def test_read_between_async_and_sync_leaves_the_frame(atlas):
    s = scenes.terrain256()
    dim = s["dim"]
    ref = _caster(s, atlas)
    assert ref.compute()
    img0, hits0, ctr0, k0 = ref.read_image().copy(), ref.read_hits().copy(), ref.counters(), ref.last_kernel()
    c = _caster(s, atlas)
    rng = np.random.default_rng(5)
    lo = rng.integers(-10, dim, size=(300, 3)).astype(I)
    pts = rng.integers(-4, dim + 4, size=(20000, 3)).astype(I)
    assert c.timing_reset()
    assert c.compute_async()
    r = c.read_regions(lo, (16, 16, 16))
    p = c.get_voxels(pts)
    assert c.sync()
    assert np.array_equal(c.read_image().view(np.uint32), img0.view(np.uint32))
    assert np.array_equal(c.read_hits(), hits0) and c.counters() == ctr0 and c.last_kernel() == k0
    assert c.timing()[0] == 1
    assert np.array_equal(r, c.read_regions(lo, (16, 16, 16))) and np.array_equal(p, c.get_voxels(pts))
    mat = br.grid_xyz(s["grid"], dim)
    assert np.array_equal(r, vr.regions(np.where(mat != 0, 5, 0).astype(np.int8), lo, (16, 16, 16)))


def test_argument_errors_and_released_staging(atlas):
    s = scenes.floor_pillars()
    dim = s["dim"]
    c = _caster(s, atlas)
    lib = vrc.lib
    pos = np.array([[5, 5, 0], [5, 5, 1], [40, 0, 0], [0, 0, 31]], I)
    val = np.full(4, SENTINEL, I)
    size = np.array([4, 4, 4], I)
    out = np.full(4 * 64, SENTINEL, np.int8)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    bp = out.ctypes.data_as(C.POINTER(C.c_int8))
    assert lib.vrc_get_voxels(None, ip(pos), 4, ip(val)) == 1
    assert lib.vrc_get_voxels(c._h, None, 4, ip(val)) == 1
    assert lib.vrc_get_voxels(c._h, ip(pos), 4, None) == 1
    assert lib.vrc_get_voxels(c._h, ip(pos), -1, ip(val)) == 1 and "n = -1" in c.last_error()
    assert lib.vrc_read_regions(None, ip(pos), 4, ip(size), bp, out.size) == 1
    assert lib.vrc_read_regions(c._h, None, 4, ip(size), bp, out.size) == 1
    assert lib.vrc_read_regions(c._h, ip(pos), 4, None, bp, out.size) == 1
    assert lib.vrc_read_regions(c._h, ip(pos), 4, ip(size), None, out.size) == 1
    assert lib.vrc_read_regions(c._h, ip(pos), -2, ip(size), bp, out.size) == 1
    for bad in ([0, 4, 4], [4, -1, 4], [4, 4, 0]):
        assert lib.vrc_read_regions(c._h, ip(pos), 4, ip(np.array(bad, I)), bp, out.size) == 1 and "size" in c.last_error()
    assert lib.vrc_read_regions(c._h, ip(pos), 4, ip(size), bp, out.size - 1) == 1            # n_bytes < n V
    huge = np.array([2 ** 31 - 1] * 3, I)
    assert lib.vrc_read_regions(c._h, ip(pos), 4, ip(huge), bp, out.size) == 6                # n V overflows size_t
    assert lib.vrc_read_regions(c._h, ip(pos), 1 << 62, ip(size), bp, out.size) == 6
    assert lib.vrc_get_voxels_device(c._h, ip(pos), 4, ip(val)) == 1                          # pageable host memory is not device memory
    assert lib.vrc_read_regions_device(c._h, ip(pos), 4, ip(size), bp, out.size) == 1
    assert (val == SENTINEL).all() and (out == SENTINEL).all()                                # nothing was launched
    assert lib.vrc_get_voxels(c._h, ip(pos), 0, ip(val)) == 0 and lib.vrc_get_voxels_device(c._h, None, 0, None) == 0
    assert lib.vrc_read_regions(c._h, ip(pos), 0, ip(size), bp, 0) == 0 and lib.vrc_read_regions_device(c._h, None, 0, ip(size), None, 0) == 0
    assert (val == SENTINEL).all() and (out == SENTINEL).all()
    mat = br.grid_xyz(s["grid"], dim)
    assert lib.vrc_get_voxels(c._h, ip(pos), 4, ip(val)) == 0 and val.tolist() == vr.points(mat, pos).tolist() == [5, 5, 0, 0]
    assert lib.vrc_read_regions(c._h, ip(pos), 4, ip(size), bp, out.size) == 0
    assert np.array_equal(out.reshape(4, 4, 4, 4), vr.regions(mat, pos, size))
    # release_viewport frees the staging (and un-validates the handle): the next read grows it again
    before = c.read_regions(np.zeros((1, 3), I), (dim,) * 3)
    assert c.release_viewport()
    assert lib.vrc_get_voxels(c._h, ip(pos), 4, ip(val)) == 2 and lib.vrc_read_regions(c._h, ip(pos), 4, ip(size), bp, out.size) == 2
    assert c.create_viewport(96, 64) and c.validate(), c.last_error()
    assert np.array_equal(c.read_regions(np.zeros((1, 3), I), (dim,) * 3), before)
    assert c.get_voxels(pos).tolist() == [5, 5, 0, 0]
    fresh = vrc.CLCaster()
    assert fresh.init(0)
    assert lib.vrc_get_voxels(fresh._h, ip(pos), 4, ip(val)) == 2 and "validate" in fresh.last_error()
    assert lib.vrc_read_regions(fresh._h, ip(pos), 4, ip(size), bp, out.size) == 2
    assert c.release_octree()
    assert lib.vrc_get_voxels(c._h, ip(pos), 4, ip(val)) == 2
