"""GPU suite (-m gpu): batched box-overlap queries (vrc_box_intersection / _device, csrc/box_query.hip).

Random boxes equal the numpy replay (tests/box_replay.py) on every record field, count and list entry in four configurations,
the SVO branch equals the array branch, solid leaves above the bottom count by volume and truncate in Morton order, device-built
shell terrains equal the column replay and a whole-map box the tree's own voxel count, ground height agrees with a ray cast
straight down, the host and device paths and group handles agree, a query leaves a frame in flight untouched, and argument
errors return their codes."""
import ctypes as C
import gc

import numpy as np
import pytest

import box_replay as br
import leaftree
import scenes
import voxel_raycaster_amd as vrc
from gpu_helpers import configure

pytestmark = pytest.mark.gpu
F = np.float32
MAXV = (0, 1, 17, 4096)


def _caster(s, atlas, using_octree=0, settings=(), octree=None, device_tree=None, group=None):
    c = vrc.CLCaster()
    assert (c.init_group(group, own_copies=True) if group else c.init(0)), c.last_error()
    dim = s["dim"]
    li = np.zeros((8, 10), dtype=F)
    li[:1] = s["lights"][:1]
    configure(c, dim, atlas, s["cam_dir"], s["cam_pos"], li, 96, 64, shadow_rays=1)
    assert c.overwrite_setting("using_octree", using_octree)
    for k, v in settings:
        assert c.add_to_settings_buffer(k, k.upper(), v), c.last_error()
    if device_tree is not None:
        info, _ = c.build_shell_terrain(device_tree, 1, 2, 2)
        assert info["n_descriptors"] > 0
    else:
        tree = octree if octree is not None else vrc.Octree.Generate(np.asarray(s["grid"], np.int8), dim)
        assert c.assign_octree(tree), c.last_error()
        assert c.assign_map(np.asarray(s["grid"], np.int8), (dim,) * 3)
    assert c.validate(), c.last_error()
    return c


def _derive(full, maxv):
    """The replay's answer for max_voxels = maxv from its answer for the largest max_voxels (a prefix of one full list)."""
    rec, counts, vox = full
    r = rec.copy()
    r[:, 0] &= ~br.TRUNCATED
    if maxv > 0:
        r[:, 0] |= np.where(counts > maxv, br.TRUNCATED, 0).astype(np.int32)
    r[:, 7] = np.minimum(counts, maxv)
    if maxv == 0:
        return r, counts, None
    v = vox[:, :maxv].copy()
    return r, counts, v


def _check(c, boxes, replays, tag):
    for stopping in (False, True):
        full = replays[stopping].query(boxes, max(MAXV))
        for maxv in MAXV:
            rec, cnt, vox = c.box_intersection(boxes, max_voxels=maxv, stopping_only=stopping)
            er, ec, ev = _derive(full, maxv)
            bad = np.nonzero((rec != er).any(1) | (cnt != ec))[0]
            assert bad.size == 0, (tag, stopping, maxv, bad[:4], rec[bad[:2]], er[bad[:2]], cnt[bad[:2]], ec[bad[:2]], boxes[bad[:2]])
            if maxv:
                badl = np.nonzero((vox != ev).any(axis=(1, 2)))[0]
                assert badl.size == 0, (tag, stopping, maxv, badl[:4], boxes[badl[:2]])


CONFIGS = [("svo-attached", 0, (), True), ("svo-plain", 0, (), False), ("svo-no-table", 0, (("coarse_log2", 0),), True),
           ("array", 1, (), True)]


@pytest.mark.parametrize("make", scenes.ALL + [scenes.terrain256], ids=lambda m: m.__name__)
def test_random_boxes_equal_the_replay(atlas, make):
    s = make()
    dim = s["dim"]
    grid = np.asarray(s["grid"], np.int8)
    mat = br.grid_xyz(grid, dim)
    plain = np.where(mat != 0, 5, 0).astype(np.int8)
    replays = {True: {st: br.GridReplay(mat, st) for st in (False, True)},
               False: {st: br.GridReplay(plain, st) for st in (False, True)}}
    rng = np.random.default_rng(dim + 17)
    boxes = br.random_boxes(rng, 1000 if dim >= 256 else 2000, dim)
    results = {}
    for name, using_octree, settings, attached in CONFIGS:
        tree = vrc.Octree.Generate(grid, dim)
        if attached:
            tree = tree.attach_materials_from_grid(grid)
        c = _caster(s, atlas, using_octree=using_octree, settings=settings, octree=tree)
        _check(c, boxes, replays[attached], name)
        results[name] = c.box_intersection(boxes, max_voxels=17)
        del c
    # the SVO branch with the grid's materials is the array branch
    for a, b in zip(results["svo-attached"], results["array"]):
        assert np.array_equal(a, b)


def test_solid_leaves_count_by_volume(atlas):
    depth = 5
    dim = 1 << depth
    cubes = [(0, 0, 0, 4), (8, 8, 8, 8), (4, 0, 0, 2), (16, 16, 0, 4), (20, 4, 6, 2)]
    rng = np.random.default_rng(5)
    vox = rng.integers(0, dim, size=(300, 3))
    desc, root, grid = leaftree.leaf_octree(vox, cubes, depth)
    s = dict(scenes.floor_pillars(dim))
    s["grid"] = grid
    c = _caster(s, atlas, octree=vrc.Octree(desc, root, dim))
    rep = {st: br.GridReplay(br.grid_xyz(grid, dim), st) for st in (False, True)}
    boxes = br.random_boxes(rng, 1500, dim)
    # boxes inside and across the leaf cubes: truncated lists inside a solid cube
    extra = np.array([[8.5, 8.5, 8.5, 5, 5, 5], [9, 9, 9, 2, 2, 2], [0, 0, 0, 4, 4, 4], [1.5, 0.5, 0.5, 4, 1, 1],
                      [7, 7, 7, 10, 10, 10], [0, 0, 0, 32, 32, 32]], F)
    boxes = np.concatenate([extra, boxes]).astype(F)
    _check(c, boxes, rep, "leaves")
    rec, cnt, v = c.box_intersection(extra, max_voxels=5)
    assert cnt[0] == 6 ** 3 and cnt[1] == 8 and cnt[2] == 64                    # [8, 14)^3, [9, 11)^3 in the 8^3 leaf; the 4^3 leaf
    assert (rec[:3, 0] & vrc.BOX_TRUNCATED).all()
    assert v[2].tolist() == [[0, 0, 0, 5], [1, 0, 0, 5], [0, 1, 0, 5], [1, 1, 0, 5], [0, 0, 1, 5]]
    # the same tree without its coarse table descends from the root
    c2 = _caster(s, atlas, octree=vrc.Octree(desc, root, dim), settings=(("coarse_log2", 0),))
    for a, b in zip(c.box_intersection(boxes, 17), c2.box_intersection(boxes, 17)):
        assert np.array_equal(a, b)


def _shell_boxes(rng, depth, n, sizes):
    dim = 1 << depth
    xy = rng.uniform(0, dim - 64, size=(n, 2))
    hi = np.array([vrc.shell_column(depth, int(x), int(y))[1] for x, y in xy], dtype=np.float64)
    ext = np.array([sizes[i % len(sizes)] for i in range(n)], dtype=np.float64)
    o = np.stack([xy[:, 0], xy[:, 1], hi - ext[:, 2] / 2 + rng.uniform(-1, 1, size=n)], axis=1)
    return np.concatenate([o, ext], axis=1).astype(F)


@pytest.mark.parametrize("depth", [12, 14, 16])
def test_shell_terrains_equal_the_columns(atlas, depth):
    import bench
    sc = bench.device_scene_header(depth)
    s = dict(dim=sc["dim"], cam_dir=sc["cam_dir"], cam_pos=sc["cam_pos"], lights=sc["lights"])
    c = _caster(s, atlas, device_tree=depth)
    rng = np.random.default_rng(depth)
    cols = {}

    def column(x, y):
        if (x, y) not in cols:
            cols[(x, y)] = vrc.shell_column(depth, x, y)
        return cols[(x, y)]

    boxes = _shell_boxes(rng, depth, 60, [(0.6, 0.6, 1.8), (3, 2, 5), (9.5, 7.25, 12), (24, 24, 24)])
    rec, cnt, vox = c.box_intersection(boxes, max_voxels=64)
    er, ec = br.column_replay(boxes, depth, column)
    assert np.array_equal(cnt, ec)
    assert np.array_equal(rec[:, 0], er[:, 0] | np.where(ec > 64, br.TRUNCATED, 0))
    assert np.array_equal(rec[:, 1:7], er[:, 1:7]) and np.array_equal(rec[:, 7], np.minimum(ec, 64))
    assert (cnt > 0).sum() > len(boxes) // 2
    lo, hi, _, _ = br.box_ranges(boxes, (1 << depth,) * 3)
    for i in range(len(boxes)):
        if (hi[i] - lo[i]).prod() <= 600:
            lst = br.column_list(lo[i], hi[i], column, 64)
            assert np.array_equal(vox[i, :len(lst)], lst), i
    del c
    gc.collect()


def _tree_voxel_count(c):
    """Solid voxels of the resident tree from its descriptors: a level-by-level walk over frontier arrays (far pointers
    resolved), bottom-level popcounts plus the volumes of the solid leaves above the bottom."""
    ncount, root = c.octree_size()
    desc = np.empty(ncount, np.uint64)
    step = 1 << 24
    for s in range(0, ncount, step):
        k = min(step, ncount - s)
        desc[s:s + k] = c.read_descriptors(s, k)
    depth = int(round(np.log2(c.get_setting("octree_dimensions"))))
    front = np.array([root], np.uint64)
    total = 0
    popc = np.array([bin(i).count("1") for i in range(256)], np.int64)
    for level in range(depth):
        d = desc[front.astype(np.int64)]
        valid = ((d >> np.uint64(16)) & np.uint64(0xff)).astype(np.int64)
        leaf = ((d >> np.uint64(24)) & np.uint64(0xff)).astype(np.int64)
        if level == depth - 1:
            total += int(popc[valid].sum())
            break
        child_size = 1 << (depth - level - 1)
        total += int(popc[valid & leaf].sum()) * child_size ** 3
        ptr = (d & np.uint64(0x7fff)).astype(np.int64)
        base = front.astype(np.int64) + ptr
        far = (d & np.uint64(0x8000)) != 0
        base[far] = desc[base[far]].astype(np.int64)
        nxt = []
        for i in range(8):
            keep = ((valid >> i) & 1).astype(bool) & ~((leaf >> i) & 1).astype(bool)
            rank = popc[valid & ((2 << i) - 1)] - 1
            nxt.append((base + rank)[keep])
        front = np.concatenate(nxt).astype(np.uint64)
    return total


def test_whole_map_count_at_depth_12(atlas):
    import bench
    depth = 12
    sc = bench.device_scene_header(depth)
    s = dict(dim=sc["dim"], cam_dir=sc["cam_dir"], cam_pos=sc["cam_pos"], lights=sc["lights"])
    c = _caster(s, atlas, device_tree=depth)
    dim = 1 << depth
    rec, cnt, _ = c.box_intersection(np.array([[0, 0, 0, dim, dim, dim]], F))
    assert cnt[0] == _tree_voxel_count(c)
    assert rec[0, 0] == vrc.BOX_ANY and cnt[0] > dim * dim
    del c
    gc.collect()


def test_ground_height_equals_a_ray_down(atlas):
    s = scenes.terrain256()
    dim = s["dim"]
    grid = np.asarray(s["grid"], np.int8)
    tree = vrc.Octree.Generate(grid, dim).attach_materials_from_grid(grid)
    rng = np.random.default_rng(9)
    n = 3000
    xy = rng.integers(0, dim, size=(n, 2))
    z0 = rng.integers(1, dim, size=n)
    boxes = np.stack([xy[:, 0] + 0.5, xy[:, 1] + 0.5, np.zeros(n), np.zeros(n), np.zeros(n), z0], axis=1).astype(F)
    rays = np.stack([xy[:, 0] + 0.5, xy[:, 1] + 0.5, z0 + 0.5, np.zeros(n), np.zeros(n), -np.ones(n)], axis=1).astype(F)
    for using_octree in (0, 1):
        c = _caster(s, atlas, using_octree=using_octree, octree=tree)
        rec, _, _ = c.box_intersection(boxes, stopping_only=True)
        hits = c.cast_rays(rays)
        hit = hits[:, 5] == vrc.RAY_HIT
        assert np.array_equal(rec[:, 6] == -1, ~hit)
        assert np.array_equal(rec[hit, 6], hits[hit, 2])
        assert hit.sum() > n // 4


def test_device_path_and_group_equal_host_path(atlas):
    torch = pytest.importorskip("torch")
    s = scenes.terrain256()
    c = _caster(s, atlas)
    boxes = br.random_boxes(np.random.default_rng(3), 5000, s["dim"])
    host = c.box_intersection(boxes, max_voxels=17, stopping_only=True)
    tb = torch.from_numpy(boxes).to("cuda:0")
    rec = torch.full((len(boxes), 8), -7, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((len(boxes),), -7, dtype=torch.int64, device="cuda:0")
    vox = torch.full((len(boxes), 17, 4), -1, dtype=torch.int32, device="cuda:0")
    assert c.box_intersection_device(tb.data_ptr(), len(boxes), rec.data_ptr(), cnt.data_ptr(), vox.data_ptr(), max_voxels=17,
                                     stopping_only=True), c.last_error()
    assert np.array_equal(rec.cpu().numpy(), host[0]) and np.array_equal(cnt.cpu().numpy(), host[1])
    assert np.array_equal(vox.cpu().numpy(), host[2])
    assert c.box_intersection_device(tb.data_ptr(), len(boxes), rec.data_ptr(), cnt.data_ptr())
    r0 = c.box_intersection(boxes)
    assert np.array_equal(rec.cpu().numpy(), r0[0]) and np.array_equal(cnt.cpu().numpy(), r0[1])
    dev_before = torch.cuda.current_device()
    group = _caster(s, atlas, group=[0, 0])
    for a, b in zip(group.box_intersection(boxes, max_voxels=17), c.box_intersection(boxes, max_voxels=17)):
        assert np.array_equal(a, b)
    assert torch.cuda.current_device() == dev_before


def test_query_between_async_and_sync_leaves_the_frame(atlas):
    s = scenes.terrain256()
    ref = _caster(s, atlas)
    assert ref.compute()
    img0, hits0, ctr0 = ref.read_image().copy(), ref.read_hits().copy(), ref.counters()
    c = _caster(s, atlas)
    boxes = br.random_boxes(np.random.default_rng(5), 20000, s["dim"])
    assert c.timing_reset()
    assert c.compute_async()
    q = c.box_intersection(boxes, max_voxels=4)
    assert c.sync()
    assert np.array_equal(c.read_image().view(np.uint32), img0.view(np.uint32))
    assert np.array_equal(c.read_hits(), hits0) and c.counters() == ctr0
    assert c.timing()[0] == 1
    for a, b in zip(q, c.box_intersection(boxes, max_voxels=4)):
        assert np.array_equal(a, b)


def test_argument_errors(atlas):
    s = scenes.floor_pillars()
    c = _caster(s, atlas)
    boxes = np.array([[5.5, 5.5, 0.0, 2, 2, 3]] * 4, F)
    rec = np.zeros((4, 8), np.int32)
    cnt = np.zeros(4, np.int64)
    vox = np.zeros((4, 2, 4), np.int32)
    fp = boxes.ctypes.data_as(C.POINTER(C.c_float))
    rp, cp, vp = (a.ctypes.data_as(t) for a, t in ((rec, C.POINTER(C.c_int32)), (cnt, C.POINTER(C.c_int64)), (vox, C.POINTER(C.c_int32))))
    lib = vrc.lib
    assert lib.vrc_box_intersection(None, fp, 4, 0, 0, rp, cp, None) == 1
    assert lib.vrc_box_intersection(c._h, None, 4, 0, 0, rp, cp, None) == 1
    assert lib.vrc_box_intersection(c._h, fp, 4, 0, 0, None, cp, None) == 1
    assert lib.vrc_box_intersection(c._h, fp, 4, 0, 0, rp, None, None) == 1
    assert lib.vrc_box_intersection(c._h, fp, 4, 2, 0, rp, cp, None) == 1          # a list without a buffer
    assert lib.vrc_box_intersection(c._h, fp, -1, 0, 0, rp, cp, None) == 1 and "n = -1" in c.last_error()
    assert lib.vrc_box_intersection(c._h, fp, 4, -3, 0, rp, cp, None) == 1
    assert lib.vrc_box_intersection(c._h, fp, 4, 0, 2, rp, cp, None) == 1 and "flag" in c.last_error()
    assert lib.vrc_box_intersection(c._h, fp, 1 << 62, 1 << 30, 0, rp, cp, vp) == 6
    assert lib.vrc_box_intersection_device(c._h, fp, 4, 0, 0, rp, cp, None) == 1    # pageable host memory is not device memory
    assert (rec == 0).all() and (cnt == 0).all()
    assert lib.vrc_box_intersection(c._h, fp, 0, 0, 0, rp, cp, None) == 0
    assert lib.vrc_box_intersection_device(c._h, None, 0, 0, 0, None, None, None) == 0
    assert lib.vrc_box_intersection(c._h, fp, 4, 2, 0, rp, cp, vp) == 0 and (rec[:, 0] & vrc.BOX_ANY).all()
    assert (rec[:, 7] == 2).all() and (vox[:, :, 3] != 0).all()
    fresh = vrc.CLCaster()
    assert fresh.init(0)
    assert lib.vrc_box_intersection(fresh._h, fp, 4, 0, 0, rp, cp, None) == 2 and "validate" in fresh.last_error()
    assert c.release_octree()
    assert lib.vrc_box_intersection(c._h, fp, 4, 0, 0, rp, cp, None) == 2
