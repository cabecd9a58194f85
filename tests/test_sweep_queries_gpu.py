"""GPU suite (-m gpu): batched swept-box queries (vrc_sweep_boxes / _device, csrc/box_sweep.hip).

All eight record fields of every sweep equal the numpy replay (tests/sweep_replay.py): every scene, both branches, with and
without attachments and the coarse table, both flags, both kernel shapes, capped events; solid leaves above the bottom;
device-built shell terrains against the column replay.  Cross-checks against the box queries (d = 0 sweeps, a box dropped onto
the ground), the host and device paths and group handles agree, a query leaves a frame in flight untouched, and argument errors
return their codes."""
import ctypes as C
import gc

import numpy as np
import pytest

import box_replay as br
import leaftree
import scenes
import sweep_replay as sr
import voxel_raycaster_amd as vrc
from gpu_helpers import configure

pytestmark = pytest.mark.gpu
F = np.float32


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


def _equal(rec, exp, sweeps, tag):
    bad = np.nonzero((rec != exp).any(axis=1))[0]
    assert bad.size == 0, (tag, len(bad), bad[:4], rec[bad[:3]], exp[bad[:3]], sweeps[bad[:3]])


def _check(c, sweeps, scenes_by_flag, tag, caps=(0,)):
    for stopping in (False, True):
        for cap in caps:
            exp = sr.sweep_replay(scenes_by_flag[stopping], sweeps, max_events=cap)
            _equal(c.sweep_boxes(sweeps, max_events=cap, stopping_only=stopping), exp, sweeps, (tag, stopping, cap))


CONFIGS = [("svo-attached", 0, (), True), ("svo-plain", 0, (), False), ("svo-no-table", 0, (("coarse_log2", 0),), True),
           ("array", 1, (), True)]


@pytest.mark.parametrize("make", scenes.ALL + [scenes.terrain256], ids=lambda m: m.__name__)
def test_random_sweeps_equal_the_replay(atlas, make):
    s = make()
    dim = s["dim"]
    grid = np.asarray(s["grid"], np.int8)
    mat = br.grid_xyz(grid, dim)
    plain = np.where(mat != 0, 5, 0).astype(np.int8)
    replays = {True: {st: sr.GridScene(mat, st) for st in (False, True)},
               False: {st: sr.GridScene(plain, st) for st in (False, True)}}
    rng = np.random.default_rng(dim + 29)
    sweeps = sr.random_sweeps(rng, 1200 if dim >= 256 else 2000, dim)
    expected = {(a, st): sr.sweep_replay(replays[a][st], sweeps) for a in (True, False) for st in (False, True)}
    kinds = np.bitwise_or.reduce(expected[(True, False)][:, 0])
    assert kinds & sr.REJECTED and kinds & sr.CLIPPED and kinds & sr.LEFT_MAP, kinds
    results = {}
    for name, using_octree, settings, attached in CONFIGS:
        tree = vrc.Octree.Generate(grid, dim)
        if attached:
            tree = tree.attach_materials_from_grid(grid)
        c = _caster(s, atlas, using_octree=using_octree, settings=settings, octree=tree)
        for st in (False, True):
            _equal(c.sweep_boxes(sweeps, stopping_only=st), expected[(attached, st)], sweeps, (name, st))
        results[name] = c.sweep_boxes(sweeps)
        if name == "svo-attached":
            # few events allowed, and each kernel shape alone: every sweep one lane, every sweep one wave
            for cap in (1, 6):
                _equal(c.sweep_boxes(sweeps, max_events=cap), sr.sweep_replay(replays[True][False], sweeps, max_events=cap), sweeps, (name, "cap", cap))
            assert c.add_to_settings_buffer("sweep_lane_face", "SWEEP_LANE_FACE", 0), c.last_error()
            for face in (0, 1 << 30):
                assert c.overwrite_setting("sweep_lane_face", face), c.last_error()
                _equal(c.sweep_boxes(sweeps), expected[(True, False)], sweeps, (name, "lane face", face))
        del c
    assert np.array_equal(results["svo-attached"], results["array"])


def test_every_outcome_occurs_on_the_terrain(atlas):
    """The seeded sweeps of the scene test are not all free: hits on all six faces, start-solid, capped, left-map, rejected."""
    s = scenes.terrain256()
    dim = s["dim"]
    grid = np.asarray(s["grid"], np.int8)
    c = _caster(s, atlas, octree=vrc.Octree.Generate(grid, dim).attach_materials_from_grid(grid))
    sweeps = sr.random_sweeps(np.random.default_rng(dim + 29), 1200, dim)
    rec = c.sweep_boxes(sweeps)
    hit = (rec[:, 0] & vrc.SWEEP_HIT) != 0
    assert set(rec[hit, 1].tolist()) == {-3, -2, -1, 1, 2, 3}
    assert hit.sum() > 80 and ((rec[:, 0] & vrc.SWEEP_START_SOLID) != 0).sum() > 80
    assert ((rec[:, 0] & vrc.SWEEP_LEFT_MAP) != 0).sum() > 20 and ((rec[:, 0] & vrc.SWEEP_REJECTED) != 0).sum() >= 6
    free = rec[:, 0] & ~vrc.SWEEP_CLIPPED == 0
    assert free.sum() > 50 and (rec[free, 2].copy().view(F) == 1).all()
    assert (c.sweep_boxes(sweeps, max_events=2)[:, 0] & vrc.SWEEP_EVENT_CAP).sum() > 200


def test_solid_leaves_above_the_bottom(atlas):
    depth = 5
    dim = 1 << depth
    cubes = [(0, 0, 0, 4), (8, 8, 8, 8), (4, 0, 0, 2), (16, 16, 0, 4), (20, 4, 6, 2)]
    rng = np.random.default_rng(5)
    vox = rng.integers(0, dim, size=(300, 3))
    desc, root, grid = leaftree.leaf_octree(vox, cubes, depth)
    s = dict(scenes.floor_pillars(dim))
    s["grid"] = grid
    rep = {st: sr.GridScene(br.grid_xyz(grid, dim), st) for st in (False, True)}
    sweeps = sr.random_sweeps(rng, 2500, dim)
    # onto, along and out of the 8^3 leaf at (8, 8, 8)
    extra = np.array([[10, 10, 20, 2, 2, 2, 0, 0, -9], [4.5, 10.5, 10.5, 1, 1, 1, 8, 0.5, 0.25], [10, 10, 16, 3, 3, 1, 5, 5, 0],
                      [9, 9, 9, 2, 2, 2, 30, 0, 0], [20.5, 12, 12, 0, 0, 0, -10, 0, 0], [0, 0, 0, 32, 32, 32, 1, 1, 1]], F)
    sweeps = np.concatenate([extra, sweeps]).astype(F)
    for settings in ((), (("coarse_log2", 0),)):
        c = _caster(s, atlas, octree=vrc.Octree(desc, root, dim), settings=settings)
        _check(c, sweeps, rep, ("leaves", settings), caps=(0, 3))
        rec = c.sweep_boxes(extra)
        assert rec[0].tolist() == [vrc.SWEEP_HIT, 3, (F(4) / F(9)).view(np.int32), 10, 10, 15, 5, rec[0, 7]]
        assert rec[1, 0] == vrc.SWEEP_HIT and rec[1, 1] == -1 and rec[1, 3] == 8
        assert rec[3, 0] & vrc.SWEEP_START_SOLID and rec[3, 3:6].tolist() == [9, 9, 9]
        assert rec[4, 0] == vrc.SWEEP_HIT and rec[4, 1] == 1 and rec[4, 3:6].tolist() == [15, 12, 12]
        del c


def _shell_sweeps(rng, depth, n, sizes):
    """Boxes a little above the surface of a shell terrain, moving down, sideways and diagonally by a few voxels."""
    dim = 1 << depth
    xy = rng.uniform(64, dim - 128, size=(n, 2))
    ext = np.array([sizes[i % len(sizes)] for i in range(n)], dtype=np.float64)
    # the highest of nine columns under the box: most boxes start in the air (steep terrain at depth 16), every sixth is sunk in
    top = np.array([max(vrc.shell_column(depth, int(x + fx * ex), int(y + fy * ey))[1] for fx in (0, 0.5, 1) for fy in (0, 0.5, 1))
                    for (x, y), (ex, ey) in zip(xy, ext[:, :2])], dtype=np.float64)
    o = np.stack([xy[:, 0], xy[:, 1], top + rng.uniform(1, 5, size=n)], axis=1)
    o[::6, 2] -= 4
    d = rng.normal(0, 5, size=(n, 3))
    d[:, 2] = -np.abs(d[:, 2]) - 2
    d[::3, :2] = 0                                               # straight down / up
    d[1::5, 2] *= -0.5                                           # some rise
    o[::7] = np.floor(o[::7])
    return np.concatenate([o, ext, d], axis=1).astype(F)


@pytest.mark.parametrize("depth", [12, 14, 16])
def test_shell_terrains_equal_the_columns(atlas, depth):
    import bench
    sc = bench.device_scene_header(depth)
    s = dict(dim=sc["dim"], cam_dir=sc["cam_dir"], cam_pos=sc["cam_pos"], lights=sc["lights"])
    c = _caster(s, atlas, device_tree=depth)
    cols = {}

    def column(x, y):
        if (x, y) not in cols:
            cols[(x, y)] = vrc.shell_column(depth, x, y)
        return cols[(x, y)]

    scene = sr.ColumnScene(depth, column)
    sweeps = _shell_sweeps(np.random.default_rng(depth), depth, 72, [(0.6, 0.6, 1.8), (3, 2, 5), (9.5, 7.25, 4), (0, 0, 0), (20, 20, 3)])
    exp = sr.sweep_replay(scene, sweeps)
    for stopping in (False, True):                                # (material 5 everywhere: the flag changes nothing)
        _equal(c.sweep_boxes(sweeps, stopping_only=stopping), exp, sweeps, (depth, stopping))
    assert ((exp[:, 0] & sr.HIT) != 0).sum() >= len(sweeps) // 4 and ((exp[:, 0] & sr.START_SOLID) != 0).sum() >= 3
    assert c.add_to_settings_buffer("coarse_log2", "COARSE_LOG2", 0), c.last_error()
    _equal(c.sweep_boxes(sweeps), exp, sweeps, (depth, "no table"))
    del c
    gc.collect()


def test_still_sweeps_equal_box_queries(atlas):
    """d = 0: START_SOLID iff the box query finds ANY, with the first voxel of its list; otherwise free with no event."""
    s = scenes.terrain256()
    dim = s["dim"]
    grid = np.asarray(s["grid"], np.int8)
    tree = vrc.Octree.Generate(grid, dim).attach_materials_from_grid(grid)
    boxes = br.random_boxes(np.random.default_rng(11), 4000, dim)
    sweeps = np.concatenate([boxes, np.zeros((len(boxes), 3), F)], axis=1)
    for using_octree in (0, 1):
        c = _caster(s, atlas, using_octree=using_octree, octree=tree)
        for stopping in (False, True):
            brec, _, bvox = c.box_intersection(boxes, max_voxels=1, stopping_only=stopping)
            rec = c.sweep_boxes(sweeps, stopping_only=stopping)
            any_ = (brec[:, 0] & vrc.BOX_ANY) != 0
            assert any_.sum() > 500 and (~any_).sum() > 500
            assert np.array_equal((rec[:, 0] & vrc.SWEEP_START_SOLID) != 0, any_)
            assert np.array_equal((rec[:, 0] & vrc.SWEEP_REJECTED) != 0, (brec[:, 0] & vrc.BOX_REJECTED) != 0)
            assert np.array_equal((rec[:, 0] & vrc.SWEEP_CLIPPED) != 0, (brec[:, 0] & vrc.BOX_CLIPPED) != 0)
            assert np.array_equal(rec[any_, 3:7], bvox[any_, 0])
            assert (rec[~any_, 3:7] == (-1, -1, -1, 0)).all() and (rec[:, 7] == 0).all() and (rec[:, 1] == 0).all()
            assert not (rec[:, 0] & (vrc.SWEEP_HIT | vrc.SWEEP_EVENT_CAP)).any()
            ok = (rec[:, 0] & (vrc.SWEEP_REJECTED | vrc.SWEEP_START_SOLID)) == 0
            assert (rec[ok, 2].copy().view(F) == 1).all() and (rec[~ok, 2] == 0).all()


def test_a_dropped_box_lands_on_the_ground_the_box_query_finds(atlas):
    """A box dropped straight down to z = 0 stops on the layer above records[6] (the highest counted voxel) of a box query
    over the column beneath it, at the time its lower face reaches that layer; with nothing beneath it falls freely."""
    s = scenes.terrain256()
    dim = s["dim"]
    grid = np.asarray(s["grid"], np.int8)
    tree = vrc.Octree.Generate(grid, dim).attach_materials_from_grid(grid)
    rng = np.random.default_rng(13)
    n = 3000
    xy = rng.uniform(0, dim - 4, size=(n, 2))
    w = rng.choice([0.0, 0.6, 2.5, 9.0], size=(n, 1)) * np.ones((1, 2))
    z0 = rng.integers(1, dim, size=n).astype(np.float64)
    h = rng.uniform(0.5, 3, size=n)
    sweeps = np.concatenate([xy, z0[:, None], w, h[:, None], np.zeros((n, 2)), -z0[:, None]], axis=1).astype(F)
    beneath = np.concatenate([xy, np.zeros((n, 1)), w, z0[:, None]], axis=1).astype(F)
    for using_octree in (0, 1):
        c = _caster(s, atlas, using_octree=using_octree, octree=tree)
        for stopping in (False, True):
            rec = c.sweep_boxes(sweeps, stopping_only=stopping)
            ground = c.box_intersection(beneath, stopping_only=stopping)[0][:, 6]
            moving = (rec[:, 0] & vrc.SWEEP_START_SOLID) == 0
            hit = (rec[:, 0] & vrc.SWEEP_HIT) != 0
            assert moving.sum() > n // 4 and not (hit & ~moving).any()
            assert np.array_equal(hit[moving], ground[moving] >= 0)
            assert np.array_equal(rec[hit, 5], ground[hit]) and (rec[hit, 1] == 3).all()
            t = (sweeps[hit, 2] - (ground[hit] + 1).astype(F)) / sweeps[hit, 2]
            assert np.array_equal(rec[hit, 2].copy().view(F), t.astype(F))
            free = moving & ~hit
            assert (rec[free, 2].copy().view(F) == 1).all()


def test_device_path_and_group_equal_host_path(atlas):
    torch = pytest.importorskip("torch")
    s = scenes.terrain256()
    c = _caster(s, atlas)
    sweeps = sr.random_sweeps(np.random.default_rng(3), 6000, s["dim"])
    host = c.sweep_boxes(sweeps, stopping_only=True)
    ts = torch.from_numpy(sweeps).to("cuda:0")
    rec = torch.full((len(sweeps), 8), -7, dtype=torch.int32, device="cuda:0")
    assert c.sweep_boxes_device(ts.data_ptr(), len(sweeps), rec.data_ptr(), stopping_only=True), c.last_error()
    assert np.array_equal(rec.cpu().numpy(), host)
    assert c.sweep_boxes_device(ts.data_ptr(), len(sweeps), rec.data_ptr(), max_events=4)
    assert np.array_equal(rec.cpu().numpy(), c.sweep_boxes(sweeps, max_events=4))
    # a 4-byte aligned view that is not 16-byte aligned
    flat = torch.zeros(len(sweeps) * 9 + 1, dtype=torch.float32, device="cuda:0")
    flat[1:] = ts.reshape(-1)
    out = torch.full((len(sweeps) * 8 + 3,), -7, dtype=torch.int32, device="cuda:0")
    assert c.sweep_boxes_device(flat.data_ptr() + 4, len(sweeps), out.data_ptr() + 12, stopping_only=True), c.last_error()
    assert np.array_equal(out[3:].cpu().numpy().reshape(-1, 8), host) and (out[:3] == -7).all()
    dev_before = torch.cuda.current_device()
    group = _caster(s, atlas, group=[0, 0])
    assert np.array_equal(group.sweep_boxes(sweeps, stopping_only=True), host)
    assert torch.cuda.current_device() == dev_before


def test_query_between_async_and_sync_leaves_the_frame(atlas):
    s = scenes.terrain256()
    ref = _caster(s, atlas)
    assert ref.compute()
    img0, hits0, ctr0 = ref.read_image().copy(), ref.read_hits().copy(), ref.counters()
    kernel0 = ref.last_kernel()
    c = _caster(s, atlas)
    sweeps = sr.random_sweeps(np.random.default_rng(5), 20000, s["dim"])
    assert c.timing_reset()
    assert c.compute_async()
    q = c.sweep_boxes(sweeps)
    assert c.sync()
    assert np.array_equal(c.read_image().view(np.uint32), img0.view(np.uint32))
    assert np.array_equal(c.read_hits(), hits0) and c.counters() == ctr0
    assert c.timing()[0] == 1 and c.last_kernel() == kernel0
    assert np.array_equal(q, c.sweep_boxes(sweeps))
    # the staging goes with the octree and comes back on demand
    assert c.release_octree()
    with pytest.raises(vrc.VrcError):
        c.sweep_boxes(sweeps[:4])


def test_argument_errors(atlas):
    s = scenes.floor_pillars()
    c = _caster(s, atlas)
    sweeps = np.array([[5.5, 5.5, 8.0, 1, 1, 1, 0, 0, -20]] * 4, F)
    rec = np.zeros((4, 8), np.int32)
    fp = sweeps.ctypes.data_as(C.POINTER(C.c_float))
    rp = rec.ctypes.data_as(C.POINTER(C.c_int32))
    lib = vrc.lib
    assert lib.vrc_sweep_boxes(None, fp, 4, 0, 0, rp) == 1
    assert lib.vrc_sweep_boxes(c._h, None, 4, 0, 0, rp) == 1
    assert lib.vrc_sweep_boxes(c._h, fp, 4, 0, 0, None) == 1
    assert lib.vrc_sweep_boxes(c._h, fp, -1, 0, 0, rp) == 1 and "n = -1" in c.last_error()
    assert lib.vrc_sweep_boxes(c._h, fp, 4, -3, 0, rp) == 1 and "max_events" in c.last_error()
    assert lib.vrc_sweep_boxes(c._h, fp, 4, 0, 2, rp) == 1 and "flag" in c.last_error()
    assert lib.vrc_sweep_boxes_device(c._h, fp, 4, 0, 0, rp) == 1          # pageable host memory is not device memory
    assert lib.vrc_sweep_boxes_device(c._h, C.c_void_p(2), 4, 0, 0, C.c_void_p(8)) == 1 and "aligned" in c.last_error()
    assert (rec == 0).all()
    assert lib.vrc_sweep_boxes(c._h, fp, 0, 0, 0, rp) == 0
    assert lib.vrc_sweep_boxes_device(c._h, None, 0, 0, 0, None) == 0
    assert lib.vrc_sweep_boxes(c._h, fp, 4, 0, 0, rp) == 0 and (rec[:, 0] == vrc.SWEEP_HIT).all() and (rec[:, 1] == 3).all()
    fresh = vrc.CLCaster()
    assert fresh.init(0)
    assert lib.vrc_sweep_boxes(fresh._h, fp, 4, 0, 0, rp) == 2 and "validate" in fresh.last_error()
    assert c.release_octree()
    assert lib.vrc_sweep_boxes(c._h, fp, 4, 0, 0, rp) == 2
