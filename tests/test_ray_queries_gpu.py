"""GPU suite (-m gpu): batched ray queries (vrc_cast_rays / vrc_cast_rays_device, csrc/raycast_query.hip).

Picking returns what a frame shows (AS_PIXEL over every pixel's ray), arbitrary rays equal the numpy replay (tests/ray_replay.py)
on every field, device-built trees equal the CPU oracle, the host and device paths agree, group handles agree, a query leaves a
frame in flight untouched, and argument errors return their codes."""
import ctypes as C
import gc

import numpy as np
import pytest

import ray_replay
import scenes
import voxel_raycaster_amd as vrc
from gpu_helpers import configure
from oracle import orc

pytestmark = pytest.mark.gpu
F = np.float32


def _caster(s, atlas, w=96, h=64, using_octree=0, settings=(), octree=None, shadow_rays=1, device_tree=None, group=None):
    c = vrc.CLCaster()
    assert (c.init_group(group, own_copies=True) if group else c.init(0)), c.last_error()
    dim = s["dim"]
    li = np.zeros((8, 10), dtype=F)
    li[:1] = s["lights"][:1]
    configure(c, dim, atlas, s["cam_dir"], s["cam_pos"], li, w, h, shadow_rays=shadow_rays)
    assert c.overwrite_setting("using_octree", using_octree)
    for k, v in settings:
        assert c.add_to_settings_buffer(k, k.upper(), v), c.last_error()
    if device_tree is not None:
        info, _ = c.build_shell_terrain(device_tree, 1, 2, 2)
        assert info["n_descriptors"] > 0
    else:
        tree = octree if octree is not None else vrc.Octree.Generate(np.asarray(s["grid"], np.int8), dim)
        assert c.assign_octree(tree), c.last_error()
        assert c.assign_map(np.asarray(s["grid"], np.int8), (dim,) * 3) if "grid" in s else True
    assert c.validate(), c.last_error()
    return c


def _pixel_rays(c, s, w, h):
    """Every pixel's primary ray, rotated on the host in float32 exactly as ray_setup does with the frame's trig."""
    vp = orc.create_viewport(w, h)
    tr = orc.camera_trig(np.asarray(s["cam_dir"], F))
    assert c.assign_camera_trig(tr)
    s1, c1, s2, c2 = (F(v) for v in tr)
    px, py, pz = vp[..., 0], vp[..., 1], vp[..., 2]
    x = pz * s1 + px * c1
    y = py
    z = pz * c1 - px * s1
    d = np.stack([x * c2 - y * s2, x * s2 + y * c2, z], axis=-1).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(s["cam_pos"], F), d.shape)
    return np.concatenate([o, d], axis=1).astype(F)


def _check_picking(c, s, w, h, md):
    rays = _pixel_rays(c, s, w, h)
    assert c.compute(), c.last_error()
    hits = c.read_hits().reshape(-1, 8)
    q = c.cast_rays(rays, max_steps=md, as_pixel=True)
    assert np.array_equal(q[:, :5], hits[:, :5]), f"{int((q[:, :5] != hits[:, :5]).any(1).sum())} pixels differ"
    assert c.overwrite_setting("shadow_rays", 0) and c.compute()
    h0 = c.read_hits().reshape(-1, 8)
    assert np.array_equal(q[:, 5] == vrc.RAY_REJECTED, (h0[:, 5] & 1) == 0)
    mirror = q[:, 3] == 6
    assert np.array_equal(q[~mirror, 6], h0[~mirror, 6])
    assert ((q[:, 5] == vrc.RAY_HIT) == (q[:, 0] >= 0)).all()
    assert c.overwrite_setting("shadow_rays", 1)
    return q


PICK_CONFIGS = [
    ("svo-default", 0, ()),
    ("svo-no-bias", 0, (("octree_bias", 0),)),
    ("svo-no-boxes", 0, (("empty_boxes", 0),)),
    ("svo-no-table", 0, (("coarse_log2", 0),)),
    ("array", 1, ()),
]


@pytest.mark.parametrize("cfg", PICK_CONFIGS, ids=[p[0] for p in PICK_CONFIGS])
@pytest.mark.parametrize("make", [scenes.floor_pillars, scenes.random_sparse, scenes.terrain256], ids=lambda m: m.__name__)
def test_picking_equals_the_frame(atlas, make, cfg):
    _, using_octree, settings = cfg
    s = make()
    w, h = 128, 96
    c = _caster(s, atlas, w, h, using_octree=using_octree, settings=settings)
    q = _check_picking(c, s, w, h, 3 * s["dim"])
    assert (q[:, 5] == vrc.RAY_HIT).sum() > 0


@pytest.mark.parametrize("make", [scenes.mirror_wall, scenes.near_mirror], ids=lambda m: m.__name__)
def test_picking_with_mirror_attachments(atlas, make):
    s = make()
    dim = s["dim"]
    tree = vrc.Octree.Generate(np.asarray(s["grid"], np.int8), dim).attach_materials_from_grid(s["grid"])
    c = _caster(s, atlas, 128, 96, octree=tree)
    q = _check_picking(c, s, 128, 96, 3 * dim)
    assert (q[:, 3] == 6).sum() > 0


@pytest.mark.parametrize("depth", [10, 12])
def test_picking_on_a_device_built_shell_terrain(atlas, depth):
    import bench
    sc = bench.device_scene_header(depth)
    s = dict(dim=sc["dim"], cam_dir=sc["cam_dir"], cam_pos=sc["cam_pos"], lights=sc["lights"])
    c = _caster(s, atlas, 256, 144, device_tree=depth)
    q = _check_picking(c, s, 256, 144, 3 * sc["dim"])
    assert (q[:, 5] == vrc.RAY_HIT).sum() > 256 * 144 // 4


def _arbitrary(rng, dim, n):
    r = ray_replay.random_rays(rng, n, dim)
    r[: n // 10, :3] = np.floor(r[: n // 10, :3])          # origins on voxel corners
    return r


@pytest.mark.parametrize("using_octree", [0, 1], ids=["svo", "array"])
@pytest.mark.parametrize("make", scenes.ALL + [scenes.mirror_wall, scenes.terrain256], ids=lambda m: m.__name__)
def test_arbitrary_rays_equal_the_replay(atlas, make, using_octree):
    s = make()
    dim = s["dim"]
    grid = np.asarray(s["grid"], np.int8)
    tree = vrc.Octree.Generate(grid, dim).attach_materials_from_grid(grid)
    c = _caster(s, atlas, octree=tree, using_octree=using_octree)
    rng = np.random.default_rng(dim + using_octree)
    rays = _arbitrary(rng, dim, 6000)
    for as_pixel in (False, True):
        bias = ray_replay.origin_bias(rays[:, :3], tree.descriptor_buffer, tree.root_index, dim) if as_pixel else None
        for max_steps in (0, 1, 5, 37):
            got = c.cast_rays(rays, max_steps=max_steps, as_pixel=as_pixel)
            ref = ray_replay.replay(rays, grid, (dim,) * 3, max_steps=max_steps, as_pixel=as_pixel, bias=bias)
            bad = np.nonzero((got != ref).any(1))[0]
            assert bad.size == 0, (as_pixel, max_steps, bad[:4], got[bad[:2]], ref[bad[:2]], rays[bad[:2]])


def test_safe_runs_and_their_traps(atlas):
    """An empty 256^3 map with a floor: long empty stretches (safe runs), |d| > 1 (delta_t < 1: no safe run), tiny components
    (t beyond 2^22), zero axes (+inf t never opens a gate nor wins a tie) -- every field equals the replay."""
    dim = 256
    g = np.zeros((dim, dim, dim), np.int8)
    g[0] = 5
    g[:, :, dim - 1] = 5
    s = dict(dim=dim, grid=g.reshape(-1), cam_pos=(100.5, 100.5, 200.5), cam_dir=(2.0, 1.5708), lights=scenes.floor_pillars()["lights"])
    c = _caster(s, atlas)
    rng = np.random.default_rng(7)
    n = 4000
    o = rng.uniform(1, dim - 1, size=(n, 3)).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[: n // 4] *= F(3.0)                                   # |d| > 1
    d[n // 4: n // 2, 0] = F(3e-6)                          # t_x far beyond 2^22
    d[n // 2: 5 * n // 8, 1] = F(0.0)                       # one +inf axis
    d[5 * n // 8: 3 * n // 4, :2] = F(0.0)                  # straight up / down
    rays = np.concatenate([o, d], axis=1).astype(F)
    for max_steps in (0, 200):
        got = c.cast_rays(rays, max_steps=max_steps)
        ref = ray_replay.replay(rays, g.reshape(-1), (dim,) * 3, max_steps=max_steps)
        assert np.array_equal(got, ref)
    down = c.cast_rays(np.array([[10.5, 20.5, 150.25, 0, 0, -1]], F))[0]
    assert down[:6].tolist() == [10, 20, 0, 5, 4, vrc.RAY_HIT] and down[6] == 149


@pytest.mark.parametrize("depth", [14, 16])
def test_device_built_big_trees_equal_the_oracle(atlas, depth):
    import bench
    sc = bench.device_scene_header(depth)
    dim = sc["dim"]
    s = dict(dim=dim, cam_dir=sc["cam_dir"], cam_pos=sc["cam_pos"], lights=sc["lights"])
    c = _caster(s, atlas, device_tree=depth)
    rng = np.random.default_rng(depth)
    n = 2000
    xy = rng.uniform(0, dim, size=(n, 2))
    z = np.array([vrc.shell_column(depth, int(x), int(y))[1] for x, y in xy], dtype=np.float64)
    o = np.stack([xy[:, 0], xy[:, 1], np.minimum(z + rng.uniform(1, 64, size=n), dim - 1)], axis=1).astype(F)
    d = rng.normal(size=(n, 3))
    d[:, 2] = -np.abs(d[:, 2]) - 0.3
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[: n // 8, :2] = 0.0                                    # ground height: straight down
    rays = np.concatenate([o, d.astype(F)], axis=1).astype(F)
    got = c.cast_rays(rays, max_steps=0)
    assert (got[:, 5] == vrc.RAY_HIT).sum() > n // 2
    assert (got[: n // 8, 5] == vrc.RAY_HIT).all()
    ncount, root = c.octree_size()
    paged = orc.PagedDescriptors(ncount, c.read_descriptors)
    sel = ~(rays[:, 3:] == 0).any(axis=1)                   # the frame rejects zero components
    ref = ray_replay.oracle_records(rays[sel], scene=s, descriptors=paged, root_index=root, using_octree=0, max_steps=0, atlas=atlas)
    assert np.array_equal(got[sel][:, :5], ref[:, :5]) and np.array_equal(got[sel][:, 6], ref[:, 6])
    iters = got[:, 6] + (got[:, 5] != vrc.RAY_STEP_CAP)
    assert np.array_equal(got[:, 7], ray_replay.entry_param(rays, iters))
    # straight down: field 7 is the height above the hit voxel's top face
    down = got[: n // 8]
    assert np.array_equal(down[:, 2] + 1, np.floor(rays[: n // 8, 2]).astype(np.int32) - down[:, 6])
    # the page table's fetch callback closes a reference cycle over the caster: give the tree's device memory back now, not at
    # the next cycle collection in some later test
    del paged, c
    gc.collect()


def test_device_path_equals_host_path(atlas):
    torch = pytest.importorskip("torch")
    s = scenes.terrain256()
    c = _caster(s, atlas)
    rays = _arbitrary(np.random.default_rng(3), s["dim"], 50000)
    host = c.cast_rays(rays, max_steps=0)
    tr = torch.from_numpy(rays).to("cuda:0")
    out = torch.full((len(rays), 8), -7, dtype=torch.int32, device="cuda:0")
    assert c.cast_rays_device(tr.data_ptr(), out.data_ptr(), len(rays)), c.last_error()
    assert np.array_equal(out.cpu().numpy(), host)
    assert c.cast_rays_device(tr.data_ptr(), out.data_ptr(), len(rays), max_steps=9, as_pixel=True)
    assert np.array_equal(out.cpu().numpy(), c.cast_rays(rays, max_steps=9, as_pixel=True))


def test_group_handle_equals_single_handle(atlas):
    torch = pytest.importorskip("torch")
    s = scenes.floor_pillars()
    single = _caster(s, atlas)
    dev_before = torch.cuda.current_device()
    group = _caster(s, atlas, group=[0, 0])
    rays = _arbitrary(np.random.default_rng(11), s["dim"], 5000)
    for as_pixel in (False, True):
        assert np.array_equal(group.cast_rays(rays, as_pixel=as_pixel), single.cast_rays(rays, as_pixel=as_pixel))
    assert torch.cuda.current_device() == dev_before


def test_query_between_async_and_sync_leaves_the_frame(atlas):
    s = scenes.terrain256()
    w, h = 256, 192
    ref = _caster(s, atlas, w, h)
    assert ref.compute()
    img0, hits0, ctr0 = ref.read_image().copy(), ref.read_hits().copy(), ref.counters()
    c = _caster(s, atlas, w, h)
    rays = _arbitrary(np.random.default_rng(5), s["dim"], 100000)
    assert c.timing_reset()
    assert c.compute_async()
    q = c.cast_rays(rays)
    assert c.sync()
    assert np.array_equal(c.read_image().view(np.uint32), img0.view(np.uint32))
    assert np.array_equal(c.read_hits(), hits0) and c.counters() == ctr0
    assert c.timing()[0] == 1
    assert np.array_equal(q, c.cast_rays(rays))


def test_argument_errors(atlas):
    s = scenes.floor_pillars()
    c = _caster(s, atlas)
    rays = np.zeros((4, 6), F)
    rays[:, :3] = 5.5
    rays[:, 5] = -1.0                                        # straight down onto the floor
    out = np.zeros((4, 8), np.int32)
    fp, ip = rays.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_int32))
    lib = vrc.lib
    assert lib.vrc_cast_rays(None, fp, 4, 0, 0, ip) == 1
    assert lib.vrc_cast_rays(c._h, None, 4, 0, 0, ip) == 1
    assert lib.vrc_cast_rays(c._h, fp, 4, 0, 0, None) == 1
    assert lib.vrc_cast_rays(c._h, fp, -1, 0, 0, ip) == 1 and "n = -1" in c.last_error()
    assert lib.vrc_cast_rays(c._h, fp, 4, -3, 0, ip) == 1
    assert lib.vrc_cast_rays(c._h, fp, 4, 0, 2, ip) == 1 and "flag" in c.last_error()
    assert lib.vrc_cast_rays_device(c._h, None, 4, 0, 0, None) == 1
    assert lib.vrc_cast_rays_device(c._h, fp, 4, 0, 0, ip) == 1          # pageable host memory is not device memory
    assert (out == 0).all()
    assert lib.vrc_cast_rays(c._h, fp, 0, 0, 0, ip) == 0
    assert lib.vrc_cast_rays_device(c._h, None, 0, 0, 0, None) == 0
    assert lib.vrc_cast_rays(c._h, fp, 4, 0, 0, ip) == 0 and (out[:, 5] == vrc.RAY_HIT).all()
    fresh = vrc.CLCaster()
    assert fresh.init(0)
    assert lib.vrc_cast_rays(fresh._h, fp, 4, 0, 0, ip) == 2 and "validate" in fresh.last_error()
    assert c.release_octree()
    assert lib.vrc_cast_rays(c._h, fp, 4, 0, 0, ip) == 2
