"""GPU suite (-m gpu): shape fills of the resident scene -- balls and axis-aligned cylinders (vrc_fill_shapes and its _device
variant, csrc/region_write.hip, csrc/shape_span.hpp).

Every comparison is exact.  The oracle is the numpy replay (tests/shape_replay.py): the shapes applied in index order, by integer
membership, to the dense grid vrc_read_regions gave before the call.  After a call the read-back is the replay, the counts are the
replay's and bricks_touched is the number of bricks that hold a voxel of a shape -- found by brute force, not by the bounding
boxes; with flags = 0 the arrays are, word for word, those of a second handle that received vrc_set_voxels of the expanded batch.
The batches are tests/shape_replay.py's batch(dims, k); tests/test_shape_fills_cpu.py asserts, without a GPU, that each of them
skips an operation, gives some brick a run of three operations and touches a brick that a ball's bounding box holds and the ball
does not.  The dims are the smallest at which every path exists: 2 and 4 (the root inside the brick), 8 (the brick is the root),
16 (one level above the bricks), 32 (two), 64 once (far pointers after growth), and one depth-10 terrain for a crater of r = 32."""
import ctypes as C

import numpy as np
import pytest

import box_replay as br
import compact_helpers as ch
import edit_replay as er
import face_replay as fr
import leaftree
import ray_replay as rr
import relayout as rl
import shape_replay as sp
import voxel_raycaster_amd as vrc
from gpu_helpers import _frame, configure

pytestmark = pytest.mark.gpu
I = np.int32
WHERE = {0: None, sp.WHERE_EMPTY: "empty", sp.WHERE_SOLID: "solid"}
INVALID, NOT_READY, LIMIT = 1, 2, 6
# one operation of each invalid kind: the host call refuses it, the _device call skips it
BAD = [([4, 3, 3, 3, 2, 1], 5), ([sp.BALL, 3, 3, 3, -1, 0], 5), ([sp.BALL, 3, 3, 3, 2 ** 30 + 1, 0], 5), ([sp.BALL, 3, 3, 3, 2, 1], 5),
       ([sp.CYLINDER_Y, 3, 3, 3, 2, 0], 5), ([sp.CYLINDER_Z, 3, 3, 3, 2, 4], 128)]


def _grid_now(c, dim):
    return ch.whole(c, dim)[1:-1, 1:-1, 1:-1]


def _fill_and_check(c, dim, before, shapes, m, flags=0, tag=""):
    """one fill_shapes against the replay: read-back, counts, the exact brick count and the growth bound"""
    want, skipped, changed = sp.fill_shapes(before, shapes, m, flags)
    info = c.fill_shapes(shapes, m, where=WHERE[flags])
    print(tag, info)
    assert info["skipped"] == skipped and info["voxels_changed"] == changed, (tag, info, skipped, changed)
    got = ch.whole(c, dim)
    assert np.array_equal(got, np.pad(want, 1)), (tag, np.argwhere(got != np.pad(want, 1))[:4] - 1)
    corners = sp.brick_corners(shapes, (dim,) * 3)
    if changed:
        bricks, above = er.touched_nodes(corners, dim)
        assert bricks == len(corners) and info["bricks_touched"] == bricks, (tag, info, bricks)
        assert info["descriptors_added"] == 72 * bricks + 16 * above + (1 if dim >= 8 else 0), (tag, info, bricks, above)
        assert info["descriptors_added"] <= 72 * info["bricks_touched"] + 16 * above + 1
    else:
        assert info["bricks_touched"] == 0 and info["descriptors_added"] == 0, (tag, info)
    assert (info["n_descriptors"], info["root_index"]) == c.octree_size()
    return want, info


def _same_arrays(a, b, tag):
    (da, ra, la, aa), (db, rb, lb, ab) = ch.state(a), ch.state(b)
    assert ra == rb and np.array_equal(da, db), (tag, np.nonzero(da != db)[0][:8] if len(da) == len(db) else (len(da), len(db)))
    assert (la is None) == (lb is None)
    if la is not None:
        assert np.array_equal(la, lb) and np.array_equal(aa, ab), tag


def _rebuilt(c, dim, want):
    desc, root, lookup, attach = ch.state(c)
    fresh = vrc.Octree.Generate(want.reshape(-1), dim, layout=vrc.LAYOUT_NO_PAGE_HEADERS)
    assert er.masks_by_position(desc, root, dim) == er.masks_by_position(fresh.descriptor_buffer, fresh.root_index, dim)
    assert np.array_equal(rl.decode(desc, root, dim, lookup, attach), want.reshape(-1))


# ---------------------------------------------------------------------------- 1. against the replay
@pytest.mark.parametrize("dim", [8, 16, 32])
def test_shape_fills_equal_the_replay(atlas, dim):
    grid = ch.grid_of(dim, 500 + dim)
    shapes, m = sp.batch(dim)
    for flags in (0, sp.WHERE_EMPTY, sp.WHERE_SOLID):
        c = ch.caster(atlas, dim, grid)
        assert np.array_equal(_grid_now(c, dim), grid)
        cur, _ = _fill_and_check(c, dim, grid, shapes, m, flags, f"shapes{dim}-{flags}")
        _fill_and_check(c, dim, cur, *sp.batch(dim, 1), flags, f"shapes{dim}-{flags}-second")      # on top of far pointers


# ---------------------------------------------------------------------------- 2. bit-identical to set_voxels of the expanded batch
@pytest.mark.parametrize("dim,attachments", [(8, True), (32, False), (64, True)])
def test_arrays_are_those_of_set_voxels_of_the_expanded_batch(atlas, dim, attachments):
    grid = ch.grid_of(dim, 511 + dim)
    before = grid if attachments else ch.plain(grid)
    a, b = ch.caster(atlas, dim, grid, attachments=attachments), ch.caster(atlas, dim, grid, attachments=attachments)
    _same_arrays(a, b, "before")
    for k in range(2):                                          # the second batch lands on a tree with far pointers
        shapes, m = sp.batch(dim, k)
        before, ia = _fill_and_check(a, dim, before, shapes, m, 0, f"twin{dim}-{k}")
        p, pm = sp.expand_shapes(shapes, m, (dim,) * 3)
        ib = b.set_voxels(p, pm)
        _same_arrays(a, b, f"twin{dim}-{k}")
        for key in ("voxels_changed", "bricks_touched", "descriptors_added", "n_descriptors", "root_index"):
            assert ia[key] == ib[key], key


# ---------------------------------------------------------------------------- 3. the same tree as a rebuild
@pytest.mark.parametrize("dim,attachments", [(8, True), (16, False), (32, True)])
def test_edited_tree_is_the_rebuilt_tree(atlas, dim, attachments):
    grid = ch.grid_of(dim, 540 + dim)
    grid[:3] = 5                                                # a floor: the frame sees the edits
    settings = (("empty_boxes", 0),)
    c = ch.caster(atlas, dim, grid, attachments=attachments, settings=settings)
    shapes, m = sp.batch(dim, 2)
    cur, _ = _fill_and_check(c, dim, grid if attachments else ch.plain(grid), shapes, m, 0, f"tree{dim}")
    _rebuilt(c, dim, cur)
    has = c.read_attachments()[0] is not None                   # (the batch holds other materials than 0 and 5: it brought them)
    assert has
    img, hits, ctr = _frame(c)
    f = ch.caster(atlas, dim, cur, settings=settings)
    fimg, fhits, fctr = _frame(f)
    assert np.array_equal(img, fimg) and np.array_equal(hits, fhits) and ctr == fctr


# ---------------------------------------------------------------------------- 4. mixed kinds in one batch, and the order
def test_mixed_kinds_and_order(atlas):
    dim = 32
    grid = ch.grid_of(dim, 560)
    pillar, crater = [sp.CYLINDER_Z, 16, 15, 2, 5, 27], [sp.BALL, 17, 16, 20, 7, 0]
    grids = []
    for order in ((0, 1), (1, 0)):
        shapes, m = np.array([pillar, crater], I)[list(order)], np.array([6, 0], I)[list(order)]
        c = ch.caster(atlas, dim, grid)
        cur, info = _fill_and_check(c, dim, grid, shapes, m, 0, f"order{order}")
        assert info["skipped"] == 0
        grids.append(cur)
    assert not np.array_equal(grids[0], grids[1])
    assert grids[0][20, 16, 17] == 0 and grids[1][20, 16, 17] == 6, "the later operation wins the overlap"


# ---------------------------------------------------------------------------- 5. the materials rule
def test_a_tree_without_materials_stays_without_them_for_0_and_5(atlas):
    """The fills' rule, as vrc_fill_boxes applies it today (test_voxel_region_edits_gpu.py, the test of the same name): a tree
    without attachments stays without them while every operation THAT HAS A VOXEL IN THE SCENE has material 0 or 5 -- whatever the
    flags let through, so the decision is a function of the batch and the scene size alone.  An operation that lies wholly
    outside the scene is skipped and does not count, whatever its material; one inside does even where the flags mask all of it,
    and the attachments then appear with the batch's commit (a batch that changes no voxel appends nothing, them included)."""
    dim = 16
    grid = ch.grid_of(dim, 565)
    shapes, m = sp.batch(dim)
    m05 = np.where(m == 0, 0, 5).astype(I)
    for flags in (0, sp.WHERE_SOLID):
        c = ch.caster(atlas, dim, grid, attachments=False)
        cur, _ = _fill_and_check(c, dim, ch.plain(grid), shapes, m05, flags, "plain05")
        assert c.read_attachments() == (None, None)
        # material 6 wholly outside the scene: skipped, and not the batch's business -- alone, and beside an operation that commits
        outside = np.array([[sp.BALL, dim + 9, 3, 3, 8, 0], [sp.BALL, -6, -6, -6, 9, 0]], I)
        cur, info = _fill_and_check(c, dim, cur, outside, np.array([6, 6], I), flags, "plain05-outside")
        assert info["skipped"] == 2 and c.read_attachments() == (None, None)
        z, y, x = np.argwhere(cur != 0)[0]
        both = np.array([outside[0], [sp.BALL, x, y, z, 0, 0]], I)
        cur, info = _fill_and_check(c, dim, cur, both, np.array([6, 0], I), flags, "plain05-outside-committed")
        assert info["voxels_changed"] == 1 and c.read_attachments() == (None, None)
        # material 7 inside, masked by the flag: nothing changes, nothing is appended ...
        solid_there = cur[3, 3, 3] != 0
        mask = sp.WHERE_EMPTY if solid_there else sp.WHERE_SOLID
        one = np.array([[sp.BALL, 3, 3, 3, 0, 0]], I)
        cur, info = _fill_and_check(c, dim, cur, one, np.array([7], I), mask, "plain-7-masked")
        assert info["voxels_changed"] == 0 and c.read_attachments() == (None, None)
        # ... and beside an operation the flag lets through, the batch commits and brings the attachments
        z, y, x = np.argwhere((cur == 0) if solid_there else (cur != 0))[0]
        two = np.array([[sp.CYLINDER_X, x, y, z, 0, 1], one[0]], I)
        cur, info = _fill_and_check(c, dim, cur, two, np.array([5 if solid_there else 0, 7], I), mask, "plain-7-masked-but-committed")
        assert info["voxels_changed"] == 1 and c.read_attachments()[0] is not None and cur[3, 3, 3] != 7


# ---------------------------------------------------------------------------- 6. shallow trees, solid leaves
@pytest.mark.parametrize("dim", [2, 4])
def test_shallow_trees(atlas, dim):
    grid = ch.grid_of(dim, 570 + dim)
    c = ch.caster(atlas, dim, grid)
    cur = grid
    for k in range(3):
        shapes, m = sp.batch(dim, k)
        cur, _ = _fill_and_check(c, dim, cur, shapes, m, (0, sp.WHERE_EMPTY, sp.WHERE_SOLID)[k], f"shallow{dim}-{k}")
        _rebuilt(c, dim, cur)
    cur, _ = _fill_and_check(c, dim, cur, np.array([[sp.BALL, 0, 0, 0, 2 ** 30, 0]], I), np.array([0], I), 0, f"shallow-clear{dim}")
    assert not cur.any() and er.masks_by_position(c.read_descriptors(), c.octree_size()[1], dim) == {(0, 0, 0, dim): (0, 0xff)}
    cur, info = _fill_and_check(c, dim, cur, np.array([[sp.CYLINDER_Y, 1, 0, 1, 0, 1]], I), np.array([-3], I), 0, f"shallow-regrow{dim}")
    assert info["voxels_changed"] == 1
    _rebuilt(c, dim, cur)


def test_a_ball_dug_into_solid_leaves(atlas):
    depth, dim = 5, 32
    cubes = [(8, 8, 8, 8), (16, 16, 0, 4), (0, 0, 0, 4), (20, 4, 6, 2), (0, 16, 16, 16)]
    desc, root, flat = leaftree.leaf_octree(np.random.default_rng(571).integers(0, dim, size=(200, 3)), cubes, depth)
    grid = flat.reshape(dim, dim, dim)
    c = ch.caster(atlas, dim, grid, octree=vrc.Octree(desc, root, dim))
    assert np.array_equal(_grid_now(c, dim), grid)
    shapes = np.array([[sp.BALL, 12, 12, 12, 3, 0], [sp.BALL, 5, 20, 25, 1, 0], [sp.CYLINDER_X, 15, 18, 2, 1, 4]], I)
    cur, info = _fill_and_check(c, dim, grid, shapes, np.zeros(3, I), 0, "dig")
    masks = er.masks_by_position(c.read_descriptors(), c.octree_size()[1], dim)
    valid, leaf = masks[(0, 16, 16, 16)]                        # the dug 16^3 leaf is a node now: seven of its children still leaves
    assert valid == 0xff and bin(leaf).count("1") == 7
    cur, _ = _fill_and_check(c, dim, cur, shapes, np.array([6, 5, 5], I), sp.WHERE_EMPTY, "refill")
    desc, root, lookup, attach = ch.state(c)
    assert np.array_equal(rl.decode(desc, root, dim, lookup, attach), cur.reshape(-1))


# ---------------------------------------------------------------------------- 7. the array branch
def _map_caster(atlas, dims, mp, tree_dim=16):
    c = vrc.CLCaster()
    assert c.init(0)
    li = np.zeros((8, 10), np.float32)
    li[0] = [0.01, 0.01, 0.01, 0.2, 12.8, 3.2, 14.4, -1, -1, -1.5]
    configure(c, tree_dim, atlas, (2.0, 1.5708), (8.37, 1.41, 7.29), li, 64, 48)
    assert c.overwrite_setting("using_octree", 1)
    assert c.assign_octree(vrc.Octree.Generate(np.where(np.arange(tree_dim ** 3) < tree_dim ** 2, 5, 0).astype(np.int8), tree_dim)) and c.assign_map(mp, dims)
    assert c.validate(), c.last_error()
    return c


@pytest.mark.parametrize("dims", [(16, 16, 16), (13, 5, 11), (24, 9, 10)])
def test_array_branch_equals_the_replay(atlas, dims):
    dx, dy, dz = dims
    rng = np.random.default_rng(580 + sum(dims))
    mp = rng.choice(np.array([0, 0, 5, 6, 1, -2], np.int8), size=dx * dy * dz)
    c = _map_caster(atlas, dims, mp)
    before = c.read_regions(np.zeros((1, 3), I), dims)[0]      # int8[dz][dy][dx] by the frame's index; past the array reads 0
    zs = min(dz, dy)                                           # rows at z >= dy have an index past the array: outside the scene
    scene = before[:zs]
    tree0 = c.read_descriptors()
    for k, flags in enumerate((0, sp.WHERE_EMPTY, sp.WHERE_SOLID)):
        shapes, m = sp.batch((dx, dy, zs), k)
        want, skipped, changed = sp.fill_shapes(scene, shapes, m, flags)
        info = c.fill_shapes(shapes, m, where=WHERE[flags])
        assert (info["skipped"], info["voxels_changed"], info["bricks_touched"], info["descriptors_added"]) == (skipped, changed, 0, 0), (k, info)
        assert changed > 0
        got = c.read_regions(np.zeros((1, 3), I), dims)[0]
        assert np.array_equal(got[:zs], want) and not got[zs:].any(), (k, np.argwhere(got[:zs] != want)[:4])
        scene = want
    assert np.array_equal(c.read_descriptors(), tree0), "the array branch left the tree alone"


def test_array_branch_refuses_a_map_whose_index_aliases(atlas):
    dims = (16, 8, 4)                                          # dy > dz: rows share bytes
    mp = np.random.default_rng(2).choice(np.array([0, 5, 6], np.int8), size=16 * 8 * 4)
    c = _map_caster(atlas, dims, mp)
    before = c.read_regions(np.full((1, 3), -1, I), (18, 10, 6))
    with pytest.raises(vrc.VrcError):
        c.fill_shapes(np.array([[sp.BALL, 3, 3, 2, 2, 0]], I), 7)
    assert c.last_status == LIMIT
    assert np.array_equal(c.read_regions(np.full((1, 3), -1, I), (18, 10, 6)), before)


# ---------------------------------------------------------------------------- 8. the _device variant
def test_device_variant(atlas):
    import torch
    dim = 16
    grid = ch.grid_of(dim, 590)
    shapes, m = sp.batch(dim)
    bad_s, bad_m = np.array([s for s, _ in BAD], np.int64).astype(I), np.array([v for _, v in BAD], I)
    at = [2, 5, 9, 13, 17, 21]                                  # the invalid ones, spread over the batch
    all_s, all_m = np.insert(shapes, at, bad_s, axis=0), np.insert(m, at, bad_m)
    for using_octree in (0, 1):
        for flags in (0, sp.WHERE_SOLID):
            c, host = ch.caster(atlas, dim, grid), ch.caster(atlas, dim, grid)
            assert c.overwrite_setting("using_octree", using_octree) and host.overwrite_setting("using_octree", using_octree)
            ts, tm = torch.from_numpy(all_s).cuda(), torch.from_numpy(all_m).cuda()
            torch.cuda.synchronize()
            info = c.fill_shapes_device(ts.data_ptr(), tm.data_ptr(), len(all_m), where=WHERE[flags])
            want, skipped, changed = sp.fill_shapes(grid, shapes, m, flags)
            assert info["skipped"] == skipped + len(BAD) and info["voxels_changed"] == changed, info
            assert np.array_equal(_grid_now(c, dim), want)
            hinfo = host.fill_shapes(shapes, m, where=WHERE[flags])
            assert ch.counts(hinfo) == dict(ch.counts(info), skipped=skipped)
            if using_octree == 0:
                _same_arrays(c, host, "device and host")
            # the host call refuses the batch with the invalid operations and changes nothing
            d0 = c.read_descriptors()
            with pytest.raises(vrc.VrcError):
                c.fill_shapes(all_s, all_m, where=WHERE[flags])
            assert c.last_status == INVALID and np.array_equal(c.read_descriptors(), d0) and np.array_equal(_grid_now(c, dim), want)
            # a misaligned pointer
            V = C.c_void_p
            assert vrc.lib.vrc_fill_shapes_device(c._h, V(ts.data_ptr() + 2), V(tm.data_ptr()), 2, 0, None) == INVALID
            assert vrc.lib.vrc_fill_shapes_device(c._h, V(ts.data_ptr()), V(tm.data_ptr() + 1), 2, 0, None) == INVALID
            assert np.array_equal(_grid_now(c, dim), want)


# ---------------------------------------------------------------------------- 9. errors
def test_errors_change_nothing(atlas):
    dim = 16
    grid = ch.grid_of(dim, 600)
    c = ch.caster(atlas, dim, grid)
    d0, size0, whole0 = c.read_descriptors(), c.octree_size(), ch.whole(c, dim)
    h, lib = c._h, vrc.lib
    i32p = C.POINTER(C.c_int32)
    good = np.array([sp.BALL, 5, 5, 5, 3, 0, sp.CYLINDER_X, 1, 2, 3, 2, 4], I)
    m = np.array([5, 0], I)
    gp, mp = good.ctypes.data_as(i32p), m.ctypes.data_as(i32p)
    info = vrc.EditInfo()
    info.struct_size = C.sizeof(vrc.EditInfo)

    def unchanged():
        return c.octree_size() == size0 and np.array_equal(c.read_descriptors(), d0) and np.array_equal(ch.whole(c, dim), whole0)

    for s, v in BAD:                                            # each invalid operation, behind a valid one
        shapes = np.concatenate([good[:6], np.array(s, np.int64).astype(I)])
        mb = np.array([5, v], I)
        assert lib.vrc_fill_shapes(h, shapes.ctypes.data_as(i32p), mb.ctypes.data_as(i32p), 2, 0, C.byref(info)) == INVALID, (s, v)
    for bad in (-129, 2 ** 31 - 1):
        mb = np.array([5, bad], I)
        assert lib.vrc_fill_shapes(h, gp, mb.ctypes.data_as(i32p), 2, 0, None) == INVALID
    for flags in (3, 4, 5, 8, 0x80000000):                      # both WHERE bits, SKIP_ZERO, unknown bits
        assert lib.vrc_fill_shapes(h, gp, mp, 2, flags, None) == INVALID, flags
        assert lib.vrc_fill_shapes_device(h, None, None, 0, flags, None) == INVALID, flags
    assert lib.vrc_fill_shapes(None, gp, mp, 2, 0, None) == INVALID
    assert lib.vrc_fill_shapes(h, None, mp, 2, 0, None) == INVALID and lib.vrc_fill_shapes(h, gp, None, 2, 0, None) == INVALID
    assert lib.vrc_fill_shapes(h, gp, mp, -1, 0, None) == INVALID and lib.vrc_fill_shapes_device(h, None, None, -1, 0, None) == INVALID
    assert lib.vrc_fill_shapes_device(h, None, C.c_void_p(16), 2, 0, None) == INVALID
    assert lib.vrc_fill_shapes_device(h, C.c_void_p(good.ctypes.data), C.c_void_p(m.ctypes.data), 2, 0, None) == INVALID, "pageable host memory"
    short = vrc.EditInfo()
    short.struct_size = 2
    assert lib.vrc_fill_shapes(h, gp, mp, 2, 0, C.byref(short)) == INVALID
    assert unchanged()
    # n = 0 succeeds and changes nothing
    assert lib.vrc_fill_shapes(h, None, None, 0, 0, C.byref(info)) == 0 and info.voxels_changed == 0 and info.n_descriptors == size0[0] and info.root_index == size0[1]
    assert lib.vrc_fill_shapes_device(h, None, None, 0, 0, None) == 0
    assert unchanged()
    # not ready: a handle that has not validated
    n = vrc.CLCaster()
    assert n.init(0)
    assert lib.vrc_fill_shapes(n._h, gp, mp, 2, 0, None) == NOT_READY
    # a tree adopted by a handle outside the group: refused, nothing changes; released, the edit goes through
    other = vrc.CLCaster()
    assert other.init(0) and other.assign_octree_from(c)
    assert lib.vrc_fill_shapes(h, gp, mp, 2, 0, C.byref(info)) == LIMIT
    assert unchanged() and other.octree_size() == size0
    assert other.release_octree()
    _fill_and_check(c, dim, grid, good.reshape(2, 6), m, 0, "after-release")


# ---------------------------------------------------------------------------- 10. determinism, no change
def test_determinism_and_no_change(atlas):
    dim = 32
    grid = ch.grid_of(dim, 610)
    shapes, m = sp.batch(dim)
    a, b = ch.caster(atlas, dim, grid), ch.caster(atlas, dim, grid)
    n0 = a.octree_size()[0]
    ia, ib = a.fill_shapes(shapes, m, where="empty"), b.fill_shapes(shapes.copy(), m.copy(), where="empty")
    assert ch.counts(ia) == ch.counts(ib) and ia["n_descriptors"] == n0 + ia["descriptors_added"] and ia["voxels_changed"] > 0
    _same_arrays(a, b, "determinism")
    # a batch that changes nothing: WHERE_SOLID over empty space, clears of empty space, shapes outside
    cur = _grid_now(a, dim)
    empty = np.argwhere(cur == 0)[:40, ::-1]
    dots = np.zeros((len(empty), 6), I)
    dots[:, 0], dots[:, 1:4] = sp.BALL, empty
    before, mem, da = a.octree_size(), a.memory_usage2()["octree_bytes"], a.read_descriptors()
    for info in (a.fill_shapes(dots, 7, where="solid"), a.fill_shapes(dots, 0),
                 a.fill_shapes(np.array([[sp.BALL, dim + 9, 0, 0, 9, 0], [sp.CYLINDER_Z, 3, 3, -9, 2, 9]], I), 7)):
        assert info["voxels_changed"] == 0 and info["descriptors_added"] == 0 and info["bricks_touched"] == 0, info
        assert a.octree_size() == before == (info["n_descriptors"], info["root_index"]) and a.memory_usage2()["octree_bytes"] == mem
    assert info["skipped"] == 2 and np.array_equal(a.read_descriptors(), da)


# ---------------------------------------------------------------------------- 11. neighbours
def test_queries_faces_and_compaction_right_after_a_fill(atlas):
    dim = 32
    grid = ch.grid_of(dim, 620)
    grid[:12] = 5                                               # ground to dig into
    c = ch.caster(atlas, dim, grid)
    crater = np.array([[sp.BALL, 15, 17, 12, 9, 0], [sp.CYLINDER_Z, 15, 17, 0, 2, 12], [sp.BALL, 20, 12, 18, 3, 0]], I)
    want, info = _fill_and_check(c, dim, grid, crater, np.array([0, 0, 6], I), 0, "crater")
    assert c.memory_usage2()["coarse_bytes"] == 0, "the table goes with the edit"
    mat = br.grid_xyz(want.reshape(-1), dim)
    rng = np.random.default_rng(621)
    rays = rr.random_rays(rng, 256, dim)
    rays[:128, :3] = rng.uniform([6, 8, 3], [24, 26, 21], size=(128, 3))          # origins inside the crater's box
    assert np.array_equal(c.cast_rays(rays), rr.replay(rays, want.reshape(-1), (dim,) * 3))
    boxes = br.random_boxes(rng, 256, dim)
    for a, b in zip(c.box_intersection(boxes, max_voxels=9), br.GridReplay(mat).query(boxes, max_voxels=9)):
        assert np.array_equal(a, b)
    lo, size = np.array([[6, 8, 3], [0, 0, 0]], I), (19, 19, 19)
    counts, faces, _ = c.extract_faces(lo, size)
    wcounts, wfaces = fr.regions(mat, lo, size)
    assert np.array_equal(counts, wcounts) and np.array_equal(faces, wfaces) and counts[0] > 0
    assert c.memory_usage2()["coarse_bytes"] == 0, "a query started a derived build"
    ci = c.compact_octree()
    assert ci["n_descriptors"] < ci["descriptors_before"] and np.array_equal(_grid_now(c, dim), want)
    _rebuilt(c, dim, want)
    _fill_and_check(c, dim, want, *sp.batch(dim, 1), 0, "after-compaction")


# ---------------------------------------------------------------------------- 12. a group
def test_group_with_own_copies(atlas):
    dim = 32
    grid = ch.grid_of(dim, 630)
    grid[:3] = 5
    shapes, m = sp.batch(dim)
    settings = (("empty_boxes", 0),)
    single = ch.caster(atlas, dim, grid, settings=settings)
    _, info1 = _fill_and_check(single, dim, grid, shapes, m, 0, "single")
    simg, shits, sctr = _frame(single)
    g = ch.caster(atlas, dim, grid, settings=settings, group=[0, 0], own_copies=True)
    assert g.group_size() == 2 and g.memory_usage2(1)["octree_shared"] == 0
    _, info = _fill_and_check(g, dim, grid, shapes, m, 0, "group")
    assert ch.counts(info) == ch.counts(info1)
    # rank 0's array is the single handle's; rank 1's own copy has no read-back of its own: it grew to the same size, and it
    # renders its rows of the frame below
    d0 = g.read_descriptors()
    assert len(d0) == info["n_descriptors"] and np.array_equal(d0, single.read_descriptors())
    assert g.memory_usage2(1)["octree_shared"] == 0 and g.memory_usage2(1)["octree_bytes"] == g.memory_usage2(0)["octree_bytes"]
    img, hits, ctr = _frame(g)
    assert np.array_equal(img, simg) and np.array_equal(hits, shits) and ctr == sctr


# ---------------------------------------------------------------------------- 13. a crater in a device-built terrain
def test_a_crater_in_the_depth_10_terrain(atlas):
    from test_terrain_edits_gpu import _terrain
    depth, r, edge = 10, 32, 80
    dim = 1 << depth
    c = _terrain(atlas, depth)
    assert c.read_attachments() == (None, None)
    column = c.read_regions(np.array([[dim // 2, dim // 2, 0]], I), (1, 1, dim))[0][:, 0, 0]
    assert column.any(), "the shell misses the map's middle column"
    centre = np.array([dim // 2, dim // 2, int(np.nonzero(column)[0].max())])      # a surface point
    lo = (centre - edge // 2).astype(I)[None]
    before = c.read_regions(lo, (edge,) * 3)[0]
    assert before.any() and not before.all()
    ball = np.array([[sp.BALL, *centre, r, 0]], I)
    local = ball.copy()
    local[0, 1:4] -= lo[0]
    want, skipped, changed = sp.fill_shapes(before, local, [0])
    n0 = c.octree_size()[0]
    info = c.fill_shapes(ball, 0)
    print("crater", info)
    assert np.array_equal(c.read_regions(lo, (edge,) * 3)[0], want)
    assert info["skipped"] == skipped == 0 and info["voxels_changed"] == changed > 0
    touched = len(sp.brick_corners(ball, (dim,) * 3))
    assert info["bricks_touched"] == touched < 9 ** 3, "the bricks of the ball, fewer than its bounding box's"
    assert info["n_descriptors"] == n0 + info["descriptors_added"] and c.read_attachments() == (None, None)
