"""GPU suite (-m gpu): voxel edits of the resident scene (vrc_set_voxels / vrc_set_voxels_device, csrc/voxel_edit.hip).

Every comparison is exact.  The oracle is the numpy replay (tests/edit_replay.py): the batch applied in index order to the dense
grid vrc_read_regions gave before the call.  After an edit the read-back is the replay; the edited tree, walked by position, has
the (valid, leaf) masks of the host builder's tree of the replayed grid and decodes to it with its own lookup and attachments;
frames, hit records, counters and queries equal those of a second caster whose tree was built fresh from the replayed grid; two
handles given the same batch end with the same array word for word; growth stays within the stated bound, a batch that changes
nothing appends nothing, the reallocation path and the group path give the same scenes, the errors leave the array untouched, and
the index-audit build renders the edited tree without a violation."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import box_replay as br
import edit_replay as er
import leaftree
import ray_replay as rr
import relayout as rl
import sweep_replay as sr
import voxel_raycaster_amd as vrc
from gpu_helpers import _frame, configure

pytestmark = pytest.mark.gpu
I = np.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATERIALS = np.array([0, 5, 6, 7, -3], np.int8)
W, H = 64, 48


def _grid(dim, seed):
    """random sparse int8[z][y][x] of the materials {0, 5, 6, 7, -3}, with an empty and a solid corner cube"""
    rng = np.random.default_rng(seed)
    g = rng.choice(MATERIALS, size=(dim, dim, dim), p=[0.8, 0.1, 0.04, 0.03, 0.03]).astype(np.int8)
    h = max(dim // 4, 1)
    g[:h, :h, :h] = 0
    g[-h:, -h:, -h:] = 5
    return g


def _caster(atlas, dim, grid=None, attachments=True, using_octree=0, settings=(), octree=None, group=None, own_copies=True):
    c = vrc.CLCaster()
    assert (c.init_group(group, own_copies=own_copies) if group else c.init(0)), c.last_error()
    li = np.zeros((8, 10), np.float32)
    li[0] = [0.01, 0.01, 0.01, 0.2, dim * 0.8, dim * 0.2, dim * 0.9, -1, -1, -1.5]
    configure(c, dim, atlas, (2.0, 1.5708), (dim * 0.5 + 0.37, 1.41, dim * 0.45 + 0.29), li, W, H)
    assert c.overwrite_setting("using_octree", using_octree)
    for k, v in settings:
        assert c.add_to_settings_buffer(k, k.upper(), v), c.last_error()
    if octree is not None:
        assert c.assign_octree(octree), c.last_error()
    elif dim >= 8:
        c.build_dense_grid(int(np.log2(dim)), grid.reshape(-1), attachments=attachments)
    else:
        o = vrc.Octree.Generate(grid.reshape(-1), dim)
        assert c.assign_octree(o.attach_materials_from_grid(grid.reshape(-1)) if attachments else o), c.last_error()
    if grid is not None:
        assert c.assign_map(grid.reshape(-1), (dim,) * 3)
    assert c.validate(), c.last_error()
    return c


def _whole(c, dim):
    """the whole map with a one-voxel apron, int8[dim + 2][dim + 2][dim + 2]"""
    return c.read_regions(np.full((1, 3), -1, I), (dim + 2,) * 3)[0]


def _check_reads(c, dim, want, positions, tag):
    got = _whole(c, dim)
    assert np.array_equal(got, np.pad(want, 1)), (tag, np.argwhere(got != np.pad(want, 1))[:4] - 1)
    inside = ((positions >= 0) & (positions < dim)).all(axis=1)
    p = positions[inside]
    expect = np.zeros(len(positions), I)
    expect[inside] = want[p[:, 2], p[:, 1], p[:, 0]]
    assert np.array_equal(c.get_voxels(positions), expect), tag


def _edit_and_check(c, dim, before, p, m, tag):
    want, skipped, changed = er.replay(before, p, m)
    info = c.set_voxels(p, m)
    print(tag, info)
    assert info["skipped"] == skipped and info["voxels_changed"] == changed, (tag, info, skipped, changed)
    _check_reads(c, dim, want, p, tag)
    return want, info


def _plain(g):
    return np.where(g != 0, 5, 0).astype(np.int8)


# ---------------------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("dim", [8, 16, 32])
def test_round_trip_equals_the_replay(atlas, dim):
    grid = _grid(dim, dim)
    p, m = er.random_batch(np.random.default_rng(100 + dim), dim)
    # the tree with materials, the tree without (the batch brings them), the array
    for tag, using_octree, attachments in (("svo-attached", 0, True), ("svo-plain", 0, False), ("array", 1, True)):
        c = _caster(atlas, dim, grid, attachments=attachments, using_octree=using_octree)
        before = grid if attachments else _plain(grid)
        assert np.array_equal(_whole(c, dim), np.pad(before, 1))
        _, info = _edit_and_check(c, dim, before, p, m, f"{tag}{dim}")
        if using_octree:
            assert info["bricks_touched"] == 0 and info["descriptors_added"] == 0
        else:
            assert info["bricks_touched"] == er.touched_nodes(p, dim)[0]
            assert (info["n_descriptors"], info["root_index"]) == c.octree_size()
    # a tree without materials stays without them while the batch writes only 0 and 5
    c = _caster(atlas, dim, grid, attachments=False)
    bytes_before = c.memory_usage2()["octree_bytes"]
    m05 = np.where(m == 0, 0, 5).astype(I)
    want, info = _edit_and_check(c, dim, _plain(grid), p, m05, f"svo-plain05-{dim}")
    assert c.read_attachments() == (None, None)
    assert c.memory_usage2()["octree_bytes"] >= bytes_before + 8 * info["descriptors_added"]
    # ... and a later batch with another material brings them: what was 5 stays 5
    _edit_and_check(c, dim, want, p[:50], np.full(50, 7, I), f"svo-plain05-then7-{dim}")
    assert c.read_attachments()[0] is not None


def test_device_variant_and_out_of_range_material(atlas):
    import torch
    dim = 16
    grid = _grid(dim, 3)
    p, m = er.random_batch(np.random.default_rng(5), dim, n=500)
    m[7], m[8] = 128, -129                                     # the device call cannot reject them: those edits are skipped
    ok = (m >= -128) & (m <= 127)
    for using_octree in (0, 1):
        c = _caster(atlas, dim, grid, using_octree=using_octree)
        tp, tm = torch.from_numpy(p).cuda(), torch.from_numpy(m).cuda()
        info = c.set_voxels_device(tp.data_ptr(), tm.data_ptr(), len(m))
        want, skipped, changed = er.replay(grid, p[ok], m[ok])
        assert info["skipped"] == skipped + 2 and info["voxels_changed"] == changed
        _check_reads(c, dim, want, p, f"device{using_octree}")
        # the host call refuses the same batch and changes nothing
        d0 = c.read_descriptors()
        with pytest.raises(vrc.VrcError):
            c.set_voxels(p, m)
        assert c.last_status == 1 and np.array_equal(c.read_descriptors(), d0)
        assert np.array_equal(_whole(c, dim), np.pad(want, 1))


# ---------------------------------------------------------------------------- 2. the same tree as a rebuild
@pytest.mark.parametrize("dim,attachments", [(8, True), (16, False), (32, True)])
def test_edited_tree_is_the_rebuilt_tree(atlas, dim, attachments):
    grid = _grid(dim, 40 + dim)
    p, m = er.random_batch(np.random.default_rng(41 + dim), dim)
    c = _caster(atlas, dim, grid, attachments=attachments)
    want, _ = _edit_and_check(c, dim, grid if attachments else _plain(grid), p, m, f"tree{dim}")
    n, root = c.octree_size()
    desc = c.read_descriptors()
    lookup, attach = c.read_attachments()
    assert lookup is not None and len(lookup) == n == len(desc)
    assert np.array_equal(rl.decode(desc, root, dim, lookup, attach), want.reshape(-1))
    fresh = vrc.Octree.Generate(want.reshape(-1), dim, layout=vrc.LAYOUT_NO_PAGE_HEADERS)
    assert er.masks_by_position(desc, root, dim) == er.masks_by_position(fresh.descriptor_buffer, fresh.root_index, dim)


# ---------------------------------------------------------------------------- 3. frames
def test_frames_equal_a_fresh_caster(atlas):
    dim = 32
    grid = _grid(dim, 9)
    grid[:3] = 5                                                # a floor: the frame sees the edits
    p, m = er.random_batch(np.random.default_rng(10), dim)
    for settings in ((("empty_boxes", 0),), ()):
        c = _caster(atlas, dim, grid, settings=settings)
        want, _ = _edit_and_check(c, dim, grid, p, m, f"frame{settings}")
        if not settings:
            assert c.prepare(), c.last_error()
        img, hits, ctr = _frame(c)
        f = _caster(atlas, dim, want, settings=settings)
        fimg, fhits, fctr = _frame(f)
        assert c.last_kernel()["name"] == f.last_kernel()["name"]
        assert np.array_equal(img, fimg) and np.array_equal(hits, fhits) and ctr == fctr, settings
        assert ctr["canonical_reads"] == bool(settings)
        if not settings:
            assert c.used_empty_boxes()
            chk = c.empty_boxes_check(samples=1 << 16)
            assert chk["boxes_sampled"] > 0 and chk["solid_voxels"] == 0


# ---------------------------------------------------------------------------- 4. queries right after an edit
def test_queries_right_after_an_edit(atlas):
    dim = 32
    grid = _grid(dim, 12)
    p, m = er.random_batch(np.random.default_rng(13), dim)
    c = _caster(atlas, dim, grid)
    assert c.memory_usage2()["coarse_bytes"] > 0 and c.memory_usage2()["box_bytes"] > 0       # validate() built them
    want, _ = _edit_and_check(c, dim, grid, p, m, "queries")
    mem = c.memory_usage2()
    assert mem["coarse_bytes"] == 0 and mem["box_bytes"] == 0 and mem["box_records"] == 0
    f = _caster(atlas, dim, want)
    rng = np.random.default_rng(14)
    rays, boxes, sweeps = rr.random_rays(rng, 256, dim), br.random_boxes(rng, 256, dim), sr.random_sweeps(rng, 256, dim)
    assert np.array_equal(c.cast_rays(rays), f.cast_rays(rays))
    for a, b in zip(c.box_intersection(boxes, max_voxels=9), f.box_intersection(boxes, max_voxels=9)):
        assert np.array_equal(a, b)
    assert np.array_equal(c.sweep_boxes(sweeps), f.sweep_boxes(sweeps))
    mem = c.memory_usage2()
    assert mem["coarse_bytes"] == 0 and mem["box_bytes"] == 0, "a query started a derived build"
    assert c.prepare() and c.memory_usage2()["coarse_bytes"] > 0
    assert np.array_equal(c.cast_rays(rays), f.cast_rays(rays))


# ---------------------------------------------------------------------------- 5. shallow trees
@pytest.mark.parametrize("dim", [2, 4])
def test_shallow_trees_toggle_single_voxels(atlas, dim):
    grid = _grid(dim, 20 + dim)
    c = _caster(atlas, dim, grid)
    rng = np.random.default_rng(21 + dim)
    cur, roots = grid, {c.octree_size()[1]}
    for k in range(64):
        p = rng.integers(0, dim, size=(1, 3)).astype(I)
        x, y, z = p[0]
        m = np.array([0 if cur[z, y, x] else int(rng.choice([5, 6, -3]))], I)
        cur, info = _edit_and_check(c, dim, cur, p, m, f"toggle{dim}-{k}")
        assert info["voxels_changed"] == 1 and info["root_index"] not in roots, "the root moves with every edit"
        roots.add(info["root_index"])
    desc, (n, root) = c.read_descriptors(), c.octree_size()
    fresh = vrc.Octree.Generate(cur.reshape(-1), dim, layout=vrc.LAYOUT_NO_PAGE_HEADERS)
    assert er.masks_by_position(desc, root, dim) == er.masks_by_position(fresh.descriptor_buffer, fresh.root_index, dim)


# ---------------------------------------------------------------------------- 6. prune and regrow
def test_prune_to_an_empty_scene_and_regrow(atlas):
    dim = 16
    grid = _grid(dim, 30)
    grid[8:16, 0:8, 0:8] = 6                                    # one brick, full
    c = _caster(atlas, dim, grid, settings=(("empty_boxes", 0),))
    g = np.arange(8)
    brick = np.stack(np.meshgrid(g, g, g + 8, indexing="ij"), axis=-1).reshape(-1, 3).astype(I)
    cur, info = _edit_and_check(c, dim, grid, brick, np.zeros(len(brick), I), "clear-brick")
    assert info["bricks_touched"] == 1 and info["voxels_changed"] == 512
    desc, (n, root) = c.read_descriptors(), c.octree_size()
    assert (0, 0, 8, 8) not in er.masks_by_position(desc, root, dim), "the emptied brick is still a node"
    g = np.arange(dim)
    everything = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(I)
    cur, info = _edit_and_check(c, dim, cur, everything, np.zeros(len(everything), I), "clear-all")
    assert not cur.any() and info["bricks_touched"] == 8
    desc, (n, root) = c.read_descriptors(), c.octree_size()
    assert (int(desc[root]) >> 16) & 0xff == 0, "the root of an empty scene has valid mask 0"
    assert er.masks_by_position(desc, root, dim) == {(0, 0, 0, dim): (0, 0xff)}
    img, hits, ctr = _frame(c)
    f = _caster(atlas, dim, cur, settings=(("empty_boxes", 0),))
    fimg, fhits, fctr = _frame(f)
    assert np.array_equal(img, fimg) and np.array_equal(hits, fhits) and ctr == fctr
    assert len(np.unique(img.reshape(-1, 4), axis=0)) == 1, "an empty scene renders one background colour"
    cur, info = _edit_and_check(c, dim, cur, np.array([[9, 3, 12]], I), np.array([7], I), "regrow")
    assert info["voxels_changed"] == 1 and c.get_voxels(np.array([[9, 3, 12]], I))[0] == 7
    desc, (n, root) = c.read_descriptors(), c.octree_size()
    fresh = vrc.Octree.Generate(cur.reshape(-1), dim, layout=vrc.LAYOUT_NO_PAGE_HEADERS)
    assert er.masks_by_position(desc, root, dim) == er.masks_by_position(fresh.descriptor_buffer, fresh.root_index, dim)


# ---------------------------------------------------------------------------- 7. leaf expansion
def test_digging_into_solid_leaves(atlas):
    depth, dim = 5, 32
    cubes = [(8, 8, 8, 8), (16, 16, 0, 4), (0, 0, 0, 4), (20, 4, 6, 2), (0, 16, 16, 16)]
    rng = np.random.default_rng(31)
    desc, root, flat = leaftree.leaf_octree(rng.integers(0, dim, size=(200, 3)), cubes, depth)
    grid = flat.reshape(dim, dim, dim)
    c = _caster(atlas, dim, grid, octree=vrc.Octree(desc, root, dim))
    assert np.array_equal(_whole(c, dim), np.pad(grid, 1))
    # one voxel inside the 8^3 leaf (a brick of its own), one inside the 4^3 leaf, one inside the 16^3 leaf (above the bricks)
    p = np.array([[11, 12, 13], [17, 18, 1], [5, 20, 25]], I)
    cur, info = _edit_and_check(c, dim, grid, p, np.zeros(3, I), "dig")
    assert info["voxels_changed"] == 3
    masks = er.masks_by_position(c.read_descriptors(), c.octree_size()[1], dim)
    valid, leaf = masks[(0, 16, 16, 16)]                        # the dug 16^3 leaf is a node now: seven of its children still leaves
    assert valid == 0xff and bin(leaf).count("1") == 7
    cur, _ = _edit_and_check(c, dim, cur, p, np.array([6, 5, 5], I), "fill")
    lookup, attach = c.read_attachments()
    assert np.array_equal(rl.decode(c.read_descriptors(), c.octree_size()[1], dim, lookup, attach), cur.reshape(-1))


# ---------------------------------------------------------------------------- 8. layouts
def test_relaid_tree_takes_the_same_batch(atlas):
    dim = 32
    grid = _grid(dim, 32)
    p, m = er.random_batch(np.random.default_rng(132), dim)
    o = vrc.Octree.Generate(grid.reshape(-1), dim).attach_materials_from_grid(grid.reshape(-1))
    d2, r2, l2 = rl.relayout(o.descriptor_buffer, o.root_index, dim, np.random.default_rng(33), 1.0, o.attachment_lookup)
    assert 0 < r2 < len(d2) - 1 and rl.FILLER in d2
    o2 = vrc.Octree(d2, r2, dim)
    o2.attachment_lookup, o2.attachment_buffer = l2, o.attachment_buffer
    c = _caster(atlas, dim, grid, octree=o2)
    assert np.array_equal(_whole(c, dim), np.pad(grid, 1))
    want, _ = _edit_and_check(c, dim, grid, p, m, "relaid")
    desc, (n, root) = c.read_descriptors(), c.octree_size()
    assert np.array_equal(desc[:len(d2)], d2), "an old word was overwritten"
    fresh = vrc.Octree.Generate(want.reshape(-1), dim, layout=vrc.LAYOUT_NO_PAGE_HEADERS)
    assert er.masks_by_position(desc, root, dim) == er.masks_by_position(fresh.descriptor_buffer, fresh.root_index, dim)


# ---------------------------------------------------------------------------- 9. determinism and growth
def test_determinism_growth_bound_and_no_change(atlas):
    dim = 32
    grid = _grid(dim, 50)
    p, m = er.random_batch(np.random.default_rng(51), dim)
    a, b = _caster(atlas, dim, grid), _caster(atlas, dim, grid)
    n0 = a.octree_size()[0]
    assert np.array_equal(a.read_descriptors(), b.read_descriptors())
    ia = a.set_voxels(p, m)
    ib = b.set_voxels(p[::-1][::-1].copy(), m.copy())
    assert {k: v for k, v in ia.items() if k != "seconds"} == {k: v for k, v in ib.items() if k != "seconds"}
    da, db = a.read_descriptors(), b.read_descriptors()
    assert np.array_equal(da, db), np.nonzero(da != db)[0][:8]
    for x, y in zip(a.read_attachments(), b.read_attachments()):
        assert np.array_equal(x, y)
    bricks, above = er.touched_nodes(p, dim)
    assert ia["bricks_touched"] == bricks and ia["n_descriptors"] == n0 + ia["descriptors_added"]
    assert 0 < ia["descriptors_added"] <= 72 * bricks + 16 * above + 1
    # what no pass stored in the appended range is zero, and nothing points outside the array
    assert np.count_nonzero(da[n0:]) < ia["descriptors_added"]
    # a batch that changes nothing: solid voxels set to their own material, empty voxels cleared
    cur = _whole(a, dim)[1:-1, 1:-1, 1:-1]
    q = np.random.default_rng(52).integers(0, dim, size=(500, 3)).astype(I)
    same = cur[q[:, 2], q[:, 1], q[:, 0]].astype(I)
    assert (same != 0).any() and (same == 0).any()
    before, mem = a.octree_size(), a.memory_usage2()["octree_bytes"]
    info = a.set_voxels(q, same)
    assert info["voxels_changed"] == 0 and info["descriptors_added"] == 0 and info["bricks_touched"] == 0
    assert a.octree_size() == before == (info["n_descriptors"], info["root_index"]) and a.memory_usage2()["octree_bytes"] == mem
    assert np.array_equal(a.read_descriptors(), da)
    info = a.set_voxels(np.zeros((0, 3), I), np.zeros(0, I))                   # n = 0
    assert info["voxels_changed"] == 0 and a.octree_size() == before


# ---------------------------------------------------------------------------- 10. reallocation
def test_exact_reserve_reallocates_every_batch(atlas):
    dim = 16
    grid = _grid(dim, 60)
    c = _caster(atlas, dim, grid, settings=(("edit_reserve", 0),))
    rng = np.random.default_rng(61)
    cur = grid
    for k in range(50):
        p = rng.integers(0, dim, size=(1, 3)).astype(I)
        x, y, z = p[0]
        m = np.array([0 if cur[z, y, x] else 6], I)
        cur, info = _edit_and_check(c, dim, cur, p, m, f"realloc{k}")
        assert c.octree_size() == (info["n_descriptors"], info["root_index"])
        lookup, attach = c.read_attachments()
        assert c.memory_usage2()["octree_bytes"] == 8 * info["n_descriptors"] + 4 * len(lookup) + 8 * len(attach), "edit_reserve = 0 is exact"
    # the default reserve: the same scene, fewer allocations than batches
    d = _caster(atlas, dim, grid)
    rng = np.random.default_rng(61)
    cur, sizes = grid, set()
    for k in range(10):
        p = rng.integers(0, dim, size=(1, 3)).astype(I)
        x, y, z = p[0]
        cur, info = _edit_and_check(d, dim, cur, p, np.array([0 if cur[z, y, x] else 6], I), f"reserve{k}")
        sizes.add(d.memory_usage2()["octree_bytes"])
    assert len(sizes) == 1


# ---------------------------------------------------------------------------- 11. errors
def test_errors_change_nothing(atlas):
    dim = 16
    grid = _grid(dim, 70)
    c = _caster(atlas, dim, grid)
    d0, size0 = c.read_descriptors(), c.octree_size()
    p, m = np.array([[1, 2, 3], [4, 5, 6]], I), np.array([5, 0], I)
    h, lib = c._h, vrc.lib
    pp, mp = p.ctypes.data_as(C.POINTER(C.c_int32)), m.ctypes.data_as(C.POINTER(C.c_int32))
    info = vrc.EditInfo()
    info.struct_size = C.sizeof(vrc.EditInfo)
    INVALID, NOT_READY, LIMIT = 1, 2, 6
    assert vrc.STATUS[LIMIT] == "VRC_ERR_LIMIT"
    assert lib.vrc_set_voxels(None, pp, mp, 2, 0, None) == INVALID
    assert lib.vrc_set_voxels(h, None, mp, 2, 0, None) == INVALID
    assert lib.vrc_set_voxels(h, pp, None, 2, 0, None) == INVALID
    assert lib.vrc_set_voxels(h, pp, mp, -1, 0, None) == INVALID
    assert lib.vrc_set_voxels(h, pp, mp, 2, 1, None) == INVALID and lib.vrc_set_voxels(h, pp, mp, 2, 0x80000000, None) == INVALID
    for bad in (128, -129, 2 ** 31 - 1):
        mb = np.array([5, bad], I)
        assert lib.vrc_set_voxels(h, pp, mb.ctypes.data_as(C.POINTER(C.c_int32)), 2, 0, C.byref(info)) == INVALID
    import torch
    tp, tm = torch.zeros(16, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    assert lib.vrc_set_voxels_device(h, C.c_void_p(tp.data_ptr() + 2), C.c_void_p(tm.data_ptr()), 2, 0, None) == INVALID
    assert lib.vrc_set_voxels_device(h, C.c_void_p(tp.data_ptr()), C.c_void_p(tm.data_ptr() + 1), 2, 0, None) == INVALID
    assert lib.vrc_set_voxels_device(h, None, C.c_void_p(tm.data_ptr()), 2, 0, None) == INVALID
    assert lib.vrc_set_voxels_device(h, C.c_void_p(tp.data_ptr()), C.c_void_p(tm.data_ptr()), 2, 2, None) == INVALID
    assert lib.vrc_set_voxels(h, None, None, 0, 0, C.byref(info)) == 0 and info.voxels_changed == 0 and info.n_descriptors == size0[0]
    assert np.array_equal(c.read_descriptors(), d0) and c.octree_size() == size0
    assert np.array_equal(_whole(c, dim), np.pad(grid, 1))
    # not ready: a handle that has not validated
    n = vrc.CLCaster()
    assert n.init(0)
    assert lib.vrc_set_voxels(n._h, pp, mp, 2, 0, None) == NOT_READY
    # a tree adopted by a handle outside the group: refused, nothing changes; released, the edit goes through
    other = vrc.CLCaster()
    assert other.init(0) and other.assign_octree_from(c)
    assert lib.vrc_set_voxels(h, pp, mp, 2, 0, C.byref(info)) == LIMIT
    assert lib.vrc_set_voxels_device(h, C.c_void_p(tp.data_ptr()), C.c_void_p(tm.data_ptr()), 2, 0, None) == LIMIT
    assert np.array_equal(c.read_descriptors(), d0) and c.octree_size() == size0 and other.octree_size() == size0
    assert other.release_octree()
    _edit_and_check(c, dim, grid, p, m, "after-release")


# ---------------------------------------------------------------------------- 12. group
def test_group_with_own_copies(atlas):
    dim = 32
    grid = _grid(dim, 80)
    grid[:3] = 5
    p, m = er.random_batch(np.random.default_rng(81), dim)
    single = _caster(atlas, dim, grid, settings=(("empty_boxes", 0),))
    want, info1 = _edit_and_check(single, dim, grid, p, m, "single")
    for using_octree in (0, 1):
        g = _caster(atlas, dim, grid, settings=(("empty_boxes", 0),), group=[0, 0], using_octree=using_octree)
        assert g.group_size() == 2 and g.memory_usage2(1)["octree_shared"] == 0
        _, info = _edit_and_check(g, dim, grid, p, m, f"group{using_octree}")
        assert single.overwrite_setting("using_octree", using_octree)
        if using_octree:
            single.set_voxels(p, m)                             # the single handle's map too
        else:
            assert {k: v for k, v in info.items() if k != "seconds"} == {k: v for k, v in info1.items() if k != "seconds"}
        img, hits, ctr = _frame(g)
        simg, shits, sctr = _frame(single)
        assert np.array_equal(img, simg) and np.array_equal(hits, shits) and ctr == sctr, using_octree


def test_group_that_shares_one_tree(atlas):
    """the ranks on rank 0's GPU hold ONE tree: the edit runs once, every rank takes the new root"""
    dim = 16
    grid = _grid(dim, 82)
    grid[:3] = 5
    p, m = er.random_batch(np.random.default_rng(83), dim, n=300)
    g = _caster(atlas, dim, grid, settings=(("empty_boxes", 0),), group=[0, 0], own_copies=False)
    assert g.memory_usage2(1)["octree_shared"] == 1 and g.memory_usage2(0)["tree_holders"] == 2
    want, info = _edit_and_check(g, dim, grid, p, m, "shared-group")
    assert g.memory_usage2(0)["tree_holders"] == 2
    f = _caster(atlas, dim, want, settings=(("empty_boxes", 0),))
    img, hits, ctr = _frame(g)
    fimg, fhits, fctr = _frame(f)
    assert np.array_equal(img, fimg) and np.array_equal(hits, fhits) and ctr == fctr


# ---------------------------------------------------------------------------- 13. the index-audit build
def test_audit_build_renders_an_edited_tree_without_a_violation(tmp_path):
    out = str(tmp_path / "edit_audit.json")
    env = dict(os.environ, VRC_LIB_PATH=os.path.join(ROOT, "voxel-raycaster_amd", "libvrc_audit.so"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "edit_audit_case.py"), out], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.load(open(out))
    report, info = got["report"], got["info"]
    bad = {a: e for a, e in report.items() if e["violations"]}
    assert not bad, bad
    for array in ("descriptors", "far_slots", "attach_lookup", "attachments", "image"):
        e = report[array]
        assert e["accesses"] > 0 and e["extent_published"] and e["max_index"] < e["extent"], (array, e)
    # edit_reserve = 0: what is allocated is what the tree holds, and that is the extent the frame was checked against
    assert report["descriptors"]["extent"] == report["far_slots"]["extent"] == report["attach_lookup"]["extent"] == info["n_descriptors"]
    assert report["attachments"]["extent"] == got["n_attachments"]
    assert report["descriptors"]["max_index"] >= got["n_before"], "the frame never read an appended word"
    assert got["reads_ok"]
