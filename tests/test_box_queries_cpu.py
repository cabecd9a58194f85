"""Box queries (vrc_box_intersection), CPU side: the numpy replay of tests/box_replay.py -- the oracle the GPU tests compare
against -- checked against brute force (the range rule, the Morton order) and against a tree-walking variant of itself (per-voxel
occupancy from vrc_octree_get_voxel on the oracle's descriptor array); the C symbols and their null-handle answer; the new
kernels' resources in libvrc.so."""
import ctypes as C
import os

import numpy as np
import pytest

import box_replay as br
import scenes
import voxel_raycaster_amd as vrc
from oracle import orc

F = np.float32


def _edge_boxes():
    b = [[3, 4, 5, 2, 2, 2], [3, 4, 5, 0, 0, 0], [3.5, 4.5, 5.5, 0, 0, 0], [3, 4, 5, 0.5, 1, 0], [2.999, 3.001, 4, 1, 1, 1],
         [-2, -2, -2, 3, 3, 3], [-5, 1, 1, 2, 2, 2], [-0.5, 0, 0, 0.5, 1, 1], [15, 15, 15, 4, 4, 4], [16, 0, 0, 1, 1, 1],
         [15.5, 0, 0, 0.5, 1, 1], [0, 0, 0, 16, 16, 16], [-1, -1, -1, 100, 100, 100], [0, 0, 0, -0.0, 1, 1],
         [0, 0, 0, -1, 1, 1], [np.nan, 0, 0, 1, 1, 1], [0, 0, 0, np.inf, 1, 1], [-np.inf, 0, 0, 1, 1, 1],
         [2.0 ** 30, 0, 0, 1, 1, 1], [2.0 ** 30 - 64, 0, 0, 64, 1, 1], [2.0 ** 30 - 128, 0, 0, 1, 1, 1], [-2.0 ** 30, 0, 0, 1, 1, 1],
         [1e-8, 0, 0, 1e-8, 0, 0], [7, 7, 7, 1e-7, 1e-7, 1e-7], [0.25, 0.25, 0.25, 0.5, 0.5, 0.5], [4, 4, 4, 1, 0, 0],
         [15.999999, 0, 0, 0, 0, 0], [1, 2, 3, 3e38, 1, 1]]
    return np.array(b, dtype=F)


def test_range_rule_equals_brute_force_overlap():
    dim = 16
    rng = np.random.default_rng(1)
    boxes = np.concatenate([_edge_boxes(), br.random_boxes(rng, 400, dim)]).astype(F)
    lo, hi, flags, rej = br.box_ranges(boxes, (dim,) * 3)
    brute = br.brute_overlap(boxes, (dim,) * 3)
    for i, axes in enumerate(brute):
        if axes is None:
            assert rej[i] and flags[i] == br.REJECTED, boxes[i]
            continue
        assert not rej[i]
        for a in range(3):
            want = axes[a]
            got = np.arange(lo[i, a], hi[i, a])
            assert np.array_equal(got, want), (i, a, boxes[i], got, want)
    # the edge cases by hand: a box resting on a face does not overlap the voxel below it; a plane lies in floor(o)
    assert lo[0].tolist() == [3, 4, 5] and hi[0].tolist() == [5, 6, 7]
    assert lo[1].tolist() == [3, 4, 5] and hi[1].tolist() == [4, 5, 6]
    assert flags[5] == br.CLIPPED and lo[5].tolist() == [0, 0, 0] and hi[5].tolist() == [1, 1, 1]
    assert flags[6] == br.CLIPPED and (lo[6] >= hi[6]).any()                     # wholly outside: clipped, not rejected
    assert flags[9] == br.CLIPPED and (lo[9] >= hi[9]).any()
    assert flags[11] == 0 and flags[12] == br.CLIPPED
    assert flags[13] == 0                                                        # -0 is not a negative extent
    assert all(flags[k] == br.REJECTED for k in (14, 15, 16, 17, 18, 19, 21, 27))   # |o| or |o + m| >= 2^30, -2^30 too
    assert flags[20] == br.CLIPPED


def test_morton_key_equals_a_brute_force_sort():
    rng = np.random.default_rng(2)
    pts = rng.integers(0, 64, size=(3000, 3))

    def brute(p):                                           # compare bit by bit from the top, z before y before x
        return tuple(int((p[a] >> k) & 1) for k in range(5, -1, -1) for a in (2, 1, 0))

    want = sorted(range(len(pts)), key=lambda i: brute(pts[i]))
    got = np.argsort(br.morton_key(pts), kind="stable")
    assert np.array_equal(pts[got], pts[want])
    assert br.morton_key([[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [0, 0, 4]]).tolist() == [1, 2, 4, 8, 256]


def _tree_materials(buf, root, dim):
    """mat[x, y, z]: 5 where vrc_octree_get_voxel on the descriptor array finds the voxel solid, else 0."""
    out = np.zeros((dim, dim, dim), np.int8)
    pos = (C.c_int32 * 3)()
    found, res, sub = C.c_int32(), C.c_int32(), (C.c_int32 * 3)()
    bp = buf.ctypes.data_as(C.POINTER(C.c_uint64))
    for x in range(dim):
        for y in range(dim):
            for z in range(dim):
                pos[0], pos[1], pos[2] = x, y, z
                assert vrc.lib.vrc_octree_get_voxel(bp, root, dim, pos, C.byref(found), C.byref(res), sub) == 0
                out[x, y, z] = 5 if found.value else 0
    return out


@pytest.mark.parametrize("make", [m for m in scenes.ALL if m()["dim"] <= 64], ids=lambda m: m.__name__)
def test_grid_replay_equals_the_tree_walk(make):
    s = make()
    dim = s["dim"]
    buf, root = orc.octree_generate(s["grid"], dim, buffer_size=200000)
    tree = _tree_materials(buf, root, dim)
    grid = np.where(br.grid_xyz(s["grid"], dim) != 0, 5, 0).astype(np.int8)
    assert np.array_equal(tree, grid)
    rng = np.random.default_rng(dim)
    boxes = br.random_boxes(rng, 300, dim)
    for stopping in (False, True):
        a = br.GridReplay(grid, stopping).query(boxes, 40)
        b = br.GridReplay(tree, stopping).query(boxes, 40)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    # the list is the Morton-sorted, range-filtered set of solid voxels, truncated; counts and corners are theirs
    rec, cnt, vox = br.GridReplay(grid).query(boxes, 40)
    lo, hi, _, _ = br.box_ranges(boxes, (dim,) * 3)
    solid = np.argwhere(grid != 0)
    for i in range(0, len(boxes), 7):
        sel = solid[((solid >= lo[i]) & (solid < hi[i])).all(axis=1)] if (hi[i] > lo[i]).all() else solid[:0]
        assert cnt[i] == len(sel)
        if len(sel):
            assert rec[i, 1:4].tolist() == sel.min(0).tolist() and rec[i, 4:7].tolist() == sel.max(0).tolist()
            order = sel[np.argsort(br.morton_key(sel), kind="stable")][:40]
            assert np.array_equal(vox[i, :len(order), :3], order)
        assert rec[i, 7] == min(len(sel), 40)


def test_leaf_tree_helper_equals_its_grid():
    """tests/leaftree.py (the GPU tests' tree with solid leaves above the bottom): vrc_octree_get_voxel finds exactly the dense
    grid it returns, leaves one, two and three levels above the bottom included."""
    import leaftree
    depth, dim = 5, 32
    rng = np.random.default_rng(5)
    desc, root, grid = leaftree.leaf_octree(rng.integers(0, dim, size=(300, 3)),
                                            [(0, 0, 0, 4), (8, 8, 8, 8), (4, 0, 0, 2), (16, 16, 0, 4), (20, 4, 6, 2)], depth)
    assert np.array_equal(_tree_materials(desc, root, dim), br.grid_xyz(grid, dim))


def test_symbols_and_null_handle():
    lib = vrc.lib
    for name in ("vrc_box_intersection", "vrc_box_intersection_device"):
        assert hasattr(lib, name)
    b = np.zeros((1, 6), F)
    r, c = np.zeros((1, 8), np.int32), np.zeros(1, np.int64)
    assert lib.vrc_box_intersection(None, b.ctypes.data_as(C.POINTER(C.c_float)), 1, 0, 0, r.ctypes.data_as(C.POINTER(C.c_int32)),
                                    c.ctypes.data_as(C.POINTER(C.c_int64)), None) == 1
    assert lib.vrc_box_intersection_device(None, None, 1, 0, 0, None, None, None) == 1
    assert (vrc.BOX_STOPPING_ONLY, vrc.BOX_ANY, vrc.BOX_TRUNCATED, vrc.BOX_CLIPPED, vrc.BOX_REJECTED) == (1, 1, 2, 4, 8)


def test_box_query_kernels_have_no_scratch():
    """The box-query kernels are in libvrc.so's gfx950 code object and use no private segment (stackless walks)."""
    import test_kernel_resources as tkr
    if not os.path.exists(os.path.join(tkr.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    table = tkr.kernel_table()
    for kernel in ("box_query_plan_kernel", "box_query_count_kernel", "box_query_finalize_kernel"):
        names = [k for k in table if kernel in k]
        assert names, kernel + " missing from libvrc.so"
        for k in names:
            assert table[k]["private_segment_fixed_size"] == 0, (k, table[k])
