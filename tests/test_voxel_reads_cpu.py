"""Voxel reads (vrc_get_voxels / vrc_read_regions), CPU side: the numpy replay of tests/voxel_replay.py -- the oracle the GPU
tests compare against -- checked against a per-voxel walk of the oracle's descriptor array (vrc_octree_get_voxel) and against
brute force on its own padding rule; the C symbols and their null-handle answer; the new kernels' resources in libvrc.so."""
import ctypes as C
import os

import numpy as np
import pytest

import box_replay as br
import scenes
import voxel_raycaster_amd as vrc
import voxel_replay as vr
from oracle import orc
from test_box_queries_cpu import _tree_materials


def _brute_region(mat, lo, size):
    out = np.zeros((size[2], size[1], size[0]), np.int8)
    for k in range(size[2]):
        for j in range(size[1]):
            for i in range(size[0]):
                x, y, z = lo[0] + i, lo[1] + j, lo[2] + k
                if 0 <= x < mat.shape[0] and 0 <= y < mat.shape[1] and 0 <= z < mat.shape[2]:
                    out[k, j, i] = mat[x, y, z]
    return out


def _check_replay_against(tree_mat, mat, dim, seed):
    """The replay on `mat` equals the tree walk's materials: the whole map, the whole map with an apron, regions and points
    inside, across and outside the map."""
    assert np.array_equal(vr.region(mat, (0, 0, 0), (dim,) * 3), tree_mat.transpose(2, 1, 0))
    apron = vr.region(mat, (-3, -3, -3), (dim + 6,) * 3)
    assert np.array_equal(apron[3:-3, 3:-3, 3:-3], tree_mat.transpose(2, 1, 0))
    inner = np.zeros_like(apron, dtype=bool)
    inner[3:-3, 3:-3, 3:-3] = True
    assert (apron[~inner] == 0).all()
    rng = np.random.default_rng(seed)
    for _ in range(40):
        lo = rng.integers(-10, dim + 3, size=3)
        size = rng.integers(1, 10, size=3)
        assert np.array_equal(vr.region(mat, lo, size), _brute_region(tree_mat, lo, size)), (lo, size)
    p = rng.integers(-4, dim + 4, size=(2000, 3))
    want = np.array([tree_mat[x, y, z] if (0 <= x < dim and 0 <= y < dim and 0 <= z < dim) else 0 for x, y, z in p], np.int32)
    assert np.array_equal(vr.points(mat, p), want)
    far = np.array([[2 ** 31 - 1, 0, 0], [-2 ** 31, 1, 1], [0, 0, dim]])
    assert (vr.points(mat, far) == 0).all()
    assert (vr.region(mat, (2 ** 31 - 4, 0, 0), (8, 2, 2)) == 0).all() and (vr.region(mat, (-2 ** 31, -2 ** 31, 0), (3, 3, 3)) == 0).all()


@pytest.mark.parametrize("make", [m for m in scenes.ALL if m()["dim"] <= 64], ids=lambda m: m.__name__)
def test_replay_equals_the_tree_walk(make):
    s = make()
    dim = s["dim"]
    buf, root = orc.octree_generate(s["grid"], dim, buffer_size=200000)
    tree = _tree_materials(buf, root, dim)
    mat = np.where(br.grid_xyz(s["grid"], dim) != 0, 5, 0).astype(np.int8)
    _check_replay_against(tree, mat, dim, dim)


def test_replay_equals_the_leaf_tree_walk():
    """... and on the tree with solid leaves one, two and three levels above the bottom (tests/leaftree.py)."""
    import leaftree
    depth, dim = 5, 32
    rng = np.random.default_rng(5)
    desc, root, grid = leaftree.leaf_octree(rng.integers(0, dim, size=(300, 3)),
                                            [(0, 0, 0, 4), (8, 8, 8, 8), (4, 0, 0, 2), (16, 16, 0, 4), (20, 4, 6, 2)], depth)
    _check_replay_against(_tree_materials(desc, root, dim), br.grid_xyz(grid, dim), dim, 6)


def test_region_layout_is_x_fastest_and_keeps_the_sign():
    mat = np.zeros((4, 3, 2), np.int8)
    mat[1, 2, 0] = -7
    mat[3, 0, 1] = 6
    r = vr.region(mat, (0, 0, 0), (4, 3, 2))
    assert r.shape == (2, 3, 4) and r[0, 2, 1] == -7 and r[1, 0, 3] == 6
    assert r.reshape(-1)[1 + 4 * (2 + 3 * 0)] == -7                  # (x - lo.x) + sx * ((y - lo.y) + sy * (z - lo.z))
    r = vr.region(mat, (-1, 1, 0), (3, 3, 1))
    assert r[0, 1, 2] == -7 and np.count_nonzero(r) == 1
    assert vr.points(mat, [[1, 2, 0], [3, 0, 1], [4, 0, 1], [-1, 0, 0]]).tolist() == [-7, 6, 0, 0]


def test_column_region_equals_the_dense_shell_terrain():
    depth, dim = 6, 64
    mat = br.grid_xyz(vrc.shell_terrain_dense(depth, seed=1, thickness=2), dim)
    assert set(np.unique(mat).tolist()) <= {0, 5}
    for lo, size in (((0, 0, 0), (dim, dim, dim)), ((-2, 5, -3), (9, 7, 70)), ((60, 60, 10), (8, 8, 40))):
        assert np.array_equal(vr.column_region(depth, lo, size), vr.region(mat, lo, size)), (lo, size)


def test_symbols_and_null_handle():
    lib = vrc.lib
    for name in ("vrc_get_voxels", "vrc_get_voxels_device", "vrc_read_regions", "vrc_read_regions_device"):
        assert hasattr(lib, name)
    p = np.zeros((1, 3), np.int32)
    o = np.zeros(1, np.int32)
    b = np.zeros(8, np.int8)
    size = np.array([2, 2, 2], np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.vrc_get_voxels(None, ip(p), 1, ip(o)) == 1
    assert lib.vrc_get_voxels_device(None, None, 1, None) == 1
    assert lib.vrc_read_regions(None, ip(p), 1, ip(size), b.ctypes.data_as(C.POINTER(C.c_int8)), 8) == 1
    assert lib.vrc_read_regions_device(None, None, 1, ip(size), None, 8) == 1
    for name in ("get_voxels", "get_voxels_device", "read_regions", "read_regions_device"):
        assert callable(getattr(vrc.CLCaster, name))


def test_voxel_read_kernels_have_no_scratch():
    """The voxel-read kernels are in libvrc.so's gfx950 code object and use no private segment."""
    import test_kernel_resources as tkr
    if not os.path.exists(os.path.join(tkr.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    table = tkr.kernel_table()
    for kernel in ("voxel_points_kernel", "voxel_regions_kernel"):
        names = [k for k in table if kernel in k]
        assert names, kernel + " missing from libvrc.so"
        for k in names:
            assert table[k]["private_segment_fixed_size"] == 0, (k, table[k])
