"""numpy restatement of the voxel reads (vrc_get_voxels / vrc_read_regions, include/vrc.h): the material of a voxel from a dense
material grid mat[x, y, z] (box_replay.grid_xyz: the array branch's bytes, or the tree's materials -- the attachments, 5 without
them) or, for device-built shell terrains, from the procedural columns (vrc.shell_column).  Outside the map is 0.  The test
oracle of tests/test_voxel_reads_*.py.  Not a test file."""
import numpy as np


def region(mat_xyz, lo, size):
    """The block vrc_read_regions returns for one region: int8[sz, sy, sx] (C order: x fastest), the slice
    [lo, lo + size) of mat[x, y, z] with zeros where the region leaves the map."""
    mat = np.asarray(mat_xyz)
    lo = np.asarray(lo, dtype=np.int64).reshape(3)
    size = np.asarray(size, dtype=np.int64).reshape(3)
    out = np.zeros(tuple(size), dtype=np.int8)                        # [x, y, z]
    a = np.clip(lo, 0, mat.shape)
    b = np.clip(lo + size, 0, mat.shape)
    if (b > a).all():
        out[a[0] - lo[0]:b[0] - lo[0], a[1] - lo[1]:b[1] - lo[1], a[2] - lo[2]:b[2] - lo[2]] = mat[a[0]:b[0], a[1]:b[1], a[2]:b[2]]
    return np.ascontiguousarray(out.transpose(2, 1, 0))


def regions(mat_xyz, lo, size):
    """region() for every row of lo: int8[n, sz, sy, sx]."""
    lo = np.asarray(lo, dtype=np.int64).reshape(-1, 3)
    size = np.asarray(size, dtype=np.int64).reshape(3)
    out = np.zeros((len(lo), size[2], size[1], size[0]), dtype=np.int8)
    for i, c in enumerate(lo):
        out[i] = region(mat_xyz, c, size)
    return out


def points(mat_xyz, p):
    """The material at each position of p (n, 3), int32; 0 outside the map."""
    mat = np.asarray(mat_xyz)
    p = np.asarray(p, dtype=np.int64).reshape(-1, 3)
    inside = ((p >= 0) & (p < np.array(mat.shape))).all(axis=1)
    out = np.zeros(len(p), dtype=np.int32)
    q = p[inside]
    out[inside] = mat[q[:, 0], q[:, 1], q[:, 2]]
    return out


def column_region(depth, lo, size, columns=None):
    """region() on a device-built shell terrain of 2^depth voxels per axis: column (x, y) is solid, material 5, for
    lo_z <= z <= hi_z of vrc.shell_column.  columns: an optional callable (x, y) -> (lo, hi) (a cache)."""
    if columns is None:
        import voxel_raycaster_amd as vrc
        columns = lambda x, y: vrc.shell_column(depth, x, y)
    dim = 1 << depth
    lo = np.asarray(lo, dtype=np.int64).reshape(3)
    size = np.asarray(size, dtype=np.int64).reshape(3)
    out = np.zeros((size[2], size[1], size[0]), dtype=np.int8)
    z = np.arange(lo[2], lo[2] + size[2])
    for iy in range(size[1]):
        for ix in range(size[0]):
            x, y = int(lo[0] + ix), int(lo[1] + iy)
            if 0 <= x < dim and 0 <= y < dim:
                c0, c1 = columns(x, y)
                out[:, iy, ix] = np.where((z >= max(c0, 0)) & (z <= min(c1, dim - 1)), 5, 0)
    return out
