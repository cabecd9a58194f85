"""numpy restatement of the face extraction (vrc_extract_faces, include/vrc.h) from a dense material grid mat[x, y, z]
(box_replay.grid_xyz: the array branch's bytes, or the tree's materials) or, for device-built shell terrains, from the
procedural columns (vrc.shell_column).  The test oracle of tests/test_face_extraction_*.py.  Not a test file.

A voxel is solid when its material is non-zero (stopping_only: 5 or 6); outside the scene nothing is solid.  Face (v, d), d =
0 .. 5 for -x, +x, -y, +y, -z, +z, exists when v is solid, lies in region and scene, and v + e_d is not solid -- read from the
scene, not from the region.  no_map_edge drops the faces whose neighbour lies outside the scene.  An entry is x, y, z,
d | (material & 0xff) << 8; a region's entries are sorted by brick (v >> 3) - (lo >> 3), z-major, then v.z, v.y, v.x, then d."""
import numpy as np

import voxel_replay as vr

NO_MAP_EDGE, STOPPING_ONLY = 1, 2


def solid_of(mat, stopping_only=False):
    mat = np.asarray(mat)
    return ((mat == 5) | (mat == 6)) if stopping_only else (mat != 0)


def block_faces(block_xyz, lo, dims, no_map_edge=False, stopping_only=False):
    """The faces of one region from `block_xyz`, the materials [x, y, z] of [lo - 1, lo + size + 1) with zeros outside the scene
    (the region and its one-voxel apron); dims: the scene's size.  (k, 4) int32, in the list's order."""
    block = np.asarray(block_xyz)
    lo = np.asarray(lo, dtype=np.int64).reshape(3)
    dims = np.broadcast_to(np.asarray(dims, dtype=np.int64), (3,))
    solid = solid_of(block, stopping_only)
    own = solid[1:-1, 1:-1, 1:-1]
    inner = block[1:-1, 1:-1, 1:-1]
    parts = []
    for d in range(6):
        axis, up = d >> 1, d & 1
        sl = [slice(1, -1)] * 3
        sl[axis] = slice(2, None) if up else slice(0, -2)
        at = np.argwhere(own & ~solid[tuple(sl)])
        v = at + lo
        code = d | ((inner[at[:, 0], at[:, 1], at[:, 2]].astype(np.int64) & 0xff) << 8)
        if no_map_edge:
            nb = v[:, axis] + (1 if up else -1)
            keep = (nb >= 0) & (nb < dims[axis])
            v, code = v[keep], code[keep]
        parts.append(np.column_stack([v, code]))
    f = np.concatenate(parts)
    b = (f[:, :3] >> 3) - (lo >> 3)
    order = np.lexsort((f[:, 3] & 0xff, f[:, 0], f[:, 1], f[:, 2], b[:, 0], b[:, 1], b[:, 2]))
    return f[order].astype(np.int32)


def region(mat_xyz, lo, size, no_map_edge=False, stopping_only=False):
    """The faces of the region [lo, lo + size) of the scene mat[x, y, z]."""
    mat = np.asarray(mat_xyz)
    lo = np.asarray(lo, dtype=np.int64).reshape(3)
    size = np.asarray(size, dtype=np.int64).reshape(3)
    block = vr.region(mat, lo - 1, size + 2).transpose(2, 1, 0)
    return block_faces(block, lo, mat.shape, no_map_edge, stopping_only)


def regions(mat_xyz, lo, size, no_map_edge=False, stopping_only=False):
    """(counts (n,) int64, the packed list (total, 4) int32) of a call with these regions."""
    lo = np.asarray(lo, dtype=np.int64).reshape(-1, 3)
    lists = [region(mat_xyz, c, size, no_map_edge, stopping_only) for c in lo]
    return packed(lists)


def packed(lists):
    counts = np.array([len(f) for f in lists], dtype=np.int64)
    return counts, (np.concatenate(lists) if lists else np.zeros((0, 4), np.int32)).reshape(-1, 4).astype(np.int32)


def column_regions(depth, lo, size, columns=None, no_map_edge=False, stopping_only=False):
    """regions() on a device-built shell terrain of 2^depth voxels per axis (voxel_replay.column_region: material 5 for
    lo_z <= z <= hi_z of vrc.shell_column)."""
    lo = np.asarray(lo, dtype=np.int64).reshape(-1, 3)
    size = np.asarray(size, dtype=np.int64).reshape(3)
    lists = [block_faces(vr.column_region(depth, c - 1, size + 2, columns).transpose(2, 1, 0), c, 1 << depth, no_map_edge, stopping_only)
             for c in lo]
    return packed(lists)


def brute_region(mat_xyz, lo, size, no_map_edge=False, stopping_only=False):
    """region() voxel by voxel, sorted by the key as Python tuples (small grids)."""
    mat = np.asarray(mat_xyz)
    dims = mat.shape
    step = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))

    def material(p):
        return int(mat[p]) if all(0 <= p[a] < dims[a] for a in range(3)) else 0

    def solid(m):
        return m in (5, 6) if stopping_only else m != 0

    rows = []
    for x in range(lo[0], lo[0] + size[0]):
        for y in range(lo[1], lo[1] + size[1]):
            for z in range(lo[2], lo[2] + size[2]):
                m = material((x, y, z))
                if not solid(m):
                    continue
                for d, e in enumerate(step):
                    nb = (x + e[0], y + e[1], z + e[2])
                    outside = not all(0 <= nb[a] < dims[a] for a in range(3))
                    if solid(material(nb)) or (no_map_edge and outside):
                        continue
                    key = ((z >> 3) - (lo[2] >> 3), (y >> 3) - (lo[1] >> 3), (x >> 3) - (lo[0] >> 3), z, y, x, d)
                    rows.append((key, (x, y, z, d | ((m & 0xff) << 8))))
    rows.sort()
    return np.array([r[1] for r in rows], dtype=np.int32).reshape(-1, 4)
