"""Test helper: the exhaustive host check of the empty boxes (vrc_read_empty_boxes), with nothing of the device's own machinery.
An independent walk of the descriptor array (treetools.empty_children) gives every EMPTY child slot the root reaches its cube,
the slot's word gives the box -- six 5-bit extent codes, -x -y -z +x +y +z, in units of the cube's size, clipped by the map --
and a summed-volume table of the dense grid must hold no solid voxel anywhere inside it.  Only words of descriptors the root
reaches are read: the words of garbage descriptors (an edited array has them) are unspecified.  Not a test file."""
import numpy as np

import treetools

_EXTENT = np.array([treetools.box_decode(c) for c in range(32)], dtype=np.int64)


def summed_volume(solid):
    """S[z, y, x] = solid voxels in [0, z) x [0, y) x [0, x) of solid bool[z][y][x]"""
    dz, dy, dx = solid.shape
    S = np.zeros((dz + 1, dy + 1, dx + 1), dtype=np.int64)
    S[1:, 1:, 1:] = np.asarray(solid).astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    return S


def solids(S, x0, y0, z0, x1, y1, z1):
    """solid voxels in [x0, x1) x [y0, y1) x [z0, z1), for numbers or arrays of corners"""
    return S[z1, y1, x1] - S[z0, y1, x1] - S[z1, y0, x1] - S[z1, y1, x0] + S[z0, y0, x1] + S[z0, y1, x0] + S[z1, y0, x0] - S[z0, y0, x0]


def boxes_of(desc, root, dim, words):
    """(slots int64[n, 6] = descriptor, slot, x, y, z, size; lo int64[n, 3]; hi int64[n, 3]; ext int64[n, 6]): the box of every
    empty child slot the root reaches, as its word in `words` (uint32[n_desc, 8]) gives it"""
    slots = np.array([(index, k, x, y, z, size) for index, k, (x, y, z), size in treetools.empty_children(desc, root, dim)],
                     dtype=np.int64).reshape(-1, 6)
    w = np.asarray(words)[slots[:, 0], slots[:, 1]].astype(np.int64)
    size = slots[:, 5:6]
    ext = _EXTENT[(w[:, None] >> (5 * np.arange(6))) & 31] * size
    lo = np.maximum(slots[:, 2:5] - ext[:, :3], 0)
    hi = np.minimum(slots[:, 2:5] + size + ext[:, 3:], dim)
    return slots, lo, hi, ext


def check_boxes(desc, root, dim, words, solid, tag="", must_grow=True):
    """Every voxel of every box is empty in solid bool[z][y][x]; every box contains its own node (extents are not negative by
    construction); and, unless must_grow is False, more than a quarter of the boxes are wider than their node (the structure is
    not vacuous).  Returns (n_boxes, grown, volume, node_volume); raises AssertionError naming the first box that holds a solid
    voxel."""
    slots, lo, hi, ext = boxes_of(desc, root, dim, words)
    S = summed_volume(solid)
    inside = solids(S, lo[:, 0], lo[:, 1], lo[:, 2], hi[:, 0], hi[:, 1], hi[:, 2])
    bad = np.nonzero(inside)[0]
    if bad.size:
        index, k, x, y, z, size = (int(v) for v in slots[bad[0]])
        raise AssertionError(f"{tag + ': ' if tag else ''}descriptor {index} slot {k}: the box {tuple(int(v) for v in lo[bad[0]])}.."
                             f"{tuple(int(v) for v in hi[bad[0]])} of the {size}^3 node at {(x, y, z)} holds a solid voxel")
    n_boxes = len(slots)
    grown = int(ext.any(axis=1).sum())
    volume = int((hi - lo).prod(axis=1).sum())
    node_volume = int((slots[:, 5] ** 3).sum())
    if must_grow:
        assert grown > n_boxes // 4, f"{tag + ': ' if tag else ''}{grown} of {n_boxes} boxes are wider than their node"
    return n_boxes, grown, volume, node_volume
