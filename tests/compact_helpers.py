"""Helpers of the compaction tests (tests/test_compaction_gpu.py, tests/compact_audit_case.py): the scenes and casters of the
voxel-edit suite -- the same construction, so that a compacted tree is compared under the conditions the edits were tested under --
the state of a resident tree as numpy arrays, and one compaction checked word for word against the replay.  Not a test file."""
import numpy as np

import compact_replay as cr
import relayout as rl
import voxel_raycaster_amd as vrc
from gpu_helpers import configure

I = np.int32
MATERIALS = np.array([0, 5, 6, 7, -3], np.int8)
W, H = 64, 48


def grid_of(dim, seed):
    """random sparse int8[z][y][x] of the materials {0, 5, 6, 7, -3}, with an empty and a solid corner cube"""
    rng = np.random.default_rng(seed)
    g = rng.choice(MATERIALS, size=(dim, dim, dim), p=[0.8, 0.1, 0.04, 0.03, 0.03]).astype(np.int8)
    h = max(dim // 4, 1)
    g[:h, :h, :h] = 0
    g[-h:, -h:, -h:] = 5
    return g


def plain(g):
    return np.where(g != 0, 5, 0).astype(np.int8)


def caster(atlas, dim, grid=None, attachments=True, settings=(), octree=None, group=None, own_copies=True):
    c = vrc.CLCaster()
    assert (c.init_group(group, own_copies=own_copies) if group else c.init(0)), c.last_error()
    li = np.zeros((8, 10), np.float32)
    li[0] = [0.01, 0.01, 0.01, 0.2, dim * 0.8, dim * 0.2, dim * 0.9, -1, -1, -1.5]
    configure(c, dim, atlas, (2.0, 1.5708), (dim * 0.5 + 0.37, 1.41, dim * 0.45 + 0.29), li, W, H)
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


def whole(c, dim):
    """the whole map with a one-voxel apron, int8[dim + 2][dim + 2][dim + 2]"""
    return c.read_regions(np.full((1, 3), -1, I), (dim + 2,) * 3)[0]


def state(c):
    """(descriptors, root, lookup, attachments) of the resident tree"""
    desc = c.read_descriptors()
    n, root = c.octree_size()
    assert n == len(desc)
    lookup, attach = c.read_attachments()
    return desc, root, lookup, attach


def counts(info):
    return {k: v for k, v in info.items() if k != "seconds"}


def compact_and_check(c, dim, reach, grid, tag):
    """One vrc_compact_octree against the replay of the array before it: the arrays word for word, the counts, the decoded grid
    and the read-back.  Returns (info, the replay's result)."""
    desc0, root0, lookup0, attach0 = state(c)
    want = cr.compact(desc0, root0, dim, reach, lookup0, attach0)
    info = c.compact_octree()
    print(tag, info)
    desc, root, lookup, attach = state(c)
    assert root == 0 and len(desc) == want["info"]["n_descriptors"], (tag, info, want["info"])
    assert np.array_equal(desc, want["descriptors"]), (tag, np.nonzero(desc != want["descriptors"])[0][:8])
    if lookup0 is None:
        assert lookup is None and attach is None, tag
    else:
        assert np.array_equal(lookup, want["lookup"]), (tag, np.nonzero(lookup != want["lookup"])[0][:8])
        assert np.array_equal(attach, want["attachments"]), tag
    assert counts(info) == want["info"], (tag, info, want["info"])
    assert np.array_equal(rl.decode(desc, 0, dim, lookup, attach), grid.reshape(-1)), tag
    assert np.array_equal(whole(c, dim), np.pad(grid, 1)), tag
    return info, want
