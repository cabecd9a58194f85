"""Child process of tests/test_compaction_gpu.py: an edit, a compaction and a frame through the index-audit library (VRC_LIB_PATH
names libvrc_audit.so, as for tests/edit_audit_case.py), and the audit's reports as JSON -- `during`: the compaction's own reads of
the old tree; `report`: the frame and the read-back of the compacted tree.  With edit_reserve = 0 the new arrays are allocated at
exactly their size, so the extents the frame is checked against must be the new ones; compact_near_reach = 16 gives the small
tree far pointers, so the frame reads far slots.  Not a test file."""
import json
import sys

import numpy as np

import conftest  # noqa: F401  (the repository root and tests/ on sys.path)
import compact_replay as cr
import edit_replay as er
import scenes
import voxel_raycaster_amd as vrc
from gpu_helpers import configure


def main(out):
    assert vrc.index_audit_report() is not None, "this process did not load the index-audit library (VRC_LIB_PATH)"
    dim = 32
    rng = np.random.default_rng(91)
    grid = rng.choice(np.array([0, 5, 6, -3], np.int8), size=(dim, dim, dim), p=[0.8, 0.1, 0.05, 0.05]).astype(np.int8)
    grid[:3] = 5
    c = vrc.CLCaster()
    assert c.init(0)
    li = np.zeros((8, 10), np.float32)
    li[0] = [0.01, 0.01, 0.01, 0.2, dim * 0.8, dim * 0.2, dim * 0.9, -1, -1, -1.5]
    configure(c, dim, scenes.hash_atlas(), (2.0, 1.5708), (dim * 0.5 + 0.37, 1.41, dim * 0.45 + 0.29), li, 64, 48)
    assert c.add_to_settings_buffer("edit_reserve", "EDIT_RESERVE", 0)
    assert c.add_to_settings_buffer("compact_near_reach", "COMPACT_NEAR_REACH", 16)
    c.build_dense_grid(5, grid.reshape(-1), attachments=True)
    assert c.validate(), c.last_error()
    p, m = er.random_batch(rng, dim, n=500)
    want, _, _ = er.replay(grid, p, m)
    c.set_voxels(p, m)
    desc0, (_, root0) = c.read_descriptors(), c.octree_size()
    lookup0, attach0 = c.read_attachments()
    vrc.index_audit_report()                                   # (clear: `during` is the compaction's alone)
    info = c.compact_octree()
    during = vrc.index_audit_report()
    assert c.compute(), c.last_error()
    got = c.read_regions(np.zeros((1, 3), np.int32), (dim,) * 3)[0]
    lookup, attach = c.read_attachments()
    report = vrc.index_audit_report()
    replay = cr.compact(desc0, root0, dim, 16, lookup0, attach0)
    replay_ok = bool(np.array_equal(c.read_descriptors(), replay["descriptors"]) and np.array_equal(lookup, replay["lookup"])
                     and np.array_equal(attach, replay["attachments"]))
    with open(out, "w") as f:
        json.dump(dict(during=during, report=report, info=info, n_attachments=len(attach), reads_ok=bool(np.array_equal(got, want)),
                       replay_ok=replay_ok), f)


if __name__ == "__main__":
    main(sys.argv[1])
