"""Child process of tests/test_voxel_edits_gpu.py: one edit through the index-audit library (VRC_LIB_PATH names libvrc_audit.so,
as for tests/index_audit_cases.py), then a frame and a read-back of the edited tree, and the audit's report as JSON.  With
edit_reserve = 0 the arrays are allocated anew at exactly their new size, so the extents the next frame is checked against must be
the new ones.  Not a test file."""
import json
import sys

import numpy as np

import conftest  # noqa: F401  (the repository root and tests/ on sys.path)
import edit_replay as er
import scenes
import voxel_raycaster_amd as vrc
from gpu_helpers import configure


def main(out):
    assert vrc.index_audit_report() is not None, "this process did not load the index-audit library (VRC_LIB_PATH)"
    dim = 32
    rng = np.random.default_rng(90)
    grid = rng.choice(np.array([0, 5, 6, -3], np.int8), size=(dim, dim, dim), p=[0.8, 0.1, 0.05, 0.05]).astype(np.int8)
    grid[:3] = 5
    c = vrc.CLCaster()
    assert c.init(0)
    li = np.zeros((8, 10), np.float32)
    li[0] = [0.01, 0.01, 0.01, 0.2, dim * 0.8, dim * 0.2, dim * 0.9, -1, -1, -1.5]
    configure(c, dim, scenes.hash_atlas(), (2.0, 1.5708), (dim * 0.5 + 0.37, 1.41, dim * 0.45 + 0.29), li, 64, 48)
    assert c.add_to_settings_buffer("edit_reserve", "EDIT_RESERVE", 0)
    c.build_dense_grid(5, grid.reshape(-1), attachments=True)
    assert c.validate(), c.last_error()
    n_before = c.octree_size()[0]
    p, m = er.random_batch(rng, dim, n=500)
    want, _, _ = er.replay(grid, p, m)
    info = c.set_voxels(p, m)
    vrc.index_audit_report()                                   # (clear: the report below is the edited tree's alone)
    assert c.compute(), c.last_error()
    got = c.read_regions(np.zeros((1, 3), np.int32), (dim,) * 3)[0]
    lookup, attach = c.read_attachments()
    report = vrc.index_audit_report()
    with open(out, "w") as f:
        json.dump(dict(report=report, info=info, n_before=n_before, n_attachments=len(attach), reads_ok=bool(np.array_equal(got, want))), f)


if __name__ == "__main__":
    main(sys.argv[1])
