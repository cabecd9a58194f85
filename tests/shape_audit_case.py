"""Child process of tests/test_voxel_shape_fills_audit_gpu.py: one batch of shape fills through the index-audit library (VRC_LIB_PATH
names libvrc_audit.so, as for tests/region_audit_case.py) into a 32^3 tree, a frame of the edited tree, then the same batch into
the dense map, and the audit's report after each step as JSON.  With edit_reserve = 0 the arrays are allocated anew at exactly
their new size, so the extents the frame is checked against must be the new ones.  Not a test file."""
import json
import sys

import numpy as np

import conftest  # noqa: F401  (the repository root and tests/ on sys.path)
import scenes
import shape_replay as sp
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
    assert c.assign_map(grid.reshape(-1), (dim,) * 3)
    assert c.validate(), c.last_error()
    n_before = c.octree_size()[0]
    first, m1 = sp.batch(dim)
    shapes, m = sp.batch(dim, 1)
    want, _, _ = sp.fill_shapes(grid, first, m1)
    want, _, _ = sp.fill_shapes(want, shapes, m)
    vrc.index_audit_report()                                   # (clear: each report below is one step's alone)
    c.fill_shapes(first, m1)
    after_first = vrc.index_audit_report()
    info = c.fill_shapes(shapes, m)                            # (the first batch's ancestor pass appended far pointers: this one reads them)
    after_second = vrc.index_audit_report()
    assert c.compute(), c.last_error()
    frame = vrc.index_audit_report()
    got = c.read_regions(np.zeros((1, 3), np.int32), (dim,) * 3)[0]
    assert c.overwrite_setting("using_octree", 1)
    vrc.index_audit_report()
    c.fill_shapes(first, m1)
    c.fill_shapes(shapes, m)
    after_map = vrc.index_audit_report()
    got_map = c.read_regions(np.zeros((1, 3), np.int32), (dim,) * 3)[0]
    with open(out, "w") as f:
        json.dump(dict(after_first=after_first, after_second=after_second, frame=frame, after_map=after_map, info=info, n_before=n_before,
                       reads_ok=bool(np.array_equal(got, want)), map_ok=bool(np.array_equal(got_map, want))), f)


if __name__ == "__main__":
    main(sys.argv[1])
