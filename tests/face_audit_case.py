"""Child process of tests/test_face_extraction_audit_gpu.py: a handful of the small face-extraction cases through the index-audit
library (VRC_LIB_PATH names libvrc_audit.so, as for tests/region_audit_case.py) -- a re-laid-out tree with far pointers and
materials, then the dense map -- and the audit's report after each as JSON, with whether the lists equal the replay.  Not a
test file."""
import json
import sys

import numpy as np

import conftest  # noqa: F401  (the repository root and tests/ on sys.path)
import box_replay as br
import face_replay as fr
import relayout as rl
import scenes
import voxel_raycaster_amd as vrc
from gpu_helpers import configure


def _equal(c, mat, dim, rng):
    ok = True
    batches = [((dim,) * 3, np.zeros((1, 3), np.int32)), ((dim + 6,) * 3, np.full((1, 3), -3, np.int32)),
               ((9, 8, 7), rng.integers(-10, dim + 3, size=(40, 3)).astype(np.int32)),
               ((21, 1, 13), rng.integers(-10, dim + 3, size=(20, 3)).astype(np.int32))]
    for size, lo in batches:
        for no_edge, stopping in ((False, False), (True, True)):
            counts, faces, _ = c.extract_faces(lo, size, no_map_edge=no_edge, stopping_only=stopping)
            want = fr.regions(mat, lo, size, no_edge, stopping)
            ok = ok and np.array_equal(counts, want[0]) and np.array_equal(faces, want[1])
    return bool(ok)


def main(out):
    assert vrc.index_audit_report() is not None, "this process did not load the index-audit library (VRC_LIB_PATH)"
    s = dict(scenes.floor_pillars())
    dim = s["dim"]
    g = rl.with_materials(s["grid"], dim)
    mat = br.grid_xyz(g, dim)
    o = vrc.Octree.Generate(g, dim, layout=2).attach_materials_from_grid(g)
    d2, r2, l2 = rl.relayout(o.descriptor_buffer, o.root_index, dim, np.random.default_rng(3), 0.5, o.attachment_lookup)
    o2 = vrc.Octree(d2, r2, dim)
    o2.attachment_lookup, o2.attachment_buffer = l2, o.attachment_buffer
    c = vrc.CLCaster()
    assert c.init(0)
    li = np.zeros((8, 10), np.float32)
    li[:1] = s["lights"][:1]
    configure(c, dim, scenes.hash_atlas(), s["cam_dir"], s["cam_pos"], li, 64, 48)
    assert c.assign_octree(o2) and c.assign_map(g, (dim,) * 3) and c.validate(), c.last_error()
    rng = np.random.default_rng(4)
    vrc.index_audit_report()                                   # (clear: each report below is one step's alone)
    tree_ok = _equal(c, mat, dim, rng)
    tree = vrc.index_audit_report()
    assert c.overwrite_setting("using_octree", 1) and c.validate(), c.last_error()
    vrc.index_audit_report()
    map_ok = _equal(c, mat, dim, rng)
    dense = vrc.index_audit_report()
    with open(out, "w") as f:
        json.dump(dict(tree=tree, dense=dense, tree_ok=tree_ok, map_ok=map_ok), f)


if __name__ == "__main__":
    main(sys.argv[1])
