"""CPU suite: csrc/svo_node.hpp -- the descriptor format every tree-walking kernel decodes through -- compiles for the host, so
the device walkers' shared descent is checked here, where there is no GPU: tests/svo_node_check.cpp, a stand-alone program
built with g++ under AddressSanitizer + UBSan, walks small trees (dim 2 to 32) node by node and voxel by voxel against their
dense material grids.  Nothing sanitized is loaded into Python."""
import os
import re
import subprocess

import numpy as np

import relayout as rl
import scenes
import voxel_raycaster_amd as vrc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trees():
    """(name, octree with attachments, material grid): builder-made trees of 2^3 .. 32^3, a tree with solid leaves above the
    bottom level, and re-laid arrays of the two 32^3 ones at far_fraction = 1 (every parent holds a far pointer, the root is
    not at index 0)."""
    out = []
    for dim in (2, 4, 8, 16):
        rng = np.random.default_rng(300 + dim)
        g = rng.choice(np.array([0, 5, 6, -3], np.int8), size=dim ** 3, p=[0.5, 0.3, 0.15, 0.05])
        out.append((f"generate{dim}", vrc.Octree.Generate(g, dim).attach_materials_from_grid(g), g))
    s = scenes.floor_pillars(32)
    g = rl.with_materials(s["grid"], 32)
    out.append(("floor_pillars32", vrc.Octree.Generate(g, 32).attach_materials_from_grid(g), g))
    desc, root, g = rl.leaf_tree()
    out.append(("leaf_octree32", vrc.Octree(desc, root, 32).attach_materials_from_grid(g), g))
    for k, (name, o, g) in enumerate(out[-2:]):
        d2, r2, l2 = rl.relayout(o.descriptor_buffer, o.root_index, 32, np.random.default_rng(40 + k), 1.0, o.attachment_lookup)
        o2 = vrc.Octree(d2, r2, 32)
        o2.attachment_lookup, o2.attachment_buffer = l2, o.attachment_buffer
        assert r2 != 0
        out.append((name + "-relaid", o2, g))
    return out


def test_shared_descent_against_the_grids_under_sanitizers(tmp_path):
    exe = str(tmp_path / "svo_node_check")
    csrc = os.path.join(ROOT, "voxel-raycaster_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "svo_node_check.cpp"),
                           os.path.join(csrc, "svo_builder.cpp"), "-o", exe])
    args = []
    for name, o, g in _trees():
        tree, grid = str(tmp_path / (name + ".oct")), str(tmp_path / (name + ".grid"))
        o.Save(tree)
        np.asarray(g, np.int8).reshape(-1).tofile(grid)
        args += [tree, grid]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"svo node ok: trees (\d+), far pointers (\d+), table starts (\d+), moved roots (\d+)", out.stdout)
    assert m, out.stdout + out.stderr
    trees, far, table_starts, moved_roots = map(int, m.groups())
    # a set of trees without far pointers, or descents that all start at a root at index 0, would pass for nothing
    assert trees == len(args) // 2 and far > 0 and table_starts > 0 and moved_roots >= 2
