"""CPU suite: the voxel edits (vrc_set_voxels, csrc/voxel_edit.hip) where there is no GPU -- the numpy replay's own properties
(tests/edit_replay.py: the oracle of the GPU tests must itself be right), the header and the built library, the brick kernel's
resources in the code object, and the expected trees of the GPU tests: the host builder's tree of a replayed grid, walked by
position, is what an edited tree is compared with, so the walk and the builder's conventions are pinned here."""
import os
import re
import subprocess

import numpy as np
import pytest

import edit_replay as er
import relayout as rl
import test_kernel_resources as kr
import voxel_raycaster_amd as vrc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "voxel-raycaster_amd")


def test_replay_last_duplicate_wins():
    g = np.zeros((4, 4, 4), np.int8)
    out, skipped, changed = er.replay(g, [[1, 2, 3], [1, 2, 3], [0, 0, 0], [1, 2, 3]], [6, 7, 5, -3])
    assert out[3, 2, 1] == -3 and out[0, 0, 0] == 5 and skipped == 0 and changed == 2
    assert not g.any(), "the replay changed its input"
    # ... also when the last write restores what was there: nothing changed
    g[3, 2, 1] = 6
    out, _, changed = er.replay(g, [[1, 2, 3], [1, 2, 3]], [0, 6])
    assert out[3, 2, 1] == 6 and changed == 0


def test_replay_counts_outside_positions_as_skipped():
    g = np.full((2, 3, 4), 5, np.int8)                         # dz, dy, dx = 2, 3, 4
    p = [[-1, 0, 0], [4, 0, 0], [0, 3, 0], [0, 0, 2], [3, 2, 1], [2 ** 31 - 1, 0, 0], [0, -2 ** 31, 0]]
    out, skipped, changed = er.replay(g, p, [0] * len(p))
    assert skipped == 6 and changed == 1 and out[1, 2, 3] == 0 and np.count_nonzero(out == 0) == 1


def test_replay_clear_and_set():
    g = np.zeros((8, 8, 8), np.int8)
    g[1, 1, 1] = 7
    out, skipped, changed = er.replay(g, [[1, 1, 1], [2, 2, 2], [3, 3, 3]], [0, -128, 127])
    assert (skipped, changed) == (0, 3) and out[1, 1, 1] == 0 and out[2, 2, 2] == -128 and out[3, 3, 3] == 127
    with pytest.raises(AssertionError):
        er.replay(g, [[0, 0, 0]], [128])


def test_random_batch_has_duplicates_outsiders_and_clears():
    p, m = er.random_batch(np.random.default_rng(1), 16)
    inside = ((p >= 0) & (p < 16)).all(axis=1)
    assert p.shape == (2000, 3) and 40 <= np.count_nonzero(~inside) <= 200
    assert len({tuple(v) for v in p[inside]}) <= np.count_nonzero(inside) - 100
    assert 800 <= np.count_nonzero(m == 0) <= 1200 and set(np.unique(m)) == {0, 5, 6, 7, -3}


def test_header_declares_the_entry_points_and_the_struct():
    text = open(os.path.join(ROOT, "include", "vrc.h")).read()
    assert re.search(r"int vrc_set_voxels\(vrc_caster \*h, const int32_t \*positions, const int32_t \*materials, int64_t n, uint32_t flags, vrc_edit_info \*info\);", text)
    assert re.search(r"int vrc_set_voxels_device\(vrc_caster \*h, const void \*d_positions, const void \*d_materials, int64_t n, uint32_t flags, vrc_edit_info \*info\);", text)
    body = re.search(r"typedef struct vrc_edit_info \{(.*?)\} vrc_edit_info;", text, re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["struct_size", "reserved_", "skipped", "voxels_changed", "bricks_touched", "descriptors_added", "n_descriptors", "root_index", "seconds"]
    # the ctypes mirror has the same fields and the C layout's size: 2 x 4 + 7 x 8 bytes
    assert [n for n, _ in vrc.EditInfo._fields_] == fields
    import ctypes
    assert ctypes.sizeof(vrc.EditInfo) == 64


def test_library_exports_the_symbols():
    for lib in ("libvrc.so", "libvrc_audit.so"):
        syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], capture_output=True, text=True, check=True).stdout
        for name in ("vrc_set_voxels", "vrc_set_voxels_device", "vrc_read_attachments"):
            assert re.search(r"\bT " + name + r"$", syms, re.M), (lib, name)
    for name in ("vrc_set_voxels", "vrc_set_voxels_device"):
        assert name in vrc.SIGNATURES and hasattr(vrc.CLCaster, name[4:])


def test_brick_kernel_has_no_scratch_and_fits_its_lds():
    if not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    table = kr.kernel_table()
    names = [n for n in table if "voxel_edit_brick_kernel" in n]
    assert len(names) == 1, names
    k = table[names[0]]
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= 64                              # 8 waves per SIMD: the pass is latency-bound reads of the old tree
    # every kernel of the edit is in the code object (the key pass, the array scatter, the brick pass, the ancestor pass)
    assert sum(1 for n in table if "voxel_edit_" in n) == 4


def _generate(grid_zyx):
    dim = grid_zyx.shape[0]
    return vrc.Octree.Generate(grid_zyx.reshape(-1), dim, layout=vrc.LAYOUT_NO_PAGE_HEADERS)


def test_expected_trees_come_from_the_host_builder():
    """The tree an edit must produce is the host builder's tree of the replayed grid, compared by position: the walk finds the same
    (valid, leaf) at every node of a re-laid array, every empty subtree is pruned (valid 0 / leaf 1 in its parent), bottom-level
    descriptors carry leaf 0xFF, no solid region is a leaf above the bottom, and an empty scene is a root with valid mask 0."""
    rng = np.random.default_rng(7)
    for dim in (2, 4, 8, 16):
        g = np.where(rng.random((dim, dim, dim)) < 0.2, 5, 0).astype(np.int8)
        g[:dim // 2, :dim // 2, :dim // 2] = 5                     # a solid octant: not collapsed
        if dim >= 8:
            g[dim // 2:, :, :] = 0                                 # an empty half: pruned
        p, m = er.random_batch(rng, dim, n=200)
        g2, _, _ = er.replay(g, p, m)
        o = _generate(g2)
        want = er.masks_by_position(o.descriptor_buffer, o.root_index, dim)
        assert np.array_equal(rl.decode(o.descriptor_buffer, o.root_index, dim) != 0, g2.reshape(-1) != 0)
        for (x, y, z, size), (valid, leaf) in want.items():
            assert (leaf == 0xff) if size == 2 else (leaf == (~valid & 0xff)), (dim, x, y, z, size)
            assert valid or size == dim
            for k in range(8):
                half = size // 2
                cx, cy, cz = x + (half if k & 1 else 0), y + (half if k & 2 else 0), z + (half if k & 4 else 0)
                assert bool(valid >> k & 1) == bool(g2[cz:cz + half, cy:cy + half, cx:cx + half].any())
        if dim >= 4:
            d2, r2, _ = rl.relayout(o.descriptor_buffer, o.root_index, dim, rng, 1.0)
            assert er.masks_by_position(d2, r2, dim) == want
    empty = _generate(np.zeros((8, 8, 8), np.int8))
    assert er.masks_by_position(empty.descriptor_buffer, empty.root_index, 8) == {(0, 0, 0, 8): (0, 0xff)}


def test_growth_bound_counts():
    assert er.touched_nodes([[0, 0, 0], [7, 7, 7], [8, 0, 0], [-1, 0, 0]], 32) == (2, 2)      # two bricks, one 16^3 node, the root
    assert er.touched_nodes([[0, 0, 0]], 8) == (1, 0) and er.touched_nodes([[1, 1, 1]], 2) == (1, 0)
