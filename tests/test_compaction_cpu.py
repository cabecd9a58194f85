"""CPU suite: the octree compaction (vrc_compact_octree, csrc/octree_compact.hip) where there is no GPU -- the numpy replay's own
properties (tests/compact_replay.py is the oracle of the GPU tests and must itself be right), the header, the bindings and the
built libraries, and the new kernels' resources in the code object."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import compact_replay as cr
import edit_replay as er
import relayout as rl
import test_kernel_resources as kr
import voxel_raycaster_amd as vrc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "voxel-raycaster_amd")
REACHES = (cr.DEFAULT_REACH, 64, 16)


def _far_pointers(desc, dim):
    """descriptors of the compacted array (every word is live) whose pointer is far: the far slots they name"""
    d = [int(v) for v in desc]
    _, parents, _ = rl._walk(d, 0, dim)
    return sorted(p + (d[p] & 0x7fff) for p, _ in parents if d[p] & 0x8000)


def _trees():
    """(tag, descriptors, root, dim, grid or None, lookup, attachments)"""
    desc, root, grid = rl.leaf_tree()
    yield "leaf", desc, root, 32, None, None, None            # (solid leaves above the bottom: no material grid decodes them apart)
    rng = np.random.default_rng(3)
    for dim in (2, 4, 8, 16, 32):
        g = rng.choice(np.array([0, 5, 6, -3], np.int8), size=dim ** 3, p=[0.7, 0.2, 0.05, 0.05]).astype(np.int8)
        if dim >= 8:
            g.reshape(dim, dim, dim)[:dim // 4, :dim // 4, :dim // 4] = 0
        o = vrc.Octree.Generate(g, dim).attach_materials_from_grid(g)
        yield f"gen{dim}", o.descriptor_buffer, o.root_index, dim, g, o.attachment_lookup, o.attachment_buffer


@pytest.mark.parametrize("reach", REACHES)
def test_replay_keeps_the_tree_and_is_canonical(reach):
    rng = np.random.default_rng(11)
    for tag, desc, root, dim, grid, lookup, attach in _trees():
        got = cr.compact(desc, root, dim, reach, lookup, attach)
        d2, info = got["descriptors"], got["info"]
        assert np.array_equal(rl.decode(d2, 0, dim, got["lookup"], got["attachments"]), rl.decode(desc, root, dim, lookup, attach)), tag
        if grid is not None:
            assert np.array_equal(rl.decode(d2, 0, dim, got["lookup"], got["attachments"]), grid), tag
        assert er.masks_by_position(d2, 0, dim) == er.masks_by_position(desc, root, dim), tag
        # every word is the root, a word of a reachable block or a far slot one descriptor names
        units, _, _ = rl._walk([int(v) for v in desc], root, dim)
        live = sum(n for _, n in units)
        slots = _far_pointers(d2, dim)
        assert len(set(slots)) == len(slots) == info["far_slots"], tag
        assert len(d2) == live + len(slots) == info["n_descriptors"] and info["live_descriptors"] == live, tag
        units2, _, _ = rl._walk([int(v) for v in d2], 0, dim)
        words = {first + k for first, n in units2 for k in range(n)} | set(slots)
        assert words == set(range(len(d2))) and sum(n for _, n in units2) == live, tag
        # these trees are far below 0x8000 words: no far pointer at the default reach; every deeper tree has some at reach 16
        if reach == cr.DEFAULT_REACH:
            assert len(desc) < 0x8000 and not slots, tag
        if reach == 16 and dim >= 8:
            assert slots, tag
        # a re-laid array is the same tree: the same output, word for word (the lookup too)
        if dim >= 4:
            d3, r3, l3 = rl.relayout(desc, root, dim, rng, 0.5, lookup)
            again = cr.compact(d3, r3, dim, reach, l3, attach)
            assert np.array_equal(again["descriptors"], d2), tag
            if lookup is not None:
                assert np.array_equal(again["lookup"], got["lookup"]) and np.array_equal(again["attachments"], got["attachments"]), tag
        # ... and so is the output itself
        twice = cr.compact(d2, 0, dim, reach, got["lookup"], got["attachments"])
        assert np.array_equal(twice["descriptors"], d2), tag
        assert twice["info"]["descriptors_before"] == twice["info"]["n_descriptors"] == len(d2)


def test_replay_far_counts_grow_as_the_reach_shrinks():
    desc, root, _ = rl.leaf_tree()
    far = [cr.compact(desc, root, 32, reach)["info"]["far_slots"] for reach in REACHES]
    assert far[0] == 0 < far[1] < far[2], far


def test_replay_drops_unused_attachment_slots_and_keeps_sharing():
    dim = 8
    g = np.zeros((dim, dim, dim), np.int8)
    g[0:2, 0:2, 0:2] = 6
    g[4:6, 4:6, 4:6] = 7
    o = vrc.Octree.Generate(g.reshape(-1), dim).attach_materials_from_grid(g.reshape(-1))
    lookup = np.asarray(o.attachment_lookup).copy()
    attach = np.concatenate([np.asarray(o.attachment_buffer, np.uint64), np.array([0x0909090909090909] * 3, np.uint64)])   # garbage slots
    got = cr.compact(o.descriptor_buffer, o.root_index, dim, lookup=lookup, attachments=attach)
    assert got["info"]["attachments_before"] == len(attach) and got["info"]["n_attachments"] == len(got["attachments"]) < len(attach)
    assert 0x0909090909090909 not in got["attachments"]
    assert np.array_equal(rl.decode(got["descriptors"], 0, dim, got["lookup"], got["attachments"]), g.reshape(-1))
    # every bottom-level descriptor naming ONE slot: one slot after the call, not one per descriptor
    plain = np.where(g != 0, 5, 0).astype(np.int8).reshape(-1)
    shared = cr.compact(o.descriptor_buffer, o.root_index, dim, lookup=np.zeros(len(lookup), np.uint32), attachments=np.array([cr.SOLID], np.uint64))
    assert shared["info"]["n_attachments"] == 1 and not shared["lookup"].any()
    assert np.array_equal(rl.decode(shared["descriptors"], 0, dim, shared["lookup"], shared["attachments"]), plain)
    # a tree without materials stays without
    none = cr.compact(o.descriptor_buffer, o.root_index, dim)
    assert none["lookup"] is None and none["attachments"] is None and none["info"]["n_attachments"] == 0


def test_replay_of_an_empty_scene_is_one_word():
    o = vrc.Octree.Generate(np.zeros(8 ** 3, np.int8), 8, layout=vrc.LAYOUT_NO_PAGE_HEADERS)
    got = cr.compact(o.descriptor_buffer, o.root_index, 8)
    assert len(got["descriptors"]) == 1 and (int(got["descriptors"][0]) >> 16) & 0xff == 0 and int(got["descriptors"][0]) & 0xffff == 0


def test_header_declares_the_entry_point_and_the_struct():
    text = open(os.path.join(ROOT, "include", "vrc.h")).read()
    assert re.search(r"int vrc_compact_octree\(vrc_caster \*h, uint32_t flags, vrc_compact_info \*info\);", text)
    assert re.search(r"#define VRC_COMPACT_DRY_RUN 1u", text) and vrc.COMPACT_DRY_RUN == 1
    body = re.search(r"typedef struct vrc_compact_info \{(.*?)\} vrc_compact_info;", text, re.S).group(1)
    fields = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == ["struct_size", "reserved_", "descriptors_before", "n_descriptors", "root_index", "live_descriptors", "far_slots",
                      "attachments_before", "n_attachments", "seconds"]
    assert [n for n, _ in vrc.CompactInfo._fields_] == fields and ctypes.sizeof(vrc.CompactInfo) == 72
    assert "there is no compaction" not in text


def test_library_exports_the_symbol():
    for lib in ("libvrc.so", "libvrc_audit.so"):
        syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], capture_output=True, text=True, check=True).stdout
        assert re.search(r"\bT vrc_compact_octree$", syms, re.M), lib
    assert "vrc_compact_octree" in vrc.SIGNATURES and hasattr(vrc.CLCaster, "compact_octree")
    assert "compact_octree" in open(os.path.join(PKG, "csrc", "clcaster.hpp")).read()


def test_compaction_kernels_have_no_scratch():
    if not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    table = kr.kernel_table()
    names = [n for n in table if "octree_compact_" in n]
    # the count, scatter, size, root and emit passes, the lookup remap and the attachment copy
    assert len(names) == 7, names
    for n in names:
        assert table[n]["private_segment_fixed_size"] == 0, (n, table[n])
        assert table[n]["vgpr_count"] <= 64, (n, table[n])
