"""CPU suite: the region edits (vrc_fill_boxes / vrc_write_regions, csrc/region_write.hip) where there is no GPU -- the numpy
replay's own properties (tests/region_replay.py: the oracle of the GPU tests must itself be right), its agreement with the voxel
edits' replay on the expanded batch, the header, the ctypes table and the built libraries, the null-handle answers, the brick
kernel's resources in the code object, and the kernel counts that other tests pin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edit_replay as er
import region_replay as rg
import test_kernel_resources as kr
import voxel_raycaster_amd as vrc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "voxel-raycaster_amd")
CALLS = ("vrc_fill_boxes", "vrc_fill_boxes_device", "vrc_write_regions", "vrc_write_regions_device")


def test_fill_order_decides_overlaps_and_flags():
    g = np.zeros((4, 4, 4), np.int8)
    out, skipped, changed = rg.fill(g, [[0, 0, 0], [1, 1, 1]], [[3, 3, 3], [3, 3, 3]], [6, 7])
    assert out[0, 0, 0] == 6 and out[1, 1, 1] == 7 and out[3, 3, 3] == 7 and out[0, 3, 3] == 0 and (skipped, changed) == (0, 27 + 27 - 8)
    assert not g.any(), "the replay changed its input"
    # the other order leaves the overlap with the other material
    out, _, _ = rg.fill(g, [[1, 1, 1], [0, 0, 0]], [3, 3, 3], [7, 6])
    assert out[1, 1, 1] == 6 and out[3, 3, 3] == 7
    # WHERE_EMPTY tests the voxel as the operations before left it: the second box only gets what the first left empty
    out, _, changed = rg.fill(g, [[0, 0, 0], [1, 1, 1]], [3, 3, 3], [6, 7], rg.WHERE_EMPTY)
    assert out[1, 1, 1] == 6 and out[3, 3, 3] == 7 and changed == 27 + 19
    # WHERE_SOLID: nothing to paint in an empty grid; then a clear followed by a paint finds nothing left
    out, _, changed = rg.fill(g, [[0, 0, 0]], [4, 4, 4], [6], rg.WHERE_SOLID)
    assert changed == 0 and not out.any()
    full = np.full((4, 4, 4), 5, np.int8)
    out, _, changed = rg.fill(full, [[0, 0, 0], [0, 0, 0]], [[2, 4, 4], [4, 4, 4]], [0, 7], rg.WHERE_SOLID)
    assert (out[:, :, :2] == 0).all() and (out[:, :, 2:] == 7).all() and changed == 64
    # a fill that restores what was there changes nothing
    out, _, changed = rg.fill(full, [[0, 0, 0], [0, 0, 0]], [4, 4, 4], [0, 5])
    assert changed == 0 and np.array_equal(out, full)


def test_fill_clips_in_64_bits_and_counts_skipped():
    g = np.zeros((2, 3, 4), np.int8)                          # dz, dy, dx = 2, 3, 4
    lo = [[-1, -1, -1], [3, 2, 1], [4, 0, 0], [0, -5, 0], [rg.INT32_MIN] * 3, [rg.INT32_MIN + 2] * 3, [2, 1, 0]]
    size = [[2, 2, 2], [9, 9, 9], [1, 1, 1], [4, 5, 2], [rg.INT32_MAX] * 3, [rg.INT32_MAX] * 3, [rg.INT32_MAX, 1, 1]]
    out, skipped, changed = rg.fill(g, lo, size, [6, 7, 5, 5, 5, -128, 127])
    assert skipped == 3                                        # the face-touching box, the one that ends at -1, INT32_MIN + INT32_MAX = -1
    assert out[0, 0, 0] == -128 and out[1, 2, 3] == 7 and out[0, 1, 2] == 127 and out[0, 1, 3] == 127 and changed == 4
    with pytest.raises(AssertionError):
        rg.fill(g, [[0, 0, 0]], [[1, 0, 1]], [5])
    with pytest.raises(AssertionError):
        rg.fill(g, [[0, 0, 0]], [[1, 1, 1]], [128])


def test_paste_is_the_inverse_of_a_region_read_and_honours_the_flags():
    rng = np.random.default_rng(3)
    g = rng.choice(np.array([0, 5, 6, -3], np.int8), size=(6, 5, 7))
    block = rng.choice(np.array([0, 7, -128], np.int8), size=(1, 3, 4, 5))        # sz, sy, sx = 3, 4, 5
    lo = [[4, -2, 5]]                                          # leaves the grid on x (7), y (-2, -1) and z (6, 7)
    out, skipped, changed = rg.paste(g, lo, block)
    assert skipped == 0 and np.array_equal(out[5:6, 0:2, 4:7], block[0, 0:1, 2:4, 0:3])
    mask = np.ones(g.shape, bool)
    mask[5:6, 0:2, 4:7] = False
    assert np.array_equal(out[mask], g[mask]) and changed == np.count_nonzero(out != g)
    for flags in (rg.SKIP_ZERO, rg.WHERE_EMPTY, rg.WHERE_SOLID, rg.SKIP_ZERO | rg.WHERE_EMPTY, rg.SKIP_ZERO | rg.WHERE_SOLID):
        out, _, _ = rg.paste(g, lo, block, flags)
        src, old, new = block[0, 0:1, 2:4, 0:3], g[5:6, 0:2, 4:7], out[5:6, 0:2, 4:7]
        ok = np.ones(src.shape, bool)
        if flags & rg.SKIP_ZERO:
            ok &= src != 0
        if flags & rg.WHERE_EMPTY:
            ok &= old == 0
        if flags & rg.WHERE_SOLID:
            ok &= old != 0
        assert np.array_equal(new, np.where(ok, src, old)), flags
    # two overlapping blocks: the later one wins, and WHERE_EMPTY sees what the first one wrote
    z = np.zeros((4, 4, 4), np.int8)
    a, b = np.full((2, 2, 2), 6, np.int8), np.full((2, 2, 2), 7, np.int8)
    out, _, _ = rg.paste(z, [[0, 0, 0], [1, 1, 1]], np.stack([a, b]))
    assert out[1, 1, 1] == 7 and out[0, 0, 0] == 6
    out, _, _ = rg.paste(z, [[0, 0, 0], [1, 1, 1]], np.stack([a, b]), rg.WHERE_EMPTY)
    assert out[1, 1, 1] == 6 and out[2, 2, 2] == 7
    out, skipped, changed = rg.paste(z, [[4, 0, 0], [0, rg.INT32_MIN, 0], [rg.INT32_MAX, 0, 0]], np.stack([a, b, a]))
    assert skipped == 3 and changed == 0
    with pytest.raises(AssertionError):
        rg.paste(z, [[0, 0, 0]], a[None], rg.WHERE_EMPTY | rg.WHERE_SOLID)


@pytest.mark.parametrize("dim", [2, 4, 8, 16])
def test_fill_replay_equals_the_voxel_replay_of_the_expanded_batch(dim):
    rng = np.random.default_rng(10 + dim)
    g = rng.choice(np.array([0, 5, 6], np.int8), size=(dim, dim, dim))
    lo, size, m = rg.random_fills(rng, dim)
    out, skipped, changed = rg.fill(g, lo, size, m)
    p, pm = rg.expand_fill(lo, size, m, (dim,) * 3)
    want, pskipped, pchanged = er.replay(g, p, pm)
    assert np.array_equal(out, want) and pskipped == 0 and pchanged == changed
    assert skipped >= 3 and skipped == sum(1 for l, s in zip(lo, size) if rg._clip(l, s, (dim,) * 3) is None)
    # the bricks of the batch are the bricks of its voxels
    corners = rg.brick_corners(lo, size, (dim,) * 3)
    assert len(corners) == er.touched_nodes(p, dim)[0] and er.touched_nodes(corners, dim) == er.touched_nodes(p, dim)
    blo, data = rg.random_pastes(rng, dim)
    out, skipped, changed = rg.paste(g, blo, data)
    p, pm = rg.expand_paste(blo, data, (dim,) * 3)
    want, _, pchanged = er.replay(g, p, pm)
    assert np.array_equal(out, want) and pchanged == changed and skipped >= 3


def test_random_batches_hold_what_the_tests_rely_on():
    dim = 16
    lo, size, m = rg.random_fills(np.random.default_rng(1), dim)
    assert lo.dtype == size.dtype == m.dtype == np.int32 and lo.shape == size.shape == (40, 3)
    assert (lo[6] == rg.INT32_MIN).all() and (size[6] == rg.INT32_MAX).all()
    assert (lo < 0).any() and (m == 0).any() and (m < 0).any() and (size >= 1).all()
    outside = [rg._clip(l, s, (dim,) * 3) is None for l, s in zip(lo, size)]
    partly = [c is not None and (np.asarray(l) < 0).any() or (np.asarray(l, np.int64) + s > dim).any() for l, s, c in
              zip(lo, size, (rg._clip(l, s, (dim,) * 3) for l, s in zip(lo, size)))]
    assert sum(outside) >= 3 and sum(partly) >= 3
    # overlaps where the order decides: the batch in reverse gives another grid
    g = np.zeros((dim, dim, dim), np.int8)
    assert not np.array_equal(rg.fill(g, lo, size, m)[0], rg.fill(g, lo[::-1], size[::-1], m[::-1])[0])
    blo, data = rg.random_pastes(np.random.default_rng(2), dim)
    assert data.dtype == np.int8 and data.shape[1:] == (7, 5, 9) and 0.3 < np.mean(data == 0) < 0.7
    assert not np.array_equal(rg.paste(g, blo, data)[0], rg.paste(g, blo[::-1], data[::-1])[0])


def test_header_declares_the_entry_points_and_the_flags():
    text = open(os.path.join(ROOT, "include", "vrc.h")).read()
    for proto in ("int vrc_fill_boxes(vrc_caster *h, const int32_t *boxes, const int32_t *materials, int64_t n, uint32_t flags, vrc_edit_info *info);",
                  "int vrc_fill_boxes_device(vrc_caster *h, const void *d_boxes, const void *d_materials, int64_t n, uint32_t flags, vrc_edit_info *info);",
                  "int vrc_write_regions(vrc_caster *h, const int32_t *lo, int64_t n, const int32_t size[3], const int8_t *data, size_t n_bytes, uint32_t flags, vrc_edit_info *info);",
                  "int vrc_write_regions_device(vrc_caster *h, const void *d_lo, int64_t n, const int32_t size[3], const void *d_data, size_t n_bytes, uint32_t flags, vrc_edit_info *info);"):
        assert proto in text, proto
    for name, value in (("VRC_WRITE_WHERE_EMPTY", 1), ("VRC_WRITE_WHERE_SOLID", 2), ("VRC_WRITE_SKIP_ZERO", 4)):
        assert re.search(r"#define " + name + r"\s+" + str(value) + r"u\b", text), name
    assert (vrc.WRITE_WHERE_EMPTY, vrc.WRITE_WHERE_SOLID, vrc.WRITE_SKIP_ZERO) == (rg.WHERE_EMPTY, rg.WHERE_SOLID, rg.SKIP_ZERO) == (1, 2, 4)
    # the section sits between the voxel edits and the compaction
    assert text.index("---- voxel edits") < text.index("---- region edits") < text.index("---- octree compaction")


def test_libraries_export_the_symbols_and_python_binds_them():
    for lib in ("libvrc.so", "libvrc_audit.so"):
        syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], capture_output=True, text=True, check=True).stdout
        for name in CALLS:
            assert re.search(r"\bT " + name + r"$", syms, re.M), (lib, name)
    for name in CALLS:
        assert name in vrc.SIGNATURES and hasattr(vrc.CLCaster, name[4:])
    assert vrc.SIGNATURES["vrc_write_regions"][1][1:6] == vrc.SIGNATURES["vrc_read_regions"][1][1:6], "the paste takes the read's arguments"


def test_null_handle_is_an_invalid_argument():
    lib = vrc.lib
    boxes, m = np.array([0, 0, 0, 1, 1, 1], np.int32), np.array([5], np.int32)
    size, data = np.array([1, 1, 1], np.int32), np.array([5], np.int8)
    i32p = C.POINTER(C.c_int32)
    bp, mp, sp, dp = boxes.ctypes.data_as(i32p), m.ctypes.data_as(i32p), size.ctypes.data_as(i32p), data.ctypes.data_as(C.POINTER(C.c_int8))
    assert lib.vrc_fill_boxes(None, bp, mp, 1, 0, None) == 1
    assert lib.vrc_fill_boxes_device(None, C.c_void_p(boxes.ctypes.data), C.c_void_p(m.ctypes.data), 1, 0, None) == 1
    assert lib.vrc_write_regions(None, bp, 1, sp, dp, 1, 0, None) == 1
    assert lib.vrc_write_regions_device(None, C.c_void_p(boxes.ctypes.data), 1, sp, C.c_void_p(data.ctypes.data), 1, 0, None) == 1
    assert vrc.STATUS[1] == "VRC_ERR_INVALID_ARGUMENT"


def test_brick_kernel_has_no_scratch_and_the_pinned_counts_hold():
    if not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    table = kr.kernel_table()
    names = [n for n in table if "region_write_brick_kernel" in n]
    assert len(names) == 1, names
    k = table[names[0]]
    assert k["private_segment_fixed_size"] == 0
    assert k["vgpr_count"] <= 64
    # the five kernels of the region edits, none of which counts as a kernel of the voxel edits or of the compaction
    mine = sorted(n for n in table if "region_write_" in n)
    assert len(mine) == 5 and all(table[n]["private_segment_fixed_size"] == 0 for n in mine), mine
    assert not any("voxel_edit_" in n or "octree_compact_" in n for n in mine)
    assert sum(1 for n in table if "voxel_edit_" in n) == 4
    assert sum(1 for n in table if "voxel_edit_brick_kernel" in n) == 1
