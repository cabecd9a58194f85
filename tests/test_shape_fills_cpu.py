"""CPU suite: the reference side of tests/test_voxel_shape_fills_gpu.py, and the closed form of the shape fills on the host.

1. csrc/shape_span.hpp compiles for the host: tests/shape_span_check.cpp, a stand-alone program built with g++ under
AddressSanitizer + UBSan, holds isqrt64 against its definition (the bare truncated double root is wrong thousands of times on the
inputs it takes), shape_row_span against per-voxel membership and shape_brick_row against the brute-force brick set.  Nothing
sanitized is loaded into Python.

2. The replay (tests/shape_replay.py) finds the touched bricks by brute force over the expanded voxels; a Python-integer
restatement of the closed form, written here, gives the same set on the shared batches.  The lattice ball of r = 32 has the
137 065 voxels DESIGN.md quotes.

3. Oracle soundness.  A batch in which nothing is skipped, no brick takes several operations or every touched brick is one the
bounding boxes give anyway would let the GPU tests pass for nothing, so those conditions on the INPUTS are asserted here, from the
replay alone: they are properties of the seeds, not tolerances."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import shape_replay as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = [(2,) * 3, (4,) * 3, (8,) * 3, (16,) * 3, (32,) * 3, (64,) * 3]
MAPS = [(16, 16, 16), (13, 5, 5), (24, 9, 9)]                  # the maps of the GPU tests, z cut at dy: the scene the edits see


def test_the_closed_form_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "shape_span_check")
    csrc = os.path.join(ROOT, "voxel-raycaster_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + csrc, os.path.join(ROOT, "tests", "shape_span_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"shape_span ok: roots (\d+), bare truncation wrong (\d+), shapes (\d+), rows (\d+), brick rows (\d+)", out.stdout)
    assert m, out.stdout + out.stderr
    roots, bare_wrong, shapes, rows, brick_rows = map(int, m.groups())
    assert roots >= (1 << 20) + 3 * (4097 + 4000) and bare_wrong > 0
    assert shapes > 12000 and rows == shapes * 12 * 17 and brick_rows > shapes * (2 * 3 + 3 * 5 + 6 * 9)


def _row_span(s, y, z):
    """shape_span.hpp's shape_row_span in Python integers: the x interval [a, b) of the shape on row (y, z), or None"""
    kind, cx, cy, cz, r, h = (int(v) for v in s)
    t = r * r
    for k, (v, c) in enumerate(((y, cy), (z, cz)), start=1):
        d = v - c
        if kind == 1 + k:
            if not 0 <= d < h:
                return None
        else:
            if abs(d) > r:
                return None
            t -= d * d
    if t < 0:
        return None
    if kind == sp.CYLINDER_X:
        return cx, cx + h
    w = math.isqrt(t)
    return cx - w, cx + w + 1


def _closed_form_bricks(shapes, dims, log2=3):
    """the touched bricks the way the kernels find them: per brick row, the span of the in-scene row nearest to the axis"""
    bricks = set()
    side = 1 << log2
    for s in np.asarray(shapes, dtype=np.int64).reshape(-1, 6):
        kind, c, h = int(s[0]), [int(v) for v in s[1:4]], int(s[5])
        for bz in range((dims[2] + side - 1) >> log2):
            for by in range((dims[1] + side - 1) >> log2):
                at = []
                for k, b in ((1, by), (2, bz)):
                    lo, hi = b << log2, min((b + 1) << log2, dims[k])
                    if kind == 1 + k:
                        lo, hi = max(lo, c[k]), min(hi, c[k] + h)
                    at.append(None if lo >= hi else min(max(c[k], lo), hi - 1))
                span = None if None in at else _row_span(s, at[0], at[1])
                if span is None:
                    continue
                a, b = max(span[0], 0), min(span[1], dims[0])
                for bx in range(a >> log2, ((b - 1) >> log2) + 1 if a < b else 0):
                    bricks.add((bx << log2, by << log2, bz << log2))
    return np.array(sorted(bricks), dtype=np.int64).reshape(-1, 3)


@pytest.mark.parametrize("dims", TREES + MAPS)
def test_brute_force_bricks_are_the_closed_form(dims):
    shapes, _ = sp.batch(dims)
    for log2 in (3, 2, 1) if dims == (32,) * 3 else (3,):
        assert np.array_equal(sp.brick_corners(shapes, dims, log2), _closed_form_bricks(shapes, dims, log2)), (dims, log2)
    assert len(sp.brick_corners(shapes, dims)) > 0


def test_the_ball_of_radius_32_has_design_mds_voxel_count():
    ball = np.array([[sp.BALL, 40, 40, 40, 32, 0]])
    p, m = sp.expand_shapes(ball, [0], (80,) * 3)
    assert len(p) == 137065 and len(np.unique(p, axis=0)) == len(p)
    g, skipped, changed = sp.fill_shapes(np.full((80,) * 3, 5, np.int8), ball, [0])
    assert (skipped, changed) == (0, 137065) and g[40, 40, 72] == 0 and g[40, 40, 73] == 5 and g[40, 41, 72] == 5
    # clipped: the half of it a scene holds, and the bricks of a ball against the bricks of its box
    assert len(sp.expand_shapes(np.array([[sp.BALL, 0, 40, 40, 32, 0]]), [0], (80,) * 3)[0]) == (137065 - 3209) // 2 + 3209
    assert len(sp.brick_corners(ball, (80,) * 3)) < 9 ** 3


def test_every_batch_holds_what_its_docstring_promises():
    for dims in TREES + MAPS:
        s, m = (a.astype(np.int64) for a in sp.batch(dims))
        assert set(s[:, 0]) == {0, 1, 2, 3} and {0, 1, 7, 8, 9} <= set(s[:, 4]) and (m == 0).any() and (m < 0).any(), dims
        assert all(sp.valid(a, b) for a, b in zip(s, m))
        assert ((s[:, 1:4] < 0).any(axis=1) & np.array([sp._voxels(a, dims) is not None for a in s])).any(), "no centre outside reaches in"
        assert [sp.BALL, -2 ** 30 + 3, 4, 4, 2 ** 30, 0] in s.tolist()
        kinds, c_a = s[:, 0], np.array([a[a[0]] if a[0] else 0 for a in s])
        assert ((kinds > 0) & (c_a == sp.INT32_MAX - 1) & (s[:, 5] == sp.INT32_MAX)).any()
        assert ((kinds > 0) & (c_a == sp.INT32_MIN) & (s[:, 5] == sp.INT32_MAX)).any()
        assert ((kinds == sp.CYLINDER_Z) & (s[:, 4] == 0)).any()
    # the cap of the giant ball: x = 3 holds the one voxel (3, 4, 4), and the planes below it are disks of radius isqrt(2^31 k - k^2)
    cap = np.array([[sp.BALL, -2 ** 30 + 3, 4, 4, 2 ** 30, 0]])
    g, _, _ = sp.fill_shapes(np.zeros((16,) * 3, np.int8), cap, [7])
    assert g[:, :, 3].sum() == 7 and g[4, 4, 3] == 7 and g[:, :, 4:].sum() == 0 and (g[:, :, :3] == 7).all()
    g, _, _ = sp.fill_shapes(np.zeros((64,) * 3, np.int8), np.array([[sp.BALL, -2 ** 30 + 1, 4, 4, 2 ** 30, 0]]), [7])
    assert g[4, 4, 1] == 7 and g[:, :, 1:].sum() == 7 and (g[:, :, 0] == 7).all()        # (at x = 0 the disk's radius is 46340)


@pytest.mark.parametrize("dims", TREES + MAPS)
def test_the_batches_can_tell_a_wrong_fill(dims):
    """the conditions the GPU tests rely on, for every batch they send (sp.batch(dims, k), k = 0 .. 2)"""
    for k in range(3):
        shapes, m = sp.batch(dims, k)
        grid = np.full(dims[::-1], 5, np.int8)
        grid[::2] = 0
        outs = [sp.fill_shapes(grid, shapes, m, flags) for flags in (0, sp.WHERE_EMPTY, sp.WHERE_SOLID)]
        assert all(skipped >= 1 and changed > 0 for _, skipped, changed in outs), (dims, k)
        assert outs[0][1] == sum(sp._voxels(s, dims) is None for s in shapes.astype(np.int64))
        assert not np.array_equal(outs[0][0], outs[1][0]) and not np.array_equal(outs[0][0], outs[2][0]) and not np.array_equal(outs[1][0], outs[2][0])
        # the order decides: the batch backwards ends somewhere else
        assert not np.array_equal(outs[0][0], sp.fill_shapes(grid, shapes[::-1], m[::-1])[0]), (dims, k)
        # a brick whose run holds at least three operations
        per_op = [set(map(tuple, sp.brick_corners(s[None], dims))) for s in shapes]
        runs = {}
        for bricks in per_op:
            for b in bricks:
                runs[b] = runs.get(b, 0) + 1
        assert max(runs.values()) >= 3, (dims, k)
        # a touched brick that a ball's bounding box holds and the ball does not: the count of a box-shaped front end would
        # differ.  (A scene of one brick per axis has no such brick: dims below 16 are excused, and only they.)
        if min(dims) >= 16:
            found = 0
            for s, bricks in zip(shapes.astype(np.int64), per_op):
                if s[0] != sp.BALL or not bricks:
                    continue
                lo = [max(int(s[1 + a] - s[4]), 0) >> 3 for a in range(3)]
                hi = [min(int(s[1 + a] + s[4]), dims[a] - 1) >> 3 for a in range(3)]
                box = {(8 * x, 8 * y, 8 * z) for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1)}
                assert bricks <= box
                found += len((box - bricks) & set(runs))
            assert found >= 1, (dims, k)
