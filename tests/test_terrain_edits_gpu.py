"""GPU suite (-m gpu): the write side of the resident scene -- vrc_set_voxels, vrc_fill_boxes, vrc_write_regions,
vrc_compact_octree -- and vrc_extract_faces on the device-built shell terrains of depth 10, 12 and 14: trees of millions of
descriptors that exist only in HBM, in the device builder's own layout with its far pointers, where a brick coordinate has 7, 9
and 11 bits, the sort key 22, 28 and 34, and the ancestor pass runs 7, 9 and 11 levels.  The other suites of these calls stop at
dims 2 to 64 (faces: depth 8), where a brick coordinate has 3 bits.

Every comparison is exact.  Everything expected comes from tests/terrain_edit_cases.py, which computes it without a GPU from the
procedural columns and the numpy replays (tests/test_terrain_edits_cpu.py asserts that its cases can fail): a few windows of
48 x 48 x 64 voxels are read back after every call and must equal the replayed windows, the positions of the batch must read the
replay's materials, the four counts and the array's size are the whole scene's, and a control set away from the windows still
equals the columns.  vrc_counters_canonical is not compared between a pristine and an edited-then-restored tree: it was not
established from the code that the device builder and the edit emit the same masks for the same bricks (a uniform block can be a
leaf of its parent or a subtree of its own), and the counter depends on the masks, not on the scene.

The file's name puts it behind tests/test_soak_slices_gpu.py in the suite's order on purpose ("Left out": that file's
group slice has shown an illegal memory access whose cause is not found, in processes that ran a new test file ahead of it), and
for the same reason it creates no group handle: single handles on device 0 only.

The whole-map fill that runs to completion runs at depth 10, not 12: every touched brick appends 72 words whatever the fill
changes (csrc/vrc_scene_edit.cpp, edit_append), which at depth 12 is 512^3 x 72 words = 77 GB of descriptors for one test."""
import gc

import numpy as np
import pytest

import region_replay as rg
import terrain_edit_cases as tc
import voxel_raycaster_amd as vrc
from gpu_helpers import _frame
from test_box_queries_gpu import _caster

pytestmark = pytest.mark.gpu
I, F = np.int32, np.float32
LIMIT = 6
WHERE = {0: None, rg.WHERE_EMPTY: "empty", rg.WHERE_SOLID: "solid"}
COUNTS = ("skipped", "voxels_changed", "bricks_touched", "descriptors_added")
SAME = ("voxels_changed", "bricks_touched", "descriptors_added", "n_descriptors", "root_index")
FLAG_PAIRS = [(False, False), (True, False), (False, True), (True, True)]         # (no_map_edge, stopping_only)


def _terrain(atlas, depth, frames=False, camera=None):
    """a single handle on device 0 with the shell terrain of `depth` built on the device; the empty boxes only for frames, which
    are rendered without the reference's octree bias (it moves a ray's start by voxels: the camera is aimed at a 10 x 9 pillar)"""
    import bench
    sc = bench.device_scene_header(depth)
    s = dict(dim=sc["dim"], cam_dir=sc["cam_dir"], cam_pos=sc["cam_pos"], lights=sc["lights"])
    if camera is not None:
        s["cam_dir"], s["cam_pos"] = camera
    return _caster(s, atlas, settings=(("octree_bias", 0),) if frames else (("empty_boxes", 0),), device_tree=depth)


def _send(c, b):
    kind, args, flags = b
    if kind == "set_voxels":
        return c.set_voxels(*args)
    if kind == "fill_boxes":
        return c.fill_boxes(*args, where=WHERE[flags])
    return c.write_regions(*args, skip_zero=bool(flags & rg.SKIP_ZERO), where=WHERE[flags & 3])


def _check_windows(c, depth, grids, tag):
    got = c.read_regions(tc.window_lo(depth), tuple(int(v) for v in tc.WINDOW))
    for w, g, want in zip(tc.windows(depth), got, grids):
        assert np.array_equal(g, want), (tag, w.name, len(np.argwhere(g != want)), np.argwhere(g != want)[:4, ::-1] + w.lo)


def _check_control(c, depth, tag):
    lo, blocks, pts, want = tc.control(depth)
    got = c.read_regions(lo, tc.CONTROL)
    bad = np.nonzero((got != blocks).any(axis=(1, 2, 3)))[0]
    assert bad.size == 0, (tag, "control regions", lo[bad[:4]])
    assert np.array_equal(c.get_voxels(pts), want), (tag, "control points")


def _step(c, depth, e, tag):
    """one batch of an expected sequence: the call, its counts, the array's size, the windows and the batch's own positions"""
    n0, _ = c.octree_size()
    b = tc.batch(depth, e.name)
    info = _send(c, b)
    print(tag, e.name, info)
    assert {k: info[k] for k in COUNTS} == e.counts, (tag, e.name, info, e.counts)
    assert (info["n_descriptors"], info["root_index"]) == c.octree_size(), (tag, e.name)
    assert info["n_descriptors"] == n0 + e.counts["descriptors_added"], (tag, e.name, n0, info)
    _check_windows(c, depth, e.grids, (tag, e.name))
    p = tc.points_of(depth, b)
    got, want = c.get_voxels(p), tc.read_points(depth, e.grids, p)
    assert np.array_equal(got, want), (tag, e.name, p[got != want][:4])
    return info


def _sequence(atlas, depth, names, tag):
    c = _terrain(atlas, depth)
    _check_windows(c, depth, [w.before for w in tc.windows(depth)], (tag, "pristine"))
    for e in tc.expected(depth, names):
        _step(c, depth, e, tag)
    _check_control(c, depth, tag)
    del c
    gc.collect()


# ---------------------------------------------------------------------------- 1. each kind of edit against the replay
@pytest.mark.parametrize("depth", tc.DEPTHS)
def test_set_voxels_equal_the_replay_and_bring_the_materials(atlas, depth):
    first, again, mixed, mixed2 = tc.expected(depth, ("set05", "set05", "setmix", "setmix2"))
    tag = f"set{depth}"
    c = _terrain(atlas, depth)
    _check_windows(c, depth, [w.before for w in tc.windows(depth)], (tag, "pristine"))
    _step(c, depth, first, tag)
    if depth <= 12:                                            # 0 and 5 alone leave a tree without materials without them
        assert c.read_attachments() == (None, None)
    _check_control(c, depth, tag)
    # the same batch again changes nothing and adds nothing
    size = c.octree_size()
    info = _step(c, depth, again, tag)
    assert info["voxels_changed"] == 0 and info["descriptors_added"] == 0 and c.octree_size() == size
    # the first material other than 0 and 5 creates the lookup: the windows read the replay's materials, all else still 5
    _step(c, depth, mixed, tag)
    if depth <= 12:
        lookup, attach = c.read_attachments()
        assert lookup is not None and len(lookup) == c.octree_size()[0] and len(attach) > 1
    _check_control(c, depth, tag)
    # ... and the next mixed batch lands on the lookup that exists now
    _step(c, depth, mixed2, tag)
    _check_control(c, depth, tag)
    del c
    gc.collect()


@pytest.mark.parametrize("depth", tc.DEPTHS)
def test_fill_boxes_equal_the_replay_in_every_where_mode(atlas, depth):
    _sequence(atlas, depth, ("fill_solid", "fill_empty", "fill"), f"fill{depth}")


@pytest.mark.parametrize("depth", tc.DEPTHS)
def test_write_regions_equal_the_replay(atlas, depth):
    _sequence(atlas, depth, ("paste_skip0", "paste"), f"paste{depth}")


# ---------------------------------------------------------------------------- 2. two routes, one array
def _twins(atlas, depth, names, tag, check=True):
    """a: the named batches as they are; b: vrc_set_voxels of the expanded batches.  Returns (a, b, the array's size before)."""
    a, b = _terrain(atlas, depth), _terrain(atlas, depth)
    n_before = a.octree_size()
    assert n_before == b.octree_size()
    for e in tc.expected(depth, names):
        ia = _step(a, depth, e, tag) if check else _send(a, tc.batch(depth, e.name))
        kind, args, flags = tc.batch(depth, e.name)
        assert flags == 0
        p, m = args if kind == "set_voxels" else tc.expanded(depth, e.name)
        ib = b.set_voxels(p, m)
        for k in SAME:
            assert ia[k] == ib[k], (tag, e.name, k, ia, ib)
        assert a.octree_size() == b.octree_size()
    return a, b, n_before[0]


@pytest.mark.parametrize("depth", tc.DEPTHS)
def test_region_edits_and_set_voxels_of_the_expanded_batch_append_the_same_words(atlas, depth):
    tag = f"twins{depth}"
    a, b, n_before = _twins(atlas, depth, ("fill", "paste"), tag)
    _check_windows(b, depth, tc.expected(depth, ("fill", "paste"))[1].grids, (tag, "expanded"))
    da, db = a.read_descriptors(first=n_before), b.read_descriptors(first=n_before)
    assert len(da) > 0 and np.array_equal(da, db), (tag, np.nonzero(da != db)[0][:8])
    if depth == 10:
        assert np.array_equal(a.read_descriptors(), b.read_descriptors())
        (la, aa), (lb, ab) = a.read_attachments(), b.read_attachments()
        assert la is not None and np.array_equal(la, lb) and np.array_equal(aa, ab)
    del a, b
    gc.collect()


# ---------------------------------------------------------------------------- 3. undo and frames
def test_undo_restores_the_frame_of_the_pristine_tree(atlas):
    depth = 12
    camera = tc.pillar_camera(depth)
    fill, undo = tc.expected(depth, ("fill", "undo"))
    p = _terrain(atlas, depth, frames=True, camera=camera)
    assert p.prepare(), p.last_error()
    pimg, phits, _ = _frame(p)
    assert p.memory_usage2()["empty_boxes"] != 0 and p.memory_usage2()["coarse_bytes"] > 0, "the frame ran without the empty boxes"
    a = _terrain(atlas, depth, frames=True, camera=camera)
    _step(a, depth, fill, "undo")
    assert a.prepare(), a.last_error()
    mimg, mhits, _ = _frame(a)
    assert (mimg != pimg).any() and not np.array_equal(mhits, phits), "the camera does not see the pillar: equal after the undo would say nothing"
    _step(a, depth, undo, "undo")
    assert a.prepare(), a.last_error()
    img, hits, _ = _frame(a)
    assert a.last_kernel()["name"] == p.last_kernel()["name"] and a.memory_usage2()["empty_boxes"] != 0
    assert np.array_equal(img, pimg) and np.array_equal(hits, phits)
    _check_control(a, depth, "undo")
    del a, p
    gc.collect()


# ---------------------------------------------------------------------------- 4. compaction
def _counts(info):
    return {k: v for k, v in info.items() if k != "seconds"}


@pytest.mark.parametrize("depth", [10, 12])
def test_compaction_after_the_three_batches(atlas, depth):
    tag = f"compact{depth}"
    names = ("fill", "paste", "setmix", "set05")
    steps = tc.expected(depth, names)
    a, b, _ = _twins(atlas, depth, names[:3], tag, check=False)
    _check_windows(a, depth, steps[2].grids, (tag, "before"))
    size = a.octree_size()
    dry = a.compact_octree(dry_run=True)
    assert a.octree_size() == size, "a dry run moved the tree"
    ia, ib = a.compact_octree(), b.compact_octree()
    print(tag, ia)
    assert _counts(dry) == _counts(ia) == _counts(ib)
    assert ia["descriptors_before"] == size[0] and ia["n_descriptors"] < ia["descriptors_before"]
    assert ia["live_descriptors"] + ia["far_slots"] == ia["n_descriptors"] and ia["root_index"] == 0
    n = ia["n_descriptors"]
    assert a.octree_size() == b.octree_size() == (n, 0)
    if depth == 10:
        assert np.array_equal(a.read_descriptors(), b.read_descriptors())
        (la, aa), (lb, ab) = a.read_attachments(), b.read_attachments()
        assert np.array_equal(la, lb) and np.array_equal(aa, ab)
    else:
        k = min(1 << 20, n)
        for first in (0, (n - k) // 2, n - k):
            assert np.array_equal(a.read_descriptors(first, k), b.read_descriptors(first, k)), (tag, first)
    for c in (a, b):
        _check_windows(c, depth, steps[2].grids, (tag, "after"))
        _check_control(c, depth, tag)
    # a second call has nothing to drop
    head = a.read_descriptors(0, min(1 << 20, n))
    again = a.compact_octree()
    assert again["descriptors_before"] == n and a.octree_size() == (n, 0)
    for k in ("n_descriptors", "root_index", "live_descriptors", "far_slots", "n_attachments"):
        assert again[k] == ia[k], (tag, k, again, ia)
    assert np.array_equal(a.read_descriptors(0, min(1 << 20, n)), head)
    # the compacted tree takes the next batch
    _step(a, depth, steps[3], tag)
    _check_control(a, depth, tag)
    del a, b
    gc.collect()


# ---------------------------------------------------------------------------- 5. faces
def _same_faces(got, want, tag):
    assert np.array_equal(got[0], want[0]), (tag, "counts", got[0], want[0])
    assert got[1].shape == want[1].shape, (tag, got[1].shape, want[1].shape)
    rows = np.nonzero((got[1] != want[1]).any(axis=1))[0]
    assert rows.size == 0, (tag, "faces", rows[:4], got[1][rows[:4]], want[1][rows[:4]])


@pytest.mark.parametrize("depth", [10, 12])
def test_faces_of_the_pristine_and_the_edited_terrain(atlas, depth):
    c = _terrain(atlas, depth)
    total = 0
    for no_edge in (False, True):
        got = c.extract_faces(tc.chunks(depth), tc.CHUNK, no_map_edge=no_edge)
        _same_faces(got, tc.chunk_faces(depth, no_edge), (depth, "chunks", no_edge))
        total += len(got[1])
    assert total > 24 * 13 * 9
    steps = tc.expected(depth, ("fill", "paste"))
    for e in steps:
        _send(c, tc.batch(depth, e.name))
    _check_windows(c, depth, steps[1].grids, (depth, "faces"))
    for no_edge, stopping in FLAG_PAIRS:
        got = c.extract_faces(tc.core_lo(depth), tuple(int(v) for v in tc.CORE), no_map_edge=no_edge, stopping_only=stopping)
        want = tc.core_faces(depth, steps[1].grids, no_edge, stopping)
        _same_faces(got, want, (depth, "cores", no_edge, stopping))
        if not no_edge and not stopping:
            assert len(got[1]) > len(tc.windows(depth)) * 16 * 16
    del c
    gc.collect()


# ---------------------------------------------------------------------------- 6. the pair limit
def test_pair_limit_and_a_whole_map_fill(atlas):
    # 16 boxes that each cover the whole depth-12 map: 16 x 512^3 = 2^31 (brick, operation) pairs, one more than the limit.  The
    # count and the scan run, nothing else.
    depth = 12
    dim = 1 << depth
    c = _terrain(atlas, depth)
    size = c.octree_size()
    with pytest.raises(vrc.VrcError):
        c.fill_boxes(np.zeros((16, 3), I), (dim, dim, dim), 5)
    assert c.last_status == LIMIT and c.octree_size() == size
    _check_windows(c, depth, [w.before for w in tc.windows(depth)], "limit")
    del c
    gc.collect()
    # one whole-map fill that clears what is solid, at depth 10 (the docstring says why): 128^3 = 2 M pairs, every brick of the map
    depth = 10
    dim = 1 << depth
    c = _terrain(atlas, depth)
    rec, cnt, _ = c.box_intersection(np.array([[0, 0, 0, dim, dim, dim]], F))
    solid = int(cnt[0])
    assert solid > dim * dim
    n0 = c.octree_size()[0]
    info = c.fill_boxes(np.zeros((1, 3), I), (dim, dim, dim), 0, where="solid")
    print("whole-map", info)
    bricks = (dim // 8) ** 3
    above = sum((dim >> k) ** 3 for k in range(4, depth + 1))
    assert info["skipped"] == 0 and info["voxels_changed"] == solid and info["bricks_touched"] == bricks
    assert info["descriptors_added"] == 72 * bricks + 16 * above + 1 and info["n_descriptors"] == n0 + info["descriptors_added"]
    n, root = c.octree_size()
    assert (n, root) == (info["n_descriptors"], info["root_index"])
    assert (int(c.read_descriptors(first=root, count=1)[0]) >> 16) & 0xff == 0, "the root of an empty scene has valid mask 0"
    got = c.read_regions(tc.window_lo(depth), tuple(int(v) for v in tc.WINDOW))
    assert not got.any()
    lo, blocks, pts, want = tc.control(depth)
    assert not c.read_regions(lo, tc.CONTROL).any() and not c.get_voxels(pts).any()
    rec, cnt, _ = c.box_intersection(np.array([[0, 0, 0, dim, dim, dim]], F))
    assert cnt[0] == 0
    del c
    gc.collect()
