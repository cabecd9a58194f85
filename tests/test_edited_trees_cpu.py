"""CPU suite: the inputs of tests/test_edited_trees_gpu.py can fail.  That file renders the arrays the scene edits and the
compaction leave behind and checks the frames, the coarse table and the empty boxes against the oracle, the host builder's tree of
the replayed grid and the exhaustive host box check (tests/box_check.py).  Here, without a GPU and with every comparison exact:

* THE CAMERAS SEE WHAT THE STEPS WROTE.  For every history that does not end empty, from either camera, the oracle's frame of the
  host-built tree of the final grid differs from that of the starting grid, in image and in hit records; every generation of loop32
  differs from the one before.  A frame rendered from the old root, or with a stale table or stale boxes, cannot pass unnoticed.
* THE HOST BOX CHECK CAN FAIL.  It passes on all-zero words (every box its own node) and on a box widened over empty space; it
  fails when one word widens an empty node by one code step over an adjacent solid voxel, and at the codes where the map's edge
  clips the extent.
* THE ORACLE TAKES THE DEGENERATE ARRAYS: a root with valid mask 0 at the end of an array of garbage, whose near pointer of 1
  points past the end, and the one-word array of a compacted empty scene -- one background colour, one descriptor read per ray."""
import numpy as np
import pytest

import box_check
import edited_tree_cases as etc
import relayout as rl
import treetools

NOT_EMPTY = [n for n in etc.NAMES if n not in etc.EMPTIED and n not in ("compacted64-far", "loop32-reserve0")]


def _differ(a, b):
    return not np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and not np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------- 1. the histories
@pytest.mark.parametrize("name", etc.NAMES)
def test_histories_are_what_they_say(name):
    h = etc.history(name)
    assert h.dim in (32, 64) and set(np.unique(h.start)) <= set(etc.MATERIALS.tolist()) and set(np.unique(h.final)) <= set(etc.MATERIALS.tolist())
    assert h.start[:2].all(), "no floor"
    for (kind, _), (g, skipped, changed) in zip(h.steps, h.after):
        assert (changed > 0) == (kind not in ("compact", "frame")), (name, kind, "a step changes nothing")
    assert h.empty == (name in etc.EMPTIED) == (not h.final.any())
    assert len(h.steps) - len(h.frames()) <= 14, "a dozen small batches at the most, and the compactions"
    for _, _, (x, y, z) in h.cameras:
        for g in [h.final] + [h.after[k][0] for k in h.frames()]:
            assert g[int(z), int(y), int(x)] == 0
    if name in etc.LOOPS:
        kinds = [kind for kind, _ in h.steps]
        assert len(h.frames()) == 12 and kinds.count("compact") == 2
        assert [k for k in kinds if k not in ("frame", "compact")] == ["set_voxels", "fill_boxes", "fill_shapes", "write_regions"] * 3
        assert [kinds[:i].count("frame") for i, k in enumerate(kinds) if k == "compact"] == [4, 9]
    if name == "shapes64":
        shapes = np.concatenate([a["shapes"] for _, a in h.steps])
        assert set(shapes[:, 0]) == {0, 1, 2, 3} and (shapes[:, 3] + shapes[:, 5] > h.dim).any(), "every kind, one clipped by the map's edge"
    if name == "leaves32":
        p = h.steps[0][1]["positions"]
        inside = [[bool(x <= v[0] < x + s and y <= v[1] < y + s and z <= v[2] < z + s) for v in p] for x, y, z, s in etc.LEAF_CUBES]
        assert (np.array(inside).sum(axis=1) == 1).all() and (np.array(inside).sum(axis=0) == 1).all(), "one voxel out of every leaf"
        assert rl.decode(*h.tree, h.dim).tolist() == np.where(h.start != 0, 5, 0).reshape(-1).tolist()
        masks = {(v >> 16 & 0xff, v >> 24 & 0xff) for v in (int(w) for w in h.tree[0])}
        assert any(valid & leaf and leaf != 0xff for valid, leaf in masks), "no solid leaf above the bottom level"


@pytest.mark.parametrize("name", NOT_EMPTY)
def test_the_cameras_see_what_the_steps_wrote(name):
    h = etc.history(name)
    for camera in h.cameras:
        before, after = etc.oracle_on_grid(h, camera, h.start), etc.oracle_on_grid(h, camera, h.final)
        assert _differ(before, after), (name, camera[0])
        assert (after[1][..., 0] >= 0).any(), (name, camera[0], "no ray hits anything")
        if name in etc.LOOPS:
            prev = before
            for gen, k in enumerate(h.frames()):
                cur = etc.oracle_on_grid(h, camera, h.after[k][0])
                assert _differ(prev, cur), (name, camera[0], gen)
                prev = cur


def test_both_stepping_modes_and_three_lights_see_it_too():
    """(the GPU file renders every history in mode B and once with three lights: those frames change with the steps as well)"""
    for name in NOT_EMPTY:
        h = etc.history(name)
        for kw in (dict(mode=1), dict(light_count=3)):
            assert any(_differ(etc.oracle_on_grid(h, cam, h.start, **kw), etc.oracle_on_grid(h, cam, h.final, **kw)) for cam in h.cameras), (name, kw)
        one, three = (etc.oracle_on_grid(h, h.cameras[0], h.final, light_count=n) for n in (1, 3))
        assert three[2]["shadow_rays"] > one[2]["shadow_rays"], name


# ---------------------------------------------------------------------------- 2. the host box check
def _host_case(name="regions32"):
    h = etc.history(name)
    o = etc.host_tree(h.final)
    return h, o, h.final != 0, np.zeros((o.descriptor_buffer.size, 8), np.uint32)


def _neighbour_slab(x, y, z, size, j, dim):
    """the cube-sized slab next to the node in direction j (-x -y -z +x +y +z), clipped: (x0, y0, z0, x1, y1, z1)"""
    lo, hi = [x, y, z], [x + size, y + size, z + size]
    a = j % 3
    if j < 3:
        lo[a], hi[a] = max(lo[a] - size, 0), lo[a]
    else:
        lo[a], hi[a] = hi[a], min(hi[a] + size, dim)
    return (*lo, *hi)


def test_box_check_passes_on_boxes_that_are_their_own_nodes():
    for name in ("regions32", "points64", "emptied32"):
        h, o, solid, words = _host_case(name)
        n_boxes, grown, volume, node_volume = box_check.check_boxes(o.descriptor_buffer, o.root_index, h.dim, words, solid, must_grow=False)
        assert n_boxes == len(list(treetools.empty_children(o.descriptor_buffer, o.root_index, h.dim))) >= 8
        assert grown == 0 and volume == node_volume == int((~solid).sum()), "the empty child slots tile the empty space"
        with pytest.raises(AssertionError, match="wider than their node"):
            box_check.check_boxes(o.descriptor_buffer, o.root_index, h.dim, words, solid)


def test_box_check_fails_on_one_box_widened_over_a_solid_voxel():
    h, o, solid, words = _host_case()
    dim = h.dim
    S = box_check.summed_volume(solid)
    seen = set()
    for index, k, (x, y, z), size in treetools.empty_children(o.descriptor_buffer, o.root_index, dim):
        for j in range(6):
            slab = _neighbour_slab(x, y, z, size, j, dim)
            if slab[j % 3] == slab[3 + j % 3]:
                continue                                        # (the node touches the map's edge on this side)
            hit = int(box_check.solids(S, *slab)) > 0
            if (size, j, hit) in seen:
                continue
            seen.add((size, j, hit))
            w = words.copy()
            w[index, k] = 1 << (5 * j)                          # one code step: the extent of one cube
            if hit:
                with pytest.raises(AssertionError, match=f"descriptor {index} slot {k}: the box .* holds a solid voxel"):
                    box_check.check_boxes(o.descriptor_buffer, o.root_index, dim, w, solid, must_grow=False)
            else:
                assert box_check.check_boxes(o.descriptor_buffer, o.root_index, dim, w, solid, must_grow=False)[1] == 1
    # every direction, on bottom-level voxels and on larger nodes, with and without a solid voxel in the slab
    assert {(1, j, hit) for j in range(6) for hit in (False, True)} <= seen and any(size > 1 and hit for size, _, hit in seen), sorted(seen)


def test_box_check_fails_where_the_maps_edge_clips_the_extent():
    h, o, solid, words = _host_case()
    dim = h.dim
    S = box_check.summed_volume(solid)
    tried = set()
    for index, k, (x, y, z), size in treetools.empty_children(o.descriptor_buffer, o.root_index, dim):
        for j in range(6):
            if j in tried:
                continue
            slab = _neighbour_slab(x, y, z, size, j, dim)
            if slab[j % 3] == slab[3 + j % 3] or not int(box_check.solids(S, *slab)):
                continue
            tried.add(j)
            room = ((x, y, z)[j] if j < 3 else dim - (x, y, z)[j - 3] - size) // size          # cubes between the node and the edge
            first = min(c for c in range(32) if treetools.box_decode(c) > room)
            assert treetools.box_decode(first - 1) <= room
            for code in (first, 31):                            # the first code the edge clips, and the largest (448 cubes)
                w = words.copy()
                w[index, k] = code << (5 * j)
                with pytest.raises(AssertionError, match=f"descriptor {index} slot {k}: the box .* holds a solid voxel") as e:
                    box_check.check_boxes(o.descriptor_buffer, o.root_index, dim, w, solid, must_grow=False)
                lo, hi = (tuple(int(v) for v in t.strip("()").split(",")) for t in str(e.value).split("the box ")[1].split(" of the ")[0].split(".."))
                assert (lo[j] == 0) if j < 3 else (hi[j - 3] == dim), (j, code, str(e.value))
    assert tried == set(range(6))
    # ... and a box clipped on all six sides in an empty map is the map
    e = etc.history("emptied32")
    o = etc.host_tree(e.final)
    full = np.full((1, 8), sum(31 << (5 * j) for j in range(6)), np.uint32)
    slots, lo, hi, _ = box_check.boxes_of(o.descriptor_buffer, o.root_index, 32, full)
    assert len(slots) == 8 and (lo == 0).all() and (hi == 32).all()
    assert box_check.check_boxes(o.descriptor_buffer, o.root_index, 32, full, e.final != 0) == (8, 8, 8 * 32 ** 3, 32 ** 3)


# ---------------------------------------------------------------------------- 3. the oracle on degenerate arrays
@pytest.mark.parametrize("name", ["emptied32", "emptied64"])
def test_the_oracle_renders_an_empty_root_and_a_one_word_array(name):
    h = etc.history(name)
    old = etc.host_tree(h.start)
    # what an edit leaves: the old tree as garbage, the new root last (valid mask 0, a near pointer of 1: past the end)
    edited = np.concatenate([old.descriptor_buffer, np.array([0xff000001], np.uint64)])
    lookup = np.concatenate([old.attachment_lookup, np.zeros(1, np.uint32)])
    one_word = np.array([0xff000000], np.uint64)
    want = None
    for desc, root, lk, at in ((edited, len(edited) - 1, lookup, old.attachment_buffer), (one_word, 0, np.zeros(1, np.uint32), old.attachment_buffer[:1]),
                               (one_word, 0, None, None)):
        assert not rl.decode(desc, root, h.dim).any()
        assert list(treetools.empty_children(desc, root, h.dim)) == [(root, k, (h.dim // 2 * (k & 1), h.dim // 2 * (k >> 1 & 1), h.dim // 2 * (k >> 2)), h.dim // 2) for k in range(8)]
        for camera in h.cameras:
            for mode, coarse in ((0, -1), (1, -1), (1, 0), (1, 2)):
                img, hits, ctr = etc.oracle_frame(h, camera, desc, root, lk, at, mode=mode, coarse=coarse)
                rays = ctr["primary_rays"]
                assert len(np.unique(img.reshape(-1, 4)[hits.reshape(-1, 8)[:, 6] > 0], axis=0)) == 1, "an empty scene renders one background colour"
                assert rays == etc.W * etc.H - ctr["unwritten"] and ctr["shadow_rays"] == ctr["n_tex"] == 0 and (hits[..., :3] == -1).all()
                if mode == 0:
                    assert ctr["n_desc"] == rays, "one descriptor read per ray: the root"
                key = (camera[0], mode, coarse)
                want = want or {}
                if key in want:
                    assert np.array_equal(want[key][0].view(np.uint32), img.view(np.uint32)) and np.array_equal(want[key][1], hits) and want[key][2] == ctr
                want[key] = (img, hits, ctr)
