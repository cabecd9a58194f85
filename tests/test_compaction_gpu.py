"""GPU suite (-m gpu): compaction of the resident octree (vrc_compact_octree, csrc/octree_compact.hip).

Every comparison is exact.  The oracle is the numpy replay (tests/compact_replay.py) of the array read back BEFORE the call: the
compacted descriptors, lookup and attachments equal it word for word at three reaches, with and without materials; the scene is
what it was (read-back, decoded grid, frames, hit records, counters, queries against a caster built fresh from the grid); the
layout is canonical (a tree and its re-laid copy compact to identical arrays) and idempotent; a dry run changes nothing and
reports what the real call reports; edits and compactions alternate; shallow trees and the empty scene; a tree that needs far
pointers at the default reach; the errors change nothing; both kinds of group; and the index-audit build."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import box_replay as br
import compact_replay as cr
import edit_replay as er
import ray_replay as rr
import relayout as rl
import sweep_replay as sr
import voxel_raycaster_amd as vrc
from compact_helpers import I, caster, compact_and_check, counts, grid_of, plain, state, whole
from gpu_helpers import _frame

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACHES = (cr.DEFAULT_REACH, 64, 16)


def _edited(atlas, dim, variant, reach=None, seed=0, settings=(), batches=3, n=600, **kw):
    """A caster whose tree took `batches` random batches: variant "attached" (built with materials), "plain" (built without; the
    batches bring them: every untouched descriptor names slot 0) or "plain05" (built without, and the batches write only 0 and 5: it
    stays without).  Returns (caster, grid after the batches)."""
    grid = grid_of(dim, 7 * dim + seed)
    attached = variant == "attached"
    if reach is not None:
        settings = tuple(settings) + (("compact_near_reach", reach),)
    c = caster(atlas, dim, grid, attachments=attached, settings=settings, **kw)
    cur = grid if attached else plain(grid)
    rng = np.random.default_rng(1000 + 7 * dim + seed)
    for _ in range(batches):
        p, m = er.random_batch(rng, dim, n=n)
        if variant == "plain05":
            m = np.where(m == 0, 0, 5).astype(I)
        cur, _, _ = er.replay(cur, p, m)
        c.set_voxels(p, m)
    return c, cur


# ---------------------------------------------------------------------------- 1. the replay, word for word
@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("variant", ["attached", "plain", "plain05"])
@pytest.mark.parametrize("dim", [8, 16, 32])
def test_compacted_arrays_equal_the_replay(atlas, dim, variant, reach):
    c, cur = _edited(atlas, dim, variant, reach)
    assert (c.read_attachments()[0] is None) == (variant == "plain05")
    info, _ = compact_and_check(c, dim, reach, cur, f"{variant}{dim}@{reach}")
    assert info["n_descriptors"] < info["descriptors_before"] and info["root_index"] == 0
    assert info["n_descriptors"] == info["live_descriptors"] + info["far_slots"]
    if reach == cr.DEFAULT_REACH:
        assert info["far_slots"] == 0
    if reach == 16 and dim >= 16:
        assert info["far_slots"] > 0
    if variant == "plain":
        assert info["n_attachments"] < info["attachments_before"], "the untouched descriptors share slot 0"
    # idempotence: the second call rewrites the same array
    before = state(c)
    again = c.compact_octree()
    for a, b in zip(before, state(c)):
        assert np.array_equal(a, b)
    assert again["descriptors_before"] == again["n_descriptors"] == info["n_descriptors"] and again["far_slots"] == info["far_slots"]
    assert again["attachments_before"] == again["n_attachments"] == info["n_attachments"]


# ---------------------------------------------------------------------------- 2. canonicity
def _canonical_cases():
    desc, root, grid = rl.leaf_tree()
    yield "leaf", vrc.Octree(desc, root, 32), 32, grid
    for dim in (8, 32):
        g = grid_of(dim, 300 + dim).reshape(-1)
        yield f"gen{dim}", vrc.Octree.Generate(g, dim).attach_materials_from_grid(g), dim, g


@pytest.mark.parametrize("reach", [cr.DEFAULT_REACH, 16])
def test_a_tree_and_its_relaid_copy_compact_to_identical_arrays(atlas, reach):
    for tag, o, dim, grid in _canonical_cases():
        lookup = getattr(o, "attachment_lookup", None)
        d2, r2, l2 = rl.relayout(o.descriptor_buffer, o.root_index, dim, np.random.default_rng(31), 0.5, lookup)
        o2 = vrc.Octree(d2, r2, dim)
        if lookup is not None:
            o2.attachment_lookup, o2.attachment_buffer = l2, o.attachment_buffer
        g3 = np.asarray(grid).reshape(dim, dim, dim)
        want = g3 if lookup is not None else plain(g3)
        results = []
        for tree in (o, o2):
            c = caster(atlas, dim, octree=tree, settings=(("compact_near_reach", reach),))
            compact_and_check(c, dim, reach, want, f"{tag}@{reach}")
            results.append(state(c))
        for a, b in zip(*results):
            assert np.array_equal(a, b), tag


# ---------------------------------------------------------------------------- 3. dry run
def test_dry_run_changes_nothing_and_reports_the_real_call(atlas):
    dim = 32
    for variant in ("attached", "plain05"):
        c, cur = _edited(atlas, dim, variant, seed=1)
        before, mem = state(c), c.memory_usage2()
        dry = c.compact_octree(dry_run=True)
        for a, b in zip(before, state(c)):
            assert np.array_equal(a, b)
        assert c.memory_usage2() == mem, "a dry run moved memory"
        real, _ = compact_and_check(c, dim, cr.DEFAULT_REACH, cur, f"dry-{variant}")
        assert counts(dry) == counts(real)
        assert dry["descriptors_before"] == len(before[0]) and real["n_descriptors"] == c.octree_size()[0]


# ---------------------------------------------------------------------------- 4. frames and queries
def test_frames_and_queries_equal_a_fresh_caster(atlas):
    dim = 32
    for settings in ((("empty_boxes", 0),), ()):
        grid = grid_of(dim, 9)
        grid[:3] = 5                                            # a floor: the frame sees the scene
        c = caster(atlas, dim, grid, settings=settings)
        rng = np.random.default_rng(10)
        cur = grid
        for _ in range(3):
            p, m = er.random_batch(rng, dim)
            cur, _, _ = er.replay(cur, p, m)
            c.set_voxels(p, m)
        assert c.prepare(), c.last_error()
        if not settings:
            assert c.memory_usage2()["coarse_bytes"] > 0 and c.memory_usage2()["box_bytes"] > 0
        compact_and_check(c, dim, cr.DEFAULT_REACH, cur, f"frame{settings}")
        mem = c.memory_usage2()
        assert mem["coarse_bytes"] == 0 and mem["box_bytes"] == 0 and mem["box_records"] == 0
        f = caster(atlas, dim, cur, settings=settings)
        qrng = np.random.default_rng(14)
        rays, boxes, sweeps = rr.random_rays(qrng, 256, dim), br.random_boxes(qrng, 256, dim), sr.random_sweeps(qrng, 256, dim)
        pts = qrng.integers(-2, dim + 2, size=(256, 3)).astype(I)
        assert np.array_equal(c.cast_rays(rays), f.cast_rays(rays))
        for a, b in zip(c.box_intersection(boxes, max_voxels=9), f.box_intersection(boxes, max_voxels=9)):
            assert np.array_equal(a, b)
        assert np.array_equal(c.sweep_boxes(sweeps), f.sweep_boxes(sweeps))
        assert np.array_equal(c.get_voxels(pts), f.get_voxels(pts))
        mem = c.memory_usage2()
        assert mem["coarse_bytes"] == 0 and mem["box_bytes"] == 0, "a query started a derived build"
        if not settings:
            assert c.prepare(), c.last_error()
        img, hits, ctr = _frame(c)
        fimg, fhits, fctr = _frame(f)
        assert c.last_kernel()["name"] == f.last_kernel()["name"]
        assert np.array_equal(img, fimg) and np.array_equal(hits, fhits) and ctr == fctr, settings
        assert ctr["canonical_reads"] == bool(settings)
        if not settings:
            assert c.used_empty_boxes()
            chk = c.empty_boxes_check(samples=1 << 16)
            assert chk["boxes_sampled"] > 0 and chk["solid_voxels"] == 0
        assert np.array_equal(c.cast_rays(rays), f.cast_rays(rays))


# ---------------------------------------------------------------------------- 5. edits and compactions alternate
def test_edits_and_compactions_alternate_with_exact_reserve(atlas):
    dim = 16
    grid = grid_of(dim, 60)
    c = caster(atlas, dim, grid, settings=(("edit_reserve", 0),))
    rng = np.random.default_rng(61)
    cur = grid
    for k in range(20):
        p, m = er.random_batch(rng, dim, n=40)
        cur, skipped, changed = er.replay(cur, p, m)
        info = c.set_voxels(p, m)
        assert (info["skipped"], info["voxels_changed"]) == (skipped, changed), k
        assert np.array_equal(whole(c, dim), np.pad(cur, 1)), k
        cinfo, _ = compact_and_check(c, dim, cr.DEFAULT_REACH, cur, f"round{k}")
        assert cinfo["descriptors_before"] == info["n_descriptors"]
        desc, _, lookup, attach = state(c)
        assert c.memory_usage2()["octree_bytes"] == 8 * len(desc) + 4 * len(lookup) + 8 * len(attach), "edit_reserve = 0 is exact"
    fresh = vrc.Octree.Generate(cur.reshape(-1), dim, layout=vrc.LAYOUT_NO_PAGE_HEADERS)
    assert er.masks_by_position(state(c)[0], 0, dim) == er.masks_by_position(fresh.descriptor_buffer, fresh.root_index, dim)


# ---------------------------------------------------------------------------- 6. shallow trees, the empty scene
@pytest.mark.parametrize("dim", [2, 4])
def test_shallow_trees(atlas, dim):
    for variant in ("attached", "plain05"):
        c, cur = _edited(atlas, dim, variant, seed=2, n=6)
        compact_and_check(c, dim, cr.DEFAULT_REACH, cur, f"shallow{dim}-{variant}")
        p = np.array([[dim - 1, 0, dim - 1]], I)
        m = np.array([0 if cur[dim - 1, 0, dim - 1] else 5], I)
        cur, _, _ = er.replay(cur, p, m)
        c.set_voxels(p, m)
        info, _ = compact_and_check(c, dim, cr.DEFAULT_REACH, cur, f"shallow{dim}-{variant}-again")
        assert info["n_descriptors"] <= 9


def test_empty_scene_and_regrowth(atlas):
    dim = 16
    grid = grid_of(dim, 30)
    c = caster(atlas, dim, grid, settings=(("empty_boxes", 0),))
    g = np.arange(dim)
    everything = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(I)
    c.set_voxels(everything, np.zeros(len(everything), I))
    cur = np.zeros_like(grid)
    info, _ = compact_and_check(c, dim, cr.DEFAULT_REACH, cur, "empty")
    desc = state(c)[0]
    assert info["n_descriptors"] == 1 and len(desc) == 1 and (int(desc[0]) >> 16) & 0xff == 0 and int(desc[0]) & 0xffff == 0
    assert info["n_attachments"] == 1, "a tree with materials keeps one slot"
    img, _, _ = _frame(c)
    assert len(np.unique(img.reshape(-1, 4), axis=0)) == 1, "an empty scene renders one background colour"
    p, m = np.array([[9, 3, 12], [0, 0, 0]], I), np.array([7, 5], I)
    cur, _, changed = er.replay(cur, p, m)
    assert c.set_voxels(p, m)["voxels_changed"] == changed == 2
    assert np.array_equal(whole(c, dim), np.pad(cur, 1))
    compact_and_check(c, dim, cr.DEFAULT_REACH, cur, "regrown")
    assert c.get_voxels(p).tolist() == [7, 5]


# ---------------------------------------------------------------------------- 7. far pointers at the default reach
def test_a_tree_that_needs_far_pointers_at_the_default_reach(atlas):
    dim = 128
    grid = np.where(np.random.default_rng(70).random((dim, dim, dim)) < 0.5, 5, 0).astype(np.int8)
    c = caster(atlas, dim, grid, attachments=False, settings=(("empty_boxes", 0),))
    img0, hits0, ctr0 = _frame(c)
    n0 = c.octree_size()[0]
    dry = c.compact_octree(dry_run=True)
    info = c.compact_octree()
    print(info)
    assert counts(dry) == counts(info)
    assert info["far_slots"] > 0 and info["descriptors_before"] == n0 and info["live_descriptors"] + info["far_slots"] == info["n_descriptors"]
    assert c.octree_size() == (info["n_descriptors"], 0)
    assert np.array_equal(whole(c, dim), np.pad(grid, 1))
    img, hits, ctr = _frame(c)
    assert np.array_equal(img, img0) and np.array_equal(hits, hits0) and ctr == ctr0


# ---------------------------------------------------------------------------- 8. errors
def test_errors_change_nothing(atlas):
    dim = 16
    c, cur = _edited(atlas, dim, "attached", seed=3, batches=1)
    before, size0 = state(c), c.octree_size()
    h, lib = c._h, vrc.lib
    INVALID, NOT_READY, LIMIT = 1, 2, 6

    def unchanged():
        return all(np.array_equal(a, b) for a, b in zip(before, state(c))) and c.octree_size() == size0

    info = vrc.CompactInfo()
    info.struct_size = C.sizeof(vrc.CompactInfo)
    assert lib.vrc_compact_octree(None, 0, C.byref(info)) == INVALID
    for flags in (2, 3, 0x80000000):
        assert lib.vrc_compact_octree(h, flags, C.byref(info)) == INVALID and unchanged(), flags
    for size in (0, 3):
        info.struct_size = size
        assert lib.vrc_compact_octree(h, 0, C.byref(info)) == INVALID and unchanged(), size
    info.struct_size = C.sizeof(vrc.CompactInfo)
    assert c.add_to_settings_buffer("compact_near_reach", "COMPACT_NEAR_REACH", 15)
    for reach in (15, 0x8000, -1, 0):
        assert c.overwrite_setting("compact_near_reach", reach)
        assert lib.vrc_compact_octree(h, 0, C.byref(info)) == INVALID and unchanged(), reach
        assert lib.vrc_compact_octree(h, vrc.COMPACT_DRY_RUN, C.byref(info)) == INVALID and unchanged(), reach
    assert c.overwrite_setting("compact_near_reach", cr.DEFAULT_REACH)
    # not ready: a handle without a tree
    n = vrc.CLCaster()
    assert n.init(0)
    assert lib.vrc_compact_octree(n._h, 0, None) == NOT_READY
    # a tree adopted by a handle outside the group: refused, nothing changes; released, the call goes through
    other = vrc.CLCaster()
    assert other.init(0) and other.assign_octree_from(c)
    assert lib.vrc_compact_octree(h, 0, C.byref(info)) == LIMIT and unchanged() and other.octree_size() == size0
    assert other.release_octree()
    # a short struct takes what fits
    short = vrc.CompactInfo()
    short.struct_size = 16
    assert lib.vrc_compact_octree(h, vrc.COMPACT_DRY_RUN, C.byref(short)) == 0 and short.struct_size == 16 and short.descriptors_before == size0[0]
    assert short.n_descriptors == 0 and unchanged()
    # the array branch succeeds and changes nothing
    assert c.overwrite_setting("using_octree", 1)
    assert c.compact_octree()["n_descriptors"] == 0 and unchanged()
    assert c.overwrite_setting("using_octree", 0)
    compact_and_check(c, dim, cr.DEFAULT_REACH, cur, "after-errors")
    assert lib.vrc_compact_octree(h, 0, None) == 0, "info may be NULL"


# ---------------------------------------------------------------------------- 9. groups
@pytest.mark.parametrize("own_copies", [True, False])
def test_groups(atlas, own_copies):
    dim = 32
    settings = (("empty_boxes", 0),)
    g, cur = _edited(atlas, dim, "attached", seed=4, settings=settings, group=[0, 0], own_copies=own_copies)
    cur = cur.copy()
    assert g.group_size() == 2 and g.memory_usage2(1)["octree_shared"] == (0 if own_copies else 1)
    holders = g.memory_usage2(0)["tree_holders"]
    compact_and_check(g, dim, cr.DEFAULT_REACH, cur, f"group-own{own_copies}")
    assert g.memory_usage2(0)["tree_holders"] == holders
    f = caster(atlas, dim, cur, settings=settings)
    img, hits, ctr = _frame(g)                                  # every rank renders its rows of the frame
    fimg, fhits, fctr = _frame(f)
    assert np.array_equal(img, fimg) and np.array_equal(hits, fhits) and ctr == fctr
    # ... and the group goes on editing
    p, m = er.random_batch(np.random.default_rng(5), dim, n=200)
    cur, _, _ = er.replay(cur, p, m)
    g.set_voxels(p, m)
    assert np.array_equal(whole(g, dim), np.pad(cur, 1))
    f2 = caster(atlas, dim, cur, settings=settings)
    img, hits, ctr = _frame(g)
    fimg, fhits, fctr = _frame(f2)
    assert np.array_equal(img, fimg) and np.array_equal(hits, fhits) and ctr == fctr


# ---------------------------------------------------------------------------- 10. the index-audit build
def test_audit_build_compacts_and_renders_without_a_violation(tmp_path):
    out = str(tmp_path / "compact_audit.json")
    env = dict(os.environ, VRC_LIB_PATH=os.path.join(ROOT, "voxel-raycaster_amd", "libvrc_audit.so"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "compact_audit_case.py"), out], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.load(open(out))
    during, report, info = got["during"], got["report"], got["info"]
    for rep in (during, report):
        bad = {a: e for a, e in rep.items() if e["violations"]}
        assert not bad, bad
    # the compaction's own reads of the old tree were checked against the old extents
    for array in ("descriptors", "attach_lookup", "attachments"):
        e = during[array]
        assert e["accesses"] > 0 and e["extent_published"] and e["max_index"] < e["extent"], (array, e)
    assert during["descriptors"]["extent"] == info["descriptors_before"]
    # the frame after it: edit_reserve = 0, so the extents are exactly the new tree's
    for array in ("descriptors", "far_slots", "attach_lookup", "attachments", "image"):
        e = report[array]
        assert e["accesses"] > 0 and e["extent_published"] and e["max_index"] < e["extent"], (array, e)
    assert report["descriptors"]["extent"] == report["far_slots"]["extent"] == report["attach_lookup"]["extent"] == info["n_descriptors"]
    assert report["attachments"]["extent"] == info["n_attachments"] == got["n_attachments"]
    assert info["far_slots"] > 0 and got["reads_ok"] and got["replay_ok"]
