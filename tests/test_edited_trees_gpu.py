"""GPU suite (-m gpu): frames, the coarse table and the empty boxes on the arrays that the scene edits and the compaction leave
behind (tests/edited_tree_cases.py: the histories).  The edit suites check the voxels; this file checks what the edits exist for.
Such an array is unlike any other input of the frame path: the root at the end with a near pointer of 1, untouched children behind
far pointers that point backwards, the live tree interleaved with garbage that looks like descriptors, n_desc below the
allocation, box records sized by n_desc (garbage included), solid leaves dug into nodes with leaf children, a root with valid
mask 0, the one-word array of a compacted empty scene.

Per history a caster is built, sent the steps (every step's counts and the read-back grid against the numpy replays), and read
back; the array must have the intended shape.  Then, in the five configurations of tests/test_layouts_gpu.py (default, no boxes, no
table, box records for the two upper levels, coarse_log2 = 2) x three kernels (exact, exact with jump_min_run = 2, mode B), and once
with three lights, from two cameras, every comparison exact:

* the frame equals the oracle ON THE READ-BACK ARRAY (its root, lookup, attachments), and that equals the oracle on the host
  builder's tree of the replayed grid: image, seven hit columns, and the canonical read counts too (not for leaves32, whose untouched
  solid leaves stay leaves where the host builder makes nodes);
* vrc_memory_usage2 reports the table and the boxes exactly when the configuration asks for them, a box word per descriptor;
* every voxel of every box is empty in the replayed grid (tests/box_check.py, no slot left out) and the device's self-check agrees;
* the boxes do something: they are used, more than a quarter are wider than their node, the frame reads fewer descriptors than
  the canonical traversal (with records for the two upper levels only: never more -- a scene of random voxels has no empty node
  that large, and points64 reads 254 988 descriptors either way); in an emptied scene every box is the map.

loop32 is the loop a host runs -- batch, vrc_prepare, frame, twelve times, two compactions -- on a handle that reallocates with
every batch (edit_reserve = 0) and on one that does not: every generation's frames equal the oracle on that generation's array, and
the structures are gone after every commit and back after vrc_prepare.  tests/test_edited_trees_cpu.py shows without a GPU that
these cases can fail: the cameras see what the steps wrote, and the host box check rejects a box that holds a solid voxel."""
import functools
import gc

import numpy as np
import pytest

import box_check
import edited_tree_cases as etc
import relayout as rl
import treetools
import voxel_raycaster_amd as vrc
from gpu_helpers import configure
from test_layouts_gpu import CONFIGS
from test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu
I = np.int32
U32 = np.uint32
KERNELS = (("exact", (), 0), ("exact-jumps", (("jump_min_run", 2),), 0), ("mode-B", (("stepping_mode", 1),), 1))
MATRIX = [n for n in etc.NAMES if n not in etc.EMPTIED and n not in etc.LOOPS]


def _caster(h, atlas, settings=(), light_count=1):
    c = vrc.CLCaster()
    assert c.init(0), c.last_error()
    _, cam_dir, cam_pos = h.cameras[0]
    configure(c, h.dim, atlas, cam_dir, cam_pos, h.lights, etc.W, etc.H, light_count=light_count)
    for k, v in h.settings + tuple(settings):
        assert c.add_to_settings_buffer(k, k.upper(), v), c.last_error()
    if h.tree is not None:
        assert c.assign_octree(vrc.Octree(*h.tree, h.dim)), c.last_error()
    else:
        c.build_dense_grid(h.dim.bit_length() - 1, h.start.reshape(-1), attachments=True)
    assert c.validate(), c.last_error()
    return c


def _look(c, camera):
    """The camera's arrays are read again at every frame.  The viewport is created anew because that clears the image: the
    along-x camera never writes the pixels whose ray has y = 0 (scenes.axis_aligned), and the oracle starts from a cleared image."""
    _, cam_dir, cam_pos = camera
    c._keep["cam"][0][:] = cam_dir
    c._keep["cam"][1][:] = cam_pos
    assert c.create_viewport(etc.W, etc.H) and c.validate(), c.last_error()


def _step(c, kind, a):
    if kind == "set_voxels":
        return c.set_voxels(a["positions"], a["materials"])
    if kind == "fill_boxes":
        return c.fill_boxes(a["lo"], a["size"], a["materials"], where=a.get("where"))
    if kind == "write_regions":
        return c.write_regions(a["lo"], a["data"], skip_zero=bool(a.get("skip_zero")))
    if kind == "fill_shapes":
        return c.fill_shapes(a["shapes"], a["materials"])
    assert kind == "compact", kind
    return c.compact_octree()


def _whole(c, dim):
    return c.read_regions(np.zeros((1, 3), I), (dim,) * 3)[0]


def _checked_step(c, h, k):
    """step k of the history: its counts and the read-back grid against the replay"""
    (kind, a), (grid, skipped, changed) = h.steps[k], h.after[k]
    info = _step(c, kind, a)
    if kind != "compact":
        assert (info["skipped"], info["voxels_changed"]) == (skipped, changed), (h.name, k, kind, info, skipped, changed)
    got = _whole(c, h.dim)
    assert np.array_equal(got, grid), (h.name, k, kind, np.argwhere(got != grid)[:4])
    return info


def _state(c):
    desc = c.read_descriptors()
    n, root = c.octree_size()
    assert n == len(desc)
    lookup, attach = c.read_attachments()
    return desc, root, lookup, attach


class Run:
    """One history on the device: the read-back array in its intended shape, and casters of any configuration that hold it."""

    def __init__(self, name, atlas):
        self.name, self.atlas = name, atlas
        self.h = h = etc.history(name)
        assert not h.frames()
        c = _caster(h, atlas)
        self.n_before = c.octree_size()[0]
        self.infos = [_checked_step(c, h, k) for k in range(len(h.steps))]
        self.desc, self.root, self.lookup, self.attach = _state(c)
        self.n_desc, dim = len(self.desc), h.dim
        # the array is the input this file is about
        assert np.array_equal(rl.decode(self.desc, self.root, dim, self.lookup, self.attach), h.final.reshape(-1)), name
        self.nodes, self.far = treetools.canonical(self.desc, self.root, dim)[1]
        word = int(self.desc[self.root])
        if name in etc.EDITED:
            assert self.root >= self.n_before and self.n_desc > self.n_before and (self.far > 0) == (not h.empty), (name, self.root, self.far)
            assert h.empty or word & 0xffff == 1, (name, "the new root stands in front of its block: a near pointer of 1")
        else:
            assert name in etc.COMPACTED and self.root == 0 and self.infos[-1]["n_descriptors"] == self.n_desc < self.infos[-1]["descriptors_before"]
            assert (self.infos[-1]["far_slots"] > 0) == (self.far > 0) == name.endswith("far"), (name, self.infos[-1], self.far)
        if h.empty:
            assert word >> 16 & 0xff == 0 and self.nodes == 1 and (self.n_desc == 1) == (name in etc.COMPACTED)
        if name == "leaves32":
            masks = {(valid, leaf) for valid, leaf in (v[:2] for v in _nodes(treetools.canonical(self.desc, self.root, dim)[0]))}
            assert any(valid == 0xff and bin(leaf).count("1") == 7 for valid, leaf in masks), "no dug leaf with seven leaf children"
        self.host = etc.host_tree(h.final)
        print(f"\nEDITED-TREES {name}: n_desc {self.n_before} -> {self.n_desc}, root {self.root}, {self.nodes} live nodes, {self.far} far pointers")
        del c

    def caster(self, settings=(), light_count=1):
        """another caster that took the same steps: the edits are deterministic, so it holds the same array word for word"""
        c = _caster(self.h, self.atlas, settings, light_count)
        for kind, a in self.h.steps:
            _step(c, kind, a)
        assert c.octree_size() == (self.n_desc, self.root) and np.array_equal(c.read_descriptors(), self.desc), self.name
        return c


def _nodes(sig):
    yield sig
    if len(sig) == 3:
        for kid in sig[2]:
            yield from _nodes(kid)


_RUNS = {}


def _run_fixture(request, atlas):
    r = _RUNS[request.param] = Run(request.param, atlas)
    yield r
    del _RUNS[request.param]
    gc.collect()


@pytest.fixture(scope="module", params=MATRIX)
def run(request, atlas):
    yield from _run_fixture(request, atlas)


@pytest.fixture(scope="module", params=etc.EMPTIED)
def emptied(request, atlas):
    yield from _run_fixture(request, atlas)


@functools.lru_cache(maxsize=None)
def _oracle(name, which, cam, mode, coarse, light_count):
    """the oracle's frame on the read-back array ("array") or on the host builder's tree of the replayed grid ("host")"""
    r = _RUNS[name]
    o = r.host
    arrays = (r.desc, r.root, r.lookup, r.attach) if which == "array" else (o.descriptor_buffer, o.root_index, o.attachment_lookup, o.attachment_buffer)
    return etc.oracle_frame(r.h, r.h.cameras[cam], *arrays, mode=mode, coarse=coarse, light_count=light_count)


def _structures(r, c, config, mode=0):
    """(table level, boxes built) as vrc_memory_usage2 reports them after vrc_prepare or a frame, asserted against what the
    configuration asks for (mode B builds no boxes)"""
    m = c.memory_usage2()
    n = r.h.dim.bit_length() - 1
    tag = (r.name, config, mode, m)
    want_table = {"no-table": 0, "coarse2": 2}.get(config, min(n - 2, 9))
    assert m["coarse_log2"] == want_table and (m["coarse_bytes"] > 0) == (want_table > 0), tag
    want_boxes = config not in ("no-boxes", "no-table") and mode == 0
    assert (m["box_bytes"] > 0) == want_boxes and m["note"] == "" and m["box_queries_cut"] == 0, tag
    if config == "upper-boxes" and want_boxes:
        # (breadth-first records of the levels that exist: an empty scene has the root's alone)
        assert m["box_levels"] == (1 if r.h.empty else 2) and m["box_records"] == 1 + (0 if r.h.empty else bin(int(r.desc[r.root]) >> 16 & 0xff).count("1")), tag
    elif want_boxes:
        assert m["box_levels"] == n and m["box_records"] == r.n_desc, tag           # a word per descriptor, garbage included
    else:
        assert m["box_records"] == 0, tag
    return want_table, want_boxes


def _check_frames(r, config, light_count=1, kernels=KERNELS):
    h = r.h
    coarse = {"no-table": 0, "coarse2": 2}.get(config, -1)
    for kernel, extra, mode in kernels:
        c = r.caster(CONFIGS[config] + extra, light_count)
        m = c.memory_usage2()
        assert m["coarse_bytes"] == 0 and m["box_bytes"] == 0 and m["box_records"] == 0, "the last commit left a structure behind"
        assert c.prepare(), c.last_error()
        for cam, camera in enumerate(h.cameras):
            tag = f"{r.name} {config} {kernel} lights={light_count} camera={camera[0]}"
            _look(c, camera)
            assert c.compute(), c.last_error()
            _, boxes = _structures(r, c, config, mode)
            assert c.used_empty_boxes() == boxes, tag
            img, hits, ctr = c.read_image(), c.read_hits(), c.counters()
            assert ctr["canonical_reads"] == (not boxes), tag
            on_array = _oracle(r.name, "array", cam, mode, coarse if mode else -1, light_count)
            try:
                assert_same(img, hits, ctr, *on_array)
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from None
            # ... and the array renders as the host builder's tree of the replayed grid does (an oracle against itself: no tolerance)
            on_host = _oracle(r.name, "host", cam, mode, coarse if mode else -1, light_count)
            assert np.array_equal(on_array[0].view(U32), on_host[0].view(U32)) and np.array_equal(on_array[1][..., :7], on_host[1][..., :7]), tag
            if r.name != "leaves32":
                assert np.array_equal(on_array[1], on_host[1]) and on_array[2] == on_host[2], (tag, "canonical read counts")
            if boxes and not h.empty:
                # A word per descriptor: strictly fewer reads than the canonical traversal.  Records for the two upper levels hold
                # boxes only for empty nodes of a half or a quarter of the map's side, and a scene of random voxels has none
                # (points64: 254 988 reads either way): never more reads, and no promise of fewer.
                canonical = _oracle(r.name, "array", cam, 0, -1, light_count)[2]["n_desc"]
                assert ctr["descriptor_reads"] < canonical + (config == "upper-boxes"), (tag, ctr["descriptor_reads"], canonical)
                if kernel == "exact" and light_count == 1 and config in ("default", "upper-boxes"):
                    print(f"\nEDITED-TREES {tag}: descriptor reads {canonical} canonical, {ctr['descriptor_reads']} with the boxes")
        del c


def _check_boxes(r, config):
    h, dim = r.h, r.h.dim
    tag = f"{r.name} {config}"
    c = r.caster(CONFIGS[config])
    assert c.prepare() and c.compute(), c.last_error()
    _, boxes = _structures(r, c, config)
    assert c.used_empty_boxes() == boxes, tag
    if not boxes:
        with pytest.raises(vrc.VrcError):
            c.empty_boxes_check(1 << 10)
        with pytest.raises(vrc.VrcError):
            c.read_empty_boxes()
        return
    chk = c.empty_boxes_check(64 * 8 * r.n_desc, seed=3)
    assert chk["solid_voxels"] == 0 and chk["boxes_sampled"] > 0, (tag, chk)
    if config == "upper-boxes":
        with pytest.raises(vrc.VrcError):
            c.read_empty_boxes()                                # (records of the upper levels are not indexed by descriptor)
        return
    words = c.read_empty_boxes()
    assert words.shape == (r.n_desc, 8)
    slots = sum(1 for _ in treetools.empty_children(r.desc, r.root, dim))
    n_boxes, grown, volume, node_volume = box_check.check_boxes(r.desc, r.root, dim, words, h.final != 0, tag=tag)
    assert n_boxes == slots >= 8 and grown > n_boxes // 4, (tag, "a slot left out", n_boxes, slots, grown)
    print(f"\nEDITED-TREES {tag}: {n_boxes} empty child slots, {grown} widened, mean box volume {volume / n_boxes:.0f} voxels ({volume / node_volume:.1f} x the nodes')")
    if h.empty:                                                 # the closed form: eight boxes, each the whole map
        _, lo, hi, _ = box_check.boxes_of(r.desc, r.root, dim, words)
        assert n_boxes == grown == 8 and (lo == 0).all() and (hi == dim).all(), (tag, lo, hi)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_frames(run, config):
    _check_frames(run, config)


def test_frames_with_three_lights(run):
    _check_frames(run, "default", light_count=3)
    assert _oracle(run.name, "array", 0, 0, -1, 3)[2]["shadow_rays"] > _oracle(run.name, "array", 0, 0, -1, 1)[2]["shadow_rays"]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_boxes(run, config):
    _check_boxes(run, config)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_emptied_scene(emptied, config):
    """A root with valid mask 0 (at the end of an array of garbage, or alone in a one-word array) under the table builder, the box
    builders and every frame kernel: one background colour, and eight boxes that are the map."""
    _check_boxes(emptied, config)
    _check_frames(emptied, config)
    if config == "default":
        _check_frames(emptied, config, light_count=3, kernels=KERNELS[:1])
    for cam in range(2):
        img, hits, ctr = _oracle(emptied.name, "array", cam, 0, -1, 1)
        assert ctr["n_desc"] == ctr["primary_rays"] and ctr["shadow_rays"] == 0 and (hits[..., :3] == -1).all()


def _gone(c, tag):
    m = c.memory_usage2()
    assert m["coarse_bytes"] == 0 and m["box_bytes"] == 0 and m["box_records"] == 0, (tag, "a commit left a structure behind", m)


@pytest.mark.parametrize("name", etc.LOOPS)
def test_loop(name, atlas):
    """edit, prepare, frame, twelve times on one handle, a compaction after generations 4 and 9"""
    h = etc.history(name)
    dim, n = h.dim, h.dim.bit_length() - 1
    c = _caster(h, atlas)
    m = c.memory_usage2()
    assert m["coarse_bytes"] > 0 and m["box_bytes"] > 0, "validate() builds the structures"
    gen, bytes_seen, roots = 0, set(), set()
    for k, (kind, _) in enumerate(h.steps):
        tag = f"{name} step {k} ({kind}), generation {gen}"
        if kind != "frame":
            info = _checked_step(c, h, k)
            _gone(c, tag)
            desc, root, lookup, attach = _state(c)
            assert (info["n_descriptors"], info["root_index"]) == (len(desc), root) and root not in roots, tag
            roots.add(root) if kind != "compact" else roots.clear()
            assert (root == 0) == (kind == "compact"), tag
            bytes_seen.add(c.memory_usage2()["octree_bytes"])
            if name.endswith("reserve0"):
                assert c.memory_usage2()["octree_bytes"] == 8 * len(desc) + 4 * len(lookup) + 8 * len(attach), (tag, "edit_reserve = 0 is exact")
            continue
        _gone(c, tag)
        assert c.prepare(), c.last_error()
        m = c.memory_usage2()
        desc, root, lookup, attach = _state(c)
        assert m["coarse_log2"] == n - 2 and m["coarse_bytes"] == 8 << (3 * (n - 2)) and m["box_bytes"] > 0 and m["note"] == "", (tag, m)
        assert m["box_records"] == len(desc) and m["box_levels"] == n and m["box_queries_cut"] == 0, (tag, m)
        grid = h.after[k][0]
        assert np.array_equal(rl.decode(desc, root, dim, lookup, attach), grid.reshape(-1)), tag
        for camera in h.cameras:
            _look(c, camera)
            assert c.compute(), c.last_error()
            assert c.used_empty_boxes(), tag
            want = etc.oracle_frame(h, camera, desc, root, lookup, attach)
            try:
                assert_same(c.read_image(), c.read_hits(), c.counters(), *want)
            except AssertionError as e:
                raise AssertionError(f"{tag} camera={camera[0]}: {e}") from None
            assert c.counters()["descriptor_reads"] <= want[2]["n_desc"], tag      # (a camera in front of the stage: nothing to skip)
        after = c.memory_usage2()
        built = ("octree_bytes", "coarse_log2", "coarse_bytes", "box_bytes", "box_build_seconds", "box_records", "box_levels", "box_queries_cut", "note")
        assert [after[k] for k in built] == [m[k] for k in built], (tag, "a frame rebuilt what vrc_prepare had built", m, after)
        chk = c.empty_boxes_check(64 * 8 * len(desc), seed=gen)
        assert chk["solid_voxels"] == 0 and chk["boxes_sampled"] > 0, (tag, chk)
        n_boxes, grown, _, _ = box_check.check_boxes(desc, root, dim, c.read_empty_boxes(), grid != 0, tag=tag)
        assert grown > n_boxes // 4, tag
        gen += 1
    assert gen == 12
    print(f"\nEDITED-TREES {name}: {len(bytes_seen)} allocation sizes over {len(h.steps) - 12} commits, final n_desc {len(desc)}, root {root}")
