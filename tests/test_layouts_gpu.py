"""GPU suite (-m gpu): every tree-walking kernel on re-laid-out arrays (tests/relayout.py): far pointers, a root in the middle
of the array, child blocks before their parents, unreferenced filler words between blocks -- on trees small enough to compare
every voxel.  Ten device-side code paths decode the child descriptors on their own (the exact frame kernel, the jump kernel
and the coarse-table builder, the empty-box builder, the ray queries, the box queries and sweeps, the voxel reads); before this
file only the large device-built terrains showed them a far pointer, on samples.

Three trees (floor_pillars 32^3 and random_sparse 64^3 with materials, a 32^3 tree with solid leaves above the bottom), each in
its original layout and re-laid with far_fraction 0.5 (floor_pillars also with 1.0: every parent far), in four configurations
(default: table and boxes; no boxes; no table; box records for the two upper levels only, which are numbered breadth-first while
the array is not) and, on the 64^3 scene, with coarse_log2 = 2, where the region read takes the table path of its descent.
Every comparison is exact: frames against the oracle on the same array and against the original layout's frame, queries and
reads against the numpy replays and against the original layout's answers.  tests/test_layouts_cpu.py shows that these inputs
would catch a kernel that ignores the far bit or the root index."""
import functools
import gc

import numpy as np
import pytest

import box_check
import box_replay as br
import ray_replay
import relayout as rl
import scenes
import sweep_replay as sr
import treetools
import voxel_raycaster_amd as vrc
from oracle import orc
from test_box_queries_gpu import _caster, _derive
from test_parity_gpu import assert_same
from test_ray_queries_gpu import _check_picking
from test_voxel_reads_gpu import _all_points, _built_from_grid, _check_scene, _random_regions

pytestmark = pytest.mark.gpu
I = np.int32
W, H = 96, 64

CONFIGS = {
    "default": (),
    "no-boxes": (("empty_boxes", 0),),
    "no-table": (("coarse_log2", 0),),
    "upper-boxes": (("empty_boxes", 2), ("empty_box_levels", 2)),
    "coarse2": (("coarse_log2", 2),),
}
LAYOUTS = {"original": None, "relaid-0.5": 0.5, "relaid-1.0": 1.0}


def _cases():
    out = []
    for tree in ("floor_pillars32", "random_sparse64", "leaf_octree32"):
        for config in CONFIGS:
            if config == "coarse2" and tree != "random_sparse64":
                continue
            for layout in LAYOUTS:
                if layout == "relaid-1.0" and tree != "floor_pillars32":
                    continue
                out.append((tree, config, layout))
    return out


@functools.lru_cache(maxsize=None)
def _tree(name):
    """The scene, its material grid, the tree in its original layout with attachments, the signature of Generate's tree."""
    if name == "leaf_octree32":
        desc, root, g = rl.leaf_tree()
        s = dict(scenes.floor_pillars(32), grid=g)
        o = vrc.Octree(desc, root, 32)
    else:
        s = dict(scenes.floor_pillars(32) if name == "floor_pillars32" else scenes.random_sparse(64))
        g = rl.with_materials(s["grid"], s["dim"])
        s["grid"] = g
        o = vrc.Octree.Generate(g, s["dim"], layout=2)
    o.attach_materials_from_grid(g)
    dim = s["dim"]
    gen = vrc.Octree.Generate(g, dim, layout=2)
    return s, g, o, treetools.canonical(gen.descriptor_buffer, gen.root_index, dim)[0]


@functools.lru_cache(maxsize=None)
def _laid(name, layout):
    s, g, o, _ = _tree(name)
    ff = LAYOUTS[layout]
    if ff is None:
        return o
    d2, r2, l2 = rl.relayout(o.descriptor_buffer, o.root_index, o.dim, np.random.default_rng(len(name) + int(10 * ff)), ff, o.attachment_lookup)
    assert treetools.canonical(d2, r2, o.dim)[0] == treetools.canonical(o.descriptor_buffer, o.root_index, o.dim)[0]
    far = treetools.canonical(d2, r2, o.dim)[1][1]
    assert far > 0 and r2 != 0 and (ff < 1 or far == rl.parents_with_children(d2, r2, o.dim))
    # these very arrays tell a decoder that ignores the far bit, or starts at index 0, from a right one (tests/test_layouts_cpu.py
    # shows the same for its own seeds): another grid, in occupancy too, or no decoding at all
    assert np.array_equal(rl.decode(d2, r2, o.dim, l2, o.attachment_buffer), g)
    for kw in (dict(root=r2, ignore_far=True), dict(root=0)):
        try:
            wrong = rl.decode(d2, kw.pop("root"), o.dim, l2, o.attachment_buffer, **kw)
        except IndexError:
            continue
        assert not np.array_equal(wrong != 0, g != 0), (name, layout, kw)
    o2 = vrc.Octree(d2, r2, o.dim)
    o2.attachment_lookup, o2.attachment_buffer = l2, o.attachment_buffer
    return o2


class Case:
    def __init__(self, tree, config, layout, atlas):
        self.tree, self.config, self.layout, self.atlas = tree, config, layout, atlas
        self.s, self.g, _, self.sig = _tree(tree)
        self.dim = self.s["dim"]
        self.o = _laid(tree, layout)
        self.tag = f"{tree} {config} {layout}"
        self.c = self.caster()

    def caster(self, extra=()):
        return _caster(self.s, self.atlas, settings=CONFIGS[self.config] + tuple(extra), octree=self.o)

    def structures(self, c, mode=0):
        """(table level, boxes built) after a frame or vrc_prepare -- asserted against what the configuration asks for (mode B
        builds no boxes)."""
        m = c.memory_usage2()
        n = self.dim.bit_length() - 1
        want_table = {"no-table": 0, "coarse2": 2}.get(self.config, min(n - 2, 9))
        assert m["coarse_log2"] == want_table and (m["coarse_bytes"] > 0) == (want_table > 0), (self.tag, m)
        want_boxes = self.config not in ("no-boxes", "no-table") and mode == 0
        assert (m["box_bytes"] > 0) == want_boxes and m["note"] == "", (self.tag, m)
        if self.config == "upper-boxes" and want_boxes:
            assert m["box_levels"] == 2 and m["box_records"] > 0, (self.tag, m)
        elif want_boxes:
            assert m["box_levels"] == n and m["box_records"] == self.o.descriptor_buffer.size, (self.tag, m)
        return want_table, want_boxes


@pytest.fixture(scope="module", params=_cases(), ids=lambda p: "-".join(p))
def case(request, atlas):
    k = Case(*request.param, atlas)
    yield k
    del k.c
    gc.collect()


# what the original layout answered, per (tree, config, what): the re-laid arrays must answer the same
_ORIGINAL = {}


def _same_as_original(case, what, compute):
    """compute(case) -> a tuple of arrays; kept for the original layout, compared with it for the others."""
    got = compute(case)
    key = (case.tree, case.config, what)
    if case.layout == "original":
        _ORIGINAL[key] = got
    else:
        if key not in _ORIGINAL:
            _ORIGINAL[key] = compute(Case(case.tree, case.config, "original", case.atlas))
        for a, b in zip(got, _ORIGINAL[key]):
            assert np.array_equal(a, b), (case.tag, what)
    return got


@functools.lru_cache(maxsize=None)
def _oracle_frame(tree, layout, mode, coarse):
    s, g, _, _ = _tree(tree)
    o = _laid(tree, layout)
    li = np.zeros((8, 10), dtype=np.float32)
    li[:1] = s["lights"][:1]
    return orc.raycast(width=W, height=H, cam_dir=s["cam_dir"], cam_pos=s["cam_pos"], lights=li, atlas=scenes.hash_atlas(), tile_dim=(16, 16),
                       descriptors=o.descriptor_buffer, root_index=o.root_index, octree_dim=o.dim, using_octree=0, max_distance=3 * o.dim,
                       stepping_mode=mode, coarse_log2=coarse, attachment_lookup=o.attachment_lookup, attachments=o.attachment_buffer)


def _frames(case):
    coarse = {"no-table": 0, "coarse2": 2}.get(case.config, -1)
    out = []
    for kernel, extra, mode in (("exact", (), 0), ("exact-jumps", (("jump_min_run", 2),), 0), ("mode-B", (("stepping_mode", 1),), 1)):
        c = case.caster(extra)
        assert c.compute(), c.last_error()
        _, boxes = case.structures(c, mode)
        assert c.used_empty_boxes() == boxes, (case.tag, kernel)
        img, hits, ctr = c.read_image(), c.read_hits(), c.counters()
        oimg, ohits, octr = _oracle_frame(case.tree, case.layout, mode, coarse if mode else -1)
        try:
            assert_same(img, hits, ctr, oimg, ohits, octr)
        except AssertionError as e:
            raise AssertionError(f"{case.tag} {kernel}: {e}") from None
        # the image, and every hit column the layout cannot change: all eight with the canonical read count (the oracle's
        # does not depend on the layout: tests/test_layouts_cpu.py), seven where the boxes count their own reads
        out += [img.view(np.uint32).copy(), hits[..., :8 if ctr["canonical_reads"] else 7].copy()]
        del c
    return tuple(out)


def test_frames(case):
    _same_as_original(case, "frames", _frames)


def test_empty_boxes(case):
    c = case.c
    assert c.compute(), c.last_error()
    _, boxes = case.structures(c)
    assert c.used_empty_boxes() == boxes
    if not boxes:
        with pytest.raises(vrc.VrcError):
            c.empty_boxes_check(1 << 10)
        with pytest.raises(vrc.VrcError):
            c.read_empty_boxes()
        return
    desc, root, dim = case.o.descriptor_buffer, case.o.root_index, case.dim
    slots = list(treetools.empty_children(desc, root, dim))
    chk = c.empty_boxes_check(64 * 8 * desc.size, seed=3)
    assert chk["solid_voxels"] == 0 and chk["boxes_sampled"] > len(slots) > 8, (case.tag, chk, len(slots))
    if case.config == "upper-boxes":
        with pytest.raises(vrc.VrcError):
            c.read_empty_boxes()                                # (records of the upper levels are not indexed by descriptor)
        return
    # every voxel of every box, on the host (tests/test_boxes_gpu.py): an independent walk of the array gives every empty child
    # slot its cube, the word its box, and the dense grid must hold no solid voxel inside it
    words = c.read_empty_boxes()
    assert words.shape == (desc.size, 8)
    solid = case.g.reshape(dim, dim, dim) != 0                  # [z, y, x]
    n_boxes, grown, _, _ = box_check.check_boxes(desc, root, dim, words, solid, tag=case.tag)
    assert n_boxes == len(slots) and grown > len(slots) // 4


@functools.lru_cache(maxsize=None)
def _expected_rays(tree):
    s, g, o, _ = _tree(tree)
    dim = o.dim
    rays = ray_replay.random_rays(np.random.default_rng(dim + 71), 2000, dim)
    rays[:200, :3] = np.floor(rays[:200, :3])                   # origins on voxel corners
    bias = ray_replay.origin_bias(rays[:, :3], o.descriptor_buffer, o.root_index, dim)
    exp = {(ap, ms): ray_replay.replay(rays, g, (dim,) * 3, max_steps=ms, as_pixel=ap, bias=bias if ap else None)
           for ap in (False, True) for ms in (0, 7)}
    kinds = set(exp[(False, 0)][:, 5].tolist())
    assert {ray_replay.HIT, ray_replay.LEFT_MAP} <= kinds and ray_replay.STEP_CAP in exp[(False, 7)][:, 5]
    return rays, exp


def _rays(case):
    rays, exp = _expected_rays(case.tree)
    out = []
    for (as_pixel, max_steps), want in exp.items():
        got = case.c.cast_rays(rays, max_steps=max_steps, as_pixel=as_pixel)
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (case.tag, as_pixel, max_steps, bad[:4], got[bad[:2]], want[bad[:2]], rays[bad[:2]])
        out.append(got)
    return tuple(out)


def test_ray_queries(case):
    case.c.prepare()
    case.structures(case.c)
    _same_as_original(case, "rays", _rays)


def test_picking(case):
    q = _same_as_original(case, "picking", lambda k: (_check_picking(k.c, k.s, W, H, 3 * k.dim),))[0]
    assert (q[:, 5] == vrc.RAY_HIT).sum() > 0
    assert case.c.assign_camera_trig(None)


@functools.lru_cache(maxsize=None)
def _expected_boxes(tree):
    s, g, o, _ = _tree(tree)
    dim = o.dim
    mat = br.grid_xyz(g, dim)
    boxes = br.random_boxes(np.random.default_rng(dim + 17), 1500, dim)
    return boxes, {st: br.GridReplay(mat, st).query(boxes, 64) for st in (False, True)}


def _boxes(case):
    boxes, full = _expected_boxes(case.tree)
    out = []
    for stopping in (False, True):
        for maxv in (0, 64):
            rec, cnt, vox = case.c.box_intersection(boxes, max_voxels=maxv, stopping_only=stopping)
            er, ec, ev = _derive(full[stopping], maxv)
            bad = np.nonzero((rec != er).any(1) | (cnt != ec))[0]
            assert bad.size == 0, (case.tag, stopping, maxv, bad[:4], rec[bad[:2]], er[bad[:2]], cnt[bad[:2]], ec[bad[:2]], boxes[bad[:2]])
            if maxv:
                badl = np.nonzero((vox != ev).any(axis=(1, 2)))[0]
                assert badl.size == 0, (case.tag, stopping, maxv, badl[:4], boxes[badl[:2]])
                out.append(vox)
            out += [rec, cnt]
    return tuple(out)


def test_box_queries(case):
    case.c.prepare()
    _same_as_original(case, "boxes", _boxes)


@functools.lru_cache(maxsize=None)
def _expected_sweeps(tree):
    s, g, o, _ = _tree(tree)
    dim = o.dim
    mat = br.grid_xyz(g, dim)
    sweeps = sr.random_sweeps(np.random.default_rng(dim + 29), 1500, dim)
    exp = {(st, cap): sr.sweep_replay(sr.GridScene(mat, st), sweeps, max_events=cap) for st in (False, True) for cap in (0, 6)}
    kinds = np.bitwise_or.reduce(exp[(False, 0)][:, 0])
    assert kinds & sr.HIT and kinds & sr.REJECTED and kinds & sr.CLIPPED and kinds & sr.LEFT_MAP and kinds & sr.START_SOLID, kinds
    assert np.bitwise_or.reduce(exp[(False, 6)][:, 0]) & sr.EVENT_CAP
    return sweeps, exp


def _sweeps(case):
    sweeps, exp = _expected_sweeps(case.tree)
    c = case.c
    out = []
    for face in (None, 0, 1 << 30):                             # the default split, every sweep a lane, every sweep a wave
        if face is not None:
            assert c.overwrite_setting("sweep_lane_face", face) or c.add_to_settings_buffer("sweep_lane_face", "SWEEP_LANE_FACE", face), c.last_error()
        for (stopping, cap), want in exp.items():
            got = c.sweep_boxes(sweeps, max_events=cap, stopping_only=stopping)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (case.tag, face, stopping, cap, len(bad), bad[:4], got[bad[:3]], want[bad[:3]], sweeps[bad[:3]])
            out.append(got)
    return tuple(out)


def test_sweeps(case):
    case.c.prepare()
    _same_as_original(case, "sweeps", _sweeps)


@functools.lru_cache(maxsize=None)
def _read_inputs(tree):
    dim = _tree(tree)[0]["dim"]
    rng = np.random.default_rng(dim + 29)
    return _random_regions(rng, dim), _all_points(dim, rng)


def _reads(case):
    regions, pts = _read_inputs(case.tree)
    whole, apron, got, p = _check_scene(case.c, br.grid_xyz(case.g, case.dim), case.dim, regions, pts, case.tag)
    return (whole, apron, p) + tuple(got)


def test_voxel_reads(case):
    case.c.prepare()
    table, _ = case.structures(case.c)
    if case.config == "coarse2":
        assert case.dim.bit_length() - 1 - table >= 3           # the region read's descent starts from the table
    _same_as_original(case, "reads", _reads)


def test_device_round_trip(case):
    c, dim = case.c, case.dim
    n, root = c.octree_size()
    assert (n, root) == (case.o.descriptor_buffer.size, case.o.root_index)
    assert np.array_equal(c.read_descriptors(), case.o.descriptor_buffer)
    whole = c.read_regions(np.zeros((1, 3), I), (dim,) * 3)
    assert np.array_equal(whole.reshape(-1), case.g)
    b = _built_from_grid(whole.reshape(-1), dim.bit_length() - 1, case.atlas, case.s)
    nb, rb = b.octree_size()
    assert treetools.canonical(b.read_descriptors(), rb, dim)[0] == case.sig, case.tag
    assert np.array_equal(b.read_regions(np.zeros((1, 3), I), (dim,) * 3), whole)
