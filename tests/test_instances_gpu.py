"""Every compiled instance of the frame kernels, launched on purpose, against the CPU oracle (-m gpu).

tests/instance_matrix.py lists the 24 raycast_svo_kernel instances, the 4 raycast_jump_kernel instances and raycast_array_kernel with
the settings that select each.  For every case: the library's own report of the launch (CLCaster.last_kernel, filled from the template
arguments the launch was instantiated with) names exactly that instance, and the frame -- image bits, fields 0-6 of every pixel's hit
record, every counter, the descriptor reads -- is the oracle's whole frame, bit for bit.  No tolerance, no sampling, no skip: a row
whose instance cannot be reached fails.

Two frames per case, on the depth-12 bench scene (the array row: on scenes.terrain256, by the same recipe):
  F1  the plain tree, 640 x 360 (900 blocks: fewer than the chip holds), max_distance = 3 * dim: every ray runs many times the jump
      thresholds, a shadow ray per light behind most of them.
  F2  the tree with procedural materials (mirror_period 64: mirrors restart rays after a jump), a ragged 333 x 187 frame (partly filled
      tiles and waves under the ballot-voted phases) and a step cap INSIDE the empty runs: max_distance = the median of field 6 over
      the oracle's own uncapped frame without shadow rays.  About half of the primary rays end at the cap in mid-air and the shadow
      rays of the rest are cut on their way to the light (the reference's step counter runs on through the shadow ray).
test_oracle_frames_are_not_vacuous asserts on the oracle's frames alone that they are what this paragraph says.

The occupancy rule behind the LDS-row instances is only as good as the runtime's answer: in a process with two HIP runtimes (libvrc.so
loaded before torch) it answers 2 blocks per CU for everything and the default frame silently runs the global-table instance.  The
package now imports torch first; the `thresholds` fixture below is what fails if that state comes back."""
import functools
import gc

import numpy as np
import pytest

import instance_matrix as im
import scenes
import voxel_raycaster_amd as vrc
from gpu_helpers import bench_scene
from oracle import orc
from test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu
SIZES = {"F1": (640, 360), "F2": (333, 187)}
THREADS = 16


# ---------------------------------------------------------------------------- scenes and the oracle's frames (CPU only)
@functools.lru_cache(maxsize=None)
def scene(kind, frame):
    """dim, tree (vrc.Octree), grid or None, camera, lights float32[8, 10] (all that exist assigned; light_count chooses), atlas."""
    if kind == "bench12":
        sc = bench_scene(12)
        tree = sc["octree"]
        if frame == "F2":                                  # the same descriptors with materials: a tree of its own, the plain one stays plain
            tree = vrc.Octree(tree.descriptor_buffer, tree.root_index, sc["dim"]).attach_materials_procedural(12, seed=1, mirror_period=64)
        return dict(dim=sc["dim"], tree=tree, grid=None, cam_dir=sc["cam_dir"], cam_pos=sc["cam_pos"], lights=sc["lights"], atlas=sc["atlas"])
    s = scenes.with_lights(scenes.terrain256(), 3)
    li = np.zeros((8, 10), dtype=np.float32)
    li[:3] = s["lights"]
    return dict(dim=s["dim"], tree=vrc.Map(s["dim"], s["grid"], buffer_size=100000).octree, grid=s["grid"],
                cam_dir=np.array(s["cam_dir"], dtype=np.float32), cam_pos=np.array(s["cam_pos"], dtype=np.float32), lights=li,
                atlas=scenes.hash_atlas())


def _oracle(kind, frame, **kw):
    s, (w, h) = scene(kind, frame), SIZES[frame]
    t = s["tree"]
    return orc.raycast(width=w, height=h, cam_dir=s["cam_dir"], cam_pos=s["cam_pos"], lights=s["lights"], atlas=s["atlas"], tile_dim=(16, 16),
                       descriptors=t.descriptor_buffer, root_index=t.root_index, octree_dim=s["dim"], using_octree=0 if s["grid"] is None else 1,
                       grid=s["grid"], attachment_lookup=t.attachment_lookup, attachments=t.attachment_buffer, threads=THREADS, **kw)


@functools.lru_cache(maxsize=None)
def max_distance(kind, frame):
    """F1: 3 * dim.  F2: the median step count of the oracle's own uncapped, primary-only frame -- from the oracle alone."""
    dim = scene(kind, frame)["dim"]
    if frame == "F1":
        return 3 * dim
    _, hits, _ = _oracle(kind, frame, max_distance=3 * dim, shadow_rays=0)
    return int(np.median(hits[..., 6]))


@functools.lru_cache(maxsize=None)
def oracle_frame(kind, frame, lights, mode=0, coarse=-1):
    """Depends only on (frame, light count, stepping mode) -- and in mode B its read count on the table's level: once per module."""
    return _oracle(kind, frame, max_distance=max_distance(kind, frame), active_lights=lights, stepping_mode=mode, coarse_log2=coarse)


# ---------------------------------------------------------------------------- casters
@pytest.fixture(scope="module")
def holders():
    """One caster per tree that only HOLDS it: the cases adopt the tree (vrc_assign_octree_from), so the descriptor array is uploaded
    once and what it derives -- coarse table, empty boxes -- stays with it from case to case; each case still gets a fresh handle, with
    no setting left over from the one before (jump_min_run has no value that means "unset")."""
    held = {}

    def get(kind, frame):
        key = (kind, frame if kind == "bench12" else "F1")         # (the array row's two frames share their tree)
        if key not in held:
            c = vrc.CLCaster()
            assert c.init(0), "vrc_create failed: is this a GPU box?"
            assert c.assign_octree(scene(*key)["tree"]), c.last_error()
            held[key] = c
        return held[key]

    yield get
    held.clear()
    gc.collect()


def _caster(holders, kind, frame, settings, lights=1):
    s, (w, h) = scene(kind, frame), SIZES[frame]
    c = vrc.CLCaster()
    assert c.init(0), "vrc_create failed: is this a GPU box?"
    base = {"octree_dimensions": s["dim"], "using_octree": 0, "max_distance": max_distance(kind, frame), "shadow_rays": 1, "light_count": lights}
    for k, v in {**base, **settings}.items():
        assert c.add_to_settings_buffer(k, k.upper(), v), c.last_error()
    assert c.assign_octree_from(holders(kind, frame)), c.last_error()
    if s["grid"] is not None:
        assert c.assign_map(s["grid"], (s["dim"],) * 3)
    assert c.assign_camera(s["cam_dir"], s["cam_pos"]) and c.create_viewport(w, h) and c.assign_lights(s["lights"])
    assert c.create_texture_atlas(s["atlas"], (16, 16))
    assert c.validate(), c.last_error()            # (ends with vrc_prepare: the derived structures for THESE settings, if the tree lacks them)
    return c


@pytest.fixture(scope="module")
def thresholds(holders):
    """The two default jump thresholds, learned from default frames: {True: tables in LDS, False: in global memory}."""
    out = {}
    for lds, settings in ((True, {}), (False, {"jump_tables_lds": 0})):
        c = _caster(holders, "bench12", "F1", settings)
        assert c.compute(), c.last_error()
        k = c.last_kernel()
        assert k["family"] == vrc.KERNEL_SVO and k["args"][0] == 1 and (k["lds_rows"] > 0) == lds, k
        out[lds] = k["jump_min_run"]
        del c
    assert 1 <= out[True] < im.JUMP_OFF and 1 <= out[False] < im.JUMP_OFF
    return out


# ---------------------------------------------------------------------------- the tests
def test_report_before_the_first_frame_and_by_rank(holders):
    c = _caster(holders, "bench12", "F1", {})
    with pytest.raises(vrc.VrcError):
        c.last_kernel()                                    # no frame yet
    assert c.last_status == 2                              # VRC_ERR_NOT_READY
    assert c.compute(), c.last_error()
    assert c.last_kernel(0)["name"].startswith("raycast_svo_kernel<")
    with pytest.raises(vrc.VrcError):
        c.last_kernel(1)                                   # a single handle has rank 0 only
    assert c.last_status == 1                              # VRC_ERR_INVALID_ARGUMENT


def test_report_of_a_group_is_per_rank(atlas):
    """A 20-row frame on 4 ranks in bands of 8: ranks 0-2 render 8, 8 and 4 rows with the same instance, rank 3 owns no rows and
    launched nothing; a rank outside the group is an argument error."""
    from gpu_helpers import configure
    s = scenes.floor_pillars()
    dim, w, h = s["dim"], 96, 20
    li = np.zeros((8, 10), dtype=np.float32)
    li[:1] = s["lights"]
    g = vrc.CLCaster()
    assert g.init_group([0, 0, 0, 0]) and g.assign_octree(vrc.Map(dim, s["grid"]).octree)
    configure(g, dim, atlas, s["cam_dir"], s["cam_pos"], li, w, h)
    assert g.validate() and g.compute(), g.last_error()
    ranks = [g.last_kernel(r) for r in range(4)]
    assert ranks[0]["family"] == vrc.KERNEL_SVO and ranks[0]["name"].startswith("raycast_svo_kernel<") and len(ranks[0]["args"]) == 6
    assert ranks[1] == ranks[0] and ranks[2] == ranks[0]
    assert ranks[3] == {"family": vrc.KERNEL_NONE, "args": (), "name": "", "jump_min_run": im.JUMP_OFF, "lds_rows": 0}
    with pytest.raises(vrc.VrcError):
        g.last_kernel(4)
    assert g.last_status == 1                              # VRC_ERR_INVALID_ARGUMENT


def test_oracle_frames_are_not_vacuous(thresholds):
    """On the oracle's frames alone: F1's rays exceed both default thresholds (as the library reports them) many times over; F2's cap
    lies inside the runs, its mirrors strike and some of its pixels stay unwritten; every exact-mode frame casts shadow rays."""
    k = max(thresholds.values())
    for n in (1, 2, 3, 4):
        for frame in ("F1", "F2"):
            _, hits, ctr = oracle_frame("bench12", frame, n)
            pixels = hits.shape[0] * hits.shape[1]
            print(f"{frame} {n} light(s): cap {max_distance('bench12', frame)}, median steps {int(np.median(hits[..., 6]))}, no hit "
                  f"{(hits[..., 0] < 0).mean():.3f}, mirror strikes {int((hits[..., 3] == 6).sum())}, {ctr}")
            assert ctr["shadow_rays"] >= 0.3 * pixels * n, (frame, n)
            if frame == "F1":
                assert (hits[..., 6] >= 4 * k).mean() >= 0.9, (n, k)
            else:
                assert 0.25 <= (hits[..., 0] < 0).mean() <= 0.75, n
                assert (hits[..., 3] == 6).sum() >= 250 and ctr["unwritten"] >= 100, n


@pytest.mark.parametrize("case", im.CASES, ids=[im.case_id(c) for c in im.CASES])
def test_instance_renders_the_oracles_frame(case, holders, thresholds):
    row, alt = case
    settings = row.settings[alt]
    mode = settings.get("stepping_mode", 0)
    for frame in ("F1", "F2"):
        for n in row.lights:
            # (a fresh handle per frame: its image starts from the clear colour, like the oracle's -- a pixel a frame leaves unwritten
            # keeps what the handle's frame before wrote there, and one pixel of the array row is unwritten with 2 lights and not with 1)
            c = _caster(holders, row.scene, frame, settings, n)
            tag = f"{im.case_id(case)} {frame} {n} light(s)"
            assert c.compute(), c.last_error()
            # 1. the launch itself says which instance ran
            k = c.last_kernel()
            assert k["name"] == im.name(row), f"{tag}: rendered by {k['name']} (lds_rows {k['lds_rows']}, jump_min_run {k['jump_min_run']})"
            assert k["args"] == tuple(int(a) for a in row.args)
            if row.family == "raycast_svo_kernel":
                jump, tuned, lds = row.args[0], row.args[2], row.args[3]
                assert k["family"] == vrc.KERNEL_SVO and k["lds_rows"] == lds
                assert k["jump_min_run"] == (im.JUMP_OFF if not jump else settings.get("jump_min_run", thresholds[lds > 0])), tag
                assert not (tuned and jump) or "jump_min_run" not in settings       # the tuned jump rows run the library's own default
            else:
                assert k["family"] == (vrc.KERNEL_JUMP if row.family == "raycast_jump_kernel" else vrc.KERNEL_ARRAY)
                assert k["jump_min_run"] == im.JUMP_OFF and k["lds_rows"] == 0
            # 2. the whole frame is the oracle's
            img, hits, ctr = c.read_image(), c.read_hits(), c.counters()
            oimg, ohits, octr = oracle_frame(row.scene, frame, n, mode, settings.get("coarse_log2", -1) if mode else -1)
            box = row.family == "raycast_svo_kernel" and row.args[5]
            assert ctr["canonical_reads"] == (not box), tag
            bad = (hits[..., :7] != ohits[..., :7])
            assert not bad.any(), f"{tag}: {int(bad.any(-1).sum())} pixels differ, per field {bad.reshape(-1, 7).sum(0).tolist()}"
            assert_same(img, hits, ctr, oimg, ohits, octr)
            # 3. descriptor reads: the oracle's count (canonical / mode B's restated one), or the box traversal's own, never more
            if box:
                assert ctr["descriptor_reads"] == int(hits[..., 7].astype(np.int64).sum()), tag
                assert ctr["descriptor_reads"] <= octr["n_desc"], tag
            else:
                assert np.array_equal(hits[..., 7], ohits[..., 7]) and ctr["descriptor_reads"] == octr["n_desc"], tag
            del c


@pytest.mark.parametrize("depth", [10, 12, 14, 16])
def test_bench_kernel_instance_names_what_the_library_launched(depth):
    """bench.py's kernel_instance derives the instance of a default frame from the tree's state with its own copy of the LDS-row rule;
    the report says what ran.  Default settings, host trees (depths 10, 12) and device-built ones (14, 16), one light and four."""
    import bench
    sc = bench_scene(depth) if depth <= 12 else bench.device_scene_header(depth)
    c = bench.make_caster(sc, 256, 144, 0)
    differ = []
    for lights in (1, 4):
        assert c.overwrite_setting("light_count", lights) and c.compute(), c.last_error()
        guess, ran = bench.kernel_instance(c, sc, lights).split("  (")[0], c.last_kernel()
        print(f"depth {depth}, {lights} light(s): bench says {guess}, launched {ran}")
        if guess != ran["name"]:
            differ.append((lights, guess, ran["name"]))
    del c
    gc.collect()
    assert not differ, differ
