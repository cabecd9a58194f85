"""The workgroup -> tile map of the exact SVO kernel (block_pixel<kTiles> in raycast_common.hpp).

The kernel's workgroup is finer than the 4-tile block the map is stated for (vrc_params.h svo_tiles_per_workgroup): a launch takes
S = 4 / T workgroups per block ("group"), the group count rounded up to a multiple of 8, and workgroup w renders sub-block
(w / 8) % S of group (w / 8S) * 8 + w % 8 -- so a group stays on the XCD it had (w % 8 == group % 8) and an XCD meets its groups in
the order it did.  What can go wrong is the map, not the rays: the shapes below are small and sit where it branches -- fewer than 8
workgroups, a width that is no multiple of 32, a tile-row count that is / is not a multiple of 8 (the interleaved branch of xcd_mode 1
and the row-major one with its remainder), a ragged last tile row -- under every xcd_mode and as row slices.

GPU cases (-m gpu): the frame -- image bits, hit records, the primary / shadow / step / unwritten counters (and the texel reads) --
is the CPU oracle's, bit for bit.  One host case restates the map in Python and checks it against the 4-tile map it refines."""
import functools

import numpy as np
import pytest

import scenes
import voxel_raycaster_amd as vrc
from gpu_helpers import configure
from oracle import orc
from test_parity_gpu import assert_same
from voxel_raycaster_amd import tiling

#          id   scene                  w    h
SHAPES = {"a": ("floor_pillars", 8, 8),          # one tile: fewer than 8 workgroups
          "b": ("floor_pillars", 40, 24),        # width no multiple of 32, 3 tile rows
          "c": ("random_sparse", 200, 136),      # 17 tile rows: the row-major branch and its remainder
          "d": ("random_sparse", 256, 192),      # 24 tile rows: the interleaved branch
          "e": ("floor_pillars", 72, 50)}        # height no multiple of 8
MODES = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def scene(name):
    s = getattr(scenes, name)()
    li = np.zeros((8, 10), dtype=np.float32)
    li[:1] = s["lights"]
    return s, vrc.Map(s["dim"], s["grid"], buffer_size=100000), li


@functools.lru_cache(maxsize=None)
def oracle_frame(shape):
    """Once per shape, shared by every mode and slicing of it; never written to."""
    name, w, h = SHAPES[shape]
    s, m, li = scene(name)
    return orc.raycast(width=w, height=h, cam_dir=s["cam_dir"], cam_pos=s["cam_pos"], lights=li, atlas=scenes.hash_atlas(), tile_dim=(16, 16),
                       descriptors=m.octree.descriptor_buffer, root_index=m.octree.root_index, octree_dim=s["dim"], using_octree=0,
                       grid=s["grid"], max_distance=3 * s["dim"])


def caster(shape, xcd_mode, atlas, row_slice=None):
    name, w, h = SHAPES[shape]
    s, m, li = scene(name)
    c = vrc.CLCaster()
    assert c.init(0), "vrc_create failed: is this a GPU box?"
    if row_slice is not None:
        assert c.set_row_slice(*row_slice), c.last_error()
    assert c.assign_octree(m.octree), c.last_error()
    assert c.add_to_settings_buffer("xcd_mode", "XCD_MODE", xcd_mode)
    configure(c, s["dim"], atlas, s["cam_dir"], s["cam_pos"], li, w, h)
    assert c.validate(), c.last_error()
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("xcd_mode", MODES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_frame_is_the_oracles_under_every_map(shape, xcd_mode, atlas):
    c = caster(shape, xcd_mode, atlas)
    assert c.compute(), c.last_error()
    assert c.last_kernel()["family"] == vrc.KERNEL_SVO
    assert_same(c.read_image(), c.read_hits(), c.counters(), *oracle_frame(shape))


@pytest.mark.gpu
@pytest.mark.parametrize("xcd_mode", MODES)
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("shape", ["c", "d"])
def test_row_slices_render_exactly_their_rows(shape, world, xcd_mode, atlas):
    """Every rank renders its bands of 8 rows into buffers that hold only those; the assembled frame and the summed counters are the
    oracle's.  The buffers start from values no frame holds, so a row nobody rendered -- or rendered into another's place -- shows."""
    _, w, h = SHAPES[shape]
    oimg, ohits, octr = oracle_frame(shape)
    img = np.full((h, w, 4), -7.0, dtype=np.float32)
    hits = np.full((h, w, 8), -7, dtype=np.int32)
    total, rows_seen = {}, 0
    for r in range(world):
        c = caster(shape, xcd_mode, atlas, row_slice=(r, world, 8))
        assert c.compute(), c.last_error()
        mine = tiling.rows_of_rank(h, r, world, 8)
        assert c.memory_usage()["rows"] == len(mine)
        before = img.copy()
        c.read_image(img); c.read_hits(hits)
        others = np.setdiff1d(np.arange(h), mine)
        assert np.array_equal(img[others].view(np.uint32), before[others].view(np.uint32)), "a rank wrote rows that are not its own"
        ctr = c.counters()
        for k, v in ctr.items():
            total[k] = (total.get(k, 0) + v) if k != "canonical_reads" else (total.get(k, True) and v)
        rows_seen += len(mine)
    assert rows_seen == h
    assert_same(img, hits, total, oimg, ohits, octr)


# ---------------------------------------------------------------------------- the map itself, on the host
def parent_map(g, groups, blocks_x, tile_rows, xcd_mode):
    """block_pixel for a workgroup of one whole group (the map before the workgroups were split): group -> (tile row, group column)."""
    per_xcd = groups >> 3
    if xcd_mode == 1 and per_xcd > 0 and g < (per_xcd << 3) and tile_rows % 8 == 0:
        j = g >> 3
        return (j // blocks_x) * 8 + (g & 7), j % blocks_x
    if xcd_mode == 0 and per_xcd > 0 and g < (per_xcd << 3):
        g = (g & 7) * per_xcd + (g >> 3)
    return g // blocks_x, g % blocks_x


def split_map(w, tiles, groups):
    """Workgroup w of a launch with `tiles` tiles per workgroup -> (group, first tile of the group it renders), or None past the last group."""
    s = 4 // tiles
    g, sub = (w // (8 * s)) * 8 + (w & 7), (w >> 3) % s
    return (g, sub * tiles) if g < groups else None


@pytest.mark.parametrize("tiles", [1, 2, 4])
def test_split_map_refines_the_group_map(tiles):
    for shape, (_, width, height) in sorted(SHAPES.items()):
        blocks_x, tile_rows = (width + 31) // 32, (height + 7) // 8
        groups = blocks_x * tile_rows
        launched = groups if tiles == 4 else (groups + 7) // 8 * 8 * (4 // tiles)      # vrc_params.h svo_workgroups
        for mode in MODES:
            seen = np.zeros((tile_rows, blocks_x * 4), dtype=np.int32)
            order = {k: [] for k in range(8)}                 # per XCD: the groups in the order their workgroups are dispatched
            for w in range(launched):
                at = (w, 0) if tiles == 4 else split_map(w, tiles, groups)
                if at is None:
                    continue
                g, first = at
                ty, bx = parent_map(g, groups, blocks_x, tile_rows, mode)
                assert 0 <= ty < tile_rows and 0 <= bx < blocks_x, (shape, mode, w)
                seen[ty, bx * 4 + first: bx * 4 + first + tiles] += 1
                # a workgroup runs on XCD w % 8; its group, launched whole, ran on XCD g % 8
                assert w % 8 == g % 8, (shape, mode, tiles, w, g)
                if not order[w % 8] or order[w % 8][-1] != g:
                    order[w % 8].append(g)
            assert (seen == 1).all(), (shape, mode, tiles, np.argwhere(seen != 1)[:4].tolist())
            for k in range(8):                                # ... and meets its groups once each, in the order the whole-group launch has
                assert order[k] == list(range(k, groups, 8)), (shape, mode, tiles, k)
