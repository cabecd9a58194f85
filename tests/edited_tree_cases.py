"""Histories: what tests/test_edited_trees_gpu.py sends to a resident scene before it renders it, and what the scene must hold
after every step.  A history is a starting grid (or a hand-made tree with solid leaves), a list of steps -- set_voxels, fill_boxes,
write_regions, fill_shapes, compact, frame (vrc_prepare, then a frame) -- the grid after every step, replayed on the host with
tests/edit_replay.py, region_replay.py and shape_replay.py, two cameras and the lights.  The arrays such histories leave behind
are the frame path's least tested input: the root at the end of the array, untouched children behind backward far pointers,
garbage between the live words, solid leaves turned into nodes with leaf children, a root with valid mask 0, a one-word array.

Materials are those of the edit tests, {0, 5, 6, 7, -3}; every scene has a floor, so that frames see what the steps wrote; every
history is 32^3 or 64^3, where the coarse table (level min(n - 2, 9) by default) and the empty boxes are in use.  Both cameras sit
in a voxel that is empty after every step: one looks across the scene, one along +x (azimuth 0: sin(yaw) = 0, rays tie on voxel
planes).  tests/test_edited_trees_cpu.py shows that the cameras see what the steps wrote.  Needs no GPU.  Not a test file."""
import functools

import numpy as np

import edit_replay as er
from gpu_helpers import lights4
import leaftree
import region_replay as rr
import shape_replay as shp

I = np.int32
MATERIALS = np.array([0, 5, 6, 7, -3], np.int8)
W, H = 96, 64
REACH_MIN = 16                                                  # kCompactReachMin (csrc/octree_compact.h)
LEAF_CUBES = [(8, 8, 8, 8), (16, 16, 0, 4), (0, 0, 0, 4), (20, 4, 6, 2), (0, 16, 16, 16)]      # tests/test_voxel_edits_gpu.py
# (cam_dir, fractions inside the voxel): across the scene, 25 degrees down; along +x (azimuth 0: sin(yaw) = 0, rays tie on voxel planes)
DIRECTIONS = (("across", (2.0, 1.5708), (0.37, 0.41, 0.29)), ("along-x", (1.9, 0.0), (0.5, 0.25, 0.4)))
# the voxel of either camera, per history: where the frame differs most between the starting and the final grid, of a lattice of
# empty voxels (tests/test_edited_trees_cpu.py asserts that it does differ)
CAMERA_VOXELS = {"points64": ((25, 9, 23), (9, 57, 19)), "regions32": ((25, 5, 27), (1, 21, 23)), "shapes64": ((25, 1, 35), (33, 25, 39)),
                 "leaves32": ((21, 1, 11), (1, 5, 11)), "regrown32": ((13, 1, 19), (1, 13, 25)), "emptied32": ((16, 1, 14), (1, 16, 16)),
                 "emptied64": ((32, 3, 28), (1, 32, 32)), "loop32": ((15, 11, 7), (1, 15, 11))}


def sparse_grid(dim, seed, solid=0.06):
    """random int8[z][y][x] of the materials {0, 5, 6, 7, -3}, `solid` of the voxels solid, on a floor three voxels thick"""
    rng = np.random.default_rng(seed)
    p = np.array([1 - solid, solid * 0.5, solid * 0.2, solid * 0.15, solid * 0.15])
    g = rng.choice(MATERIALS, size=(dim, dim, dim), p=p).astype(np.int8)
    g[:3] = 5
    return g


class History:
    """name, dim, start (int8[z][y][x]), tree ((descriptors, root) of a hand-made starting tree, or None: the start grid is built
    on the device with its materials), settings (of the caster), steps [(kind, arguments)], after [(grid, skipped, voxels_changed)
    per step], cameras [(name, cam_dir, cam_pos)], lights float32[8, 10] (gpu_helpers.lights4: light_count chooses how many shine)."""

    def __init__(self, name, start, steps, cameras, tree=None, settings=()):
        self.name, self.start, self.steps, self.tree, self.settings = name, start, steps, tree, tuple(settings)
        self.dim = start.shape[0]
        self.after = []
        g = start
        for kind, a in steps:
            if kind == "set_voxels":
                got = er.replay(g, a["positions"], a["materials"])
            elif kind == "fill_boxes":
                got = rr.fill(g, a["lo"], a["size"], a["materials"], {None: 0, "empty": rr.WHERE_EMPTY, "solid": rr.WHERE_SOLID}[a.get("where")])
            elif kind == "write_regions":
                got = rr.paste(g, a["lo"], a["data"], rr.SKIP_ZERO if a.get("skip_zero") else 0)
            elif kind == "fill_shapes":
                got = shp.fill_shapes(g, a["shapes"], a["materials"])
            else:
                assert kind in ("compact", "frame"), kind
                got = (g, 0, 0)
            self.after.append(got)
            g = got[0]
        self.final = g
        self.empty = not g.any()
        self.lights = lights4(self.dim)
        # both cameras sit in a voxel that is empty whenever a frame is rendered
        self.cameras = []
        for (cname, cam_dir, frac), (x, y, z) in zip(DIRECTIONS, cameras):
            for g in [self.final] + [self.after[k][0] for k in self.frames()]:
                assert g[z, y, x] == 0, (name, cname, "the camera's voxel is solid")
            self.cameras.append((cname, cam_dir, (x + frac[0], y + frac[1], z + frac[2])))

    def frames(self):
        """indices of the steps that render"""
        return [k for k, (kind, _) in enumerate(self.steps) if kind == "frame"]


def _points64():
    rng = np.random.default_rng(640)
    steps = []
    for _ in range(3):
        p, m = er.random_batch(rng, 64)
        steps.append(("set_voxels", dict(positions=p, materials=m)))
    return sparse_grid(64, 64), steps


def _regions32():
    rng = np.random.default_rng(320)
    block = rng.choice(MATERIALS[1:], size=(1, 7, 9, 11))
    block[rng.random(block.shape) < 0.5] = 0
    return sparse_grid(32, 32, 0.1), [
        ("fill_boxes", dict(lo=np.array([[5, 6, 1]], I), size=(13, 9, 11), materials=0)),                 # cleared, not brick-aligned
        ("fill_boxes", dict(lo=np.array([[16, 16, 0]], I), size=(16, 16, 16), materials=6)),              # an aligned 16^3 box, solid
        ("fill_boxes", dict(lo=np.array([[0, 20, 3]], I), size=(12, 10, 6), materials=7, where="empty")),
        ("write_regions", dict(lo=np.array([[3, 3, 5]], I), data=block.astype(np.int8), skip_zero=True)),
    ]


def _shapes64():
    g = np.zeros((64, 64, 64), np.int8)
    g[:3] = 5
    g[0:32, 32:64, 0:32] = 5                                    # a solid 32^3 block
    return g, [
        ("fill_shapes", dict(shapes=np.array([[shp.BALL, 20, 32, 16, 9, 0]], I), materials=0)),           # a crater in its face
        ("fill_shapes", dict(shapes=np.array([[shp.CYLINDER_X, 36, 20, 20, 3, 20], [shp.CYLINDER_Y, 45, 30, 12, 2, 25],
                                              [shp.CYLINDER_Z, 50, 45, 50, 4, 30]], I),                   # (the last leaves the map at z = 64)
                             materials=np.array([6, 7, -3], I))),
    ]


def _leaves32():
    """the tree of test_voxel_edits_gpu.test_digging_into_solid_leaves -- 2^3, 4^3, 8^3 and 16^3 solid leaves above the bottom
    level -- on a floor; one voxel dug out of every leaf, two of them filled again"""
    rng = np.random.default_rng(31)
    g = np.arange(32)
    floor = np.stack(np.meshgrid(g, g, np.arange(2), indexing="ij"), axis=-1).reshape(-1, 3)
    desc, root, flat = leaftree.leaf_octree(np.concatenate([rng.integers(0, 32, size=(200, 3)), floor]), LEAF_CUBES, 5)
    # one voxel on a face of every leaf, where a camera can see it: the 8^3, the upper 4^3, the 16^3, the lower 4^3, the 2^3
    p = np.array([[12, 8, 11], [17, 17, 3], [8, 16, 20], [1, 2, 3], [21, 5, 7]], I)
    return flat.reshape(32, 32, 32), [("set_voxels", dict(positions=p, materials=np.zeros(5, I))),
                                      ("set_voxels", dict(positions=p[:2], materials=np.array([6, 5], I)))], (desc, root)


def _emptied(dim):
    return sparse_grid(dim, dim + 1), [("fill_boxes", dict(lo=np.zeros((1, 3), I), size=(dim,) * 3, materials=0))]


def _regrown32():
    g, steps = _emptied(32)
    return g, steps + [("set_voxels", dict(positions=np.array([[9, 3, 12]], I), materials=np.array([7], I))),
                       ("fill_boxes", dict(lo=np.zeros((1, 3), I), size=(32, 32, 2), materials=5))]


STAGE = ((14, 14, 3), (5, 5, 9))                                # lo, size of the box both cameras of loop32 look at


def _loop32():
    """twelve generations: a small batch -- points, boxes, shapes, a pasted block, in turn --, vrc_prepare, a frame; a compaction
    after generations 4 and 9.  Besides its random part every batch rewrites the stage, in another form and another material than
    the generation before: that is what the cameras see change."""
    rng = np.random.default_rng(3200)
    (sx, sy, sz), (wx, wy, wz) = STAGE
    steps = []
    for gen in range(12):
        kind, mat = gen % 4, int(MATERIALS[1 + gen % 3])
        top = sz + 3 + (5 * gen) % 7                            # the stage's height changes too
        if kind == 0:
            p, m = er.random_batch(rng, 32, n=300)
            ax = np.stack(np.meshgrid(np.arange(sx, sx + wx), np.arange(sy, sy + wy), np.arange(sz, sz + wz), indexing="ij"), axis=-1).reshape(-1, 3)
            p = np.concatenate([p, ax.astype(I)])
            m = np.concatenate([m, np.where(ax[:, 2] < top, mat, 0).astype(I)])
            steps.append(("set_voxels", dict(positions=p, materials=m)))
        elif kind == 1:
            lo = rng.integers(0, 24, size=(4, 3)).astype(I)
            size = rng.integers(3, 10, size=(4, 3)).astype(I)
            lo[2], size[2] = (sx, sy, sz), (wx, wy, wz)
            lo[3], size[3] = (sx + 1, sy, sz), (wx - 2, wy, top - sz)
            steps.append(("fill_boxes", dict(lo=lo, size=size, materials=np.array([0, 6, 0, mat], I))))
        elif kind == 2:
            c = rng.integers(4, 28, size=(2, 3))
            shapes = np.array([[shp.BALL, c[0, 0], c[0, 1], 4, 4, 0], [shp.CYLINDER_Z, c[1, 0], c[1, 1], 0, 2, 14],
                               [shp.CYLINDER_Z, sx + 2, sy + 2, sz, 4, wz], [shp.CYLINDER_Z, sx + 2, sy + 2, sz, 2, top - sz],
                               [shp.BALL, sx + 2, sy + 2, top, 1, 0]], I)
            steps.append(("fill_shapes", dict(shapes=shapes, materials=np.array([0, 7, 0, mat, -3], I))))
        else:
            block = rng.choice(MATERIALS, size=(2, wz, wy, wx)).astype(np.int8)
            block[1] = 0
            block[1, :top - sz, ::2, :] = mat                   # slats
            lo = rng.integers(0, 24, size=(2, 3)).astype(I)
            lo[0, 2], lo[1] = 1, (sx, sy, sz)
            steps.append(("write_regions", dict(lo=lo, data=block)))
        steps.append(("frame", {}))
        if gen + 1 in (4, 9):
            steps.append(("compact", {}))
    return sparse_grid(32, 33, 0.04), steps


NAMES = ("points64", "regions32", "shapes64", "leaves32", "emptied32", "emptied64", "regrown32", "compacted64", "compacted64-far",
         "compacted-empty32", "loop32", "loop32-reserve0")
EMPTIED = ("emptied32", "emptied64", "compacted-empty32")
LOOPS = ("loop32", "loop32-reserve0")
EDITED = ("points64", "regions32", "shapes64", "leaves32", "emptied32", "emptied64", "regrown32")      # the last step is an edit
COMPACTED = ("compacted64", "compacted64-far", "compacted-empty32")                                     # the last step is a compaction


@functools.lru_cache(maxsize=None)
def history(name):
    base = {"compacted64": "points64", "compacted64-far": "points64", "compacted-empty32": "emptied32", "loop32-reserve0": "loop32"}.get(name, name)
    cameras = CAMERA_VOXELS[base]
    settings, tree = (), None
    if base == "points64":
        g, steps = _points64()
    elif base == "regions32":
        g, steps = _regions32()
    elif base == "shapes64":
        g, steps = _shapes64()
    elif base == "leaves32":
        g, steps, tree = _leaves32()
    elif base in ("emptied32", "emptied64"):
        g, steps = _emptied(int(base[-2:]))
    elif base == "regrown32":
        g, steps = _regrown32()
    elif base == "loop32":
        g, steps = _loop32()
    else:
        raise KeyError(name)
    if name in COMPACTED:
        steps = steps + [("compact", {})]
    if name == "compacted64-far":
        settings = (("compact_near_reach", REACH_MIN),)
    if name == "loop32-reserve0":
        settings = (("edit_reserve", 0),)
    return History(name, g, steps, cameras, tree=tree, settings=settings)


def host_tree(grid_zyx):
    """the host builder's tree of a grid, with its materials attached: vrc.Octree"""
    import voxel_raycaster_amd as vrc
    flat = np.ascontiguousarray(grid_zyx, np.int8).reshape(-1)
    return vrc.Octree.Generate(flat, grid_zyx.shape[0], layout=vrc.LAYOUT_NO_PAGE_HEADERS).attach_materials_from_grid(flat)


def oracle_frame(h, camera, descriptors, root, lookup, attachments, mode=0, coarse=-1, light_count=1):
    """(image, hit records, counters) of the CPU oracle on any descriptor array, for camera (name, cam_dir, cam_pos) of history h"""
    import scenes
    from oracle import orc
    _, cam_dir, cam_pos = camera
    return orc.raycast(width=W, height=H, cam_dir=cam_dir, cam_pos=cam_pos, lights=h.lights, atlas=scenes.hash_atlas(), tile_dim=(16, 16),
                       descriptors=descriptors, root_index=root, octree_dim=h.dim, using_octree=0, max_distance=3 * h.dim, stepping_mode=mode,
                       coarse_log2=coarse, attachment_lookup=lookup, attachments=attachments, active_lights=light_count)


def oracle_on_grid(h, camera, grid_zyx, **kw):
    o = host_tree(grid_zyx)
    return oracle_frame(h, camera, o.descriptor_buffer, o.root_index, o.attachment_lookup, o.attachment_buffer, **kw)
