"""CPU suite: tests/relayout.py gives the same tree in another array -- far pointers, a root in the middle, child blocks before
their parents, filler words between blocks -- and the host code and the oracle do not care.  The GPU suite
(tests/test_layouts_gpu.py) puts such arrays under every tree-walking kernel; this file checks the inputs themselves:

* the re-laid array is the same tree (treetools.canonical), has far pointers (all parents at far_fraction = 1), and
  Octree.GetVoxel, the material attachments, Octree.Save / Load and the oracle's frames (image bits, all eight hit columns, all
  counters, both stepping modes, with and without attachments) do not change with the layout;
* SENSITIVITY: read with the far bit ignored, or from index 0 instead of the root, every re-laid array gives another material
  grid or does not decode at all -- so a kernel that forgets far pointers or the root setting cannot pass on these inputs."""
import functools

import numpy as np
import pytest

import relayout as rl
import scenes
import treetools
import voxel_raycaster_amd as vrc
from oracle import orc

FRACTIONS = (0.0, 0.5, 1.0)

def _small_map(dim):
    rng = np.random.default_rng(100 + dim)
    return rng.choice(np.array([0, 5, 6, -3], np.int8), size=dim ** 3, p=[0.5, 0.3, 0.15, 0.05])


def _trees():
    out = {}
    for make in scenes.ALL:
        s = make()
        g = rl.with_materials(s["grid"], s["dim"])
        for name, layout in (("brick", 2), ("paged", None)):
            out[f"{s['name']}-{name}"] = (lambda g=g, s=s, layout=layout: (vrc.Octree.Generate(g, s["dim"], layout=layout), g, s))
    for dim in (2, 4, 8):
        s = dict(scenes.floor_pillars(32), dim=dim, cam_pos=(dim * 0.5 + 0.37, -1.59, dim * 0.45 + 0.29))
        g = _small_map(dim)
        out[f"generate{dim}"] = (lambda g=g, s=s, dim=dim: (vrc.Octree.Generate(g, dim), g, s))

    def leaves():
        desc, root, g = rl.leaf_tree()
        return vrc.Octree(desc, root, 32), g, dict(scenes.floor_pillars(32))
    out["leaf_octree32"] = leaves
    return out


TREES = _trees()


@functools.lru_cache(maxsize=None)
def _case(name):
    """The tree with its attachments, its material grid, the scene, and its three re-laid arrays (one seed per far_fraction)."""
    o, g, s = TREES[name]()
    o.attach_materials_from_grid(g)
    dim = o.dim
    sig, (nodes, far) = treetools.canonical(o.descriptor_buffer, o.root_index, dim)
    relaid = []
    for k, ff in enumerate(FRACTIONS):
        for seed in range(1000 * dim + 7 * k + len(name), 1 << 30):
            d2, r2, l2 = rl.relayout(o.descriptor_buffer, o.root_index, dim, np.random.default_rng(seed), ff, o.attachment_lookup)
            # (a 4^3 tree has one parent: at far_fraction 0 the next seed is taken until its block lies behind it)
            if dim == 2 or treetools.canonical(d2, r2, dim)[1][1] > 0:
                break
        o2 = vrc.Octree(d2, r2, dim)
        o2.attachment_lookup, o2.attachment_buffer = l2, o.attachment_buffer
        relaid.append(o2)
    return o, g, s, sig, nodes, far, relaid


@pytest.mark.parametrize("name", list(TREES))
def test_the_relaid_array_is_the_same_tree(name):
    o, g, s, sig, nodes, far0, relaid = _case(name)
    dim = o.dim
    parents = rl.parents_with_children(o.descriptor_buffer, o.root_index, dim)
    assert far0 == 0 and (parents > 0) == (dim > 2)
    assert np.array_equal(rl.decode(o.descriptor_buffer, o.root_index, dim, o.attachment_lookup, o.attachment_buffer), g)
    for ff, o2 in zip(FRACTIONS, relaid):
        sig2, (nodes2, far) = treetools.canonical(o2.descriptor_buffer, o2.root_index, dim)
        assert sig2 == sig and nodes2 == nodes, (name, ff)
        # a 2^3 map is one bottom-level word: it holds no pointer at all
        assert (far > 0) == (parents > 0) and far <= parents, (name, ff, far, parents)
        if ff == 1.0:
            assert far == parents
        assert o2.root_index != 0 and o2.descriptor_buffer.size > o.descriptor_buffer.size
        print(f"{name} far_fraction {ff}: {o.descriptor_buffer.size} -> {o2.descriptor_buffer.size} words, root {o2.root_index}, "
              f"{far} far pointers of {parents} parents")


@pytest.mark.parametrize("name", list(TREES))
def test_sensitivity_to_the_far_bit_and_the_root(name):
    """Without this the inputs could not catch a kernel that ignores far pointers or the root setting."""
    o, g, s, sig, nodes, far0, relaid = _case(name)
    dim = o.dim
    for ff, o2 in zip(FRACTIONS, relaid):
        args = (o2.descriptor_buffer, o2.root_index, dim, o2.attachment_lookup, o2.attachment_buffer)
        assert np.array_equal(rl.decode(*args), g), (name, ff)
        wrong = []
        if dim > 2:
            wrong.append(("far bit ignored", lambda: rl.decode(*args, ignore_far=True)))
        wrong.append(("root 0", lambda: rl.decode(o2.descriptor_buffer, 0, dim, o2.attachment_lookup, o2.attachment_buffer)))
        for what, read in wrong:
            try:
                got = read()
            except IndexError:
                continue
            assert not np.array_equal(got, g), (name, ff, what)
            # ... and not only in the materials, unless the map is solid throughout (app_default: any all-solid word at index 0
            # decodes to its occupancy; its materials still tell)
            assert not np.array_equal(got != 0, g != 0) or (g != 0).all(), (name, ff, what)


@pytest.mark.parametrize("name", list(TREES))
def test_get_voxel_attachments_and_files(name, tmp_path):
    o, g, s, sig, nodes, far0, relaid = _case(name)
    dim = o.dim
    if dim <= 32:
        ax = np.arange(dim)
        pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    else:
        pts = np.random.default_rng(dim).integers(0, dim, size=(4000, 3))
    want = [o.GetVoxel(p) for p in pts]
    solid = g.reshape(dim, dim, dim)[pts[:, 2], pts[:, 1], pts[:, 0]] != 0
    assert [w[0] for w in want] == solid.tolist()
    for ff, o2 in zip(FRACTIONS, relaid):
        assert [o2.GetVoxel(p) for p in pts] == want, (name, ff)
        # attachments built on the re-laid array itself: the same material byte for every bottom-level descriptor
        own = vrc.Octree(o2.descriptor_buffer, o2.root_index, dim).attach_materials_from_grid(g)
        bottom = np.nonzero(o2.attachment_lookup)[0]
        assert bottom.size == np.count_nonzero(o.attachment_lookup) == np.count_nonzero(own.attachment_lookup)
        assert np.array_equal(own.attachment_buffer[own.attachment_lookup[bottom]], o2.attachment_buffer[o2.attachment_lookup[bottom]])
        assert np.array_equal(np.nonzero(own.attachment_lookup)[0], bottom)
        path = str(tmp_path / f"relaid_{ff}.oct")
        o2.Save(path)
        back = vrc.Octree.Load(path)
        assert back.root_index == o2.root_index and back.dim == dim
        assert np.array_equal(back.descriptor_buffer, o2.descriptor_buffer)
        assert np.array_equal(back.attachment_lookup, o2.attachment_lookup) and np.array_equal(back.attachment_buffer, o2.attachment_buffer)


@pytest.mark.parametrize("name", list(TREES))
def test_the_oracle_renders_the_same_frame(name, atlas):
    """Image bits, all eight hit columns and all counters: no column and no counter of the oracle depends on the layout."""
    o, g, s, sig, nodes, far0, relaid = _case(name)
    dim = o.dim
    li = np.zeros((8, 10), dtype=np.float32)
    li[:1] = np.asarray(s["lights"], np.float32).reshape(-1, 10)[:1]

    def frame(t, attached, mode):
        kw = dict(attachment_lookup=t.attachment_lookup, attachments=t.attachment_buffer) if attached else {}
        return orc.raycast(width=64, height=48, cam_dir=s["cam_dir"], cam_pos=s["cam_pos"], lights=li, atlas=atlas, tile_dim=(16, 16),
                           descriptors=t.descriptor_buffer, root_index=t.root_index, octree_dim=dim, using_octree=0,
                           max_distance=3 * dim, stepping_mode=mode, **kw)

    for attached in (False, True):
        for mode in (0, 1):
            img, hits, ctr = frame(o, attached, mode)
            assert ctr["primary_rays"] > 0
            for ff, o2 in zip(FRACTIONS, relaid):
                img2, hits2, ctr2 = frame(o2, attached, mode)
                assert np.array_equal(img2.view(np.uint32), img.view(np.uint32)), (name, attached, mode, ff)
                assert np.array_equal(hits2, hits), (name, attached, mode, ff)
                assert ctr2 == ctr, (name, attached, mode, ff)
