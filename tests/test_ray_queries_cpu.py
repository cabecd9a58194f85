"""Ray queries (vrc_cast_rays), CPU side: the numpy replay of tests/ray_replay.py -- the oracle the GPU tests compare against --
checked against the CPU oracle's own frames (each ray rendered as a 1 x 1 frame), and the query kernel's resources in libvrc.so."""
import os

import numpy as np
import pytest

import ray_replay
import scenes
from oracle import orc

MAKERS = scenes.ALL + [scenes.terrain256]


@pytest.fixture(scope="module")
def scene_trees():
    out = {}
    for make in MAKERS:
        s = make()
        buf, root = orc.octree_generate(s["grid"], s["dim"], buffer_size=200000)
        out[s["name"]] = (s, buf, root)
    return out


def _rays(rng, s, n):
    r = ray_replay.random_rays(rng, n, s["dim"])
    # a few rays from the scene's camera (picking-like), and origins on exact voxel boundaries
    r[: n // 8, :3] = np.asarray(s["cam_pos"], dtype=np.float32)
    r[n // 8: n // 4, :3] = np.floor(r[n // 8: n // 4, :3])
    return r


@pytest.mark.parametrize("as_pixel", [False, True])
@pytest.mark.parametrize("name", [m().get("name") if m is not scenes.terrain256 else "terrain256" for m in MAKERS])
def test_replay_equals_oracle_frames(scene_trees, atlas, name, as_pixel):
    s, buf, root = scene_trees[name]
    rng = np.random.default_rng(1000 + len(name) + (7 if as_pixel else 0))
    n = 500 if name == "terrain256" else 400
    rays = _rays(rng, s, n)
    dim = s["dim"]
    for max_steps in (0, 7):
        bias = ray_replay.origin_bias(rays[:, :3], buf, root, dim) if as_pixel else None
        for using_octree in (0, 1):
            mat = s["grid"] if using_octree else np.where(np.asarray(s["grid"]) != 0, 5, 0).astype(np.int8)
            got = ray_replay.replay(rays, mat, (dim,) * 3, max_steps=max_steps, as_pixel=as_pixel, bias=bias)
            # the frame rejects every zero component: in the default mode only the rays without one have a 1 x 1 frame to compare with
            sel = np.ones(len(rays), bool) if as_pixel else ~(rays[:, 3:] == 0).any(axis=1)
            ref = ray_replay.oracle_records(rays[sel], scene=s, descriptors=buf, root_index=root, using_octree=using_octree,
                                            max_steps=max_steps, as_pixel=as_pixel, atlas=atlas)
            g = got[sel]
            assert np.array_equal(g[:, :5], ref[:, :5]), (name, max_steps, using_octree, np.nonzero((g[:, :5] != ref[:, :5]).any(1))[0][:5])
            mirror = g[:, 3] == 6
            assert np.array_equal(g[~mirror, 6], ref[~mirror, 6])
            # the frame's unwritten pixels are exactly the rejected rays
            assert np.array_equal(g[:, 5] == ray_replay.REJECTED, (rays[sel, 3:] == 0).any(axis=1))
            assert ((g[:, 5] == ray_replay.HIT) == (g[:, 0] >= 0)).all()


def test_replay_zero_axes_never_step():
    """Default mode: a zero (or -0) component never steps; straight down from above the floor lands on it; the entry parameter
    of an axis-aligned unit ray is its distance to the face."""
    dim = 16
    g = np.zeros((dim, dim, dim), np.int8)
    g[0] = 5                                                   # the floor, z = 0
    rays = np.array([[3.5, 4.25, 9.5, 0.0, -0.0, -1.0],
                     [3.5, 4.25, 9.5, 0.0, 0.0, -0.5],
                     [3.5, 4.25, 9.5, 1.0, 0.0, 0.0],
                     [3.5, 4.25, 9.5, 0.0, 0.0, 0.0],
                     [3.5, 4.25, 9.5, np.nan, 0.0, 1.0]], np.float32)
    rec = ray_replay.replay(rays, g.reshape(-1), (dim,) * 3)
    assert rec[0].tolist()[:6] == [3, 4, 0, 5, 4, ray_replay.HIT] and rec[0, 6] == 8
    assert rec[0, 7] == np.float32(8.5).view(np.int32)         # t at the entering iteration: 9.5 - 1 face = 8.5
    assert rec[1, :6].tolist() == [3, 4, 0, 5, 4, ray_replay.HIT] and rec[1, 7] == np.float32(17.0).view(np.int32)
    assert rec[2, 5] == ray_replay.LEFT_MAP and rec[2, 6] == dim - 4
    assert rec[3, 5] == ray_replay.REJECTED and rec[4, 5] == ray_replay.REJECTED
    assert ray_replay.replay(rays[:1], g.reshape(-1), (dim,) * 3, max_steps=3)[0, 5] == ray_replay.STEP_CAP


def test_query_kernel_has_no_scratch():
    """raycast_query_kernel is in libvrc.so's gfx950 code object and uses no private segment (one lane per ray, a stackless
    re-descent per node event: no traversal stack)."""
    import test_kernel_resources as tkr
    if not os.path.exists(os.path.join(tkr.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    table = tkr.kernel_table()
    names = [k for k in table if "raycast_query_kernel" in k]
    assert names, "raycast_query_kernel missing from libvrc.so"
    for k in names:
        assert table[k]["private_segment_fixed_size"] == 0, (k, table[k])
