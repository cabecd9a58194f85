"""Face extraction (vrc_extract_faces), CPU side: the numpy replay of tests/face_replay.py -- the oracle the GPU tests compare
against -- checked against a voxel-by-voxel loop, against the partition property and on a hand-written case that pins the
list's order; the C symbols and their null-handle answer; the new kernels' resources in libvrc.so; the Python wrapper's
count-then-exact logic against a stub of the library."""
import ctypes as C
import os

import numpy as np
import pytest

import face_replay as fr
import voxel_raycaster_amd as vrc

FLAGS = [(False, False), (True, False), (False, True), (True, True)]
MATERIALS = np.array([0, 0, 0, 5, 6, 1, -2], np.int8)


def _grid(rng, shape, fill=None):
    if fill is None:
        return rng.choice(MATERIALS, size=shape)
    return np.where(rng.random(shape) < fill, rng.choice(MATERIALS[3:], size=shape), 0).astype(np.int8)


@pytest.mark.parametrize("shape", [(8, 8, 8), (11, 9, 13), (16, 16, 16)], ids=str)
def test_replay_equals_the_voxel_loop(shape):
    rng = np.random.default_rng(sum(shape))
    mat = _grid(rng, shape)
    cases = [((0, 0, 0), shape), ((-3, -3, -3), tuple(s + 6 for s in shape)), ((3, 5, 1), (7, 8, 9)), ((-2, 6, 7), (5, 1, 12)),
             ((shape[0] - 1, 0, 0), (4, 4, 4)), ((40, 0, 0), (3, 3, 3))]
    seen = 0
    for no_edge, stopping in FLAGS:
        for lo, size in cases:
            got = fr.region(mat, lo, size, no_edge, stopping)
            want = fr.brute_region(mat, lo, size, no_edge, stopping)
            assert np.array_equal(got, want), (lo, size, no_edge, stopping)
            seen += len(got)
        # what the flags mean, on the whole map: the edge faces are exactly those whose neighbour is outside, and a stopping-only
        # owner is 5 or 6
        f = fr.region(mat, (0, 0, 0), shape, no_edge, stopping)
        nb = f[:, :3].astype(np.int64)
        d = f[:, 3] & 0xff
        nb[np.arange(len(f)), d >> 1] += np.where(d & 1, 1, -1)
        outside = ((nb < 0) | (nb >= np.array(shape))).any(axis=1)
        assert outside.any() != no_edge
        if stopping:
            assert set(np.unique(f[:, 3] >> 8).tolist()) <= {5, 6}
    assert seen > 1000
    assert len(fr.region(mat, (40, 0, 0), (3, 3, 3))) == 0


def test_tiles_partition_the_map():
    """Regions that tile the map yield disjoint face sets whose union is the whole map's set: 11^3 tiles, shifted."""
    rng = np.random.default_rng(32)
    dim = 32
    mat = _grid(rng, (dim,) * 3, fill=0.3)
    for no_edge, stopping in FLAGS:
        whole = fr.region(mat, (0, 0, 0), (dim,) * 3, no_edge, stopping)
        g = np.arange(-8, dim, 11)
        lo = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.array([3, 5, 1])
        counts, tiles = fr.regions(mat, lo, (11, 11, 11), no_edge, stopping)
        assert (lo.min(axis=0) <= 0).all() and (lo.max(axis=0) + 11 >= dim).all()
        assert counts.sum() == len(tiles) == len(whole) > 5000
        rows = {tuple(r) for r in tiles.tolist()}
        assert len(rows) == len(tiles) and rows == {tuple(r) for r in whole.tolist()}


def test_the_order_key_on_two_bricks():
    mat = np.zeros((16, 8, 8), np.int8)
    mat[7, 0, 0], mat[8, 0, 0], mat[0, 1, 0] = 5, 6, -2
    a, b, c = 5 << 8, 6 << 8, 254 << 8
    want = ([(7, 0, 0, d | a) for d in (0, 2, 3, 4, 5)] + [(0, 1, 0, d | c) for d in range(6)]      # brick 0: y = 0 before y = 1
            + [(8, 0, 0, d | b) for d in (1, 2, 3, 4, 5)])                                             # then brick 1
    assert fr.region(mat, (0, 0, 0), (16, 8, 8)).tolist() == [list(r) for r in want]
    # a region that starts inside brick 0 counts its bricks from there, and owns only what lies in it
    assert fr.region(mat, (4, 0, 0), (8, 8, 8)).tolist() == [list(r) for r in want[:5] + want[11:]]
    assert fr.region(mat, (0, 0, 0), (16, 8, 8), no_map_edge=True).tolist() == [list(r) for r in (
        [(7, 0, 0, d | a) for d in (0, 3, 5)] + [(0, 1, 0, d | c) for d in (1, 2, 3, 5)] + [(8, 0, 0, d | b) for d in (1, 3, 5)])]
    assert fr.region(mat, (0, 0, 0), (16, 8, 8), stopping_only=True).tolist() == [list(r) for r in want[:5] + want[11:]]
    # z is the slowest key inside a brick, the brick's z the slowest of all
    mat = np.zeros((16, 16, 16), np.int8)
    for p in ((9, 0, 0), (0, 9, 0), (0, 0, 9), (2, 0, 1), (0, 1, 0), (0, 0, 1)):
        mat[p] = 5
    f = fr.region(mat, (0, 0, 0), (16, 16, 16))
    assert [tuple(r) for r in f[::6, :3].tolist()] == [(0, 1, 0), (0, 0, 1), (2, 0, 1), (9, 0, 0), (0, 9, 0), (0, 0, 9)]


def test_symbols_and_null_handle():
    lib = vrc.lib
    for name in ("vrc_extract_faces", "vrc_extract_faces_device"):
        assert hasattr(lib, name) and name in vrc.SIGNATURES
    lo = np.zeros((1, 3), np.int32)
    size = np.array([2, 2, 2], np.int32)
    counts = np.zeros(1, np.int64)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.vrc_extract_faces(None, ip(lo), 1, ip(size), 0, 0, counts.ctypes.data_as(C.POINTER(C.c_int64)), None, None) == 1
    assert lib.vrc_extract_faces_device(None, None, 1, ip(size), 0, 0, None, None, None) == 1
    for name in ("extract_faces", "extract_faces_device"):
        assert callable(getattr(vrc.CLCaster, name))
    assert C.sizeof(vrc.FacesInfo) == 32 and (vrc.FACES_NO_MAP_EDGE, vrc.FACES_STOPPING_ONLY) == (1, 2)


def test_face_kernels_have_no_scratch():
    """The face kernels are in libvrc.so's gfx950 code object and use no private segment."""
    import test_kernel_resources as tkr
    if not os.path.exists(os.path.join(tkr.LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    table = tkr.kernel_table()
    for kernel in ("face_count_kernel", "face_region_kernel", "face_emit_kernel"):
        names = [k for k in table if kernel in k]
        assert names, kernel + " missing from libvrc.so"
        for k in names:
            assert table[k]["private_segment_fixed_size"] == 0, (k, table[k])


class _StubLib:
    """vrc_extract_faces of a scene with `total` faces: records each call, fills counts, the list and the info as the library does."""

    def __init__(self, total):
        self.total, self.calls = total, []

    def vrc_extract_faces(self, h, lo, n, size, capacity, flags, counts, faces, info):
        self.calls.append((capacity, faces is None, flags))
        counts[0] = self.total
        for i in range(1, n):
            counts[i] = 0
        written = min(self.total, capacity)
        for i in range(4 * written):
            faces[i] = i
        out = info._obj
        out.truncated, out.faces_total, out.faces_written, out.seconds = int(self.total > capacity), self.total, written, 0.5
        return 0


def test_wrapper_counts_then_asks_for_exactly_that(monkeypatch):
    c = vrc.CLCaster.__new__(vrc.CLCaster)
    c._h, c._keep, c.last_status = None, {}, 0
    lo = np.zeros((2, 3), np.int32)
    stub = _StubLib(7)
    monkeypatch.setattr(vrc, "lib", stub)
    counts, faces, info = c.extract_faces(lo, (8, 8, 8), no_map_edge=True)
    assert stub.calls == [(0, True, 1), (7, False, 1)]
    assert counts.tolist() == [7, 0] and faces.shape == (7, 4) and faces.reshape(-1).tolist() == list(range(28))
    assert info == dict(truncated=0, faces_total=7, faces_written=7, seconds=0.5)
    stub.calls.clear()
    counts, faces, info = c.extract_faces(lo, (8, 8, 8), capacity=3, stopping_only=True)       # a given capacity: one call
    assert stub.calls == [(3, False, 2)] and faces.shape == (3, 4) and info["truncated"] == 1 and info["faces_written"] == 3
    stub.calls.clear()
    counts, faces, info = c.extract_faces(lo, (8, 8, 8), capacity=0)
    assert stub.calls == [(0, True, 0)] and faces.shape == (0, 4) and info["faces_total"] == 7 and info["truncated"] == 1
    empty = _StubLib(0)
    monkeypatch.setattr(vrc, "lib", empty)
    counts, faces, info = c.extract_faces(lo, (8, 8, 8))                                          # nothing to list: no second call
    assert empty.calls == [(0, True, 0)] and faces.shape == (0, 4) and counts.tolist() == [0, 0]
    with pytest.raises(vrc.VrcError):
        c.extract_faces(np.zeros((2, 2), np.int32), (8, 8, 8))
    with pytest.raises(vrc.VrcError):
        c.extract_faces(lo, (8, 8))
