"""numpy restatement of the voxel edits (vrc_set_voxels, include/vrc.h): the edits applied IN INDEX ORDER to a dense material
grid int8[z][y][x] -- the block vrc_read_regions returns for the whole map --, so the highest index wins a position that occurs
more than once; an edit outside the grid is skipped and counted.  Also the random batches the tests share and the walk that
compares two descriptor arrays node by node.  The test oracle of tests/test_voxel_edits_*.py.  Not a test file."""
import numpy as np


def replay(grid_zyx, positions, materials):
    """(grid after the batch, skipped, voxels_changed): grid_zyx int8[dz, dy, dx] is not modified."""
    before = np.asarray(grid_zyx, dtype=np.int8)
    g = before.copy()
    p = np.asarray(positions, dtype=np.int64).reshape(-1, 3)
    m = np.asarray(materials, dtype=np.int64).reshape(-1)
    assert len(p) == len(m) and ((m >= -128) & (m <= 127)).all()
    dz, dy, dx = g.shape
    skipped = 0
    for (x, y, z), v in zip(p, m):                          # one by one on purpose: the order is the specification
        if 0 <= x < dx and 0 <= y < dy and 0 <= z < dz:
            g[z, y, x] = v
        else:
            skipped += 1
    return g, skipped, int(np.count_nonzero(g != before))


def random_batch(rng, dim, n=2000, materials=(5, 6, 7, -3), duplicates=0.10, outside=0.05, clears=0.5):
    """(positions (n, 3) int32, materials (n,) int32): random voxels of a dim^3 map, about `duplicates` of them repeating an
    earlier position of the batch (with another material as often as not), about `outside` of them outside the map on one axis
    or more, half of the materials 0."""
    p = rng.integers(0, dim, size=(n, 3))
    dup = np.nonzero(rng.random(n) < duplicates)[0]
    dup = dup[dup > 0]
    p[dup] = p[(rng.random(len(dup)) * dup).astype(np.int64)]
    out = np.nonzero(rng.random(n) < outside)[0]
    far = np.array([-1, dim, dim + 7, -9, 2 ** 31 - 1, -2 ** 31])
    for i in out:
        p[i, rng.integers(0, 3)] = far[rng.integers(0, len(far))]
    m = np.where(rng.random(n) < clears, 0, rng.choice(np.asarray(materials), size=n))
    return p.astype(np.int32), m.astype(np.int32)


def masks_by_position(desc, root, dim):
    """{(x, y, z, size): (valid, leaf)} of every descriptor the root reaches -- where a tree keeps its words does not enter."""
    d = [int(v) for v in np.asarray(desc).reshape(-1)]
    out, stack = {}, [(int(root), 0, 0, 0, int(dim))]
    while stack:
        index, x, y, z, size = stack.pop()
        v = d[index]
        valid, leaf = (v >> 16) & 0xff, (v >> 24) & 0xff
        assert (x, y, z, size) not in out
        out[(x, y, z, size)] = (valid, leaf)
        if size == 2:
            continue
        at = index + (v & 0x7fff)
        if v & 0x8000:
            at = d[at]
        half, rank = size // 2, 0
        for k in range(8):
            if valid >> k & 1:
                if not (leaf >> k & 1):
                    stack.append((at + rank, x + (half if k & 1 else 0), y + (half if k & 2 else 0), z + (half if k & 4 else 0), half))
                rank += 1
    return out


def touched_nodes(positions, dim):
    """(bricks, nodes above the bricks) a batch touches in a dim^3 tree: the growth bound's two counts."""
    p = np.asarray(positions, dtype=np.int64).reshape(-1, 3)
    p = p[((p >= 0) & (p < dim)).all(axis=1)]
    bricks = {tuple(v) for v in (p >> 3)}
    above, level, size = 0, bricks, 8
    while size < dim:
        level = {(x >> 1, y >> 1, z >> 1) for x, y, z in level}
        above += len(level)
        size *= 2
    return len(bricks), above
