"""Swept-box queries (vrc_sweep_boxes), CPU side: the numpy replay of tests/sweep_replay.py -- the oracle the GPU tests compare
against -- checked against an exact-rational brute force on dyadic sweeps, its invariants on general floats, hand cases for
every outcome, the C symbols and their null-handle answer, and the new kernels' resources in libvrc.so."""
import ctypes as C

import numpy as np

import box_replay as br
import sweep_replay as sr
import voxel_raycaster_amd as vrc

F = np.float32
SCALE = 16                                                        # dyadic inputs: multiples of 1 / 16


def _scene(dim=16, seed=0, density=0.08):
    rng = np.random.default_rng(seed)
    mat = np.where(rng.random((dim, dim, dim)) < density, rng.integers(1, 8, size=(dim, dim, dim)), 0).astype(np.int8)
    return mat


def _flt(rec):
    return rec[:, 2].copy().view(F)


# ---- exact-rational brute force -----------------------------------------------------------------------------------------------
# Times are fractions (num, den) of int64 with den >= 0; den = 0 is -inf (num < 0) or +inf (num > 0).  Compared by cross
# multiplication, so nothing is rounded.

def _gt(n1, d1, n2, d2):
    return n1 * d2 > n2 * d1


def _brute(vox, sweep):
    """vox (k, 3) counted voxels; sweep 9 floats, multiples of 1 / SCALE.  Per axis the translated box [o + t d, e + t d)
    overlaps voxel [v, v + 1) for t in an interval with ends inf_a < sup_a (for e = o: the voxel holding the point); the box
    touches the voxel over the intersection of the three, when that has positive length.  Returns ('solid', tied) when a
    voxel is overlapped at t = 0 (the box query's rule), ('hit', (num, den), tied, inf_n, inf_d) for the smallest start of
    contact in [0, 1), else ('free',)."""
    s = np.round(np.asarray(sweep, dtype=np.float64) * SCALE).astype(np.int64)
    assert np.array_equal(s / SCALE, np.asarray(sweep, dtype=np.float64))
    O, M, D = s[:3], s[3:6], s[6:]
    E = O + M
    V, W = vox * SCALE, (vox + 1) * SCALE
    k = len(vox)
    static = np.ones(k, dtype=bool)
    inf_n, inf_d = np.zeros((k, 3), np.int64), np.zeros((k, 3), np.int64)
    sup_n, sup_d = np.zeros((k, 3), np.int64), np.zeros((k, 3), np.int64)
    for a in range(3):
        now = ((V[:, a] < E[a]) & (W[:, a] > O[a])) if M[a] > 0 else ((V[:, a] <= O[a]) & (O[a] < W[:, a]))
        static &= now
        if D[a] > 0:
            inf_n[:, a], inf_d[:, a], sup_n[:, a], sup_d[:, a] = V[:, a] - E[a], D[a], W[:, a] - O[a], D[a]
        elif D[a] < 0:
            inf_n[:, a], inf_d[:, a], sup_n[:, a], sup_d[:, a] = O[a] - W[:, a], -D[a], E[a] - V[:, a], -D[a]
        else:
            inf_n[:, a], sup_n[:, a] = np.where(now, -1, 1), np.where(now, 1, -1)
    if static.any():
        return ("solid", vox[static])
    # the latest start and the earliest end over the axes, then over [0, 1)
    bn, bd = np.zeros(k, np.int64), np.ones(k, np.int64)         # max(inf, 0)
    en, ed = np.ones(k, np.int64), np.ones(k, np.int64)          # min(sup, 1)
    for a in range(3):
        g = _gt(inf_n[:, a], inf_d[:, a], bn, bd)
        bn, bd = np.where(g, inf_n[:, a], bn), np.where(g, inf_d[:, a], bd)
        g = _gt(en, ed, sup_n[:, a], sup_d[:, a])
        en, ed = np.where(g, sup_n[:, a], en), np.where(g, sup_d[:, a], ed)
    touch = _gt(en, ed, bn, bd)
    if not touch.any():
        return ("free",)
    idx = np.nonzero(touch)[0]
    best = idx[0]
    for i in idx[1:]:
        if _gt(bn[best], bd[best], bn[i], bd[i]):
            best = i
    tied = idx[(bn[idx] * bd[best] == bn[best] * bd[idx])]
    return ("hit", (int(bn[best]), int(bd[best])), vox[tied], inf_n[tied], inf_d[tied])


def _dyadic_sweeps(rng, n, dim):
    q = lambda x: np.round(x * SCALE) / SCALE
    o = q(rng.uniform(-2, dim + 2, size=(n, 3)))
    m = q(rng.uniform(0, 3, size=(n, 3)) ** 2)
    d = q(rng.normal(0, 5, size=(n, 3)))
    kind = rng.integers(0, 8, size=n)
    k = np.nonzero(kind == 0)[0]
    m[k, rng.integers(0, 3, size=len(k))] = 0                     # planes, lines
    k = kind == 1
    m[k] = 0                                                      # points
    k = np.nonzero(kind == 2)[0]
    d[k, rng.integers(0, 3, size=len(k))] = 0
    k = np.nonzero(kind == 3)[0]
    for a in range(3):
        d[k[rng.integers(0, 2, size=len(k)) == 0], a] = 0         # several zero components, none moving among them
    k = kind == 4
    o[k], m[k], d[k] = np.floor(o[k]), np.floor(m[k]), np.round(d[k])     # integers: resting contacts and ties
    k = kind == 5
    o[k] = np.floor(o[k])
    m[k] = 0                                                      # points on the lattice
    return np.concatenate([o, m, d], axis=1).astype(F)


def test_replay_equals_exact_brute_force_on_dyadic_sweeps():
    """2 400 seeded sweeps whose components are multiples of 1 / 16 below 64, so o + m, the subtractions from integer bounds and
    the sign flips are exact in float32 and an event time is the correctly rounded quotient of two integers below 2^11.  Two
    different such quotients below 1 differ by more than 2^-22, more than float32's spacing there, so rounding keeps their
    order and their ties; the brute force's fraction, divided in float64 and rounded to float32, is the replay's t bit for
    bit (the float64 quotient of such integers is never within 2^-53 of a float32 midpoint without being one)."""
    dim = 16
    total = dict(solid=0, hit=0, free=0)
    for seed, stopping in ((1, False), (2, True), (3, False)):
        mat = _scene(dim, seed)
        scene = sr.GridScene(mat, stopping)
        cnt = ((mat == 5) | (mat == 6)) if stopping else (mat != 0)
        vox = np.argwhere(cnt).astype(np.int64)
        sweeps = _dyadic_sweeps(np.random.default_rng(10 + seed), 800, dim)
        rec = sr.sweep_replay(scene, sweeps, max_events=100000)
        t = _flt(rec)
        for i, s in enumerate(sweeps):
            b = _brute(vox, s)
            total[b[0]] += 1
            assert not rec[i, 0] & (sr.REJECTED | sr.EVENT_CAP), (s, rec[i])
            if b[0] == "solid":
                assert rec[i, 0] & sr.START_SOLID and not rec[i, 0] & sr.HIT and t[i] == 0 and rec[i, 1] == 0 and rec[i, 7] == 0, (s, rec[i])
                assert (b[1] == rec[i, 3:6]).all(axis=1).any(), (s, rec[i])
                assert rec[i, 6] == mat[tuple(rec[i, 3:6])]
            elif b[0] == "hit":
                assert rec[i, 0] & sr.HIT and not rec[i, 0] & sr.START_SOLID, (s, rec[i], b[1])
                assert t[i] == F(b[1][0] / b[1][1]), (s, rec[i], b[1])
                where = np.nonzero((b[2] == rec[i, 3:6]).all(axis=1))[0]
                assert len(where) == 1, (s, rec[i], b[2])
                a = abs(int(rec[i, 1])) - 1                       # the face: an axis whose contact starts at t, against the motion
                assert rec[i, 1] != 0 and np.sign(rec[i, 1]) == -np.sign(s[6 + a])
                assert b[3][where[0], a] * b[1][1] == b[1][0] * b[4][where[0], a] or (b[1][0] == 0 and b[3][where[0], a] <= 0)
                assert rec[i, 6] == mat[tuple(rec[i, 3:6])]
            else:
                assert not rec[i, 0] & (sr.HIT | sr.START_SOLID) and t[i] == 1 and rec[i, 1] == 0 and (rec[i, 3:7] == (-1, -1, -1, 0)).all(), (s, rec[i])
    assert min(total.values()) > 150, total


def test_invariants_on_general_floats():
    dim = 32
    mat = _scene(dim, 4, 0.02)
    scene = sr.GridScene(mat)
    sweeps = sr.random_sweeps(np.random.default_rng(7), 4000, dim)
    trace = {}
    rec = sr.sweep_replay(scene, sweeps, max_events=1 << 30, trace=trace)
    ok = (rec[:, 0] & sr.REJECTED) == 0
    assert ok.sum() > 3500 and (~ok).sum() >= 6
    assert (trace["min_width"][ok] >= 0).all()                    # the range never inverts
    bound = 2 * (np.ceil(np.abs(sweeps[:, 6:].astype(np.float64))) + 1).sum(axis=1)
    assert (rec[ok, 7] <= bound[ok]).all()
    t = _flt(rec)
    hit = (rec[:, 0] & sr.HIT) != 0
    assert hit.sum() > 500 and (t[hit] >= 0).all() and (t[hit] < 1).all()
    assert (rec[hit, 1] != 0).all() and (rec[hit, 3:6] >= 0).all() and (rec[hit, 6] != 0).all()
    free = ok & ~hit & ((rec[:, 0] & (sr.START_SOLID | sr.EVENT_CAP)) == 0)
    assert (t[free] == 1).all() and (rec[free, 3:6] == -1).all()
    assert (rec[~ok] == np.array([sr.REJECTED, 0, 0, -1, -1, -1, 0, 0])).all()
    # the default cap is never reached by a sweep that stays near the map
    assert not (sr.sweep_replay(scene, sweeps)[:, 0] & sr.EVENT_CAP).any()


def _floor_scene(dim=16):
    """A floor z < 4, a one-voxel wall at x = 10 (material 3), a pillar of material 6 at (2, 2)."""
    mat = np.zeros((dim, dim, dim), np.int8)
    mat[:, :, :4] = 5
    mat[10, :, 4:] = 3
    mat[2, 2, 4:9] = 6
    return mat


def _one(scene, *sweep, max_events=0):
    rec = sr.sweep_replay(scene, np.array([sweep], dtype=F), max_events=max_events)[0]
    return rec, rec[2:3].copy().view(F)[0]


def test_hand_cases():
    scene = sr.GridScene(_floor_scene())
    # resting on the floor, moving down: stopped at once by the face below, normal +z
    rec, t = _one(scene, 5, 5, 4, 1, 1, 2, 0, 0, -1)
    assert rec.tolist() == [sr.HIT, 3, 0, 5, 5, 3, 5, 1] and t == 0
    # the same box moving sideways along the floor is free
    rec, t = _one(scene, 5, 5, 4, 1, 1, 2, 2.5, 1.25, 0)
    assert rec[0] == 0 and t == 1 and rec[1] == 0 and rec[3:7].tolist() == [-1, -1, -1, 0] and rec[7] > 0
    # ... and stops at the wall: leading face 6 + 0.5 t' = 10
    rec, t = _one(scene, 5, 5, 4, 1, 1, 2, 8, 0, 0)
    assert rec[0] == sr.HIT and rec[1] == -1 and t == F(0.5) and rec[3:7].tolist() == [10, 5, 4, 3]
    # a one-voxel wall between start and end is hit however long the step (no tunnelling), from either side
    rec, t = _one(scene, 8.25, 5, 6, 0.5, 0.5, 0.5, 6, 0, 0)
    assert rec[0] == sr.HIT and rec[1] == -1 and t == F(1.25) / F(6) and rec[3] == 10
    rec, t = _one(scene, 12.5, 5, 6, 0.5, 0.5, 0.5, -8, 0, 0)
    assert rec[0] == sr.HIT and rec[1] == 1 and t == F(1.5) / F(8) and rec[3] == 10
    # the wall is material 3: it does not block with stopping_only, the pillar (6) does
    stop = sr.GridScene(_floor_scene(), stopping_only=True)
    rec, t = _one(stop, 8.25, 5, 6, 0.5, 0.5, 0.5, 6, 0, 0)
    assert rec[0] == 0 and t == 1
    rec, t = _one(stop, 2.25, 6.5, 6, 0.5, 0.5, 0.5, 0, -8, 0)
    assert rec[0] == sr.HIT and rec[1] == 2 and rec[3:7].tolist() == [2, 2, 6, 6] and t == F(3.5) / F(8)
    # starting inside: the first counted voxel of the start range in Morton order
    rec, t = _one(scene, 4.5, 4.5, 3.5, 1, 1, 1, 1, 0, 0)
    assert rec.tolist() == [sr.START_SOLID, 0, 0, 4, 4, 3, 5, 0]
    # a diagonal fall onto the floor: z reaches 4 at t = 0.5, before x changes anything
    rec, t = _one(scene, 5.25, 5.25, 6, 0.5, 0.5, 1, 1, 1, -4)
    assert rec[0] == sr.HIT and rec[1] == 3 and t == F(0.5) and rec[5] == 3
    # leaving the map: free, and nothing more is examined
    rec, t = _one(scene, 14, 5, 8, 1, 1, 1, 500, 0, 0)
    assert rec[0] == sr.LEFT_MAP | sr.CLIPPED and t == 1 and rec[7] <= 4
    rec, t = _one(scene, -9, 5, 8, 1, 1, 1, -1, 0, 0)
    assert rec[0] == sr.LEFT_MAP | sr.CLIPPED and rec[7] == 0
    rec, t = _one(scene, -9, 5, 8, 1, 1, 1, 12.5, 0, 0)              # from outside onto the map
    assert rec[0] == sr.CLIPPED and t == 1
    # the event cap: t of the last processed event
    rec, t = _one(scene, 5.5, 5, 8, 1, 1, 1, 3, 0, 0, max_events=3)
    assert rec[0] == sr.EVENT_CAP and rec[7] == 3 and t == F(1.5) / F(3)     # leading 7, trailing 5 (0.5 / 3), leading 8 (1.5 / 3)
    rec, t = _one(scene, 5.5, 5, 8, 1, 1, 1, 3, 0, 0, max_events=7)
    assert rec[0] == 0 and t == 1 and rec[7] == 6
    # the default cap: 2 * 48 + 64 events
    rec, t = _one(sr.GridScene(np.zeros((16, 16, 16), np.int8)), -2.0 ** 20, 5, 5, 2.0 ** 21, 1, 1, 1000, 0, 0)
    assert rec[0] == sr.EVENT_CAP | sr.CLIPPED and rec[7] == 160 and t == F(80) / F(1000)    # (larger than the map: it never leaves)
    rec, t = _one(sr.GridScene(np.zeros((16, 16, 16), np.int8)), 2, 5, 5, 1, 1, 1, 5000, 0, 0)
    assert rec[0] & sr.LEFT_MAP
    rec, t = _one(sr.GridScene(np.zeros((16, 16, 16), np.int8)), 2, 5, 5, 1, 1, 1, 8, 1e-3, 1e-3, max_events=0)
    assert rec[0] == 0 and rec[7] == 17                                     # x: layers 3 .. 10 entered, 2 .. 8 left; y and z: one layer entered at t = 0


def test_each_rejection():
    scene = sr.GridScene(_floor_scene())
    good = [5, 5, 6, 1, 1, 1, 1, 0, 0]
    bad = []
    for i, v in ((0, np.nan), (1, np.inf), (3, -1.0), (4, np.nan), (5, np.inf), (6, np.nan), (7, np.inf), (8, -np.inf), (0, 2.0 ** 30), (2, -2.0 ** 30),
                 (6, 2.0 ** 30), (8, -2.0 ** 30), (3, 2.0 ** 30)):
        s = list(good)
        s[i] = v
        bad.append(s)
    bad.append([2.0 ** 29, 5, 6, 1, 1, 1, 2.0 ** 29, 0, 0])                 # o + d = 2^30
    bad.append([5, 5, -2.0 ** 29, 1, 1, 1, 0, 0, -2.0 ** 29])
    rec = sr.sweep_replay(scene, np.array(bad, dtype=F))
    assert (rec == np.array([sr.REJECTED, 0, 0, -1, -1, -1, 0, 0])).all(), rec
    ok = np.array([[2.0 ** 29, 5, 6, 1, 1, 1, 2.0 ** 28, 0, 0], [5, 5, 6, 1, 1, 1, -0.0, 0, 0], [5, 5, 6, 0, 0, 0, 0, 0, 0]], dtype=F)
    rec = sr.sweep_replay(scene, ok)
    assert not (rec[:, 0] & sr.REJECTED).any() and rec[0, 0] == sr.LEFT_MAP | sr.CLIPPED and rec[1, 0] == 0 and rec[2, 0] == 0


def test_subnormal_components():
    """A subnormal displacement component is a moving axis whose events lie beyond t = 1 (or at t = 0 for a resting face)."""
    scene = sr.GridScene(_floor_scene())
    tiny = F(1e-41)
    assert tiny != 0 and tiny < np.finfo(F).tiny
    rec, t = _one(scene, 5.5, 5.5, 6.5, 1, 1, 1, tiny, -tiny, tiny)
    assert rec[0] == 0 and t == 1 and rec[7] == 0
    rec, t = _one(scene, 5, 5, 4, 1, 1, 1, 0, 0, -tiny)                     # resting, pressed down by a subnormal
    assert rec.tolist() == [sr.HIT, 3, 0, 5, 5, 3, 5, 1]
    rec, t = _one(scene, 5, 5, 4, 1, 1, 1, tiny, 0, 0)                       # leading face on the lattice: enters layer 6 at t = 0
    assert rec[0] == 0 and t == 1 and rec[7] == 1
    rec, t = _one(scene, 9, 5, 4, 1, 1, 1, tiny, 0, 0)                       # ... and that layer is the wall
    assert rec[0] == sr.HIT and rec[1] == -1 and t == 0 and rec[3] == 10
    rec, t = _one(scene, tiny, 5, 4, 1, 1, 1, -1, 0, 0)                      # a subnormal origin: (o - 0) / 1 is that subnormal
    assert rec[0] == sr.CLIPPED and t == 1 and rec[7] >= 1


def test_symbols_and_null_handle():
    lib = vrc.lib
    for name in ("vrc_sweep_boxes", "vrc_sweep_boxes_device"):
        assert hasattr(lib, name) and name in vrc.SIGNATURES
    s, r = np.zeros((1, 9), F), np.zeros((1, 8), np.int32)
    assert lib.vrc_sweep_boxes(None, s.ctypes.data_as(C.POINTER(C.c_float)), 1, 0, 0, r.ctypes.data_as(C.POINTER(C.c_int32))) == 1
    assert lib.vrc_sweep_boxes_device(None, None, 1, 0, 0, None) == 1
    assert (vrc.SWEEP_STOPPING_ONLY, vrc.SWEEP_HIT, vrc.SWEEP_START_SOLID, vrc.SWEEP_CLIPPED, vrc.SWEEP_REJECTED, vrc.SWEEP_EVENT_CAP,
            vrc.SWEEP_LEFT_MAP) == (1, 1, 2, 4, 8, 16, 32)
    assert (sr.HIT, sr.START_SOLID, sr.CLIPPED, sr.REJECTED, sr.EVENT_CAP, sr.LEFT_MAP) == (1, 2, 4, 8, 16, 32)
    assert hasattr(vrc.CLCaster, "sweep_boxes") and hasattr(vrc.CLCaster, "sweep_boxes_device")


def test_sweep_kernels_have_no_scratch():
    """The sweep kernels are in libvrc.so's gfx950 code object and use no private segment (stackless walks, unrolled axes); the
    box-query kernels they share the walk with still use none either."""
    import test_kernel_resources as tkr
    table = tkr.kernel_table()
    for kernel in ("box_sweep_plan_kernel", "box_sweep_lane_kernel", "box_sweep_wave_kernel", "box_query_count_kernel"):
        names = [k for k in table if kernel in k]
        assert names, kernel + " missing from libvrc.so"
        for k in names:
            assert table[k]["private_segment_fixed_size"] == 0, (k, table[k])
