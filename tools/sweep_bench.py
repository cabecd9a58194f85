"""Swept-box query times (vrc_sweep_boxes_device, csrc/box_sweep.hip) on the depth-12 bench scene, device-built, with the coarse
table built by validate: (a) 1 M player-sized sweeps of 0.6 x 0.6 x 1.8 starting just above the surface, moving a voxel or two
sideways and down; (b) 4096 sweeps of 64 x 64 x 8 slabs (64 x 64 faces) lowered onto the terrain.  Beside each, the time of
vrc_box_intersection_device(max_voxels = 1) on the same start boxes -- the part of the work a sweep reuses.  --box-only measures
just that (a library without the sweep entry points can be measured with this script: --root names its tree).  --crossover times
--crossover-n sweeps (default 65 536) per face size with every sweep forced into the lane shape, then the wave shape (setting sweep_lane_face).
Each figure: hip events around the device-pointer call, the median of --reps calls after 2 warm-ups.
Usage: python tools/sweep_bench.py [--depth 12] [--reps 10] [--box-only] [--crossover [--crossover-n N] [--no-legs]] [--root DIR] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

F = np.float32


def surface_sweeps(vrc, rng, depth, n, ext, drop, cols=4096):
    """n sweeps of extent `ext` whose lower face starts 1 .. 3 voxels above the highest of 16 columns sampled under the box,
    at fractional (x, y), moving (N(0, 1.5), N(0, 1.5), -U(0.5, drop)): the heights of `cols` random places, reused."""
    dim = 1 << depth
    xy = rng.uniform(0, dim - ext[0] - 2, size=(cols, 2))
    top = np.zeros(cols)
    for i, (x, y) in enumerate(xy):
        top[i] = max(vrc.shell_column(depth, int(x + fx * ext[0]), int(y + fy * ext[1]))[1] for fx in (0, 0.33, 0.67, 1) for fy in (0, 0.33, 0.67, 1))
    pick = rng.integers(0, cols, size=n)
    jitter = rng.uniform(0, 1, size=(n, 2))
    o = np.stack([xy[pick, 0] + jitter[:, 0], xy[pick, 1] + jitter[:, 1], top[pick] + 2 + rng.uniform(0, 2, n)], axis=1)
    d = np.stack([rng.normal(0, 1.5, n), rng.normal(0, 1.5, n), -rng.uniform(0.5, drop, n)], axis=1)
    return np.concatenate([o, np.broadcast_to(np.asarray(ext, np.float64), (n, 3)), d], axis=1).astype(F)


def timed(call, reps):
    for _ in range(2):
        assert call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--box-only", action="store_true")
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--crossover-n", type=int, default=1 << 16, help="sweeps per face size of --crossover")
    ap.add_argument("--no-legs", action="store_true", help="only --crossover")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import bench
    import voxel_raycaster_amd as vrc

    sc = bench.device_scene_header(args.depth)
    c = bench.make_caster(sc, 256, 144, 0)
    rng = np.random.default_rng(1)
    legs = [] if args.no_legs else [("a_player_1M", surface_sweeps(vrc, rng, args.depth, 1 << 20, (0.6, 0.6, 1.8), 3.0)),
            ("b_face_64x64", surface_sweeps(vrc, rng, args.depth, 4096, (64.0, 64.0, 8.0), 6.0))]
    mem = c.memory_usage2() if hasattr(c, "memory_usage2") else {}
    lines = [f"# tools/sweep_bench.py: depth {args.depth} device-built bench scene, {torch.cuda.get_device_name(0)}, coarse table log2 "
             f"{mem.get('coarse_log2', '?')}; library of {os.path.abspath(args.root) if args.box_only else 'this tree'}; median of "
             f"{args.reps} calls after 2 warm-ups (hip events around the synchronous device-pointer call)",
             "# leg  sweeps  sweep ms  Msweeps/s  box query (max_voxels 1) on the start boxes ms  hit  start-solid  free  mean events"]
    for name, sweeps in legs:
        n = len(sweeps)
        ts = torch.from_numpy(np.ascontiguousarray(sweeps)).to("cuda:0")
        tb = torch.from_numpy(np.ascontiguousarray(sweeps[:, :6])).to("cuda:0")
        rec = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
        cnt = torch.empty((n,), dtype=torch.int64, device="cuda:0")
        vox = torch.empty((n, 1, 4), dtype=torch.int32, device="cuda:0")
        box_ms = timed(lambda: c.box_intersection_device(tb.data_ptr(), n, rec.data_ptr(), cnt.data_ptr(), vox.data_ptr(), 1), args.reps)
        if args.box_only:
            lines.append(f"{name:14s} {n:8d}         -         - {box_ms:9.3f}")
        else:
            ms = timed(lambda: c.sweep_boxes_device(ts.data_ptr(), n, rec.data_ptr()), args.reps)
            r = rec.cpu().numpy()
            hit, solid = int((r[:, 0] & vrc.SWEEP_HIT != 0).sum()), int((r[:, 0] & vrc.SWEEP_START_SOLID != 0).sum())
            lines.append(f"{name:14s} {n:8d} {ms:9.3f} {n / ms / 1e3:9.3f} {box_ms:9.3f} {hit:8d} {solid:8d} {n - hit - solid:8d} {r[:, 7].mean():7.2f}")
        print(lines[-1], flush=True)
    if args.crossover and not args.box_only:
        lines.append(f"# crossover: {args.crossover_n} sweeps of f x f x f voxels (extent f - 0.4, fractional origins) per face size; every sweep one lane "
                     "(sweep_lane_face 2^30), every sweep one wave (0)")
        lines.append("# f  lane ms  wave ms")
        assert c.add_to_settings_buffer("sweep_lane_face", "SWEEP_LANE_FACE", 0), c.last_error()
        for f in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 24, 32):
            sweeps = surface_sweeps(vrc, rng, args.depth, args.crossover_n, (f - 0.4, f - 0.4, f - 0.4), 3.0, cols=1024)
            ts = torch.from_numpy(sweeps).to("cuda:0")
            rec = torch.empty((len(sweeps), 8), dtype=torch.int32, device="cuda:0")
            got = []
            for face in (1 << 30, 0):
                assert c.overwrite_setting("sweep_lane_face", face)
                got.append(timed(lambda: c.sweep_boxes_device(ts.data_ptr(), len(sweeps), rec.data_ptr()), max(3, args.reps // 2)))
            lines.append(f"{f:4d} {got[0]:9.3f} {got[1]:9.3f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fo:
            fo.write(text)


if __name__ == "__main__":
    main()
