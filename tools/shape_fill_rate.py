"""Shape-fill rates (vrc_fill_shapes, csrc/region_write.hip + csrc/shape_span.hpp) against the only way to write the same voxels
before the call existed -- vrc_set_voxels of the shapes expanded to one (x, y, z, material) tuple per voxel, upload included -- on
the device-built shell terrain of the headline depth (a tree that exists only in HBM):
  ball_r8 / ball_r32 / ball_r128   one ball cleared at the terrain's surface
  tunnel_r4_h512                   one cylinder along x, r = 4, h = 512, cleared just below the surface
  balls_1024_r4                    1024 balls of r = 4 on a 32 x 32 grid of surface points, cleared in one batch
Both routes are the HOST calls, from host arrays.  Per call: the wall time of the call and the device time of its kernels
(vrc_edit_info.seconds).  Every repetition runs on a fresh tree of its own (a new handle, the terrain built again), the two routes
alternate, and the arrays' sizes, the counts and the bytes read back after either route must be the same.  The expansion into
positions is made once, untimed; pairs -- (brick, operation) pairs, the front end's output -- are counted on the host by brute
force.  Each figure: the median and the spread (min .. max) of --reps repetitions after 2 warm-ups.
Usage: python tools/shape_fill_rate.py [--reps 5] [--depth 12] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import bench
import shape_replay as sp
import voxel_raycaster_amd as vrc


def stat(ms):
    return f"{np.median(ms):9.3f} ({min(ms):.3f} .. {max(ms):.3f})"


def legs(depth):
    dim = 1 << depth
    cx = cy = dim // 2
    top = lambda x, y: int(vrc.shell_column(depth, int(x), int(y))[1])
    hi = top(cx, cy)
    out = [(f"ball_r{r}", np.array([[sp.BALL, cx, cy, hi, r, 0]], np.int32)) for r in (8, 32, 128)]
    out.append(("tunnel_r4_h512", np.array([[sp.CYLINDER_X, cx - 256, cy, max(hi - 6, 0), 4, 512]], np.int32)))
    grid = [(cx - 192 + 12 * i, cy - 192 + 12 * j) for j in range(32) for i in range(32)]
    out.append(("balls_1024_r4", np.array([[sp.BALL, x, y, top(x, y), 4, 0] for x, y in grid], np.int32)))
    made = []
    for name, shapes in out:
        parts = [sp.expand_shapes(s[None], [0], (dim,) * 3)[0] for s in shapes]
        bricks = [p.astype(np.int64) >> 3 for p in parts]
        pairs = sum(len(np.unique(b[:, 0] + (b[:, 1] << 21) + (b[:, 2] << 42))) for b in bricks)
        positions = np.concatenate(parts)
        made.append(dict(name=name, shapes=shapes, positions=positions, materials=np.zeros(len(positions), np.int32), pairs=pairs))
    return made


def run(leg, route, sc):
    """one repetition on a fresh tree: (wall ms, kernels ms, info, the bytes of the shapes' bounding box afterwards)"""
    c = bench.make_caster(sc, 256, 144, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if route == "set_voxels":
        info = c.set_voxels(leg["positions"], leg["materials"])
    else:
        info = c.fill_shapes(leg["shapes"], 0)
    t1 = time.perf_counter()
    assert info["voxels_changed"] > 0 and info["skipped"] == 0, info
    p = leg["positions"]
    box_lo, box_size = p.min(axis=0), p.max(axis=0) - p.min(axis=0) + 1
    after = c.read_regions(box_lo[None], tuple(int(v) for v in box_size))
    return 1e3 * (t1 - t0), 1e3 * info["seconds"], info, after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3
    lines = [f"# tools/shape_fill_rate.py: {torch.cuda.get_device_name(0)}; depth-{args.depth} shell terrain, a fresh tree per repetition, the routes alternating;",
             f"# median (min .. max) of {args.reps} repetitions after 2 warm-ups, milliseconds.  call = wall time of the host call (staging included);",
             "# kernels = vrc_edit_info.seconds.  set_voxels = the same shapes expanded to their voxels, the route that existed before: the baseline.",
             "# ratio = set_voxels / fill_shapes, of the medians",
             "# leg  route  operations  pairs  bricks  voxels changed  words added  call ms  kernels ms"]
    sc = bench.device_scene_header(args.depth)
    for leg in legs(args.depth):
        times = {"fill_shapes": ([], []), "set_voxels": ([], [])}
        infos, after = {}, {}
        for k in range(args.reps + 2):
            for route in (("fill_shapes", "set_voxels") if k % 2 == 0 else ("set_voxels", "fill_shapes")):
                wall, dev, infos[route], after[route] = run(leg, route, sc)
                if k >= 2:
                    times[route][0].append(wall); times[route][1].append(dev)
            assert np.array_equal(after["fill_shapes"], after["set_voxels"]), "the two routes left different scenes"
            for key in ("voxels_changed", "bricks_touched", "descriptors_added", "n_descriptors", "root_index"):
                assert infos["fill_shapes"][key] == infos["set_voxels"][key], key
        for route in ("fill_shapes", "set_voxels"):
            n = len(leg["shapes"]) if route == "fill_shapes" else len(leg["positions"])
            pairs = leg["pairs"] if route == "fill_shapes" else len(leg["positions"])
            i = infos[route]
            lines.append(f"{leg['name']:15s} {route:11s} {n:8d} {pairs:8d} {i['bricks_touched']:6d} {i['voxels_changed']:8d} {i['descriptors_added']:8d} "
                         f"{stat(times[route][0])} {stat(times[route][1])}")
            print(lines[-1], flush=True)
        lines.append(f"{leg['name']:15s} ratio: call {np.median(times['set_voxels'][0]) / np.median(times['fill_shapes'][0]):.2f}x, "
                     f"kernels {np.median(times['set_voxels'][1]) / np.median(times['fill_shapes'][1]):.2f}x")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
