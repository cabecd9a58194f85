"""Region-edit rates (vrc_fill_boxes / vrc_write_regions, csrc/region_write.hip) against the only way to write the same voxels
before these calls existed, vrc_set_voxels of the expanded batch, on the depth-9 device-built shell terrain (a tree that exists
only in HBM):
  (a) one 64^3 box at the terrain's surface, cleared: vrc_fill_boxes of 1 box / vrc_set_voxels of its 262 144 positions
  (b) 64 blocks of 32^3 random {0, 5} bytes, at unaligned corners around the surface: vrc_write_regions / vrc_set_voxels of their
      2 097 152 positions
All four are the HOST calls, from host arrays: what a host that holds a shape pays, staging included.  Per call: the wall time
of the call and the device time of its kernels (vrc_edit_info.seconds).  Every repetition runs on a fresh tree of its own (a new
handle, the terrain built again), the two routes alternate, and the region read back after either route must be the same bytes.
The expansion into positions is made once, untimed.  Each figure: the median and the spread (min .. max) of --reps repetitions
after 2 warm-ups.  Usage: python tools/region_write_rate.py [--reps 7] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import bench
import voxel_raycaster_amd as vrc

DEPTH = 9


def stat(ms):
    return f"{np.median(ms):9.3f} ({min(ms):.3f} .. {max(ms):.3f})"


def expand(lo, size):
    """the positions of the box [lo, lo + size), x fastest, (k, 3) int32"""
    z, y, x = np.meshgrid(*(np.arange(lo[a], lo[a] + size[a]) for a in (2, 1, 0)), indexing="ij")
    return np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.int32)


def legs(rng):
    dim = 1 << DEPTH
    cx = cy = dim // 2
    _, hi = vrc.shell_column(DEPTH, cx, cy)
    # (a) the box and its positions
    lo = np.array([[cx - 32, cy - 32, max(hi - 40, 0)]], np.int32)
    fill = dict(name="fill_one_64^3", lo=lo, size=(64, 64, 64), positions=expand(lo[0], (64, 64, 64)))
    fill["materials"] = np.zeros(len(fill["positions"]), np.int32)
    # (b) the blocks, on an 8 x 8 grid of corners three voxels off the bricks' alignment, and their positions block by block
    corners = np.array([[cx - 128 + 32 * i + 3, cy - 128 + 32 * j + 3, max(hi - 20, 0)] for j in range(8) for i in range(8)], np.int32)
    data = np.where(rng.random((64, 32, 32, 32)) < 0.5, 5, 0).astype(np.int8)
    paste = dict(name="paste_64_x_32^3", lo=corners, data=data, positions=np.concatenate([expand(c, (32, 32, 32)) for c in corners]))
    paste["materials"] = data.reshape(-1).astype(np.int32)
    return fill, paste


def run(leg, route, sc):
    """one repetition on a fresh tree: (wall ms, kernels ms, info, the bytes of the written region's bounding box afterwards)"""
    c = bench.make_caster(sc, 256, 144, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if route == "set_voxels":
        info = c.set_voxels(leg["positions"], leg["materials"])
    elif "data" in leg:
        info = c.write_regions(leg["lo"], leg["data"])
    else:
        info = c.fill_boxes(leg["lo"], leg["size"], 0)
    t1 = time.perf_counter()
    assert info["voxels_changed"] > 0 and info["skipped"] == 0, info
    p = leg["positions"]
    box_lo, box_size = p.min(axis=0), p.max(axis=0) - p.min(axis=0) + 1
    after = c.read_regions(box_lo[None], tuple(int(v) for v in box_size))
    return 1e3 * (t1 - t0), 1e3 * info["seconds"], info, after


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 5
    lines = [f"# tools/region_write_rate.py: {torch.cuda.get_device_name(0)}; depth-{DEPTH} shell terrain, a fresh tree per repetition, the routes alternating;",
             f"# median (min .. max) of {args.reps} repetitions after 2 warm-ups, milliseconds.  call = wall time of the host call (staging included);",
             "# kernels = vrc_edit_info.seconds.  ratio = set_voxels / region call, of the medians",
             "# leg  route  operations  voxels changed  bricks  words added  call ms  kernels ms"]
    sc = bench.device_scene_header(DEPTH)
    for leg in legs(np.random.default_rng(1)):
        times = {"region": ([], []), "set_voxels": ([], [])}
        infos, after = {}, {}
        for k in range(args.reps + 2):
            for route in (("region", "set_voxels") if k % 2 == 0 else ("set_voxels", "region")):
                wall, dev, infos[route], after[route] = run(leg, route, sc)
                if k >= 2:
                    times[route][0].append(wall); times[route][1].append(dev)
            assert np.array_equal(after["region"], after["set_voxels"]), "the two routes left different scenes"
            for key in ("voxels_changed", "bricks_touched", "descriptors_added", "n_descriptors", "root_index"):
                assert infos["region"][key] == infos["set_voxels"][key], key
        for route in ("region", "set_voxels"):
            n = len(leg["lo"]) if route == "region" else len(leg["positions"])
            i = infos[route]
            lines.append(f"{leg['name']:16s} {route:10s} {n:8d} {i['voxels_changed']:8d} {i['bricks_touched']:6d} {i['descriptors_added']:8d} "
                         f"{stat(times[route][0])} {stat(times[route][1])}")
            print(lines[-1], flush=True)
        lines.append(f"{leg['name']:16s} ratio: call {np.median(times['set_voxels'][0]) / np.median(times['region'][0]):.2f}x, "
                     f"kernels {np.median(times['set_voxels'][1]) / np.median(times['region'][1]):.2f}x")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
