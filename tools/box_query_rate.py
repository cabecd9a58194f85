"""Box-query rates (vrc_box_intersection_device, csrc/box_query.hip) on the depth-12 bench scene, device-built, with the coarse
table built by validate: (a) 1 M player AABBs of 0.6 x 0.6 x 1.8 at fractional positions on the surface, count and corners;
(b) the same with max_voxels = 16; (c) 4096 brush boxes of 64^3 on the surface, max_voxels = 4096; (d) 16 regions of 512^3,
count only; (e) one box over the whole map, count only.  Each leg: hip events around the device-pointer call, the median of
--reps calls after 2 warm-ups.  Usage: python tools/box_query_rate.py [--depth 12] [--reps 10] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import bench
import voxel_raycaster_amd as vrc

F = np.float32


def surface_boxes(rng, depth, n, ext, cols=4096):
    """n boxes of extent `ext` centred in z on the surface (shell_column hi) at fractional (x, y): the column heights of `cols`
    random columns, reused."""
    dim = 1 << depth
    xy = rng.uniform(0, dim - ext[0], size=(cols, 2))
    hi = np.array([vrc.shell_column(depth, int(x), int(y))[1] for x, y in xy], dtype=np.float64)
    pick = rng.integers(0, cols, size=n)
    jitter = rng.uniform(0, 1, size=(n, 2))
    o = np.stack([xy[pick, 0] + jitter[:, 0], xy[pick, 1] + jitter[:, 1], hi[pick] + 1 - ext[2] / 2 + rng.uniform(0, 1, n)], axis=1)
    o[:, :2] = np.minimum(o[:, :2], dim - ext[0])
    return np.concatenate([o, np.broadcast_to(np.asarray(ext, np.float64), (n, 3))], axis=1).astype(F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sc = bench.device_scene_header(args.depth)
    dim = sc["dim"]
    c = bench.make_caster(sc, 256, 144, 0)
    rng = np.random.default_rng(1)
    player = surface_boxes(rng, args.depth, 1 << 20, (0.6, 0.6, 1.8))
    brush = surface_boxes(rng, args.depth, 4096, (64.0, 64.0, 64.0))
    reg = rng.integers(0, dim // 512, size=(16, 3)) * 512
    regions = np.concatenate([reg, np.full((16, 3), 512)], axis=1).astype(F)
    whole = np.array([[0, 0, 0, dim, dim, dim]], F)
    legs = [("a_player_aabbs", player, 0), ("b_player_list16", player, 16), ("c_brush_64", brush, 4096),
            ("d_regions_512", regions, 0), ("e_whole_map", whole, 0)]
    mem = c.memory_usage2() if hasattr(c, "memory_usage2") else {}
    lines = [f"# tools/box_query_rate.py: depth {args.depth} device-built bench scene, {torch.cuda.get_device_name(0)}, coarse table "
             f"log2 {mem.get('coarse_log2', '?')}; median of {args.reps} calls after 2 warm-ups (hip events)",
             "# leg  boxes  max_voxels  device ms  Mboxes/s  counted voxels  Gvoxels/s  boxes with any"]
    for name, boxes, maxv in legs:
        n = len(boxes)
        tb = torch.from_numpy(np.ascontiguousarray(boxes)).to("cuda:0")
        rec = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
        cnt = torch.empty((n,), dtype=torch.int64, device="cuda:0")
        vox = torch.empty((n, maxv, 4), dtype=torch.int32, device="cuda:0") if maxv else None
        call = lambda: c.box_intersection_device(tb.data_ptr(), n, rec.data_ptr(), cnt.data_ptr(), vox.data_ptr() if maxv else 0, maxv)
        for _ in range(2):
            assert call(), c.last_error()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        dev_ms = float(np.median(ms))
        counts = cnt.cpu().numpy()
        total = int(counts.sum())
        lines.append(f"{name:16s} {n:8d} {maxv:6d} {dev_ms:9.3f} {n / dev_ms / 1e3:9.3f} {total:14d} {total / dev_ms / 1e6:9.3f} "
                     f"{int((counts > 0).sum()):8d}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
