#!/usr/bin/env python3
"""Idle wave slots inside a workgroup: a workgroup's slots, registers and LDS go back when its LAST wave ends, so a wave that
finishes its tile early holds them for nothing.  From a -DVRC_TIME_STATS build (per workgroup: the sum and the longest of its waves'
lives, raycast_kernel.hip g_time_stats[9..14]) on the headline frame, the 4-light headline and depth-10 primary-only:
    share = 1 - sum(life) / (waves per workgroup x sum over workgroups of the longest life)
split by workgroups none of whose rays cast a shadow ray / the others.
  bash tools/build_variant.sh time4 -DVRC_TIME_STATS -DVRC_SVO_TILES=4
  VRC_LIB_PATH=<the libvrc_time4.so that build wrote> python tools/block_imbalance.py"""
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import voxel_raycaster_amd as vrc

FRAMES = [("headline: depth 12, 1920x1080, 1 light", 12, dict()),
          ("depth 12, 1920x1080, 4 lights", 12, dict(light_count=4)),
          ("depth 10, 1920x1080, primary only", 10, dict(shadow_rays=0))]
scenes = {}
for name, depth, kw in FRAMES:
    sc = scenes.setdefault(depth, bench.build_scene(depth))
    c = bench.make_caster(sc, 1920, 1080, 0, hit_records=0, **kw)
    for _ in range(3):
        assert c.compute(), c.last_error()
    buf = (C.c_ulonglong * 16)()
    assert vrc.lib.vrc_stats_time(buf, 1) == 0
    assert c.compute(), c.last_error()
    assert vrc.lib.vrc_stats_time(buf, 1) == 0
    row = {"frame": name, "kernel": c.last_kernel()["name"]}
    for tag, o in (("no_shadow_ray", 9), ("shadow_rays", 12)):
        life, held, groups = buf[o], buf[o + 1], buf[o + 2]
        row[tag] = {"workgroups": int(groups), "idle_share": round(1 - life / held, 4) if held else None, "share_of_held_time": 0.0}
    life, held = buf[9] + buf[12], buf[10] + buf[13]
    for tag, o in (("no_shadow_ray", 9), ("shadow_rays", 12)):
        row[tag]["share_of_held_time"] = round(buf[o + 1] / held, 4)
    row["idle_share"] = round(1 - life / held, 4)
    row["wave_life_Mticks_sum"] = round(life / 1e6, 1)
    print(json.dumps(row), flush=True)
    del c
