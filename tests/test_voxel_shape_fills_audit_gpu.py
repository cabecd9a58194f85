"""GPU suite (-m gpu): the shape fills through the index-audit build (libvrc_audit.so, csrc/index_audit.hpp): a child process
(tests/shape_audit_case.py) sends two batches into a 32^3 tree with edit_reserve = 0, renders a frame and sends them into the dense
map; the read-backs equal the replay, every scene array the brick pass indexes was read through the audited accessors against a
published extent, and no index left its array.  The front end's own arrays (the counts, their scan, the shapes) have no entry in
the audit's table, which is full: they are plain loads, like the boxes'."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_audit_build_fills_shapes_and_renders_without_a_violation(tmp_path):
    out = str(tmp_path / "shape_audit.json")
    env = dict(os.environ, VRC_LIB_PATH=os.path.join(ROOT, "voxel-raycaster_amd", "libvrc_audit.so"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shape_audit_case.py"), out], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.load(open(out))
    for name in ("after_first", "after_second", "after_map", "frame"):
        bad = {a: e for a, e in got[name].items() if e["violations"]}
        assert not bad, (name, bad)
    for name in ("after_first", "after_second"):                # the brick pass read the old tree through the audited accessors
        # (the builder's tree has no far pointer; the first batch's ancestor pass appends them, so the second reads far slots)
        for array in ("descriptors", "attach_lookup", "attachments") + (("far_slots",) if name == "after_second" else ()):
            e = got[name][array]
            assert e["accesses"] > 0 and e["extent_published"] and e["max_index"] < e["extent"], (name, array, e)
    e = got["after_map"]["map"]
    assert e["accesses"] > 0 and e["extent_published"] and e["max_index"] < e["extent"], e
    frame = got["frame"]
    assert frame["descriptors"]["extent"] == got["info"]["n_descriptors"], "edit_reserve = 0: the frame is checked against the new size"
    assert frame["descriptors"]["max_index"] >= got["n_before"], "the frame never read an appended word"
    assert got["reads_ok"] and got["map_ok"]
