"""GPU suite (-m gpu): the face extraction through the index-audit build (libvrc_audit.so, csrc/index_audit.hpp): a child
process (tests/face_audit_case.py) runs a handful of the small cases; the lists equal the replay, every scene array the kernels
index was read through the audited accessors against a published extent, and no index left its array."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_audit_build_extracts_without_a_violation(tmp_path):
    out = str(tmp_path / "face_audit.json")
    env = dict(os.environ, VRC_LIB_PATH=os.path.join(ROOT, "voxel-raycaster_amd", "libvrc_audit.so"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "face_audit_case.py"), out], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.load(open(out))
    for name in ("tree", "dense"):
        bad = {a: e for a, e in got[name].items() if e["violations"]}
        assert not bad, (name, bad)
    for array in ("descriptors", "far_slots", "attach_lookup", "attachments"):
        e = got["tree"][array]
        assert e["accesses"] > 0 and e["extent_published"] and e["max_index"] < e["extent"], (array, e)
    e = got["dense"]["map"]
    assert e["accesses"] > 0 and e["extent_published"] and e["max_index"] < e["extent"], e
    assert got["dense"]["descriptors"]["accesses"] == 0, "the array branch read the tree"
    assert got["tree_ok"] and got["map_ok"]
