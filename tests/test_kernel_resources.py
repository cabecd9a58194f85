"""Register / scratch budget of the built kernels, read from the code objects inside voxel-raycaster_amd/libvrc.so
(llvm-objdump --offloading + llvm-readelf --notes: no GPU, no recompile).  Guards what round 4 paid for: the headline
instance of the SVO kernel keeps its 5 waves per SIMD (96 VGPRs) with no more than 40 B of scratch per lane -- every
scratch byte is written to HBM once per wave, and at 52 B the launch wrote 5.1 x the frame (profiles/HISTORY.md)."""
import os, re, shutil, subprocess, tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_table():
    lib = os.path.join(ROOT, "voxel-raycaster_amd", "libvrc.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    tmp = tempfile.mkdtemp(prefix="vrc_co_")
    try:
        shutil.copy(lib, os.path.join(tmp, "libvrc.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "libvrc.so"], cwd=tmp, check=True, capture_output=True)
        table = {}
        for name in sorted(os.listdir(tmp)):
            if "amdgcn" not in name:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, name)], capture_output=True, text=True).stdout
            cur = None
            for line in notes.splitlines():
                m = re.match(r"\s+\.(name|private_segment_fixed_size|vgpr_count|sgpr_count):\s+(\S+)", line)
                if not m:
                    continue
                if m.group(1) == "name":
                    cur = table.setdefault(m.group(2), {})
                elif cur is not None:
                    cur[m.group(1)] = int(m.group(2))
        return table
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    t = kernel_table()
    assert t, "no gfx950 code object found in libvrc.so"
    return t


def svo(jump, multi, tuned, lds, coarse, box=False):
    """lds: rows of the Euclid-table ring in LDS (True = 3), 0 / False = tables in global memory."""
    b = lambda v: "Lb1E" if v else "Lb0E"
    rows = 3 if lds is True else int(lds)
    return "_ZN3vrc18raycast_svo_kernelI" + b(jump) + b(multi) + b(tuned) + f"Li{rows}E" + b(coarse) + b(box) + "EEvNS_13RaycastParamsE"


def test_headline_instance_budget(kernels):
    for box in (True, False):                          # round 5: the headline frame runs the instance with the empty boxes
        k = kernels[svo(True, False, True, True, True, box)]
        assert k["vgpr_count"] <= 96                       # 5 waves per SIMD
        # round 3: 76 B, round 4: 20, round 5: 28 with the boxes, round 6: NONE -- the event phase no longer touches the ray's cold state
        # (colours: settle_segment), voxel_step lives in three flag bits, the voxel is the cursor's, the cursor's entry is re-read from
        # the LDS stack: 12 registers less through the round loop, and the 126 MB of spill write-backs per frame are gone
        assert k["private_segment_fixed_size"] == 0


def test_plain_instance_budget(kernels):
    for box in (True, False):
        k = kernels[svo(False, False, True, False, True, box)]  # trees below depth 12 (BASELINE configs[0], configs[1])
        assert k["vgpr_count"] <= 80                       # 6 waves per SIMD
        assert k["private_segment_fixed_size"] == 0


def test_multi_light_instance_budget(kernels):
    """The multi-light instances carry the first-strike state (voxel, face position, mask * step, distance: ten dwords) through the
    shadow segments -- in scratch, and that is where it belongs: what a spill costs is where it is EXECUTED, not how many bytes the
    segment has (round 6: 84 -> 100 B while the 4-light frame went from 3.66 to 3.19 ms, then 3.00 at 88 B).  The byte budget only
    keeps the allocation from growing unnoticed; test_no_spill_in_the_hot_phases is the real guard."""
    for box in (True, False):
        k = kernels[svo(True, True, True, True, True, box)]
        assert k["vgpr_count"] <= 96
        assert k["private_segment_fixed_size"] <= 104


def test_no_spill_in_the_hot_phases():
    """tools/spill_map.py on the instances a default launch reaches from depth 11 on: no scratch load or store between the round
    loop's jump rows and the end of the event phase (the `; VRC_MARK` comments of raycast_kernel.hip).  Round 5's headline instance
    reloaded and re-spilled a colour in every event pass (126 MB of write-backs per frame); the multi-light instances held the SVO
    cursor in scratch (2.5 GB per 4-light frame)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import spill_map
    if not os.path.exists(spill_map.g.HIPCC):
        pytest.skip("no hipcc in this image")
    text = spill_map.assembly()
    for inst in ("ILb1ELb0ELb1ELi3ELb1ELb1E", "ILb1ELb1ELb1ELi3ELb1ELb1E", "ILb1ELb0ELb1ELi3ELb1ELb0E", "ILb1ELb1ELb1ELi3ELb1ELb0E", "ILb1ELb0ELb1ELi2ELb1ELb1E", "ILb1ELb1ELb1ELi2ELb1ELb1E"):
        rows = spill_map.spill_map(text, inst)
        assert rows is not None and "event_begin" in rows and "jump_block_begin" in rows, inst
        hot = {ph: r[:2] for ph, r in rows.items() if ph in spill_map.HOT_PHASES and (r[0] or r[1])}
        assert not hot, f"raycast_svo_kernel<{inst}>: scratch instructions in hot phases {hot}"
    single = spill_map.spill_map(text, "ILb1ELb0ELb1ELi3ELb1ELb1E")
    assert sum(r[0] + r[1] for r in single.values()) == 0           # the headline instance: no spill anywhere


def test_every_svo_instance_keeps_its_occupancy(kernels):
    names = [n for n in kernels if n.startswith("_ZN3vrc18raycast_svo_kernelI")]
    # 36 -> 24.  Knobs at their defaults: {no jumps | tables in global memory | 3 rows in LDS} x {no table | coarse |
    # + boxes} x {one light | multi-light}, jumps only with the table = 14, + the box instances with a 2-row ring (deep trees) = 16;
    # run-time knobs: the same 8 once, multi-light code compiled in
    assert len(names) == 24
    for n in names:
        jump = n[len("_ZN3vrc18raycast_svo_kernelI"):].startswith("Lb1E")
        assert kernels[n]["vgpr_count"] <= (96 if jump else 80), n


def test_mode_b_budget(kernels):
    k = kernels["_ZN3vrc19raycast_jump_kernelILb0ELb1EEEvNS_13RaycastParamsE"]
    assert k["vgpr_count"] <= 64                       # 8 waves per SIMD
    assert k["private_segment_fixed_size"] <= 48


def test_instance_matrix_is_exactly_the_compiled_frame_kernels(kernels):
    """tests/instance_matrix.py has one row per frame-kernel instance in the code object, and no other: an instance added without a
    row (tests/test_instances_gpu.py would never launch it on purpose) or a row whose instance is gone fails here, on any machine."""
    import instance_matrix as im
    families = ("raycast_svo_kernel", "raycast_jump_kernel", "raycast_array_kernel")
    built = {n for n in kernels if any(n.startswith(f"_ZN3vrc{len(f)}{f}") for f in families)}
    rows = {}
    for r in im.ROWS:
        assert im.symbol(r) not in rows, f"two rows for {im.name(r)}"
        rows[im.symbol(r)] = im.name(r)
    assert all(im.symbol(r) == svo(*r.args) for r in im.ROWS if r.family == "raycast_svo_kernel")       # one mangling rule
    missing = sorted(built - set(rows))
    gone = sorted(rows[s] for s in set(rows) - built)
    assert not missing and not gone, f"compiled instances without a row: {missing}; rows without a compiled instance: {gone}"
    assert all(len(r.settings) >= 1 and len(r.lights) >= 1 for r in im.ROWS)
