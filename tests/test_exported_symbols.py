"""Every function include/vrc.h declares is a defined dynamic symbol of libvrc.so and of its index-audit twin.  The host layer is
several translation units: a function lost when code moves between them still links, and without this test it would fail only
when ctypes first looks it up."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NM, OBJDUMP = "/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/llvm/bin/llvm-objdump"


def declared():
    """the names of the functions declared in include/vrc.h: a return type at the start of a line, then vrc_name("""
    text = open(os.path.join(ROOT, "include", "vrc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)            # (the comments name functions too)
    return sorted(set(re.findall(r"^(?!typedef\b)[A-Za-z_][\w \t]*[ \t\*]+(vrc_\w+)[ \t]*\(", text, flags=re.M)))


def test_the_header_declares_what_the_regex_finds():
    names = declared()
    assert len(names) > 80, names
    for name in ("vrc_create", "vrc_last_error", "vrc_compute", "vrc_memory_usage2", "vrc_set_voxels", "vrc_set_voxels_device", "vrc_fill_boxes",
                 "vrc_fill_boxes_device", "vrc_write_regions", "vrc_write_regions_device", "vrc_compact_octree", "vrc_read_regions_device"):
        assert name in names, name


@pytest.mark.parametrize("lib", ["libvrc.so", "libvrc_audit.so"])
def test_every_declared_function_is_exported(lib):
    path = os.path.join(ROOT, "voxel-raycaster_amd", lib)
    assert os.path.exists(path), path + " is missing: build() makes it"
    if os.path.exists(NM):
        out = subprocess.run([NM, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.split()[-2:-1] == ["T"]}
    else:       # a ROCm install without llvm-nm: the same table from llvm-objdump (defined: a function in .text, not *UND*)
        out = subprocess.run([OBJDUMP, "-T", path], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " DF .text" in line and " g " in line}
    missing = [name for name in declared() if name not in exported]
    assert not missing, (lib, missing)
