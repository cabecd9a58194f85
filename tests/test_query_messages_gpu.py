"""GPU suite (-m gpu): the refusals of the twelve calls that read the resident scene (csrc/vrc_query.cpp), text and code.

Every refusal a call can give before its first launch -- n < 0, a negative cap, a bad size, unknown flag bits, null arrays, a
null list with room asked for, an info struct without its size, an output too small, a handle that is not validated, and for the
_device calls a misaligned address and memory the GPU cannot reach -- is compared for EQUALITY with the text and the status code
the call has always given, through ctypes as a C host sees them.  A refused call leaves its outputs as they were.  The order of
the checks is pinned where two would fire: readiness before alignment, n == 0 before both, an unused list never looked at.

Nothing here launches a kernel with bad arguments: every case returns before the first launch (the addresses 2, 4, 8 and 9 are
compared and masked, never dereferenced).  The scene is one depth-4 tree."""
import ctypes as C

import numpy as np
import pytest

import scenes
import voxel_raycaster_amd as vrc
from gpu_helpers import configure

pytestmark = pytest.mark.gpu
INVALID, NOT_READY = 1, 2
SENTINEL = -77
N = 4
UNREACHABLE = " must be memory the GPU of the handle (device 0) can read and write"


@pytest.fixture(scope="module")
def casters(atlas):
    s = scenes.axis_aligned(16)
    c = vrc.CLCaster()
    assert c.init(0), c.last_error()
    li = np.zeros((8, 10), dtype=np.float32)
    li[:1] = s["lights"][:1]
    configure(c, 16, atlas, s["cam_dir"], s["cam_pos"], li, 96, 64)
    grid = np.asarray(s["grid"], np.int8)
    assert c.assign_octree(vrc.Octree.Generate(grid, 16)) and c.assign_map(grid, (16,) * 3), c.last_error()
    assert c.validate(), c.last_error()
    fresh = vrc.CLCaster()
    assert fresh.init(0), fresh.last_error()
    return c, fresh


class Call:
    """One family: the arguments of vrc_<name> and vrc_<name>_device in order, valid by default (arrays in pageable host memory,
    the outputs filled with SENTINEL); a case overrides some of them by name."""

    def __init__(self, name, **defaults):
        self.name, self.defaults = name, defaults
        self.outputs = [v for k, v in defaults.items() if isinstance(v, np.ndarray) and (v == SENTINEL).all()]

    def __call__(self, h, device, **over):
        assert set(over) <= set(self.defaults), over
        fn = getattr(vrc.lib, "vrc_" + self.name + ("_device" if device else ""))
        args = []
        for (key, default), ctype in zip(self.defaults.items(), fn.argtypes[1:]):
            v = over.get(key, default)
            if isinstance(v, np.ndarray):
                v = v.ctypes.data
            if isinstance(v, vrc.FacesInfo):
                v = C.byref(v)
            elif v is not None and ctype not in (C.c_int64, C.c_int32, C.c_uint32, C.c_size_t):
                v = C.cast(C.c_void_p(v), ctype)                  # (an address: a numpy array's, or a small number never dereferenced)
            args.append(v)
        return fn(h, *args)

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.outputs)


def _out(shape, dtype):
    return np.full(shape, SENTINEL, dtype)


def _info():
    info = vrc.FacesInfo()
    info.struct_size, info.truncated, info.faces_total, info.faces_written, info.seconds = C.sizeof(vrc.FacesInfo), 7, 7, 7, 7.0
    return info


SIZE = np.array([2, 2, 2], np.int32)
CALLS = {
    "cast_rays": Call("cast_rays", rays=np.ones((N, 6), np.float32), n=N, max_steps=0, flags=0, out=_out((N, 8), np.int32)),
    "box_intersection": Call("box_intersection", boxes=np.ones((N, 6), np.float32), n=N, max_voxels=3, flags=0, records=_out((N, 8), np.int32),
                             counts=_out(N, np.int64), voxels=_out((N, 3, 4), np.int32)),
    "sweep_boxes": Call("sweep_boxes", sweeps=np.ones((N, 9), np.float32), n=N, max_events=0, flags=0, records=_out((N, 8), np.int32)),
    "get_voxels": Call("get_voxels", positions=np.ones((N, 3), np.int32), n=N, out=_out(N, np.int32)),
    "read_regions": Call("read_regions", lo=np.ones((N, 3), np.int32), n=N, size=SIZE, out=_out(N * 8, np.int8), n_bytes=N * 8),
    "extract_faces": Call("extract_faces", lo=np.ones((N, 3), np.int32), n=N, size=SIZE, capacity=6, flags=0, counts=_out(N, np.int64),
                          faces=_out((6, 4), np.int32), info=_info()),
}
BAD_SIZE = np.array([2, 0, 2], np.int32)

# (family, overrides, status code, text behind "<call>: ") -- the same for the host call and the _device call, which gives them
# before it looks at an address
SHARED = [
    ("cast_rays", dict(n=-1), INVALID, "n = -1 < 0"),
    ("cast_rays", dict(max_steps=-3), INVALID, "max_steps = -3 < 0"),
    ("cast_rays", dict(flags=0x81), INVALID, "unknown flag bits 0x80"),
    ("cast_rays", dict(rays=None), INVALID, "null rays or output"),
    ("cast_rays", dict(out=None), INVALID, "null rays or output"),
    ("box_intersection", dict(n=-1), INVALID, "n = -1 < 0"),
    ("box_intersection", dict(max_voxels=-2), INVALID, "max_voxels = -2 < 0"),
    ("box_intersection", dict(flags=0x6), INVALID, "unknown flag bits 0x6"),
    ("box_intersection", dict(boxes=None), INVALID, "null boxes, records or counts"),
    ("box_intersection", dict(records=None), INVALID, "null boxes, records or counts"),
    ("box_intersection", dict(counts=None), INVALID, "null boxes, records or counts"),
    ("box_intersection", dict(voxels=None), INVALID, "null voxels with max_voxels = 3"),
    ("sweep_boxes", dict(n=-1), INVALID, "n = -1 < 0"),
    ("sweep_boxes", dict(max_events=-3), INVALID, "max_events = -3 < 0"),
    ("sweep_boxes", dict(flags=0x3), INVALID, "unknown flag bits 0x2"),
    ("sweep_boxes", dict(sweeps=None), INVALID, "null sweeps or records"),
    ("sweep_boxes", dict(records=None), INVALID, "null sweeps or records"),
    ("get_voxels", dict(n=-1), INVALID, "n = -1 < 0"),
    ("get_voxels", dict(positions=None), INVALID, "null rays or output"),
    ("get_voxels", dict(out=None), INVALID, "null rays or output"),
    ("read_regions", dict(n=-1), INVALID, "n = -1 < 0"),
    ("read_regions", dict(size=None), INVALID, "null size"),
    ("read_regions", dict(size=BAD_SIZE), INVALID, "size[1] = 0 < 1"),
    ("read_regions", dict(lo=None), INVALID, "null corners or output"),
    ("read_regions", dict(out=None), INVALID, "null corners or output"),
    ("read_regions", dict(n_bytes=31), INVALID, "output holds 31 bytes, the regions need 32"),
    ("extract_faces", dict(n=-1), INVALID, "n = -1 < 0"),
    ("extract_faces", dict(size=None), INVALID, "null size"),
    ("extract_faces", dict(size=BAD_SIZE), INVALID, "size[1] = 0 < 1"),
    ("extract_faces", dict(capacity=-5), INVALID, "capacity = -5 < 0"),
    ("extract_faces", dict(flags=0xb), INVALID, "unknown flag bits 0x8"),
    ("extract_faces", dict(lo=None), INVALID, "null corners or counts"),
    ("extract_faces", dict(counts=None), INVALID, "null corners or counts"),
    ("extract_faces", dict(faces=None), INVALID, "null faces with capacity = 6"),
    ("extract_faces", dict(info=vrc.FacesInfo()), INVALID, "info->struct_size is not set"),
]

# (family, overrides, the whole text) of the _device calls alone: a misaligned address (code 1) ...
MISALIGNED = [
    ("cast_rays", dict(rays=2), "cast_rays_device: rays and output must be 4-byte aligned"),
    ("cast_rays", dict(out=9), "cast_rays_device: rays and output must be 4-byte aligned"),
    ("box_intersection", dict(boxes=2), "box_intersection_device: boxes, records and voxels must be 4-byte aligned, counts 8-byte aligned"),
    ("box_intersection", dict(records=2), "box_intersection_device: boxes, records and voxels must be 4-byte aligned, counts 8-byte aligned"),
    ("box_intersection", dict(counts=4), "box_intersection_device: boxes, records and voxels must be 4-byte aligned, counts 8-byte aligned"),
    ("box_intersection", dict(voxels=2), "box_intersection_device: boxes, records and voxels must be 4-byte aligned, counts 8-byte aligned"),
    ("sweep_boxes", dict(sweeps=2, records=8), "sweep_boxes_device: sweeps and records must be 4-byte aligned"),
    ("sweep_boxes", dict(records=2), "sweep_boxes_device: sweeps and records must be 4-byte aligned"),
    ("get_voxels", dict(positions=2), "get_voxels_device: positions and output must be 4-byte aligned"),
    ("get_voxels", dict(out=2), "get_voxels_device: positions and output must be 4-byte aligned"),
    ("read_regions", dict(lo=2), "read_regions_device: the corners must be 4-byte aligned"),
    ("extract_faces", dict(lo=2), "extract_faces_device: the corners and faces must be 4-byte aligned, counts 8-byte aligned"),
    ("extract_faces", dict(counts=4), "extract_faces_device: the corners and faces must be 4-byte aligned, counts 8-byte aligned"),
    ("extract_faces", dict(faces=2), "extract_faces_device: the corners and faces must be 4-byte aligned, counts 8-byte aligned"),
]
# ... and aligned arrays in pageable host memory (code 1).  With no room asked for, the list is not looked at, whatever its
# address; a region's bytes need no alignment.
PAGEABLE = [
    ("cast_rays", dict(), "cast_rays_device: rays and output" + UNREACHABLE),
    ("box_intersection", dict(), "box_intersection_device: boxes and outputs" + UNREACHABLE),
    ("box_intersection", dict(max_voxels=0, voxels=2), "box_intersection_device: boxes and outputs" + UNREACHABLE),
    ("sweep_boxes", dict(), "sweep_boxes_device: sweeps and records" + UNREACHABLE),
    ("get_voxels", dict(), "get_voxels_device: input and output" + UNREACHABLE),
    ("read_regions", dict(), "read_regions_device: input and output" + UNREACHABLE),
    ("read_regions", dict(out=CALLS["read_regions"].defaults["out"][1:], n_bytes=N * 8), "read_regions_device: input and output" + UNREACHABLE),
    ("extract_faces", dict(), "extract_faces_device: corners and outputs" + UNREACHABLE),
    ("extract_faces", dict(capacity=0, faces=2), "extract_faces_device: corners and outputs" + UNREACHABLE),
]


def _ids(cases):
    return ["%s-%s" % (c[0], "-".join("%s" % k for k in c[1]) or "plain") + "-%d" % i for i, c in enumerate(cases)]


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("family,over,code,text", SHARED, ids=_ids(SHARED))
def test_argument_refusals(casters, family, over, code, text, device):
    c, _ = casters
    call = CALLS[family]
    assert call(c._h, device, **over) == code
    assert c.last_error() == "%s%s: %s" % (family, "_device" if device else "", text)
    assert call.untouched() and call.defaults.get("info", _info()).faces_total == 7


@pytest.mark.parametrize("family,over,text", MISALIGNED + PAGEABLE, ids=_ids(MISALIGNED + PAGEABLE))
def test_device_address_refusals(casters, family, over, text):
    c, _ = casters
    call = CALLS[family]
    assert call(c._h, True, **over) == INVALID
    assert c.last_error() == text
    assert call.untouched() and call.defaults.get("info", _info()).faces_total == 7


@pytest.mark.parametrize("family", list(CALLS))
def test_order_of_the_checks(casters, family):
    c, fresh = casters
    call = CALLS[family]
    first = next(iter(call.defaults))
    for device in (False, True):
        name = family + ("_device" if device else "")
        assert call(None, device) == INVALID                                       # (no handle: no text either)
        # the argument checks come before the handle's readiness, readiness before the addresses, n == 0 before both
        assert call(fresh._h, device, n=-1) == INVALID and fresh.last_error() == name + ": n = -1 < 0"
        assert call(fresh._h, device, **{first: 2}) == NOT_READY and fresh.last_error() == name + ": validate() has not succeeded"
        assert call(fresh._h, device, n=0) == NOT_READY and fresh.last_error() == name + ": validate() has not succeeded"
        if family != "extract_faces":
            assert call(c._h, device, n=0, **{first: 2}) == 0
        else:                                                                      # n == 0 reports: nothing found, nothing cut
            info = _info()
            assert call(c._h, device, n=0, info=info, **{first: 2}) == 0
            assert (info.struct_size, info.truncated, info.faces_total, info.faces_written, info.seconds) == (C.sizeof(vrc.FacesInfo), 0, 0, 0, 0.0)
        assert call.untouched() and call.defaults.get("info", _info()).faces_total == 7
