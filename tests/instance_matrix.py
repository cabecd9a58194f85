"""Every compiled instance of the frame kernels, and the settings that make a frame run it.  Not a test file.

One Row per instance: csrc/raycast_kernel.hip launch_raycast picks one of 24 raycast_svo_kernel<kJump, kMulti, kTuned, kLdsRows,
kCoarse, kBox> per frame, csrc/raycast_jump_kernel.hip launch_raycast_jump one of 4 raycast_jump_kernel<kMulti, kCoarse>, and the
array branch has raycast_array_kernel.  tests/test_instances_gpu.py renders every row and asks the library which kernel ran
(CLCaster.last_kernel); tests/test_kernel_resources.py checks on any machine that the rows are exactly the kernels in the built
code object.

All SVO rows are settings of the depth-12 bench scene (gpu_helpers.bench_scene(12): default coarse_log2 9, 3 stack levels):

  structure (kJump, kLdsRows, kCoarse, kBox)
    no table                          coarse_log2 = 0
    table, no jumps                   empty_boxes = 0, jump_min_run = 1 << 24
    table, jumps, global tables       empty_boxes = 0, jump_tables_lds = 0
    table, jumps, 3 rows in LDS       empty_boxes = 0 (the occupancy rule) and + jump_tables_lds = 1 (forced)
    boxes, no jumps                   jump_min_run = 1 << 24
    boxes, jumps, global tables       jump_tables_lds = 0
    boxes, jumps, 3 rows in LDS       defaults: the headline instance
    boxes, jumps, 2 rows in LDS       coarse_log2 = 7: five stack levels, where jump_tables_lds_rows' occupancy question gives two
                                      rows; also with empty_boxes = 2 (box records for the upper levels)
  mode (kMulti, kTuned)
    tuned, one light                  light_count = 1
    tuned, multi-light                light_count = 2 and 4
    run-time knobs                    single_step = 0 (no default has that value), with 1 and 3 lights; the jump structures also with
                                      jump_min_run = 2: jumps forced everywhere
  jump_min_run stays UNSET in the tuned jump rows: the library's own default -- which depends on where the tables live -- applies.

Rows are ordered so that what a tree derives (coarse table per level, empty boxes per form) is built once per tree."""
from collections import namedtuple

JUMP_OFF = 1 << 24

# family: the kernel's name; args: its template arguments in declaration order; scene: "bench12" / "terrain256";
# settings: alternatives (dicts of settings on top of the scene's defaults), every one of which must select the instance;
# lights: the light counts each alternative is rendered with
Row = namedtuple("Row", "family args scene settings lights")


def name(row):
    """The instance as C++ writes it and CLCaster.last_kernel()["name"] / bench.kernel_instance report it."""
    if not row.args:
        return row.family
    return row.family + "<" + ", ".join(str(a).lower() if isinstance(a, bool) else str(a) for a in row.args) + ">"


def symbol(row):
    """The Itanium-mangled name of the instance in the gfx950 code object."""
    enc = "".join(("Lb1E" if a else "Lb0E") if isinstance(a, bool) else f"Li{a}E" for a in row.args)
    if not row.args:
        return f"_ZN3vrc{len(row.family)}{row.family}ENS_13RaycastParamsE"
    return f"_ZN3vrc{len(row.family)}{row.family}I{enc}EEvNS_13RaycastParamsE"


# (kJump, kLdsRows, kCoarse, kBox), the alternatives that select the structure, build group (rows of one group share what the tree derives)
_STRUCTURES = [
    ((False, 0, True, False), [{"empty_boxes": 0, "jump_min_run": JUMP_OFF}], 0),
    ((True, 0, True, False), [{"empty_boxes": 0, "jump_tables_lds": 0}], 0),
    ((True, 3, True, False), [{"empty_boxes": 0}, {"empty_boxes": 0, "jump_tables_lds": 1}], 0),
    ((False, 0, True, True), [{"jump_min_run": JUMP_OFF}], 0),
    ((True, 0, True, True), [{"jump_tables_lds": 0}], 0),
    ((True, 3, True, True), [{}], 0),
    ((True, 2, True, True), [{"coarse_log2": 7}, {"coarse_log2": 7, "empty_boxes": 2}], 2),
    ((False, 0, False, False), [{"coarse_log2": 0}], 3),
]


def _svo_rows(group):
    rows = []
    for (jump, lds, coarse, box), alts, g in _STRUCTURES:
        if g != group:
            continue
        rows.append(Row("raycast_svo_kernel", (jump, False, True, lds, coarse, box), "bench12", alts, (1,)))
        rows.append(Row("raycast_svo_kernel", (jump, True, True, lds, coarse, box), "bench12", alts, (2, 4)))
        knobs = [dict(a, single_step=0) for a in alts]
        if jump:
            knobs += [dict(a, single_step=0, jump_min_run=2) for a in alts]
        rows.append(Row("raycast_svo_kernel", (jump, True, False, lds, coarse, box), "bench12", knobs, (1, 3)))
    return rows


def _mode_b_rows(coarse):
    s = {"stepping_mode": 1} if coarse else {"stepping_mode": 1, "coarse_log2": 0}
    return [Row("raycast_jump_kernel", (False, coarse), "bench12", [s], (1,)),
            Row("raycast_jump_kernel", (True, coarse), "bench12", [s], (3,))]


ROWS = (_svo_rows(0) + _mode_b_rows(True)          # the table at the default level (+ its boxes): built once
        + _svo_rows(2)                             # the table at level 7, boxes per descriptor, then for the upper levels
        + _svo_rows(3) + _mode_b_rows(False)       # no table
        + [Row("raycast_array_kernel", (), "terrain256", [{"using_octree": 1}], (1, 3))])

def _derived(case):
    """What the case's tree derives: (table level, upper-levels box form) -- cases are rendered in this order, so that every table and
    every form of the boxes is built once per tree (a box form switched off and on again is kept; another form replaces it)."""
    row, i = case
    s = row.settings[i]
    return (row.scene != "bench12", {None: 0, 7: 1, 0: 2}[s.get("coarse_log2")], s.get("empty_boxes") == 2)


# one case per (row, alternative): what tests/test_instances_gpu.py is parametrised over
CASES = sorted(((r, i) for r in ROWS for i in range(len(r.settings))), key=_derived)


def case_id(case):
    row, i = case
    tag = ",".join(f"{k}={v}" for k, v in row.settings[i].items()) or "defaults"
    return f"{name(row)}[{tag}]".replace(" ", "")
