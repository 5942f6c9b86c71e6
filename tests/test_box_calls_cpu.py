"""CPU (no GPU needed): what the calls that take a box and read the world refuse, with which code and text and in which order
(tests/box_calls_rules.cpp, on a bare context: no device, no world).  The table below is the library's behaviour as it stood before the box
rules, the world gate and the list driver were each written once; it pins what that work may not move.

Every entry runs the same cases (CASES; an entry whose box lies in a struct has no NULL-pointer cases, an entry without the argument a case
breaks ignores that).  A case an entry's table does not name passes every check and ends at NOT_READY: there is no world."""
import subprocess

import pytest

import ruleslib

NOT_READY = "-3|world LOD 0 has not been uploaded"

CASES = [
    "NULL boxMin", "NULL boxMax",
    "min == max on axis 0", "min > max on axis 0", "min == max on axis 1", "min > max on axis 1", "min == max on axis 2", "min > max on axis 2",
    "max at 2^30", "min at -2^30", "max at 2^30 + 1", "min at -2^30 - 1",
    "2048 x 1024 x 1024", "2047 x 1024 x 1024", "65536 x 1 x 32768", "65535 x 1 x 32768",
    "negative capacity", "capacity with a NULL list", "bad flags", "NULL output",
    "empty box and bad flags", "empty box and NULL output",
    "valid, no world yet",
]


def empty_axes(prefix):
    """The six empty-axis cases: every family words them alike, behind its own prefix."""
    return {
        "min == max on axis 0": f"-1|{prefix}the box [3, 3) on axis 0 is empty",
        "min > max on axis 0": f"-1|{prefix}the box [5, 4) on axis 0 is empty",
        "min == max on axis 1": f"-1|{prefix}the box [3, 3) on axis 1 is empty",
        "min > max on axis 1": f"-1|{prefix}the box [5, 4) on axis 1 is empty",
        "min == max on axis 2": f"-1|{prefix}the box [3, 3) on axis 2 is empty",
        "min > max on axis 2": f"-1|{prefix}the box [5, 4) on axis 2 is empty",
    }


def beyond(prefix):
    """The two coordinates one past +-2^30, where the family tests them."""
    return {
        "max at 2^30 + 1": f"-1|{prefix}the box [1073741824, 1073741825) on axis 1 has a coordinate beyond 2^30",
        "min at -2^30 - 1": f"-1|{prefix}the box [-1073741825, -1073741824) on axis 2 has a coordinate beyond 2^30",
    }


def voxels(prefix):
    return {"2048 x 1024 x 1024": f"-1|{prefix}a box of 2^31 or more voxels", "65536 x 1 x 32768": f"-1|{prefix}a box of 2^31 or more voxels"}


def dense(extra):
    """read / write voxels, distance: NULL, +-2^30, empty, 2^31 voxels, all behind "<call>: "."""
    return {"NULL boxMin": "-1|{call}: a NULL box", "NULL boxMax": "-1|{call}: a NULL box", **empty_axes("{call}: "), **beyond("{call}: "), **voxels("{call}: "),
            "empty box and bad flags": "-1|{call}: the box [0, 0) on axis 1 is empty", "empty box and NULL output": "-1|{call}: the box [0, 0) on axis 1 is empty", **extra}


def heights(extra):
    return {**dense(extra), "2048 x 1024 x 1024": NOT_READY, "65536 x 1 x 32768": "-1|{call}: a footprint of 2^31 or more columns"}


def clipped(null, extra):
    """The families that clip the box to the world: no test of +-2^30 or of the voxel count, the empty axis without a prefix."""
    table = {**empty_axes(""), "empty box and bad flags": "-1|the box [0, 0) on axis 1 is empty", "empty box and NULL output": "-1|the box [0, 0) on axis 1 is empty", **extra}
    if null:
        table.update({"NULL boxMin": null, "NULL boxMax": null})
    return table


def instance_box(extra):
    return {**empty_axes("{call}: instance 0: "), **beyond("{call}: instance 0: "), "empty box and bad flags": "-1|{call}: instance 0: the box [0, 0) on axis 1 is empty",
            "empty box and NULL output": "-1|{call}: instance 0: the box [0, 0) on axis 1 is empty", **extra}


LIGHT = {**{case: "-1|cvx_light_params: bad boxMin >= boxMax" for case in empty_axes("")}, "bad flags": "-1|levelCount 9 outside 0 .. 5",
         "empty box and bad flags": "-1|cvx_light_params: bad boxMin >= boxMax", "empty box and NULL output": "-1|cvx_light_params: bad boxMin >= boxMax"}

# entry -> (the box is two pointers, {case: line}); "{call}" is the entry's own name
TABLE = {
    "cvx_world_read_voxels": (True, dense({"NULL output": "-1|{call}: argb and solid are both NULL"})),
    "cvx_world_write_voxels": (True, dense({"bad flags": "-1|{call}: bad op 99", "NULL output": "-1|{call}: argb is NULL (only a CARVE with a solid mask may leave it out)"})),
    "cvx_world_read_heights": (True, heights({"NULL output": "-1|{call}: heights, argb and bottoms are all NULL"})),
    "cvx_world_write_heights": (True, heights({"bad flags": "-1|{call}: unknown flag bits 0x80", "NULL output": "-1|{call}: heights is NULL"})),
    "cvx_world_distance": (True, dense({"bad flags": "-1|{call}: solidOutside 0x40 has bits above 0x3F", "NULL output": "-1|{call}: out is NULL"})),
    # (a NULL out is named before the box)
    "cvx_world_spread": (False, {**empty_axes("{call}: "), **beyond("{call}: "), **voxels("{call}: "), "bad flags": "-1|{call}: bad medium 7",
                                 "NULL output": "-1|{call}: out is NULL", "empty box and bad flags": "-1|{call}: the box [0, 0) on axis 1 is empty",
                                 "empty box and NULL output": "-1|{call}: out is NULL"}),
    "cvx_world_surface": (True, clipped("-1|{call}: a NULL box", {"negative capacity": "-1|quadCapacity -1 with a list", "capacity with a NULL list": "-1|quadCapacity 2 with no list",
                                                                 "bad flags": "-1|unknown flags bits 0x80"})),
    "cvx_world_surface_rects": (True, clipped("-1|{call}: a NULL box", {"negative capacity": "-1|rectCapacity -1 with a list",
                                                                       "capacity with a NULL list": "-1|rectCapacity 2 with no list", "bad flags": "-1|unknown flags bits 0x80"})),
    "cvx_world_pieces": (True, clipped("-1|the box is NULL", {"negative capacity": "-1|pieceCapacity -1 with a list", "capacity with a NULL list": "-1|pieceCapacity 2 with no list",
                                                             "bad flags": "-1|unknown anchors bits 0x80"})),
    "cvx_world_cavities": (False, clipped(None, {"negative capacity": "-1|cavityCapacity -1 with a list", "capacity with a NULL list": "-1|cavityCapacity 2 with no list",
                                                 "bad flags": "-1|unknown openFaces bits 0x40"})),
    # (a NULL outField is named before the box, the box before the body's measures)
    "cvx_world_nav_build": (False, clipped(None, {"bad flags": "-1|width 0 outside 1 .. 8, height 3 outside 1 .. 64, stepUp 1 outside 0 .. height or maxDrop 4 outside 0 .. 4096",
                                                  "NULL output": "-1|params or outField is NULL", "empty box and NULL output": "-1|params or outField is NULL"})),
    "cvx_world_light": (False, LIGHT),
    "cvx_world_light_lamps": (False, LIGHT),
    "cvxc_world_contacts": (False, instance_box({"negative capacity": "-1|{call}: pointCapacity -1 with a list", "capacity with a NULL list": "-1|{call}: pointCapacity 2 with no list",
                                                 "bad flags": "-1|{call}: unknown solidOutside bits 0x40", "NULL output": "-1|{call}: results is NULL"})),
    # (an instance's op is named before its box)
    "cvx_world_place_models": (False, instance_box({"bad flags": "-1|{call}: instance 0: bad op 99", "empty box and bad flags": "-1|{call}: instance 0: bad op 99"})),
}
WITH_DEVICE_FORM = ["cvx_world_read_voxels", "cvx_world_write_voxels", "cvx_world_read_heights", "cvx_world_write_heights", "cvx_world_distance", "cvx_world_spread",
                    "cvx_world_surface", "cvx_world_surface_rects", "cvxc_world_contacts", "cvx_world_place_models"]
ENTRIES = [(name + suffix, name) for name in TABLE for suffix in (("", "_device") if name in WITH_DEVICE_FORM else ("",))]

# NULL snapshot; bad flags; negative capacity; NULL list; bad flags and negative capacity; NULL snapshot, bad flags and NULL list; two valid calls
SNAPSHOT_DIFF = ["-1|{call}: snap is NULL", "-1|{call}: unknown flags bits 0x80", "-1|{call}: changeCapacity -1 with a list", "-1|{call}: changeCapacity 2 with no list",
                 "-1|{call}: unknown flags bits 0x80", "-1|{call}: snap is NULL", NOT_READY, NOT_READY]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """entry -> its lines, and the program's case names."""
    program = ruleslib.build("box_calls_rules", tmp_path_factory.mktemp("box_calls"))
    blocks, entry = {}, None
    for line in subprocess.run([program], check=True, capture_output=True, text=True).stdout.splitlines():
        if line.startswith("# "):
            entry = line[2:]
            blocks[entry] = []
        else:
            blocks[entry].append(line)
    return blocks, subprocess.run([program, "cases"], check=True, capture_output=True, text=True).stdout.splitlines()


def test_the_cases_are_the_programs(printed):
    assert printed[1] == CASES


def test_every_entry_is_in_the_table(printed):
    assert sorted(printed[0]) == sorted([entry for entry, _ in ENTRIES] + ["cvx_world_snapshot_diff", "cvx_world_snapshot_diff_device"])


@pytest.mark.parametrize("entry,family", ENTRIES, ids=[entry for entry, _ in ENTRIES])
def test_box_refusals(printed, entry, family):
    pointers, table = TABLE[family]
    assert set(table) <= set(CASES)
    cases = [case for case in CASES if pointers or not case.startswith("NULL box")]
    expected = [table.get(case, NOT_READY).replace("{call}", entry) for case in cases]
    assert list(zip(cases, printed[0][entry])) == list(zip(cases, expected))
    assert len(printed[0][entry]) == len(cases)


@pytest.mark.parametrize("entry", ["cvx_world_snapshot_diff", "cvx_world_snapshot_diff_device"])
def test_snapshot_diff_refusals(printed, entry):
    assert printed[0][entry] == [line.replace("{call}", entry) for line in SNAPSHOT_DIFF]
