"""CPU: the Phase-2 rule itself (oraclelib.blit_reference, the numpy restatement of blit_classify in cvx_kernels.h) over the blit catalogue
(tests/blitposes.py), against the independent float64 rule (oraclelib.blit_reference_f64).

Raybuffers come from the oracle, cleared to a sentinel no voxel colour has; the image clear colour is a second sentinel.  The whole catalogue is
rendered once, in a child process under a time limit, the way tests/test_edge_poses.py does (it holds that catalogue's frames).

One check is deliberately not here -- that the rays a segment's pixels reference are contiguous from the first to the last: it does not hold
for the rule, for a geometric reason.  A segment has as many rays as its base edge has pixels along the longer screen dimension, and that base is cut by the screen or runs at an
angle to the pixel grid, so neighbouring rays lie closer than one pixel on screen and a ray's wedge can pass between pixel centres without holding
one (edge_roll180: one segment of 89 rays on a 64-pixel-wide screen, ray 44 is never shown; random_1000x1_0: 422 such rays).  An off-by-one in
blit_ray's clamp is caught by test_rule_equals_the_float64_rule_outside_the_margin, whose margin includes the ray coordinate."""
import json
import os
import subprocess
import sys

import pytest

import blitposes as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = B.CPU_NAMES


def render_catalogue_in_child(timeout=300):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")])
    env["CVX_NO_TORCH_PRELOAD"] = "1"
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "blitposes.py")], capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the oracle and the rules did not finish the blit catalogue within {timeout} s")
    assert r.returncode == 0, f"child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.loads(r.stdout.split("RESULT", 1)[1])


_rendered = {}


@pytest.fixture(scope="module")
def results():
    if "ok" not in _rendered and "failed" not in _rendered:  # one child per session, also when it fails
        try:
            _rendered["ok"] = render_catalogue_in_child()
        except (AssertionError, pytest.fail.Exception) as e:
            _rendered["failed"] = str(e)
    if "failed" in _rendered:
        pytest.fail(_rendered["failed"])
    return _rendered["ok"]


@pytest.fixture(scope="module")
def fixture():
    return B.load_fixture()


@pytest.mark.parametrize("name", NAMES)
def test_no_holes(results, name):
    """A pixel carries the image clear colour only where the float64 rule assigns no segment either.  Before the seam rule of blit_classify:
    28, 9 and 2 such pixels on sweep_pitch30_roll45, sweep_pitch20_roll45, sweep_pitch29_roll45 (a dotted line along the seam of segments 0 and 2)."""
    r = results[name]
    print(name, "holes", r["holes"], "before the seam rule", r["holesBeforeSeamRule"], "pixels the seam rule assigns", r["seamRulePixels"])
    assert r["holes"] == 0, f"{name}: {r['holes']} pixels that the float64 rule gives to a segment carry the clear colour"


@pytest.mark.parametrize("name", NAMES)
def test_seam_rule_claims_nothing_away_from_a_boundary(results, name):
    """The other side of the seam rule's eps: no pixel the float64 rule leaves to no segment with a margin above 1e-4 is given to one."""
    assert results[name]["claimedBeyondMargin"] == 0, name


def test_seam_frames_had_the_holes_the_rule_repairs(results):
    """The three frames the seam rule was made for, with the rule switched off in the numpy restatement: the pixel counts measured on the parent."""
    for name, holes in B.SEAM_FRAMES.items():
        assert results[name]["holesBeforeSeamRule"] == holes, (name, results[name]["holesBeforeSeamRule"])
        assert results[name]["seamRulePixels"] == holes and results[name]["holes"] == 0, name


@pytest.mark.parametrize("name", NAMES)
def test_rule_equals_the_float64_rule_outside_the_margin(results, fixture, name):
    """blit_reference == blit_reference_f64 at every pixel whose margin is above 1e-4: a hard zero.  Inside the margin the two may differ; how many
    pixels do is recorded, and stays under 2e-3 of the screen except where the reference rule alone cannot keep that: frames whose VP is the
    screen centre (the diagonals pass through pixel centres all along) and screens of fewer pixels than one tile."""
    r, b, want = results[name], B.BY_NAME[name], fixture[name]
    share = r["differInsideMargin"] / r["pixels"]
    print(name, "differ inside the margin", r["differInsideMargin"], "of", r["pixels"], f"({share:.2e})", "beyond", r["differBeyondMargin"])
    assert r["differBeyondMargin"] == 0, f"{name}: {r['differBeyondMargin']} pixels away from every boundary differ from the float64 rule"
    assert r["rayCounts"] == want["rayCounts"], name
    assert r["differInsideMargin"] == want["differInsideMargin"], (name, r["differInsideMargin"], want["differInsideMargin"])
    assert r["crcImage"] == want["crcImage"], name
    if "vp_centre" not in b.tags and "tiny" not in b.tags:
        assert share < 2e-3, f"{name}: {r['differInsideMargin']} of {r['pixels']} pixels differ from the float64 rule"


@pytest.mark.parametrize("name", NAMES)
def test_reads_only_written_pixels(results, name):
    assert results[name]["readsUnwritten"] == 0, f"{name}: {results[name]['readsUnwritten']} image pixels read a raybuffer pixel Phase 1 never wrote"


@pytest.mark.parametrize("name", NAMES)
def test_tagged_entries_have_their_property(results, name):
    r = results[name]
    for tag in B.BY_NAME[name].tags:
        assert r["tags"][tag], f"{name} is tagged {tag} and its frame does not have the property"
    for tag in ("tiny", "vp_centre"):  # the tags that exempt an entry from the share cap are exactly the property
        assert r["tags"][tag] == (tag in B.BY_NAME[name].tags), (name, tag)


def test_every_tag_is_carried():
    carried = {t for b in B.CATALOGUE for t in b.tags}
    assert set(B.TAGS) <= carried, set(B.TAGS) - carried
    assert set(B.SEAM_FRAMES) <= {b.name for b in B.CATALOGUE if "seam_through_centres" in b.tags}


def test_catalogue_holds_what_the_issue_lists():
    import edgeposes as E

    names = set(B.BY_NAME)
    assert {"edge_" + e.name for e in E.CATALOGUE} <= names
    assert {f"sweep_pitch{p:g}_roll{r:g}" for p in B.SWEEP_PITCH for r in B.SWEEP_ROLL} <= names and len(B.SWEEP_PITCH) * len(B.SWEEP_ROLL) == 42
    sizes = {(b.width, b.height) for b in B.CATALOGUE if b.name.startswith("random_")}
    assert sizes == {(333, 217), (97, 401), (65, 17), (63, 15), (129, 65), (1000, 1), (640, 360), (2049, 70)}
    assert {"scene_" + n for n in B.BLIT_SCENES} <= names and B.BY_NAME["scene_mill512_t075_1080p"].gpu_only
    assert sum(1 for b in B.CATALOGUE if b.gpu_only) == 1


def test_partial_width_tiles_of_every_kind(results):
    """What makes the image comparison and the guard rows of tests/test_gpu_blit.py sensitive to a wrong bound in a partial tile (x1, `x0 + c <= x1`,
    `px <= x1`): the catalogue holds partial-width tiles that the kernel treats each of its three ways -- owned by a top / bottom segment (straight
    stores), owned by a left / right segment (LDS gather) and searched per pixel -- for the single blit (16 rows) and the batch blit (64 rows).
    From the tile arithmetic alone (blitposes.tile_kinds: the owner test of blit_block over the float64 weights), no out-of-range launch."""
    for rows in ("16", "64"):
        kinds = {k for n in NAMES for k in results[n]["tileKinds"][rows]}
        assert kinds == {"td", "lr", "search"}, (rows, kinds)
    # ... and a last tile of one pixel, a screen narrower than a tile, one past 2048
    widths = {B.BY_NAME[n].width for n in NAMES}
    assert any(w % 64 == 1 and w > 64 for w in widths) and any(w < 64 for w in widths) and any(w > 2048 for w in widths)
