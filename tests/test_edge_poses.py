"""CPU: the edge-pose catalogue (tests/edgeposes.py) through the oracle.

The oracle renders the whole catalogue in a child process under a time limit: the reference's walk did not end on some of these frames
(an axis-parallel ray entering the world on a grid plane), and a regression must fail here instead of hanging the suite."""
import json
import os
import subprocess
import sys

import pytest

import edgeposes as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [e.name for e in E.CATALOGUE]
COUNTERS = ("S", "E", "C", "P", "R", "lodVisits")


def render_catalogue_in_child(extra_env=None, timeout=120):
    env = dict(os.environ)
    env.update(extra_env or {})
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")])
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "edgeposes.py")], capture_output=True, text=True, env=env, timeout=timeout,
                           cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the oracle did not finish the edge-pose catalogue within {timeout} s")
    assert r.returncode == 0, f"oracle child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return json.loads(r.stdout.split("RESULT", 1)[1])


_rendered = {}


@pytest.fixture(scope="module")
def results():
    if "ok" not in _rendered and "failed" not in _rendered:  # one child per session, also when it fails (no minutes of timeouts per test)
        try:
            _rendered["ok"] = render_catalogue_in_child()
        except (AssertionError, pytest.fail.Exception) as e:
            _rendered["failed"] = str(e)
    if "failed" in _rendered:
        pytest.fail(_rendered["failed"])
    return _rendered["ok"]


@pytest.fixture(scope="module")
def fixture():
    return E.load_fixture()


@pytest.mark.parametrize("name", NAMES)
def test_entry_reaches_its_events(results, name):
    ev = results[name]["events"]
    for key, least in E.BY_NAME[name].events.items():
        assert ev[key] >= least, f"{name}: {key} = {ev[key]}, the entry needs at least {least} ({ev})"


@pytest.mark.parametrize("name", NAMES)
def test_oracle_walk_is_bounded(results, name):
    """Every ray of a bounded world leaves it within dimX + dimZ + 16 column steps: the bound the kernels' step guard assumes."""
    r = results[name]
    assert r["events"]["maxSteps"] <= r["stepBound"], (name, r["events"]["maxSteps"], r["stepBound"])


@pytest.mark.parametrize("name", NAMES)
def test_region_written_exactly_once(results, name):
    assert results[name]["region"] == [], (name, results[name]["region"])


@pytest.mark.parametrize("name", NAMES)
def test_raybuffers_match_fixture(results, fixture, name):
    r, want = results[name], fixture[name]
    assert r["rayCounts"] == want["rayCounts"]
    assert r["crcs"] == [want["crcTopDown"], want["crcLeftRight"]], name
    for k in COUNTERS:
        assert r["counters"][k] == want["counters"][k], (name, k)


def test_catalogue_covers_the_issue_list():
    """Worlds and event kinds the catalogue is meant to reach (a trimmed catalogue fails here, not silently)."""
    worlds = {e.world for e in E.CATALOGUE}
    assert {"proc256", "mill256"} <= worlds
    assert any(E.load_world(w).dims[0] != E.load_world(w).dims[2] for w in worlds)
    assert "pillars64" in worlds  # full-height columns
    reached = {k for e in E.CATALOGUE for k, v in e.events.items() if v > 0}
    assert {"dirClamped", "startOnGrid", "entrySteps", "entryNonFinite", "ties", "f2iInvalid", "projNonOrdinary", "clipExact"} <= reached
    sizes = {(e.width, e.height) for e in E.CATALOGUE}
    assert {(1, 1), (2, 1), (1, 64), (3, 2)} <= sizes and any(max(w, h) > 2048 for w, h in sizes)
    yaws = {e.euler[1] % 360 for e in E.CATALOGUE}
    assert {0.0, 90.0, 180.0, 270.0, 45.0} <= yaws
    assert {90.0, -90.0, 0.0} <= {e.euler[0] for e in E.CATALOGUE} and {90.0, 180.0} <= {e.euler[2] for e in E.CATALOGUE}


def test_events_do_not_change_the_result():
    """orc_draw_segments_events only counts: its raybuffers and counters are orc_draw_segments'."""
    import oraclelib as O

    for name in ("hang_proc256_x-3_z0", "down_proc256_integer", "yaw45_half_proc256"):
        e = E.BY_NAME[name]
        ws, fr = E.frame(e)
        a = O.draw_segments(ws, fr, e.width, e.height, clear=E.CLEAR)
        b = O.draw_segments_events(ws, fr, e.width, e.height, clear=E.CLEAR)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2].as_dict() == b[2].as_dict(), name


def test_axis_parallel_entry_draws_the_world():
    """The deviation's result: the direction-(1, 0) ray from x = -3 on the integer z = 128 (the reference never finished it) walks into proc256 --
    every column is solid there -- and draws colours, not only skybox, like its neighbours."""
    import oraclelib as O

    e = E.BY_NAME["hang_proc256_x-3_y40_z128"]
    ws, fr = E.frame(e)
    td, lr, cnt, ev = O.draw_segments_events(ws, fr, e.width, e.height, clear=E.CLEAR)
    assert ev.entryNonFinite == 1 and cnt.C > 0
    n_td, _ = E.scenes.used_rows(fr)
    rows = td[:n_td]
    drawn = [r for r in range(n_td) if ((rows[r] != E.CLEAR) & (rows[r] != E.SKYBOX)).any()]
    assert len(drawn) == n_td, f"{n_td - len(drawn)} rays of {n_td} drew nothing but skybox"
