"""The progress window of a workgroup in the two-level stream (nabo_amd/csrc/l2c_window.h), compiled for the host through
tests/wave_window_host: four threads walk a few thousand tiles as the four waves of a workgroup do in l2c_topk.hip, with
seeded random delays per tile.  Whatever the delays, every thread ends; while nobody has given up, no thread is ever seen
more than window + one check interval ahead of the slowest live one (it passes a check at most `window` ahead and runs
`check` tiles to the next); a finished wave holds nobody back; and a wave that stops publishing is got past by the give-up
bound alone.  The program is a stand-alone executable: nothing is loaded into Python."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = 4000
WIN_MAX, CHECK_MAX, WIN_DEFAULT, CHECK_DEFAULT = 4096, 64, 8, 16     # l2c_window.h


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wwin") / "window_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-I" + os.path.join(REPO, "nabo_amd", "csrc"),
                           os.path.join(REPO, "tests", "wave_window_host", "window_host.cpp"), "-o", exe])
    return exe


def _run(exe, window, check, mode, seed=1, tiles=TILES, polls_max=1 << 30):
    r = subprocess.run([exe] + [str(a) for a in (window, check, tiles, seed, mode, polls_max)], stdout=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout
    out = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in r.stdout.split()}
    print(out)
    assert out["done_passes"] == 1
    return out


def test_the_options_resolve_to_the_defaults_and_the_clamps(host):
    assert (_run(host, 0, 0, 0, tiles=8)["window"], _run(host, 0, 0, 0, tiles=8)["check"]) == (WIN_DEFAULT, CHECK_DEFAULT)
    out = _run(host, 10 ** 6, 10 ** 6, 0, tiles=8)
    assert (out["window"], out["check"]) == (WIN_MAX, CHECK_MAX)
    out = _run(host, -1, 3, 0, tiles=8)
    assert (out["window"], out["check"]) == (0, 4)                   # no window; checks fall on pairs of tiles


@pytest.mark.parametrize("window,check", [(1, 2), (0, 0), (8, 8), (32, 2), (WIN_MAX, CHECK_MAX)])
@pytest.mark.parametrize("seed", [1, 2])
def test_four_waves_stay_within_the_window_and_all_end(host, window, check, seed):
    out = _run(host, window, check, 0, seed=seed)
    assert out["ended"] == 4 and out["gave_up"] == 0
    assert out["max_ahead"] <= out["window"] + out["check"], out
    if window == 1:
        assert out["waits"] > 0, out                                 # the delays do pull the waves apart: the window acted


@pytest.mark.parametrize("window", [1, 0, WIN_MAX])
def test_a_wave_that_leaves_at_once_holds_nobody_back(host, window):
    out = _run(host, window, 2, 1)
    assert out["ended"] == 4 and out["gave_up"] == 0
    assert out["max_ahead"] <= out["window"] + out["check"], out
    # ... and a wave alone among three finished ones is the slowest live wave itself: it never waits
    out = _run(host, window, 2, 2)
    assert out["ended"] == 4 and out["gave_up"] == 0 and out["waits"] == 0 and out["max_ahead"] == 0, out


@pytest.mark.parametrize("window", [1, WIN_DEFAULT])
def test_a_wave_that_stops_publishing_is_passed_by_giving_up(host, window):
    """wave 1 falls silent half way and moves again only when the other three are out: they get there by the bound alone"""
    out = _run(host, window, 2, 3, polls_max=300)
    assert out["ended"] == 4 and out["gave_up"] == 3, out
    assert out["max_ahead"] <= out["window"] + out["check"], out      # (measured until the first of them gave up)
    assert out["polls"] >= 3 * 300
