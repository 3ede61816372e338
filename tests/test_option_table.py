"""The option sweep's reach, checked without a GPU: every option of plan.hip has sweep values and a line in the header,
the sweep's queries are planned down every launch shape nabo_query_plan describes, and no tool or test sets an
environment variable that nothing reads."""
import ast
import glob
import os
import re

import pytest

import _option_sweep as S

REPO = S.REPO


def test_every_option_has_sweep_values_and_is_documented():
    names = S.option_names()
    assert len(names) == len(set(names))
    assert set(names) == set(S.OPTION_VALUES), "OPTION_NAMES (plan.hip) and OPTION_VALUES (tests/_option_sweep.py) differ"
    hdr = open(os.path.join(REPO, "include", "nabo_knn.h")).read()
    para = hdr[hdr.index("/* Tuning options of ONE index"):hdr.index("int nabo_index_set_option")]
    missing = [n for n in names if '"%s"' % n not in para]
    assert not missing, "options missing from the nabo_index_set_option paragraph of include/nabo_knn.h: %s" % missing


def test_cases_are_deterministic_and_within_the_documented_limits():
    for metric in (0, 1, 2):
        for seed in S.SEEDS:
            a, b = S.cases(metric, seed), S.cases(metric, seed)
            assert a == b
            for c in a:
                assert c["n"] <= 70000 and 1 <= c["g"] <= 128
                assert not set(c["options"]) & set(S.REFUSED_OPTIONS)
                assert 2 <= len(c["steps"]) and c["steps"][0][0] == "query"
                for st in c["steps"]:
                    if st[0] == "query":
                        _, m, k, drop = st
                        assert 1 <= m and 1 <= k and k + drop <= c["n"] and m * c["n"] * c["g"] <= S.CAP[metric]
                        if drop:
                            assert m <= c["n"]


def _plans():
    from nabo_amd import _knn
    seen = []
    for metric in (0, 2):
        for seed in S.SEEDS:
            for case, n, g, m, k, drop, mode, opts in S.planned_queries(metric, seed):
                p = _knn.query_plan(n, g, m, k, metric=metric, drop_first=drop, l2_mode=mode, options=opts)
                assert p == _knn.query_plan(n, g, m, k, metric=metric, drop_first=drop, l2_mode=mode, options=opts), \
                    "query_plan is documented as a pure function"
                seen.append((mode, p))
    for c in S.large_cases():
        p = _knn.query_plan(c["n"], c["g"], c["m"], c["k"], metric=c["metric"], drop_first=c["drop"], l2_mode=c.get("mode"),
                            options=c["options"])
        if "tail" in c["name"]:
            assert p["workgroups_tail"] > 0, (c["name"], p)
        seen.append((c.get("mode"), p))
    return seen


def test_sweep_queries_are_planned_down_every_launch_shape():
    """The GPU sweep (tests/test_option_sweep_gpu.py) only has teeth where its queries take each route: first passes,
    one-product geometries, reference splits, tail launches, tournament seeds, both list lengths, both second filters."""
    plans = _plans()
    got = lambda f: {p[f] for _, p in plans}                                      # noqa: E731
    assert {0, 2, 4} <= got("first_pass"), got("first_pass")
    assert {0, 1, 2} <= got("geometry"), got("geometry")
    assert max(got("splits")) > 1
    assert max(got("workgroups_tail")) > 0
    assert 0 in got("tournament_tiles") and max(got("tournament_tiles")) > 0
    assert {32, 64} <= got("list_len")
    first2 = {p["kernel"].split("<")[0] for _, p in plans if p["first_pass"] == 2}
    assert {"l2q_topk_kernel", "l2_topk_kernel"} <= first2, first2              # the f16x3 and the fp32 first pass
    assert any(m == "f16x3" and p["kernel"].startswith("l2q") for m, p in plans)
    assert any(m == "f32" and p["kernel"].startswith("l2_topk") for m, p in plans)


def test_canberra_cases_cross_the_bitmap_threshold_and_every_mode():
    cs = [c for seed in S.SEEDS for c in S.cases(1, seed)]
    assert {c["mode"] for c in cs} == set(S.CANBERRA_MODES)
    assert {c["dist_factor"] for c in cs} == set(S.DIST_FACTORS)
    assert any(c["n"] >= S.CB_BITMAP_REFS for c in cs) and any(c["n"] < S.CB_BITMAP_REFS for c in cs)


# ---- no silent knobs --------------------------------------------------------------------------------------------------

NABO_NAME = re.compile(r"NABO_[A-Z0-9_]+\Z")


def _py_files(*parts):
    out = []
    for p in parts:
        full = os.path.join(REPO, p)
        out += [full] if full.endswith(".py") else glob.glob(os.path.join(full, "**", "*.py"), recursive=True)
    return sorted(out)


def _is_environ(node):
    return isinstance(node, ast.Attribute) and node.attr == "environ"


def _env_reads(path):
    """NABO_* names read through os.environ.get(...), os.environ[...] or os.getenv(...)."""
    names = set()
    for node in ast.walk(ast.parse(open(path).read(), path)):
        key = None
        if isinstance(node, ast.Call) and node.args and isinstance(node.args[0], ast.Constant):
            f = node.func
            if isinstance(f, ast.Attribute) and ((f.attr == "get" and _is_environ(f.value)) or f.attr == "getenv"):
                key = node.args[0].value
        elif isinstance(node, ast.Subscript) and _is_environ(node.value) and isinstance(node.ctx, ast.Load):
            key = node.slice.value if isinstance(node.slice, ast.Constant) else None
        if isinstance(key, str) and NABO_NAME.match(key):
            names.add(key)
    return names


def _nabo_names_set(path):
    """Every NABO_* name a file could put into an environment: string constants that ARE such a name (os.environ[...] =,
    setenv, env dicts, lists of switches) and keyword names (dict(os.environ, NABO_X=...))."""
    names = set()
    for node in ast.walk(ast.parse(open(path).read(), path)):
        if isinstance(node, ast.Constant) and isinstance(node.value, str) and NABO_NAME.match(node.value):
            names.add(node.value)
        elif isinstance(node, ast.keyword) and node.arg and NABO_NAME.match(node.arg):
            names.add(node.arg)
    return names


def read_names():
    names = set()
    for path in glob.glob(os.path.join(REPO, "nabo_amd", "csrc", "*.hip")) + glob.glob(os.path.join(REPO, "nabo_amd", "csrc", "*.h")):
        names |= set(re.findall(r'getenv\(\s*"(NABO_[A-Z0-9_]+)"', open(path).read()))
    for path in _py_files("nabo_amd", "bench.py", "oracle", "tests"):
        names |= _env_reads(path)
    return names


def test_no_tool_or_test_sets_a_variable_nothing_reads():
    """Options moved from environment variables to nabo_index_set_option once, and two randomised sweeps went on setting
    the old names for months -- covering the default configuration only.  A NABO_* name set by a tool or a test must be
    one the library, the package, bench.py, the oracle or the tests read."""
    read = read_names()
    assert {"NABO_L2_MODE", "NABO_CANBERRA_MODE"} <= read, read
    silent = {}
    for path in _py_files("tests") + sorted(glob.glob(os.path.join(REPO, "tools", "*.py"))):
        extra = _nabo_names_set(path) - read
        if extra:
            silent[os.path.relpath(path, REPO)] = sorted(extra)
    assert not silent, "NABO_* names set but read by nothing: %s" % silent


@pytest.mark.parametrize("snippet,caught", [('import os\nos.environ["NABO_SPLITS"] = "1"\n', True),
                                            ('import os\nenv = dict(os.environ, NABO_LKEEP="3")\n', True),
                                            ('def f(mp):\n    mp.setenv("NABO_L2_MODE", "f32")\n', False)])
def test_the_silent_knob_scan_sees_the_usual_forms(tmp_path, snippet, caught):
    p = tmp_path / "t.py"
    p.write_text(snippet)
    assert bool(_nabo_names_set(str(p)) - read_names()) == caught
