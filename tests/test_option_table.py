"""The option sweeps' reach, checked without a GPU: every option of plan.hip's three tables has sweep values and a line in
the header, the option sweep's queries are planned down every launch shape nabo_query_plan describes, most of the stream
sweep's queries are planned down the two-level stream with local seeds (and every edge it was drawn for occurs there),
and no tool or test sets an environment variable that nothing reads."""
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


# ---- the stream sweep (tests/test_stream_sweep_gpu.py): the two-level stream and the local seeds -----------------------

STREAM_FLOOR = 0.6              # share of a metric's planned queries that must lie on the path: a condition on the generator

# cases(metric, 1)[0] and [-1] as the commit before stream_cases() returned them: replay lines name cases by their number
PINNED_CASES = {
    (0, 0): {'metric': 0, 'seed': 1, 'case': 0, 'n': 300, 'g': 17, 'flavour': 'pca', 'data_seed': 919862692, 'offset': 10.0, 'scale': 1000.0, 'quantum': 0.25, 'mask': 'few', 'mask_seed': 525378447, 'mode': None, 'dist_factor': 0.25, 'options': {'coarse_slack': 0, 'cand_slack': 0, 'seeded_pass': 0, 'coarse_adapt': 1, 'refine_overlap': 0, 'cosine_centre': 1}, 'steps': [('query', 4000, 43, False), ('set_ref', {'scale': 0.001, 'offset': 0.0, 'quantum': None}), ('query', 1, 34, False), ('query', 300, 11, True)]},
    (0, -1): {'metric': 0, 'seed': 1, 'case': 47, 'n': 40, 'g': 94, 'flavour': 'clusters', 'data_seed': 697361488, 'offset': 400.0, 'scale': 100000000000000.0, 'quantum': 0.25, 'mask': 0.05, 'mask_seed': 341015398, 'mode': None, 'dist_factor': 0.25, 'options': {'lkeep': 11, 'coarse_adapt': 1, 'wide_retry': 0, 'prepass': 50, 'split_refs_max': 0, 'cosine_centre': 0, 'coarse_kernel_q': 1}, 'steps': [('query', 1500, 10, False), ('query', 1, 32, False)]},
    (1, 0): {'metric': 1, 'seed': 1, 'case': 0, 'n': 2000, 'g': 10, 'flavour': 'lattice', 'data_seed': 235099071, 'offset': 40.0, 'scale': 0.001, 'quantum': 0.25, 'mask': 0.5, 'mask_seed': 211473360, 'mode': 'exact', 'dist_factor': 1.0, 'options': {'lkeep': 36, 'coarse_slack': 0, 'refine_overlap': 0, 'pieces': 1, 'merge_lists': 1}, 'steps': [('query', 1000, 36, False), ('set_option', 'wide_retry', 1), ('query', 1, 15, True), ('set_mask', 0.5, 648201163), ('query', 300, 55, True), ('set_mask', 0.9, 800778452), ('query', 1, 19, True)]},
    (1, -1): {'metric': 1, 'seed': 1, 'case': 39, 'n': 40, 'g': 116, 'flavour': 'clusters', 'data_seed': 112119471, 'offset': 40.0, 'scale': 100000000000.0, 'quantum': 1.0, 'mask': 0.5, 'mask_seed': 206065671, 'mode': 'exact', 'dist_factor': 0.25, 'options': {'splits': 2, 'cand_slack': 0, 'l2c_geo': 1, 'coarse_kernel_q': 0}, 'steps': [('query', 4000, 1, False), ('set_option', 'cosine_centre', 1), ('query', 40, 39, True)]},
    (2, 0): {'metric': 2, 'seed': 1, 'case': 0, 'n': 9000, 'g': 126, 'flavour': 'dups', 'data_seed': 235446697, 'offset': 400.0, 'scale': 10000000000000.0, 'quantum': 0.25, 'mask': 0.05, 'mask_seed': 670570776, 'mode': None, 'dist_factor': 0.25, 'options': {'tail_split': 1, 'coarse_slack': 20, 'seeded_pass': 1, 'coarse_adapt': 1, 'pieces': 0, 'split_refs_max': 0, 'cosine_centre': 1}, 'steps': [('query', 52, 55, True), ('set_option', 'tail_split', 0), ('set_option', 'cosine_centre', 0), ('set_ref', {'scale': 1.0, 'offset': 0.0, 'quantum': None}), ('query', 52, 28, False), ('query', 52, 57, True)]},
    (2, -1): {'metric': 2, 'seed': 1, 'case': 47, 'n': 2000, 'g': 9, 'flavour': 'dups', 'data_seed': 375124235, 'offset': 10.0, 'scale': 1000.0, 'quantum': 1.0, 'mask': 0.05, 'mask_seed': 807810139, 'mode': None, 'dist_factor': 0.25, 'options': {'coarse_slack': 0}, 'steps': [('query', 300, 15, False), ('set_mask', 0.5, 2102357), ('query', 3333, 50, False)]},
}


def test_the_stream_options_have_sweep_values_and_are_documented():
    names = S.option_names(table="LOCAL_SEED_OPTION_NAMES") + S.option_names(table="TWO_LEVEL_OPTION_NAMES")
    assert len(names) == 9 == len(set(names)) and not set(names) & set(S.option_names())
    assert set(names) == set(S.STREAM_OPTION_VALUES) == set(S.STREAM_OPTION_DEFAULTS)
    assert not set(S.STREAM_OPTION_VALUES) & set(S.OPTION_VALUES), "the two value tables stay separate"
    for name, vals in S.STREAM_OPTION_VALUES.items():
        assert len(set(vals) - {S.STREAM_OPTION_DEFAULTS[name]}) >= 1, name
    hdr = open(os.path.join(REPO, "include", "nabo_knn.h")).read()
    para = hdr[hdr.index("/* Tuning options of ONE index"):hdr.index("int nabo_index_set_option")]
    missing = [n for n in names if '"%s"' % n not in para]
    assert not missing, "options missing from the nabo_index_set_option paragraph of include/nabo_knn.h: %s" % missing


def test_the_old_sweep_still_yields_its_first_and_last_case():
    for (metric, which), want in PINNED_CASES.items():
        assert S.cases(metric, 1)[which] == want, (metric, which)


def test_stream_cases_are_deterministic_and_within_their_caps():
    with pytest.raises(ValueError):
        S.stream_cases(1, 1)
    for metric in (0, 2):
        assert S.stream_cases(metric, 1) != S.stream_cases(metric, 2)
        for seed in S.SEEDS:
            a, b = S.stream_cases(metric, seed), S.stream_cases(metric, seed)
            assert a == b and len(a) == S.STREAM_CASES
            assert a[:5] == S.stream_cases(metric, seed, 5), "a case does not depend on how many are drawn"
            for c in a:
                n, o = c["n"], c["options"]
                assert c["sweep"] == "stream" and c["mode"] is None and n in S.STREAM_N and 29 <= c["g"] <= 59
                assert c["flavour"] in S.FLAVOURS and c["mask"] in S.MASKS
                assert o["two_level"] == 2 and o["splits"] == 1 and 1 <= o["local_anchors"] <= min(n, 256)
                assert o.get("local_seeds", 1) != 0 and not set(o) & set(S.REFUSED_OPTIONS)
                assert not [name for name, leaves in S.STREAM_LEAVES.items() if name in o and name != "splits" and leaves(o[name])]
                assert 2 <= len(c["steps"]) and c["steps"][0][0] == "query" and c["steps"][-1][0] == "query"
                for st in c["steps"]:
                    if st[0] == "query":
                        _, m, k, drop = st
                        assert 1 <= m <= 1500 and 1 <= k and k + drop <= min(n, S.NABO_MAX_K) and m * n * c["g"] <= S.STREAM_CAP
                        if drop:
                            assert m <= n
                    elif st[0] == "set_option":
                        assert st[1] in S.STREAM_OPTION_VALUES or st[1] in S.OPTION_VALUES
                        assert st[1] not in S.REFUSED_OPTIONS and (st[1] != "local_anchors" or st[2] <= n)


def _stream_plans(metric):
    """(case, step, n, g, m, k, drop, options, mask, plan) of every query of the stream sweep for one metric"""
    from nabo_amd import _knn
    out = []
    for seed in S.SEEDS:
        for case, n, g, m, k, drop, mode, opts, step, mask in S.stream_planned_queries(metric, seed):
            p = _knn.query_plan(n, g, m, k, metric=metric, drop_first=drop, l2_mode=mode, options=opts)
            out.append((case, step, n, g, m, k, drop, opts, mask, p))
    return out


@pytest.mark.parametrize("metric", [0, 2])
def test_the_stream_sweep_reaches_the_two_level_stream(metric):
    """tests/test_stream_sweep_gpu.py only has teeth where the planner sends its queries down the two-level stream with local
    seeds: most of them, and among those every edge the sweep was drawn for."""
    plans = _stream_plans(metric)
    on = [q for q in plans if q[9]["two_level"] == 2 and q[9]["local_seed_buckets"] > 0]
    print("metric %d: %d of %d planned queries on the two-level stream with local seeds (%.1f %%)" % (
        metric, len(on), len(plans), 100.0 * len(on) / len(plans)))
    assert len(on) >= STREAM_FLOOR * len(plans), (len(on), len(plans))
    for _, _, n, g, m, k, drop, opts, _, p in on:
        assert p["kernel"].startswith("l2c_topk_kernel<2,1,23,6,32,4,2>") and k + drop <= S.STREAM_MAX_KK and 29 <= g <= 59, p
        assert p["splits"] == 1 and p["local_seed_buckets"] == min(opts["local_anchors"], 256), (opts, p)

    def has(what, f):
        assert any(f(*q) for q in on), "no on-path query of metric %d with %s" % (metric, what)

    has("n < 128", lambda c, s, n, g, m, k, drop, o, mask, p: n < 128)
    has("n no multiple of 32", lambda c, s, n, g, m, k, drop, o, mask, p: n % 32 != 0)
    for gg in (29, 59):
        has("g = %d" % gg, lambda c, s, n, g, m, k, drop, o, mask, p: g == gg)
    for a in (1, 256):
        has("local_anchors = %d" % a, lambda c, s, n, g, m, k, drop, o, mask, p: o["local_anchors"] == a)
    for mm in (1, 97, 385):
        has("m = %d" % mm, lambda c, s, n, g, m, k, drop, o, mask, p: m == mm)
    has("k = 1", lambda c, s, n, g, m, k, drop, o, mask, p: k == 1)
    has("k + drop = 15", lambda c, s, n, g, m, k, drop, o, mask, p: k + drop == 15)
    has("the self-drop", lambda c, s, n, g, m, k, drop, o, mask, p: drop)
    for kind in ("few", 0.9):
        has("mask %s" % kind, lambda c, s, n, g, m, k, drop, o, mask, p: mask == kind)
    for fl in S.FLAVOURS:
        has("flavour %s" % fl, lambda c, s, n, g, m, k, drop, o, mask, p: c["flavour"] == fl)
    has("no tournament", lambda c, s, n, g, m, k, drop, o, mask, p: p["tournament_tiles"] == 0)
    has("a tournament", lambda c, s, n, g, m, k, drop, o, mask, p: p["tournament_tiles"] > 0)
    for name in S.option_names(table="TWO_LEVEL_OPTION_NAMES") + ["local_cap"]:
        if name != "two_level":                               # (on the path two_level is 2: never its default)
            has("%s off its default" % name,
                lambda c, s, n, g, m, k, drop, o, mask, p: o.get(name, S.STREAM_OPTION_DEFAULTS[name]) != S.STREAM_OPTION_DEFAULTS[name])
    assert all(o["two_level"] == 2 != S.STREAM_OPTION_DEFAULTS["two_level"] for _, _, _, _, _, _, _, o, _, _ in on)
    # a resident index leaves the path and returns to it
    by_case = {}
    for q in plans:
        by_case.setdefault((q[0]["seed"], q[0]["case"]), []).append(q[9]["two_level"] == 2)
    back = [key for key, tl in by_case.items() if any(tl[a] and not tl[b] and any(tl[b + 1:]) for a in range(len(tl)) for b in range(a + 1, len(tl)))]
    assert back, "no script of metric %d leaves the two-level stream and returns to it" % metric


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
