"""Seeded cases for the option sweep (tests/test_option_sweep_gpu.py, tests/test_option_table.py, tools/stress_sweep3.py)
and for the stream sweep (tests/test_stream_sweep_gpu.py, tests/test_option_table.py).

include/nabo_knn.h promises that every index option returns the SAME BITS: an option chooses how a launch is cut or which
filter pass answers a row, never what the answer is.  The only guard against a subtly wrong pass is oracle parity on inputs
that actually route rows through that pass, so this module draws index options, L2 / Canberra modes, shapes, data flavours
and short scripts of calls on one resident index that reach every pass.  Pure Python + numpy: no GPU, no oracle.

Two generators, each with a random stream and value tables of its own.  cases() draws from OPTION_NAMES[] of plan.hip over
shapes up to 70 000 references -- below the sizes at which the planner takes the two-level stream and the local seeds, so it
never reaches them.  stream_cases() starts every index ON that path (two_level = 2, one reference split, d = 29..59) and
draws the nine options of LOCAL_SEED_OPTION_NAMES[] and TWO_LEVEL_OPTION_NAMES[] as well, from STREAM_OPTION_VALUES.

A case is a plain dict; make_ref / make_targets / make_mask rebuild its arrays from the seeds it carries, so a failing
case is reproduced from (metric, seed, case number) alone."""
import os
import re

import numpy as np

from nabo_amd._synth import pca_like

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API_SOURCE = os.path.join(REPO, "nabo_amd", "csrc", "plan.hip")

NABO_MAX_K = 56                 # include/nabo_knn.h: k + drop_first of the filter kernels; beyond it the exact route
CB_BITMAP_REFS = 12 * 2048      # set_ref.hip: a modified-Canberra index builds bitmaps from this many references on
L2_MODES = (None, "f16x3", "f32")                    # NABO_L2_MODE (read once, in nabo_index_create)
CANBERRA_MODES = (None, "exact", "swar", "bits")     # NABO_CANBERRA_MODE (None: by the size of the reference set)
DIST_FACTORS = (0.1, 0.25, 1.0, 3.0)
FLAVOURS = ("pca", "clusters", "scaled", "lattice", "dups")
MASKS = (None, 0.05, 0.5, 0.9, "few")
SEEDS = (1, 2, 3)                                    # the sweep runs cases(metric, seed) for each
CAP = {0: 6 * 10 ** 7, 1: 2 * 10 ** 7, 2: 6 * 10 ** 7}   # m * n * g of one query (the oracle's full-row cost)

# The values drawn for every option of nabo_index_set_option.  Strings are resolved per query shape (resolve()):
# "kk" = k + drop_first, "kk+1", "list" = the longest list the first pass can keep (64), "fit" = the smallest
# split_refs_max that keeps a query within the 1024 / L splits refine merges.
OPTION_VALUES = {
    "splits": (0, 1, 2, 5, 32),
    "tail_split": (0, 1),
    "lkeep": (0, "kk", "kk+1", "list", 1000),          # 1000: out of range, ignored by design
    "coarse_slack": (-1, 0, 6, 20),
    "cand_slack": (-1, 0, 3, 8),
    "seeded_pass": (0, 1),
    "coarse_adapt": (0, 1),
    "wide_retry": (0, 1),
    "refine_overlap": (0, 1),
    "prepass": (0, 50, 100, 400),
    "pieces": (0, 1),                                  # removed; accepted as a no-op
    "merge_lists": (0, 1),
    "one_round": (0, 1),
    "l2c_geo": (-1, 0, 1, 2),
    "l2_r1": (-1, 0, 1),
    "split_refs_max": (0, "fit"),
    "cosine_centre": (0, 1),                           # takes effect at the next set_ref
    "coarse_kernel_q": (0, 1),
    "order_flags": (0, 1),                             # removed; REFUSED by nabo_index_set_option
}
REFUSED_OPTIONS = ("order_flags",)                     # never drawn into a case; tests check the refusal itself


def option_names(path=API_SOURCE, table="OPTION_NAMES"):
    """The names of one option table of plan.hip (OPTION_NAMES[], LOCAL_SEED_OPTION_NAMES[] or TWO_LEVEL_OPTION_NAMES[]),
    in table order."""
    src = open(path).read()
    body = re.search(r"\b%s\[\]\s*=\s*\{(.*?)\n\};" % re.escape(table), src, re.S).group(1)
    return re.findall(r'\{\s*"([a-z0-9_]+)"\s*,', body)


def resolve(name, value, n, kk):
    """An OPTION_VALUES entry as the integer nabo_index_set_option gets for a query of k' = kk over n references."""
    if not isinstance(value, str):
        return int(value)
    if value == "kk":
        return kk
    if value == "kk+1":
        return kk + 1
    if value == "list":
        return 64
    if value == "fit":
        # plan.hip: split_tiles = (split_refs_max - 1) / 32, s_min = ceil(ref_tiles / split_tiles) <= 1024 / 64 = 16
        tiles = (n + 31) // 32
        split_tiles = max(2, -(-tiles // 16))
        return 32 * split_tiles + 1
    raise ValueError("unknown symbolic option value %r of %s" % (value, name))


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _draw_options(rng, metric, n, kk, p):
    """Each drawable option with probability p, its value uniformly from OPTION_VALUES."""
    opts = {}
    for name, vals in OPTION_VALUES.items():
        if name in REFUSED_OPTIONS or rng.random() >= p:
            continue
        opts[name] = resolve(name, _pick(rng, vals), n, kk)
    return opts


def _shape(rng, metric, big):
    if metric == 1:
        n = int(_pick(rng, (40, 300, 2000, 9000, 26000, 40000) if big else (40, 300, 2000, 9000)))
    else:
        n = int(_pick(rng, (40, 300, 2000, 9000, 30000, 70000) if big else (40, 300, 2000, 9000)))
    if rng.random() < 0.5:
        g = int(_pick(rng, (1, 2, 29, 30, 50, 61, 62, 64, 93, 94, 100, 125, 126, 128)))
    else:
        g = int(rng.integers(1, 129))
    return n, g


def _query(rng, metric, n, g, cap, exact_share=0.06):
    """("query", m, k, drop): k + drop up to NABO_MAX_K, now and then beyond it; m capped by m * n * g <= cap."""
    drop = bool(rng.random() < 0.3)
    kmax = min(n - (1 if drop else 0), NABO_MAX_K - (1 if drop else 0))
    if rng.random() < exact_share and n > NABO_MAX_K + 10:
        k = int(rng.integers(NABO_MAX_K, min(n - 1, 90)))       # beyond the filter kernels: the exact route
    elif rng.random() < 0.5:
        k = int(min(kmax, _pick(rng, (1, 5, 11, 15, 20, 23, 24, 25, 28, 29, 32, 40, 43, 50, 55, 56))))
    else:
        k = int(rng.integers(1, kmax + 1))
    m = int(_pick(rng, (1, 33, 300, 1500, 4000)))
    m = max(1, min(m, cap // (n * g)))
    if drop:
        m = min(m, n)
    return ("query", m, k, drop)


def cases(metric, seed, n_cases=None):
    """The deterministic case list of one metric (0 Euclidean, 1 modified Canberra, 2 cosine) and seed."""
    rng = np.random.default_rng([metric, seed, 0x5eed])
    if n_cases is None:
        n_cases = 40 if metric == 1 else 48
    cap = CAP[metric]
    out = []
    for i in range(n_cases):
        n, g = _shape(rng, metric, big=rng.random() < 0.35)
        flavour = _pick(rng, FLAVOURS)
        case = {
            "metric": metric, "seed": seed, "case": i, "n": n, "g": g, "flavour": flavour,
            "data_seed": int(rng.integers(1, 1 << 30)),
            "offset": float(_pick(rng, (10.0, 40.0, 400.0))),            # clusters: how far from the origin
            "scale": float(10.0 ** int(rng.integers(-15, 16))),           # scaled: 1e-15 .. 1e15
            "quantum": float(_pick(rng, (0.25, 1.0))),                    # lattice: exact ties
            "mask": _pick(rng, MASKS), "mask_seed": int(rng.integers(1, 1 << 30)),
            "mode": _pick(rng, CANBERRA_MODES if metric == 1 else L2_MODES + (None, None)),
            "dist_factor": float(_pick(rng, DIST_FACTORS)) if metric == 1 else 0.25,
        }
        first = _query(rng, metric, n, g, cap)
        case["options"] = _draw_options(rng, metric, n, first[2] + first[3], 0.3)
        steps = [first]
        for _ in range(int(rng.integers(1, 4))):
            what = rng.random()
            if what < 0.3:
                name = _pick(rng, [o for o in OPTION_VALUES if o not in REFUSED_OPTIONS])
                steps.append(("set_option", name, resolve(name, _pick(rng, OPTION_VALUES[name]), n, NABO_MAX_K)))
            elif what < 0.5:
                steps.append(("set_mask", _pick(rng, MASKS), int(rng.integers(1, 1 << 30))))
            elif what < 0.75:
                # new reference data: another scale / offset / quantisation of the same shape (every cached pack, centre,
                # weak-bound memory, quantile edge and valid-count must follow it)
                steps.append(("set_ref", {"scale": float(_pick(rng, (1e-3, 0.5, 1.0, 7.0, 1e6))),
                                          "offset": float(_pick(rng, (0.0, 3.0, -50.0, 1e3))),
                                          "quantum": _pick(rng, (None, None, 0.5))}))
            if metric == 2 and rng.random() < 0.25:
                steps.append(("set_option", "cosine_centre", int(rng.integers(0, 2))))
                steps.append(("set_ref", {"scale": 1.0, "offset": 0.0, "quantum": None}))
            steps.append(_query(rng, metric, n, g, cap))
        case["steps"] = steps
        out.append(case)
    return out


# ---- the stream sweep: the two-level stream and the local seeds (tests/test_stream_sweep_gpu.py) ---------------------

# cases() above never reaches the two-level stream (option two_level = 2 or n >= 2^18) nor the local seeds' buckets, and its
# draws are pinned by replay lines.  stream_cases() is a generator of its own -- own rng stream, own value tables -- whose
# cases start ON that path: two_level = 2, one reference split, d in 29..59, k + drop <= 15 in four queries of five.
STREAM_TAG = 0x2712e
STREAM_CAP = 2 * 10 ** 7                                # m * n * g of one query
STREAM_CASES = 24                                       # per (metric, seed)
STREAM_N = (4, 5, 33, 64, 127, 300, 2000, 4983, 5000, 9000, 20000)
STREAM_G = (29, 30, 32, 33, 45, 50, 58, 59)
STREAM_ANCHORS = (1, 2, 3, 4, 16, 64, 256)              # local_anchors, capped at n (above 256: clamped to it)
STREAM_M = (1, 33, 96, 97, 384, 385, 700, 1500)         # a wave's 96 rows, a workgroup's 384, one either side
STREAM_MAX_KK = 15                                      # k + drop of the stream's geometry (lkeep <= 23)

# The values drawn for the options of LOCAL_SEED_OPTION_NAMES and TWO_LEVEL_OPTION_NAMES (plan.hip), the clamps included.
STREAM_OPTION_VALUES = {
    "local_seeds": (0, 1, 2),
    "local_anchors": STREAM_ANCHORS,
    "local_cap": (0, 2048, 32768),
    "two_level": (0, 1, 2),
    "two_level_share": (0, 1, 25, 100),
    "two_level_stretch": (0, 16),
    "two_level_burst": (0, 1, 3, 64),
    "two_level_window": (-1, 0, 1, 8, 4096),
    "two_level_check": (0, 2, 16, 64),
}
STREAM_OPTION_DEFAULTS = {"local_seeds": 1, "local_anchors": 0, "local_cap": 0, "two_level": 1, "two_level_share": 0,
                          "two_level_stretch": 0, "two_level_burst": 0, "two_level_window": 0, "two_level_check": 0}
# values that appear as set_option steps only: a case's first options keep two_level = 2 and the local seeds on
STREAM_STEP_ONLY = {"two_level": (0, 1, 2), "local_seeds": (0,)}
# companion options (OPTION_VALUES) whose values leave the stream: kept out of a case's FIRST options, allowed in later steps
STREAM_LEAVES = {
    "splits": lambda v: v != 1,
    "prepass": lambda v: v == 0,
    "l2c_geo": lambda v: v in (0, 2),
    "coarse_kernel_q": lambda v: v == 1,
    "coarse_slack": lambda v: v >= 6,
    "split_refs_max": lambda v: v != 0,
}


def _stream_query(rng, n, g):
    """("query", m, k, drop): k + drop within 1..15 in about four of five, else k in 16..56 (which leaves the stream)."""
    drop = bool(rng.random() < 0.3)
    d = 1 if drop else 0
    top = min(n, STREAM_MAX_KK)
    if rng.random() < 0.2 and n >= 16 + d:
        k = int(rng.integers(16, min(n, NABO_MAX_K) - d + 1))
    elif rng.random() < 0.4:
        k = int(min(top, _pick(rng, (1 + d, 2 + d, 14, 15)))) - d      # the ends: k = 1, k + drop = 15
    else:
        k = int(rng.integers(1 + d, top + 1)) - d
    m = int(_pick(rng, STREAM_M))
    m = max(1, min(m, STREAM_CAP // (n * g)))
    if drop:
        m = min(m, n)
    return ("query", m, k, drop)


def _stream_step_option(rng, n):
    """One set_option step from any of the three tables; every value is allowed here, those that leave the stream too."""
    if rng.random() < 0.5:
        name = _pick(rng, list(STREAM_OPTION_VALUES))
        value = int(_pick(rng, STREAM_OPTION_VALUES[name]))
        if name == "local_anchors":
            value = min(value, n)
        return ("set_option", name, value)
    name = _pick(rng, [o for o in OPTION_VALUES if o not in REFUSED_OPTIONS])
    return ("set_option", name, resolve(name, _pick(rng, OPTION_VALUES[name]), n, STREAM_MAX_KK))


def stream_cases(metric, seed, n_cases=None):
    """The deterministic case list of the stream sweep for one metric (0 Euclidean, 2 cosine) and seed: cases() in form, but
    every index starts with two_level = 2 on one reference split, and the shapes, k and options are drawn around that path."""
    if metric not in (0, 2):
        raise ValueError("the two-level stream serves the Euclidean and the cosine metric")
    rng = np.random.default_rng([metric, seed, STREAM_TAG])
    if n_cases is None:
        n_cases = STREAM_CASES
    out = []
    for i in range(n_cases):
        n = int(_pick(rng, STREAM_N))
        g = int(rng.integers(29, 60)) if rng.random() < 0.5 else int(_pick(rng, STREAM_G))
        case = {
            "sweep": "stream", "metric": metric, "seed": seed, "case": i, "n": n, "g": g, "flavour": _pick(rng, FLAVOURS),
            "data_seed": int(rng.integers(1, 1 << 30)),
            "offset": float(_pick(rng, (10.0, 40.0, 400.0))),
            "scale": float(10.0 ** int(rng.integers(-15, 16))),
            "quantum": float(_pick(rng, (0.25, 1.0))),
            "mask": _pick(rng, MASKS), "mask_seed": int(rng.integers(1, 1 << 30)),
            "mode": None, "dist_factor": 0.25,
        }
        first = _stream_query(rng, n, g)
        opts = {"two_level": 2, "splits": 1, "local_anchors": min(int(_pick(rng, STREAM_ANCHORS)), n)}
        for name, vals in STREAM_OPTION_VALUES.items():
            if name in ("two_level", "local_anchors") or rng.random() >= 0.5:
                continue
            opts[name] = int(_pick(rng, [v for v in vals if v not in STREAM_STEP_ONLY.get(name, ())]))
        for name, value in _draw_options(rng, metric, n, first[2] + first[3], 0.3).items():
            if name == "splits" or (name in STREAM_LEAVES and STREAM_LEAVES[name](value)):
                continue
            opts[name] = value
        case["options"] = opts
        steps = [first]
        for _ in range(int(rng.integers(1, 4))):
            what = rng.random()
            if what < 0.3:
                steps.append(_stream_step_option(rng, n))
            elif what < 0.5:
                steps.append(("set_mask", _pick(rng, MASKS), int(rng.integers(1, 1 << 30))))
            elif what < 0.75:
                steps.append(("set_ref", {"scale": float(_pick(rng, (1e-3, 0.5, 1.0, 7.0, 1e6))),
                                          "offset": float(_pick(rng, (0.0, 3.0, -50.0, 1e3))),
                                          "quantum": _pick(rng, (None, None, 0.5))}))
            if metric == 2 and rng.random() < 0.25:
                steps.append(("set_option", "cosine_centre", int(rng.integers(0, 2))))
                steps.append(("set_ref", {"scale": 1.0, "offset": 0.0, "quantum": None}))
            steps.append(_stream_query(rng, n, g))
        case["steps"] = steps
        out.append(case)
    return out


# ---- the fixed large cases (sampled rows against the oracle) -------------------------------------------------------

def large_cases():
    """Shapes the random draws cannot afford on full rows: a long reference stream (>= 8192 tiles: the one-round plan
    with its tail launch), the cost model's tail launch (more column-workgroups than slots), and a query whose seeded
    pass has to take four reference splits (k' = 50 on 64-entry lists: cosine, d = 100; a first pass kept without slack fails most rows)."""
    return [
        {"name": "long_stream_one_round_tail", "metric": 0, "n": 270000, "g": 50, "m": 120000, "k": 15, "drop": False,
         "flavour": "pca", "options": {}, "data_seed": 11},
        {"name": "long_stream_cosine_masked", "metric": 2, "n": 262144, "g": 30, "m": 90000, "k": 20, "drop": False,
         "flavour": "pca", "options": {"prepass": 400}, "mask": 0.05, "data_seed": 12},
        {"name": "cost_model_tail_f32", "metric": 0, "n": 9000, "g": 100, "m": 70000, "k": 11, "drop": False,
         "flavour": "pca", "options": {"refine_overlap": 0}, "mode": "f32", "data_seed": 13},
        {"name": "seeded_pass_four_splits", "metric": 2, "n": 30000, "g": 100, "m": 3000, "k": 50, "drop": False,
         "flavour": "pca", "options": {"lkeep": 50}, "data_seed": 14},
    ]


# ---- arrays -----------------------------------------------------------------------------------------------------------

def _base(n, g, case, seed):
    fl = case["flavour"]
    if fl == "clusters":
        crng = np.random.default_rng(case["data_seed"])
        centres = crng.standard_normal((6, g)) * case.get("offset", 40.0)
        rng = np.random.default_rng(seed)
        return centres[rng.integers(0, 6, size=n)] + rng.standard_normal((n, g)) * 0.2
    Y = pca_like(n, g, seed=seed)
    if fl == "scaled":
        Y = Y * case["scale"]
    elif fl == "lattice":
        Y = np.round(Y / case["quantum"]) * case["quantum"]
    return Y


def _transform(case, Y, variant):
    if case["flavour"] == "dups" and len(Y) > 8:
        rng = np.random.default_rng(case["data_seed"] + len(Y))
        Y[rng.integers(0, len(Y), len(Y) // 3)] = Y[rng.integers(0, len(Y))]
    if variant is not None:
        Y = Y * variant["scale"] + variant["offset"]
        if variant.get("quantum"):
            Y = np.round(Y / variant["quantum"]) * variant["quantum"]
    return np.ascontiguousarray(Y)


def make_ref(case, variant=None):
    """The references of `case` (variant: a set_ref step's new scale / offset / quantisation of them)."""
    return _transform(case, _base(case["n"], case["g"], case, case["data_seed"]), variant)


def make_targets(case, variant, Y, m, drop, tag):
    """Targets of one query: the first m references for the positional self-drop, else fresh rows of the same flavour
    and transform, a quarter of them copies of references (zero distances, exact ties)."""
    if drop:
        return np.ascontiguousarray(Y[:m])
    X = _transform(case, _base(m, case["g"], case, case["data_seed"] * 7 + 1000 + tag), variant)
    if m > 3:
        X[: m // 4] = Y[np.random.default_rng(tag).integers(0, len(Y), m // 4)]
    return X


def make_mask(kind, n, seed):
    """None, a random share of masked references, or "few": all but a handful masked (the masked tail)."""
    if kind is None:
        return None
    rng = np.random.default_rng(seed)
    if kind == "few":
        mask = np.ones(n, dtype=np.uint8)
        mask[rng.choice(n, min(n, int(rng.integers(1, 6))), replace=False)] = 0
        return mask
    mask = (rng.random(n) < kind).astype(np.uint8)
    if mask.all():
        mask[int(rng.integers(0, n))] = 0
    return mask


def mode_env(case):
    """(variable, value) of the mode the case pins at index creation, or None."""
    if case.get("mode") is None:
        return None
    return ("NABO_CANBERRA_MODE" if case["metric"] == 1 else "NABO_L2_MODE", case["mode"])


def planned_queries(metric, seed):
    """Every query of the cases of (metric, seed) as query_plan arguments: (case, n, g, m, k, drop, mode, options) -- the
    options in force at that step (set_option steps included)."""
    return _planned(cases(metric, seed))


def stream_planned_queries(metric, seed):
    """planned_queries for stream_cases(metric, seed); the tuple carries the step's number and the mask in force as well:
    (case, n, g, m, k, drop, mode, options, step, mask)."""
    return _planned(stream_cases(metric, seed), more=True)


def _planned(case_list, more=False):
    out = []
    for case in case_list:
        opts, mask = dict(case["options"]), case["mask"]
        for i, st in enumerate(case["steps"]):
            if st[0] == "set_option":
                opts[st[1]] = st[2]
            elif st[0] == "set_mask":
                mask = st[1]
            elif st[0] == "query":
                q = (case, case["n"], case["g"], st[1], st[2], st[3], case["mode"], dict(opts))
                out.append(q + (i, mask) if more else q)
    return out


def describe(case, step=None):
    """One line that names a case: how to replay it and what it set."""
    script = "tests/test_stream_sweep_gpu.py" if case.get("sweep") == "stream" else "tests/test_option_sweep_gpu.py"
    s = "metric=%d seed=%d case=%d (replay: python %s %d %d %d) n=%d g=%d flavour=%s mask=%s mode=%s f=%g options=%s" % (
        case["metric"], case["seed"], case["case"], script, case["metric"], case["seed"], case["case"], case["n"], case["g"],
        case["flavour"], case["mask"], case["mode"], case["dist_factor"], case["options"])
    if step is not None:
        s += " step=%d %s" % (step, case["steps"][step])
    return s
