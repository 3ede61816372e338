"""Seeded cases for the option sweep (tests/test_option_sweep_gpu.py, tests/test_option_table.py, tools/stress_sweep3.py).

include/nabo_knn.h promises that every index option returns the SAME BITS: an option chooses how a launch is cut or which
filter pass answers a row, never what the answer is.  The only guard against a subtly wrong pass is oracle parity on inputs
that actually route rows through that pass, so this module draws index options, L2 / Canberra modes, shapes, data flavours
and short scripts of calls on one resident index that reach every pass.  Pure Python + numpy: no GPU, no oracle.

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


def option_names(path=API_SOURCE):
    """The names of OPTION_NAMES[] in plan.hip, in table order."""
    src = open(path).read()
    body = re.search(r"OPTION_NAMES\[\]\s*=\s*\{(.*?)\n\};", src, re.S).group(1)
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
    out = []
    for case in cases(metric, seed):
        opts = dict(case["options"])
        for st in case["steps"]:
            if st[0] == "set_option":
                opts[st[1]] = st[2]
            elif st[0] == "query":
                out.append((case, case["n"], case["g"], st[1], st[2], st[3], case["mode"], dict(opts)))
    return out


def describe(case, step=None):
    """One line that names a case: how to replay it and what it set."""
    s = "metric=%d seed=%d case=%d (replay: python tests/test_option_sweep_gpu.py %d %d %d) n=%d g=%d flavour=%s mask=%s mode=%s f=%g options=%s" % (
        case["metric"], case["seed"], case["case"], case["metric"], case["seed"], case["case"], case["n"], case["g"],
        case["flavour"], case["mask"], case["mode"], case["dist_factor"], case["options"])
    if step is not None:
        s += " step=%d %s" % (step, case["steps"][step])
    return s
