"""CPU model of the two-level stream's MODE CONTROL (nabo_amd/csrc/l2c_topk.hip): given which tiles of a wave's
stream pass the first step's bound, how many tiles each rule runs one-step, refetches inside the one-step loop, and runs
two-step -- and what that costs for an assumed refetch cost R.  numpy only, float64, no GPU.  Extends tools/two_level_model.py.
    python tools/two_level_mode_model.py [n] [waves]           (default 1000000 x 1000000, d = 50, 12 sampled waves)
Setup: bench.py's data; 64 anchors at stride n / 64, both sides sorted by nearest anchor, every bucket of the references padded
to whole tiles of 32 (the ordered copy's layout); waves of 96 consecutive sorted rows; LB1 = d^2 over the 28 leading components
+ (||x_tail|| - ||y_tail||)^2.  Verdicts: per ROW (a tile passes when LB1 < the row's threshold for any pair: what the kernel's
per-pair filter computes up to its lane grouping) and per LANE (the lane's six rows, r, r + 16, ... of the wave, share the
largest of their six thresholds: one minimum and one compare per lane).  Thresholds: each row's final 23rd-smallest score, and
the local seeds (23rd smallest over the first 16384 cells of the wave's own bucket).
Rules, walking a wave's stream in pairs of tiles like the kernel's loops:
  * leaky bucket (the control before): one account per one-step segment, credit `burst`, `share` percent of the segment's tiles;
    overdrawn -> finish the pair, two-step for a stretch (64, doubling while the probe behind it lasts < 64 tiles), probe again;
  * per bucket: one account per reference bucket, burst + share x (tiles since the bucket's start) / 100 refetches; the refetch
    that takes the last of it -> finish the pair, two-step to that bucket's end (in twos), back to one-step;
  * oracle: every passing tile two-step, none refetched.
Costs are in one-step tiles: a two-step tile 168 / 104, a refetch R; with the per-lane verdict a one-step tile 292 / 312.
Left out: the kernel's thresholds EVOLVE from the seeds to the final ones along the stream (the model uses one or the other for
the whole stream); a segment's last tile is completed whatever its bounds say; f16 rounding of the bound; the tail bound's
rounding factors; lists, drains and everything the refetch does to the SIMD's other wave; memory.  R is an input, not a result."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nabo_amd._synth import pca_like  # noqa: E402

TWO = 168.0 / 104.0


def d2(P, Q):
    return np.maximum((P * P).sum(1)[:, None] + (Q * Q).sum(1)[None] - 2 * P @ Q.T, 0)


def leaky(hit, ends, burst=8, share=25, stretch0=64, probe=64):
    """tiles (one-step, refetched, two-step) of one wave under the control before"""
    T, t, one, ref, two, stretch = len(hit), 0, 0, 0, 0, stretch0
    while t < T:
        t0, r, leave = t, 0, False
        while t < T and not leave:                        # one-step, in twos; tile t - 1 is judged at step t
            for s in (t, t + 1):
                if s > t0 and s - 1 < T and hit[s - 1]:
                    r += 1
                    if r * 100 > burst * 100 + share * (s - t0):
                        leave = True
            t += 2
        one += min(t, T) - t0
        ref += r
        if t - t0 >= probe:
            stretch = stretch0
        e = min(t + stretch, T)
        two += max(e - t, 0)
        t = max(e, t)
        stretch *= 2
    return one, ref, two


def by_bucket(hit, ends, burst=3, share=25):
    """the same under the per-bucket rule; ends: the buckets' ends in tiles, non-decreasing"""
    T, t, one, ref, two = len(hit), 0, 0, 0, 0
    cur, b0, acct = 0, 0, 0
    while t < T:
        t0, t2, leave = t, 0, False
        while t < T and not leave:
            for s in (t, t + 1):
                if s > t0 and s - 1 < T and hit[s - 1]:
                    ref += 1
                    moved = False
                    while cur < len(ends) and ends[cur] <= s - 1:
                        b0, cur, moved = ends[cur], cur + 1, True
                    acct = 1 if moved else acct + 1
                    if not leave and (acct + 1) * 100 > burst * 100 + share * (s - 1 - b0):
                        leave = True
                        t2 = min((ends[cur] + 1) // 2 * 2 if cur < len(ends) else T, T)
            t += 2
        one += min(t, T) - t0
        if leave and t2 > t:
            two += t2 - t
            t = t2
    return one, ref, two


def oracle(hit, ends):
    return int((~hit).sum()), 0, int(hit.sum())


def run(n, m, nw, d=50, head=28, C=64, L=23, gen=pca_like):
    Y, X = gen(n, d, 1003), gen(m, d, 2003)
    A = Y[:: n // C][:C]
    bY, bX = d2(Y, A).argmin(1), d2(X, A).argmin(1)
    cnt = np.bincount(bY, minlength=C)
    ends = np.cumsum(-(-cnt // 32))                       # lseed_bucket_ends
    pos = np.concatenate([(ends[b] - -(-cnt[b] // 32)) * 32 + np.arange(cnt[b]) for b in range(C)])
    oy = np.argsort(bY, kind="stable")
    T = int(ends[-1])
    Yo = np.full((T * 32, d), np.nan)
    Yo[pos] = Y[oy]                                       # padding cells: NaN, never below a threshold
    tile_bucket = np.searchsorted(ends, np.arange(T), side="right")
    ox = np.argsort(bX, kind="stable")
    Yh, Yt = Yo[:, :head], np.linalg.norm(Yo[:, head:], axis=1)
    rng = np.random.default_rng(1)
    rules = (("leaky bucket per segment (share 25, burst 8, stretch 64 doubling)", leaky, {}),
             ("per bucket, burst 3, share 10", by_bucket, {"share": 10}),
             ("per bucket, burst 3, share 25", by_bucket, {}),
             ("per bucket, burst 7, share 25", by_bucket, {"burst": 7}),
             ("oracle", oracle, {}))
    kinds = [(thr, verdict) for thr in ("final", "seed") for verdict in ("row", "lane")]
    tot = {(k, r[0]): np.zeros(3) for k in kinds for r in rules}
    dens = {k: [] for k in kinds}
    for w in rng.choice(m // 96, nw, replace=False):
        rows = ox[w * 96:(w + 1) * 96]
        Xw = X[rows]
        with np.errstate(invalid="ignore"):
            full = np.where(np.isnan(Yo[:, 0])[None], np.inf, d2(Xw, np.nan_to_num(Yo)))
            lb1 = d2(Xw[:, :head], np.nan_to_num(Yh)) + (np.linalg.norm(Xw[:, head:], axis=1)[:, None] - np.nan_to_num(Yt)[None]) ** 2
        lb1[:, np.isnan(Yo[:, 0])] = np.inf
        tau = {"final": np.partition(full, L - 1, axis=1)[:, L - 1]}
        own = full[:, np.repeat(tile_bucket, 32) == np.bincount(bX[rows]).argmax()][:, :16384]
        tau["seed"] = np.partition(own, L - 1, axis=1)[:, L - 1] if own.shape[1] >= L else np.full(96, np.inf)
        for thr, verdict in kinds:
            t = tau[thr]
            if verdict == "lane":                         # the lane's six rows share the largest of their thresholds
                t = np.tile(t.reshape(6, 16).max(axis=0), 6)
            hit = (lb1 < t[:, None]).reshape(96, T, 32).any(axis=(0, 2))
            for name, fn, kw in rules:
                tot[((thr, verdict), name)] += fn(hit, ends, **kw)
            dens[(thr, verdict)].append(np.array([[hit[tile_bucket == b].mean() if (tile_bucket == b).any() else 0.0,
                                                   hit[tile_bucket == b].sum()] for b in range(C)]))
    for k in kinds:
        print("\n## thresholds: %s, verdict per %s (%d x %d, %d waves)" % (k[0], k[1], n, m, nw))
        dd = np.concatenate(dens[k])
        print("| hit density of the (wave, reference bucket) pair | share of pairs | share of all hits |\n|---|---|---|")
        for lo, hi, name in ((-1, 0.001, "< 0.1 %"), (0.001, 0.1, "0.1 - 10 %"), (0.1, 0.5, "10 - 50 %"), (0.5, 0.9, "50 - 90 %"), (0.9, 2, ">= 90 %")):
            sel = (dd[:, 0] >= lo) & (dd[:, 0] < hi) if lo >= 0 else dd[:, 0] < hi
            print("| %s | %.1f %% | %.1f %% |" % (name, 100 * sel.mean(), 100 * dd[sel, 1].sum() / max(dd[:, 1].sum(), 1)))
        one_cost = 292.0 / 312.0 if k[1] == "lane" else 1.0
        print("| rule | one-step | refetched | two-step | cost R = 1.5 | R = 2 | R = 4 |\n|---|---|---|---|---|---|---|")
        for name, _, _ in rules:
            one, ref, two = tot[(k, name)] / (nw * T)
            print("| %s | %.1f %% | %.2f %% | %.1f %% | %s |" % (name, 100 * one, 100 * ref, 100 * two,
                                                            " | ".join("%.3f" % (one * one_cost + two * TWO + ref * R) for R in (1.5, 2.0, 4.0))))


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    run(n, n, int(sys.argv[2]) if len(sys.argv) > 2 else 12)
