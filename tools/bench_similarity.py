#!/usr/bin/env python3
"""Cost of the set-similarity analysis (`set_similarity.jensen_shannon_divergences` -> `uda_nn_dist2_np`; reference
active_learning_eval.py:458-583, 946-1029): the JSDs of one table, --classes x --methods, of seeded D = 3 log-normal crop metrics
with a few hundred to a few thousand boxes per class and --samples resampled points per set.

    end_to_end  jensen_shannon_divergences: resampling of every pair on the host, then ONE device call with four problems per pair
    device      that call alone on prepared arrays: upload of the points, fill + one launch, download of the squared distances; the
                host clock around the C entry point, which ends in a device-to-host copy (a synchronise)
    resample    the host half alone: log, filter, three gaussian_kde fits and draws per pair (scipy)
    kdtree      the reference's route on this machine's CPU: per pair and per KL two cKDTree builds and two queries with eps=0.01,
                one pair after the other, on the same resampled sets

The device's KLs are exact, the reference's are within D * ln 1.01 of them (each distance within a factor 1.01 of the nearest);
the script asserts that on every KL of the table before it prints a time.  `kernel_pairs` counts the squared distances the launch
evaluates, `bytes_up` / `bytes_down` what the call copies each way (points, tables and work items up; distances down).

Wall-clock p50 / mean over --steps runs after --warmup, each part in its own loop.  Prints ONE JSON line.

    python tools/bench_similarity.py [--classes 10] [--methods 9] [--samples 10000] [--steps 5] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D = 3
KNN_BLOCKS = 1024          # uda_services.hip: the number of blocks a call fills before it stops cutting references into spans


def synthetic(classes, methods, seed=7):
    """(P, Q) per (class, method): Q is the class's validation set, P what a method selected, a shifted and rescaled log-normal."""
    rng = np.random.default_rng([seed, classes, methods])
    pairs = []
    for c in range(classes):
        mu, sigma = rng.normal(0.0, 0.5, D), rng.uniform(0.3, 0.8, D)
        val = np.exp(rng.normal(mu, sigma, (int(rng.integers(300, 4000)), D)))
        for _ in range(methods):
            n = int(rng.integers(200, 3000))
            pairs.append((np.exp(rng.normal(mu + rng.normal(0, 0.15, D), sigma * rng.uniform(0.8, 1.25, D), (n, D))), val))
    return pairs


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(p50_ms=round(float(np.median(t)), 3), mean_ms=round(float(np.mean(t)), 3))


def kdtree_kl(sample_p, sample_q, tree):
    """The reference's estimator with its own neighbour search (eps=0.01)."""
    n, d = sample_p.shape
    dp = tree(sample_p).query(sample_p, k=2, eps=0.01, p=2)[0][:, 1]
    dq = tree(sample_q).query(sample_p, k=1, eps=0.01, p=2)[0]
    return -np.log(dp / dq).sum() * d / n + np.log(sample_q.shape[0] / (n - 1))


def work_items(q_off, r_off, rows, cols):
    """The size of the call's work table, by the rule of the entry point."""
    n, m = np.diff(q_off), np.diff(r_off)
    row_blocks, chunks = -(-n // rows), -(-m // cols)
    want = max(1, -(-KNN_BLOCKS // int(row_blocks.sum())))
    spans = np.minimum(chunks, want)
    per = -(-chunks // spans)
    return int((row_blocks * -(-chunks // per)).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--methods", type=int, default=9)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    from scipy.spatial import cKDTree
    from uda_amd import capi
    from uda_amd import set_similarity as S
    pairs = synthetic(a.classes, a.methods)
    triples = [S.resample_sets(p, q, a.samples) for p, q in pairs]

    # the one call, on prepared arrays: per triple P against itself, P against M, Q against itself, Q against M
    probs = [pr for p, q, m in triples for pr in ((p, p, 1), (p, m, 0), (q, q, 1), (q, m, 0))]
    q_off = np.concatenate([[0], np.cumsum([x.shape[0] for x, _, _ in probs])]).astype(np.int64)
    r_off = np.concatenate([[0], np.cumsum([y.shape[0] for _, y, _ in probs])]).astype(np.int64)
    queries, refs = np.concatenate([x for x, _, _ in probs]), np.concatenate([y for _, y, _ in probs])
    self = np.array([s for _, _, s in probs], np.uint8)
    d2 = np.empty(int(q_off[-1]))
    lib = capi.load()

    def device_call():
        rc = lib.uda_nn_dist2_np(0, D, len(probs), queries.ctypes.data, q_off.ctypes.data, refs.ctypes.data, r_off.ctypes.data,
                                 self.ctypes.data, d2.ctypes.data)
        capi.check(lib, None, rc, "uda_nn_dist2_np")

    got = S.jensen_shannon_from_samples(triples)               # the device's KLs ...
    want = [(kdtree_kl(p, m, cKDTree), kdtree_kl(q, m, cKDTree)) for p, q, m in triples]     # ... and the reference's
    diff = max(abs(g - w) for (_, g_pm, g_qm), w_pair in zip(got, want) for g, w in zip((g_pm, g_qm), w_pair))
    bound = D * float(np.log(1.01))
    assert diff <= bound, "a KL of the device differs from the KD-tree's by %g, more than D ln 1.01 = %g" % (diff, bound)
    e2e = S.jensen_shannon_divergences(pairs, a.samples)
    assert np.array_equal(e2e, [j for j, _, _ in got]), "end to end and from the resampled sets disagree"

    items = work_items(q_off, r_off, capi.KNN_ROWS, capi.KNN_COLS)
    res = dict(classes=a.classes, methods=a.methods, pairs=len(pairs), samples=a.samples, dims=D, problems=len(probs),
               kernel_pairs=int((np.diff(q_off) * np.diff(r_off)).sum()), work_items=items,
               bytes_up=int(queries.nbytes + refs.nbytes + q_off.nbytes + r_off.nbytes + self.nbytes + 16 * items), bytes_down=int(d2.nbytes),
               max_abs_kl_diff_vs_kdtree=float(diff), kl_diff_bound=round(bound, 6),
               end_to_end=timed(lambda: S.jensen_shannon_divergences(pairs, a.samples), a.steps, a.warmup),
               device=timed(device_call, a.steps, a.warmup),
               resample=timed(lambda: [S.resample_sets(p, q, a.samples) for p, q in pairs], a.steps, a.warmup),
               kdtree=timed(lambda: [(kdtree_kl(p, m, cKDTree), kdtree_kl(q, m, cKDTree)) for p, q, m in triples], a.steps, a.warmup))
    res["kdtree_over_device"] = round(res["kdtree"]["p50_ms"] / res["device"]["p50_ms"], 1)
    res["kdtree_plus_resample_over_end_to_end"] = round((res["kdtree"]["p50_ms"] + res["resample"]["p50_ms"]) / res["end_to_end"]["p50_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
