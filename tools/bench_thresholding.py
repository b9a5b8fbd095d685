#!/usr/bin/env python3
"""Cost of one objective batch of the thresholding search (`thresholding.roc_objective` -> `uda_thr_objective_np`; reference
uncertainty_analysis.py:44-152).

  For two validation-set sizes - --n-kitti (a KITTI-sized set of matched rows) and --n-bdd (a BDD-sized one) - with U = 2
  uncertainties and the 6 default IoU thresholds:
    device      one call with --candidates weight vectors: upload, mask, one sort per candidate, 6 curves on it, download; the host
                clock around the call, which ends in a device-to-host copy (a synchronise)
    cpu         the same --cpu-candidates problems as the reference runs them: a loop over sklearn.metrics.roc_curve + auc +
                numpy.interp per (candidate, threshold) where sklearn is importable, else over tests/thr_ref.py; on this
                machine's CPU, scaled to --candidates by the per-problem time
  The two must agree (thr and rate bit for bit on the candidates the CPU ran) before their times mean anything.

Wall-clock p50 / mean over --steps calls after --warmup.  Prints ONE JSON line.

    python tools/bench_thresholding.py [--candidates 256] [--n-kitti 12000] [--n-bdd 180000] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
THRS = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75]


def synthetic(N, P, seed=3):
    rng = np.random.default_rng(seed)
    tp = rng.random(N) < 0.9
    ious = np.round(rng.uniform(0.05, 0.999, N), 3)
    wrong = ~(tp & (ious >= 0.5))
    unc = np.stack([np.round(rng.uniform(0, 1.2, N) * np.where(wrong, 1.0, 0.6), 4), np.round(rng.gamma(2.0, 0.05, N), 4)])
    return unc, ious, tp, rng.uniform(0, 1, (P, 2))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(p50_ms=round(float(np.median(t)), 3), mean_ms=round(float(np.mean(t)), 3))


def cpu_loop(unc, ious, tp, params, fix_cd, budget):
    """(thr, rate) [P, K] the way the reference computes them, and which implementation did."""
    try:
        from sklearn.metrics import auc, roc_curve
    except ImportError:
        import thr_ref as R
        thr, rate, _ = R.roc_objective(unc, ious, tp, THRS, params, fix_cd, budget)
        return thr, rate, "numpy mirror"
    out = np.zeros((2, len(params), len(THRS)))
    for p, row in enumerate(params):
        u = sum(w * c for w, c in zip(row, unc))
        for k, t in enumerate(THRS):
            fpr, tpr, thresholds = roc_curve(np.asarray((ious >= t) * tp, dtype=int), u, pos_label=0)
            auc(fpr, tpr)
            if fix_cd:
                r = 1 - np.interp(1 - budget, fpr, tpr)
                out[:, p, k] = thresholds[np.argmin(np.abs(1 - tpr - r))], r
            else:
                r = np.interp(budget, tpr, fpr)
                out[:, p, k] = thresholds[np.argmin(np.abs(fpr - r))], r
    return out[0], out[1], "sklearn.metrics.roc_curve"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--cpu-candidates", type=int, default=8)
    ap.add_argument("--n-kitti", type=int, default=12000)
    ap.add_argument("--n-bdd", type=int, default=180000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from uda_amd import thresholding as TH
    res = dict(candidates=a.candidates, uncertainties=2, iou_thresholds=len(THRS))
    for name, N in (("kitti", a.n_kitti), ("bdd", a.n_bdd)):
        unc, ious, tp, params = synthetic(N, a.candidates)
        got = TH.roc_objective(unc, ious, tp, THRS, params, True, 0.95)
        q = min(a.cpu_candidates, a.candidates)
        t0 = time.perf_counter()
        thr, rate, how = cpu_loop(unc, ious, tp, params[:q], True, 0.95)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(got[0][:q], thr) and np.array_equal(got[1][:q], rate), "device and CPU disagree"
        r = dict(rows=N, device=timed(lambda: TH.roc_objective(unc, ious, tp, THRS, params, True, 0.95), a.steps, a.warmup),
                 cpu=dict(how=how, candidates_run=q, ms=round(cpu_ms, 1), ms_scaled_to_all=round(cpu_ms * a.candidates / q, 1)))
        r["speedup_vs_cpu"] = round(r["cpu"]["ms_scaled_to_all"] / r["device"]["p50_ms"], 1)
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
