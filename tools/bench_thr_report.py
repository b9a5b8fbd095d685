#!/usr/bin/env python3
"""Cost of the thresholding report (`thresholding.report_np` -> `uda_thr_report_np`; reference uncertainty_analysis.py:517-749,
utils_extra.py:25-36) on a seeded synthetic validation set: --rows matched rows (default 70 000, a BDD-sized set), --classes
ground-truth classes (default 10), two uncertainties, so S = 4 score columns (the two, their global combination, the per-class
combination), the default six IoU thresholds - once over all rows alone (B = 1) and once with the class segments (B = 1 + classes).

    device      the C entry point alone on prepared arrays: one packed upload, the mask, per segment the sort and curve launches,
                one launch for counts and moments, one packed download; the host clock around the call, which ends in a
                device-to-host copy (a synchronise)
    upload /    copies of the same byte counts between pageable host memory and the device, timed apart with torch; `rest` =
    download    device - upload - download is the packing, the allocations, the launches and the kernels together (a difference
                of medians, not a measurement of its own)
    thr_report  the Python call around it (class order, checks) and the 1000-point JSD of every (segment, column, threshold)
    save        save_thr_performance end to end: the combinations, the call, the JSDs, the table and the text file
    host        the reference-shaped evaluation on this machine's CPU, once: per (segment, column, threshold)
                sklearn.metrics.roc_curve + auc + numpy.interp as `roc_metrics` writes them, `calc_jsd`, and the three removal
                compares (needs sklearn and scipy; left out with a note when either is missing)

The script asserts that every label count, every removal count and every threshold of the device EQUALS the host's before it
prints a time.  Wall-clock p50 / mean over --steps runs after --warmup.  Prints ONE JSON line.  For the kernels alone run it with
--device-only under a kernel trace.

    python tools/bench_thr_report.py [--rows 70000] [--classes 10] [--steps 5] [--warmup 1] [--device-only]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT6 = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75]


def synthetic(rows, classes, seed=23):
    rng = np.random.default_rng([seed, rows, classes])
    tp = rng.random(rows) < 0.85
    ious = np.round(rng.uniform(0.05, 0.999, rows), 3)
    wrong = ~(tp & (ious >= 0.5))
    ent = rng.uniform(0, 1.2, rows) * np.where(wrong, 1.0, 0.6)
    albox = rng.gamma(2.0, 0.05, rows) * np.where(wrong, 1.5, 1.0)
    gt = rng.integers(1, classes + 1, rows).astype(np.float64)
    return [ent, albox], ious, tp, gt, [0.7, 0.4], [float(v) for v in np.round(rng.uniform(0.1, 1.0, 2 * classes), 2)]


def host_roc_metrics(uncert, y_true, fix_cd, budget):
    """`roc_metrics` (uncertainty_analysis.py:44-83), its interpolation branches."""
    from sklearn.metrics import auc, roc_curve
    fpr, tpr, thresholds = roc_curve(y_true, uncert, pos_label=0)
    roc_auc = auc(fpr, tpr)
    if fix_cd:
        rate = 1 - np.interp(1 - budget, fpr, tpr)
        return thresholds[np.argmin(np.abs(1 - tpr - rate))], rate, roc_auc
    rate = np.interp(budget, tpr, fpr)
    return thresholds[np.argmin(np.abs(fpr - rate))], rate, roc_auc


def host_report(scores, ious, tp, thrs, fix_cd, budget, lo, hi, calc_jsd):
    B, S, K = len(lo), len(scores), len(thrs)
    thr, jsd = np.zeros((B, S, K)), np.zeros((B, S, K))
    n_label, removed = np.zeros((B, K, 2), np.int64), np.zeros((B, S, K, 3), np.int64)
    for b in range(B):
        sl = slice(lo[b], hi[b])
        for k, t in enumerate(thrs):
            correct = np.asarray((ious[sl] >= t) * tp[sl])
            n_label[b, k] = correct.sum(), (~correct).sum()
            for s in range(S):
                u = scores[s, sl]
                jsd[b, s, k] = np.nan_to_num(calc_jsd(u[correct], u[~correct]))
                thr[b, s, k] = host_roc_metrics(u, correct, fix_cd, budget)[0]
                rem = u >= thr[b, s, k]
                removed[b, s, k] = (rem & ~correct).sum(), (rem & correct).sum(), (~rem & ~correct).sum()
    return thr, jsd, n_label, removed


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(p50_ms=round(float(np.median(t)), 3), mean_ms=round(float(np.mean(t)), 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=70000)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device-only", action="store_true", help="time the device call and the copies only (for a kernel trace)")
    a = ap.parse_args()
    import torch
    from uda_amd import capi
    from uda_amd import thresholding as th
    lib = capi.load()
    uncerts, ious, tp, gt, w_all, w_cls = synthetic(a.rows, a.classes)
    fix_cd, budget, N, K = True, 0.95, a.rows, len(DEFAULT6)
    params = {"thr_cd": fix_cd, "thr_fpr_tpr": budget, "thr_iou_thrs": DEFAULT6}
    opt_all = sum(p * u for p, u in zip(w_all, uncerts))
    opt_cls = th.combine_per_class(uncerts, gt, w_cls, a.classes)
    order, lo, hi = th.segments_by_class(gt, a.classes)
    scores = np.ascontiguousarray(np.stack(uncerts + [opt_all, opt_cls])[:, order])
    ious_o, tp_o = np.ascontiguousarray(ious[order]), np.ascontiguousarray(tp[order].astype(np.uint8))
    thrs = np.asarray(DEFAULT6)
    S = len(scores)
    res = dict(rows=N, classes=a.classes, columns=S, thresholds=K)
    try:
        import scipy.stats      # noqa: F401
        import sklearn.metrics  # noqa: F401
        have_host = True
    except ImportError:
        have_host = False
        res["host"] = "left out: sklearn or scipy is not installed"

    for tag, B in (("all_rows", 1), ("with_classes", 1 + a.classes)):
        seg_lo, seg_hi = np.ascontiguousarray(lo[:B]), np.ascontiguousarray(hi[:B])
        outs = [np.zeros((B, S, K, 3)), np.zeros((B, K, 2), np.int64), np.zeros((B, S, K, 2, 2)), np.zeros((B, S, K, 3), np.int64)]

        def device_call():
            rc = lib.uda_thr_report_np(0, scores.ctypes.data, ious_o.ctypes.data, tp_o.ctypes.data, N, S, thrs.ctypes.data, K,
                                       seg_lo.ctypes.data, seg_hi.ctypes.data, B, int(fix_cd), budget, *[o.ctypes.data for o in outs])
            capi.check(lib, None, rc, "uda_thr_report_np")

        r = dict(segments=B)
        device_call()
        if have_host and not a.device_only:
            t0 = time.perf_counter()
            h_thr, h_jsd, h_label, h_removed = host_report(scores, ious_o, tp_o.astype(bool), DEFAULT6, fix_cd, budget, seg_lo, seg_hi,
                                                           th.calc_jsd)
            r["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert np.array_equal(outs[0][..., 0], h_thr), "thresholds differ from the host's"
            assert np.array_equal(outs[1], h_label) and np.array_equal(outs[3], h_removed), "counts differ from the host's"
            rep = th.ThrReport(*outs, order, seg_lo, seg_hi)
            r["jsd_max_rel_diff"] = float("%.3g" % np.max(np.abs(rep.jsd - h_jsd) / np.abs(h_jsd).clip(1e-300)))
        up = int(scores.nbytes + ious_o.nbytes + tp_o.nbytes + 8 * S * S + 8 * B)
        down = int(sum(o.nbytes for o in outs))
        h_up, h_down = torch.empty(up, dtype=torch.uint8), torch.empty(down, dtype=torch.uint8)
        d_up, d_down = torch.empty(up, dtype=torch.uint8, device="cuda"), torch.empty(down, dtype=torch.uint8, device="cuda")

        def copy_up():
            d_up.copy_(h_up)
            torch.cuda.synchronize()

        def copy_down():
            h_down.copy_(d_down)
            torch.cuda.synchronize()

        r.update(bytes_up=up, bytes_down=down, device=timed(device_call, a.steps, a.warmup), upload=timed(copy_up, a.steps, a.warmup),
                 download=timed(copy_down, a.steps, a.warmup))
        r["rest_ms"] = round(r["device"]["p50_ms"] - r["upload"]["p50_ms"] - r["download"]["p50_ms"], 3)
        if not a.device_only:
            cls = gt if B > 1 else None
            r["thr_report"] = timed(lambda: th.thr_report(np.stack(uncerts + [opt_all, opt_cls]), ious, tp, DEFAULT6, fix_cd, budget,
                                                          gt_classes=cls, num_classes=a.classes if B > 1 else None).jsd,
                                    a.steps, a.warmup)
            with tempfile.TemporaryDirectory() as tmp:
                r["save"] = timed(lambda: th.save_thr_performance(tmp, params, uncerts, opt_all, tp, ious, gt_classes=cls,
                                                                  opt_params=w_cls if B > 1 else None), a.steps, a.warmup)
            if "host_ms" in r:
                r["host_over_device"] = round(r["host_ms"] / r["device"]["p50_ms"], 2)
                r["host_over_thr_report"] = round(r["host_ms"] / r["thr_report"]["p50_ms"], 2)
        res[tag] = r
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
