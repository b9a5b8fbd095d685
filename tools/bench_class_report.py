#!/usr/bin/env python3
"""Cost of the classification calibration report (`class_report.report_np` -> `uda_class_report_np`; reference
calibrate_classification.py:97-143, 250-440) on a seeded synthetic evaluation split: --rows rows (default 70 000, a BDD-sized set),
--classes classes (default 10), --tables probability tables (default 5: uncalibrated, TS all, TS per class, isotonic all, isotonic per
class), the uniform edges of 10 bins, one segment.

    device      the C entry point alone on prepared arrays: upload of the tables, the labels, the edges and the run table, two
                launches, one copy per output array; the host clock around the call, which ends in a device-to-host copy (a
                synchronise)
    upload /    copies of the same byte counts between pageable host memory and the device, timed apart with torch (the entry
    download    point uses plain hipMemcpy on pageable memory too); `rest` = device - upload - download is the allocations, the
                memsets, the launches and the kernels together (a difference of medians, not a measurement of its own)
    report_np   the Python call around it: the float64 copy of the tables, the label check, the edges, the outputs
    titles      class_report.title_lines of every (table, target) from the tallies: bins, ECE, MCE, Brier, NLL, SCE, np.around
    host        the reference-shaped evaluation in numpy on this machine's CPU, once: per (table, target) the np.digitize and the
                three np.bincount of `_calibr_bins`, the non-empty selection, ECE and MCE, and per table the Brier expressions and
                the arg-max gather of `_calibr_plot` (vectorised numpy throughout, as the reference's is)

The script asserts that every bin count and every hit count of the device EQUALS the host's before it prints a time.  Wall-clock
p50 / mean over --steps runs after --warmup.  Prints ONE JSON line.

    python tools/bench_class_report.py [--rows 70000] [--classes 10] [--tables 5] [--steps 5] [--warmup 1] [--device-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(rows, classes, tables, seed=19):
    """Softmax of seeded logits at `tables` temperatures; labels follow the first table's arg-max seven times in ten."""
    rng = np.random.default_rng([seed, rows, classes, tables])
    logits = rng.normal(0, 2.5, (rows, classes))
    prob = []
    for m in range(tables):
        x = logits / (0.6 + 0.35 * m)
        e = np.exp(x - x.max(axis=1, keepdims=True))
        prob.append(e / e.sum(axis=1, keepdims=True))
    prob = np.ascontiguousarray(np.stack(prob))
    label = np.where(rng.random(rows) < 0.7, prob[0].argmax(axis=1), rng.integers(0, classes, rows)).astype(np.int32)
    return prob, label


def host_numbers(y_true, y_pred, bins):
    """`_calibr_bins` (:124-143) for one target -> bin_total, bin_true, ece, mce."""
    binids = np.digitize(y_pred, bins)
    bin_sums = np.bincount(binids, weights=y_pred, minlength=len(bins))
    bin_true = np.bincount(binids, weights=y_true, minlength=len(bins))
    bin_total = np.bincount(binids, minlength=len(bins))
    nonzero = bin_total != 0
    prob_true = bin_true[nonzero] / bin_total[nonzero]
    prob_pred = bin_sums[nonzero] / bin_total[nonzero]
    ece = np.sum(np.abs(prob_true - prob_pred) * (bin_total[nonzero] / len(y_true)))
    return bin_total, bin_true, ece, np.max(np.abs(prob_true - prob_pred))


def host_report(prob, label, bins):
    """The loop of `_calibr_plot` (:346-393) over the tables: every class, then the arg-max target, with the Brier expressions."""
    M, N, C = prob.shape
    y_true = np.eye(C)[label]
    out = []
    for m in range(M):
        y_pred = prob[m]
        per = []
        for t in range(C):
            per.append(host_numbers(y_true[:, t], y_pred[:, t].astype("float64"), bins) + (np.mean((y_pred[:, t] - y_true[:, t]) ** 2),))
        brier = np.mean((y_pred - y_true) ** 2)
        maxim = y_pred.argmax(axis=-1)
        idx = np.arange(N)
        per.append(host_numbers(y_true[idx, maxim].T.astype(np.float64), y_pred[idx, maxim].T.astype(np.float64), bins) + (brier,))
        out.append(per)
    return out


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
    ap.add_argument("--tables", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device-only", action="store_true", help="time the device call and the copies only (for a kernel trace)")
    a = ap.parse_args()
    import torch
    from uda_amd import capi
    from uda_amd import class_report as cr
    lib = capi.load()
    prob, label = synthetic(a.rows, a.classes, a.tables)
    M, N, C = prob.shape
    bins = cr.uniform_edges()
    off, ne = np.array([0, N], np.int64), np.array([len(bins)], np.int32)
    E = len(bins)
    outs = [np.zeros((1, M, C + 1, E + 1), np.int64), np.zeros((1, M, C + 1, E + 1), np.int64), np.zeros((1, M, C + 1, E + 1)),
            np.zeros((1, M, C)), np.zeros((1, M)), np.zeros((1, M, 2), np.int64)]

    def device_call():
        rc = lib.uda_class_report_np(0, 1, M, C, 1, E, off.ctypes.data, prob.ctypes.data, label.ctypes.data, bins.ctypes.data, ne.ctypes.data,
                                     *[o.ctypes.data for o in outs])
        capi.check(lib, None, rc, "uda_class_report_np")

    names = ["table%d" % m for m in range(M)]

    def titles(rep):
        return [cr.title_lines(rep, m, t) for m in range(M) for t in range(C + 1)]

    rep = cr.report(prob, label, names)
    res = dict(rows=N, classes=C, tables=M, edges=E, targets=M * (C + 1))
    if not a.device_only:
        t0 = time.perf_counter()
        host = host_report(prob, label, bins)
        res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        worst = 0.0
        for m in range(M):
            for t in range(C + 1):
                total, true, ece, mce, brier = host[m][t]
                assert len(total) == E, "the reference would raise: a probability at or above the last edge"
                assert np.array_equal(rep.bin_count[0, m, t, :E], total) and np.array_equal(rep.bin_hits[0, m, t, :E], true.astype(np.int64)), \
                    "bin counts of table %d target %d differ from the host's" % (m, t)
                mine = (rep.ece(m, t), rep.mce(m, t), rep.brier(m, t) if t < C else rep.brier_all(m))
                worst = max([worst] + [abs(float(x) - float(y)) / abs(float(y)) for x, y in zip(mine, (ece, mce, brier)) if y])
        res["ece_mce_brier_max_rel_diff"] = float("%.3g" % worst)

    up = int(prob.nbytes + label.nbytes + bins.nbytes + ne.nbytes + 2 * off.nbytes + 12 * (N // capi.CLASSREP_ROWS + 1))
    down = int(sum(o.nbytes for o in outs))
    h_up, h_down = torch.empty(up, dtype=torch.uint8), torch.empty(down, dtype=torch.uint8)
    d_up, d_down = torch.empty(up, dtype=torch.uint8, device="cuda"), torch.empty(down, dtype=torch.uint8, device="cuda")

    def copy_up():
        d_up.copy_(h_up)
        torch.cuda.synchronize()

    def copy_down():
        h_down.copy_(d_down)
        torch.cuda.synchronize()

    res.update(bytes_up=up, bytes_down=down, device=timed(device_call, a.steps, a.warmup), upload=timed(copy_up, a.steps, a.warmup),
               download=timed(copy_down, a.steps, a.warmup))
    res["rest_ms"] = round(res["device"]["p50_ms"] - res["upload"]["p50_ms"] - res["download"]["p50_ms"], 3)
    if not a.device_only:
        res["report_np"] = timed(lambda: cr.report_np(prob, label), a.steps, a.warmup)
        res["titles"] = timed(lambda: titles(rep), a.steps, a.warmup)
        res["report_and_titles"] = timed(lambda: titles(cr.report(prob, label, names)), a.steps, a.warmup)
        res["host_over_device"] = round(res["host_ms"] / res["device"]["p50_ms"], 2)
        res["host_over_report_and_titles"] = round(res["host_ms"] / res["report_and_titles"]["p50_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
