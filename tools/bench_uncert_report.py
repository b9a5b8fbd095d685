#!/usr/bin/env python3
"""Cost of the validation uncertainty report (`uncertainty_report.report_np` -> `uda_uncert_report_np`; reference utils_box.py:17-102,
calibrate_regression.py:231-349) on a seeded synthetic validation set: --rows matched rows (default 70 000, a BDD-sized set), --columns
sigma columns (default 14: two served, six calibrated variants of each), one segment per class (10 classes).

    device      the C entry point alone on prepared arrays: upload of the rows, the columns and the run table, two launches, one
                copy per output array; the host clock around the call, which ends in a device-to-host copy (a synchronise)
    upload /    copies of the same byte counts between pageable host memory and the device, timed apart with torch (the entry
    download    point uses plain hipMemcpy on pageable memory too); `rest` = device - upload - download is the allocations, the
                memsets, the launches and the kernels together (a difference of medians, not a measurement of its own)
    report_np   the Python call around it: the float64 copies, the stacked columns, the levels (scipy's norm.ppf), the outputs
    per_class   uncertainty_report.per_class: the sort into class segments, report_np, and every column's ECE, NLL, RMSUE, sharpness
                and coverage of every class from the tallies
    host        the reference-shaped numpy evaluation on this machine's CPU, once: per (class, column) the level loop of calc_ece
                on the flattened arrays and on the [n, 4] arrays (norm.ppf inside the loop, as the reference has it), scipy's
                logpdf for the NLL, the masked RMSUE, the float32 sharpness, and the +-sigma coverage (vectorised here; the
                reference walks the rows in Python)

The script asserts that every flattened and [n, 4] ECE and every coverage count from the device's tallies EQUALS the host's
before it prints a time.  Wall-clock p50 / mean over --steps runs after --warmup.  Prints ONE JSON line.

    python tools/bench_uncert_report.py [--rows 70000] [--columns 14] [--steps 5] [--warmup 1] [--device-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLASSES = 10


def synthetic(rows, columns, seed=17):
    rng = np.random.default_rng([seed, rows, columns])
    y1, x1 = rng.uniform(0, 600, rows), rng.uniform(0, 1100, rows)
    gt = np.stack([y1, x1, y1 + rng.uniform(8, 300, rows), x1 + rng.uniform(8, 300, rows)], 1)
    true_sigma = rng.uniform(0.5, 6, (rows, 4))
    pred = gt + rng.normal(0, 1, (rows, 4)) * true_sigma
    sig = [true_sigma * rng.uniform(0.4, 2.5) * rng.uniform(0.8, 1.25, (rows, 4)) for _ in range(columns)]
    gc = rng.integers(1, CLASSES + 1, rows).astype(np.float64)
    pc = np.where(rng.random(rows) < 0.1, rng.integers(1, CLASSES + 1, rows), gc).astype(np.float64)
    return gt, pred, sig, gc, pc


def host_numbers(gt, pred, s):
    """What the reference computes for one subset and one sigma column, in its shape: -> ece_flat, ece_box, covered, nll, rmsue, sharp."""
    from scipy import stats
    p_m = np.linspace(0, 1, 100)
    out = []
    for g, p, u in ((gt.flatten(), pred.flatten(), s.flatten()), (gt, pred, s)):
        emp = [0] * 100
        for i in range(100):
            emp[i] = np.mean(np.less_equal(np.abs(p - g), np.abs(u * stats.norm.ppf((1 - p_m[i]) / 2))), axis=0)
        out.append(np.mean(np.abs(emp - (p_m if g.ndim == 1 else np.swapaxes([p_m] * 4, 0, 1)))))
    res = np.abs(gt - pred).flatten()
    covered = int(((pred - s <= gt) & (gt <= pred + s)).all(axis=1).sum())
    nll = -np.sum(np.nan_to_num(stats.norm.logpdf(res, scale=s.flatten()))) / res.size
    rmsue = np.sqrt(np.mean(np.square(s.flatten() - res)[res != 0.0]))
    sharp = np.sqrt(np.mean(np.square(s.astype(np.float32).flatten())))
    return out[0], out[1], covered, nll, rmsue, sharp


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
    ap.add_argument("--columns", type=int, default=14)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device-only", action="store_true", help="time the device call and the copies only (for a kernel trace)")
    a = ap.parse_args()
    import torch
    from uda_amd import capi
    from uda_amd import uncertainty_report as ur
    lib = capi.load()
    gt, pred, sig, gc, pc = synthetic(a.rows, a.columns)
    ids = [float(c) for c in range(1, CLASSES + 1)]
    order = np.argsort(gc, kind="stable")
    off = np.concatenate([[0], np.cumsum([(gc == c).sum() for c in ids])]).astype(np.int64)
    sgt, spred, sgc, spc = (np.ascontiguousarray(x[order]) for x in (gt, pred, gc, pc))
    ssig = np.ascontiguousarray(np.stack([s[order] for s in sig]))
    _, z = ur.levels_z(100)
    B, K, L = CLASSES, a.columns, 100
    outs = [np.zeros((B, 4), np.int64), np.zeros((B, K, 3), np.int64), np.zeros((B, K, 4, L), np.int64), np.zeros((B, 2)), np.zeros((B, K, 3))]

    def device_call():
        rc = lib.uda_uncert_report_np(0, B, K, L, off.ctypes.data, sgt.ctypes.data, spred.ctypes.data, sgc.ctypes.data, spc.ctypes.data,
                                      ssig.ctypes.data, z.ctypes.data, *[o.ctypes.data for o in outs])
        capi.check(lib, None, rc, "uda_uncert_report_np")

    def per_class():
        rep = ur.per_class(gt, pred, sig, gc, pc, ids)
        return rep, [[(rep.ece(k, b), rep.ece_box(k, b), rep.count("covered_all", b, k), rep.nll(k, b), rep.rmsue(k, b), rep.sharpness(k, b))
                      for k in range(K)] for b in range(B)]

    rep, numbers = per_class()
    res = dict(rows=a.rows, columns=K, classes=B, levels=L, compares=int(a.rows) * 4 * K * L)
    if not a.device_only:
        t0 = time.perf_counter()
        host = [[host_numbers(sgt[off[b]:off[b + 1]], spred[off[b]:off[b + 1]], ssig[k, off[b]:off[b + 1]]) for k in range(K)] for b in range(B)]
        res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        worst = 0.0
        for b in range(B):
            for k in range(K):
                d, h = numbers[b][k], host[b][k]
                assert d[0] == h[0] and d[1] == h[1] and d[2] == h[2], "ECE or coverage of class %d column %d differs from the host's" % (b, k)
                worst = max([worst] + [abs(float(x) - float(y)) / abs(float(y)) for x, y in zip(d[3:], h[3:])])
        res["nll_rmsue_sharp_max_rel_diff"] = float("%.3g" % worst)

    up = int(sgt.nbytes + spred.nbytes + sgc.nbytes + spc.nbytes + ssig.nbytes + z.nbytes + 2 * off.nbytes + 12 * (a.rows // capi.REPORT_ROWS + B))
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
        res["report_np"] = timed(lambda: ur.report_np(sgt, spred, list(ssig), sgc, spc, off), a.steps, a.warmup)
        res["per_class"] = timed(per_class, max(1, a.steps // 2), a.warmup)
        res["host_over_device"] = round(res["host_ms"] / res["device"]["p50_ms"], 1)
        res["host_over_per_class"] = round(res["host_ms"] / res["per_class"]["p50_ms"], 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
