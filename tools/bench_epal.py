#!/usr/bin/env python3
"""Cost of the epistemic-vs-aleatoric comparison (`epal.compare_epal` / `compare_many` -> `uda_kde_eval_np`; reference
uncertainty_ep_vs_al.py:456-545, its KDE :361-375): --rows seeded validation records, a --mesh x --mesh mesh, one configuration
(uncalib, MC dropout) and five (uncalib, uncalib with the entropy, iso_all, iso_percoo, ts_all).

    device_1 / device_5      the C entry point alone on the prepared (whitened) arrays of one / five configurations: upload of rows
                             and points, two launches, download of the sums; the host clock around the call, which ends in a
                             device-to-host copy (a synchronise)
    upload_* / download_*    copies of the same byte counts between pageable host memory and the device, timed apart with torch;
                             `rest_*` = device - upload - download is what is left for the launches, the allocations and the tables
    compare_epal / compare_many   end to end from the records: the IoU filter, the columns, the grid search, whitening, the device
                             call, the norm, the metric lists
    scipy_ms                 scipy.stats.gaussian_kde(...)(positions) of the first configuration on this machine's CPU, measured ONCE
                             (`cpu_reference`).  scipy is required: `epal.kde_eval` itself whitens with scipy.linalg

Before any time is printed every value of the device's pdf is asserted to lie within (n + 16) * 2^-52 relative (1e-300 absolute) of
that CPU reference; `max_rel_diff_over_bound` is the largest ratio met.  `kernel_pairs` counts the Gaussian terms a call evaluates.

Wall-clock p50 / mean over --steps runs after --warmup.  Prints ONE JSON line.  For the kernels alone run it with --device-only
under a kernel trace.

    python tools/bench_epal.py [--rows 70000] [--mesh 100] [--steps 5] [--warmup 1] [--device-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = [("uncalib", False), ("uncalib", True), ("iso_all", False), ("iso_percoo", False), ("ts_all", False)]
CLASS_NAMES = ["car", "pedestrian", "cyclist"]


def synthetic(n, seed=11):
    """n validation records with the keys compare_epal reads; every detection overlaps its ground truth."""
    rng = np.random.default_rng([seed, n])
    y1, x1 = rng.uniform(0, 300, n), rng.uniform(0, 900, n)
    h, w = rng.uniform(24, 200, n), rng.uniform(24, 260, n)
    box = np.stack([y1, x1, y1 + h, x1 + w], 1)
    gt = box + rng.normal(0, 3, (n, 4))
    hw = np.stack([h, w, h, w], 1)
    al = rng.lognormal(-3.0, 0.6, n)
    mc = 0.4 * al + rng.lognormal(-3.6, 0.7, n)
    cols = {"uncalib_albox": al[:, None] * hw * rng.uniform(0.9, 1.1, (n, 4)), "uncalib_mcbox": mc[:, None] * hw * rng.uniform(0.9, 1.1, (n, 4))}
    for k, name in enumerate(("iso_all", "iso_percoo", "ts_all")):
        cols[name + "_albox"] = cols["uncalib_albox"] * (0.6 + 0.1 * k) + 0.1
        cols[name + "_mcbox"] = cols["uncalib_mcbox"] * (1.5 + 0.2 * k) + 0.2
    cols = {k: v.tolist() for k, v in cols.items()}
    box, gt = box.tolist(), gt.tolist()
    score, ent = rng.uniform(0.3, 1.0, n).tolist(), rng.uniform(0.0, 1.09, n).tolist()
    cls, gcls = rng.integers(1, 4, n).tolist(), rng.integers(1, 4, n).tolist()
    recs = []
    for i in range(n):
        r = {"image_name": "%06d.png" % (i // 10), "score": score[i], "bbox": box[i], "gt_bbox": gt[i], "class": cls[i], "gt_class": gcls[i],
             "entropy": ent[i]}
        for k, v in cols.items():
            r[k] = v[i]
        recs.append(r)
    return recs


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
    ap.add_argument("--mesh", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device-only", action="store_true", help="time the device calls and the copies only (for a kernel trace)")
    a = ap.parse_args()
    import torch
    from uda_amd import capi, epal
    recs = synthetic(a.rows)
    res = dict(rows=a.rows, mesh=a.mesh, configs=len(CONFIGS))

    # the prepared arrays of the one call, captured from compare_many's own
    captured = {}

    def capture(*args, **kw):
        captured[len(args[2]) - 1] = args
        return epal.kde_eval_np(*args, **kw)

    one = epal.compare_many(recs, CLASS_NAMES, CONFIGS[:1], mesh=a.mesh, engine=capture)[0]
    five = epal.compare_many(recs, CLASS_NAMES, CONFIGS, mesh=a.mesh, engine=capture)
    assert five[0].pdf.tobytes() == one.pdf.tobytes(), "a configuration alone and among five give different bits"
    n = int(one.keep.sum())
    res.update(kept_rows=n, grid_size=[c.grid_size for c in five])

    if not a.device_only:
        positions = np.vstack([one.pdf_x.ravel(), one.pdf_y.ravel()])
        dataset = np.stack([one.raw_al, one.raw_mc])
        t0 = time.perf_counter()
        from scipy.stats import gaussian_kde
        want, res["cpu_reference"] = gaussian_kde(dataset)(positions), "scipy.stats.gaussian_kde"
        res["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        bound = (n + 16) * 2.0 ** -52 * np.abs(want) + 1e-300
        worst = float(np.max(np.abs(one.pdf.ravel() - want) / bound))
        assert worst <= 1.0, "a pdf value of the device differs from the CPU reference's by %g times its bound" % worst
        res["max_rel_diff_over_bound"] = round(worst, 4)

    lib = capi.load()
    p = lambda x: None if x is None else x.ctypes.data          # noqa: E731
    for B in (1, len(CONFIGS)):
        D, data, d_off, weight, points, p_off = captured[B]
        data, points = np.ascontiguousarray(data), np.ascontiguousarray(points)
        out = np.empty(int(p_off[-1]))

        def device_call():
            rc = lib.uda_kde_eval_np(0, D, B, p(data), p(d_off), p(weight), p(points), p(p_off), p(out))
            capi.check(lib, None, rc, "uda_kde_eval_np")

        up, down = int(data.nbytes + points.nbytes + d_off.nbytes + p_off.nbytes), int(out.nbytes)
        h_up, h_down = torch.empty(up, dtype=torch.uint8), torch.empty(down, dtype=torch.uint8)
        d_up, d_down = torch.empty(up, dtype=torch.uint8, device="cuda"), torch.empty(down, dtype=torch.uint8, device="cuda")

        def copy_up():
            d_up.copy_(h_up)
            torch.cuda.synchronize()

        def copy_down():
            h_down.copy_(d_down)
            torch.cuda.synchronize()

        runs = -(-np.diff(d_off) // capi.KDE_RUN)
        res.update({"kernel_pairs_%d" % B: int((np.diff(d_off) * np.diff(p_off)).sum()), "bytes_up_%d" % B: up, "bytes_down_%d" % B: down,
                    "run_sum_bytes_%d" % B: int((runs * np.diff(p_off)).sum() * 8),
                    "device_%d" % B: timed(device_call, a.steps, a.warmup), "upload_%d" % B: timed(copy_up, a.steps, a.warmup),
                    "download_%d" % B: timed(copy_down, a.steps, a.warmup)})
        res["rest_%d_ms" % B] = round(res["device_%d" % B]["p50_ms"] - res["upload_%d" % B]["p50_ms"] - res["download_%d" % B]["p50_ms"], 3)
    if not a.device_only:
        res["compare_epal"] = timed(lambda: epal.compare_epal(recs, CLASS_NAMES, mesh=a.mesh), a.steps, a.warmup)
        res["compare_many"] = timed(lambda: epal.compare_many(recs, CLASS_NAMES, CONFIGS, mesh=a.mesh), a.steps, a.warmup)
        res["scipy_over_device_1"] = round(res["scipy_ms"] / res["device_1"]["p50_ms"], 1)
        res["scipy_over_compare_epal"] = round(res["scipy_ms"] / res["compare_epal"]["p50_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
