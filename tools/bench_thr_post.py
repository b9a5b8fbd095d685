#!/usr/bin/env python3
"""Cost of the post-thresholding analysis (`post_thresholding.heat_np` -> `uda_heat_maps_np`, `post_np` -> `uda_thr_post_np`;
reference uncertainty_analysis.py:838-880, :920-1068) on a seeded synthetic validation set: --rows matched rows (default 70 000, a
BDD-sized set) on --images images (default 7 000), a --height x --width map (default 720 x 1280), all ten maps, the default six
IoU thresholds.

    heat_device the C entry point alone on prepared arrays (ten maps, no counts): the uploads, one launch of tiles x 10 blocks, the
                download of 10 * H * W * 8 bytes; the host clock around the call, which ends in a device-to-host copy
    post_device the tally entry point alone at six thresholds with the per-image outputs
    upload /    copies of the heat call's byte counts between pageable host memory and the device, timed apart with torch; `rest` =
    download    heat_device - upload - download is the allocations, the launch and the kernel together (a difference of medians)
    heat_maps   the Python call around it: box_slices, the value columns, the checks, nan_to_num
    spider /    spider_metrics and rank_images end to end, each with its thr_report call
    rank
    host        the reference-shaped numpy loop on this machine's CPU, once: per map `mask[int(y1):int(y2), int(x1):int(x2)] += v`
                and the normalizer's `+= 1` once per row, as `_heatmap_plot` writes them

The script asserts that every map of the device EQUALS the host loop's bit for bit before it prints a time.  Wall-clock p50 / mean
over --steps runs after --warmup.  Prints ONE JSON line.  For the kernels alone run it with --device-only under a kernel trace.

    python tools/bench_thr_post.py [--rows 70000] [--images 7000] [--height 720] [--width 1280] [--steps 5] [--warmup 1] [--device-only]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT6 = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75]


def synthetic(rows, images, H, W, seed=29):
    rng = np.random.default_rng([seed, rows, images])
    tp = rng.random(rows) < 0.85
    ious = np.round(rng.uniform(0.05, 0.999, rows), 3)
    wrong = ~(tp & (ious >= 0.5))
    h, w = rng.gamma(2.0, H / 24.0, rows) + 8, rng.gamma(2.0, W / 28.0, rows) + 8        # about 70 x 100 pixels on 720 x 1280
    y1, x1 = rng.uniform(-5, H - 10, rows), rng.uniform(-5, W - 10, rows)
    gt = np.stack([y1, x1, y1 + h, x1 + w], 1)
    pred = gt + rng.normal(0, 3.0, (rows, 4))
    albox = rng.gamma(2.0, 0.05, (rows, 4)) * np.where(wrong, 1.5, 1.0)[:, None]
    entropy = rng.uniform(0, 1.2, rows) * np.where(wrong, 1.0, 0.6)
    names = np.array(["%06d.png" % i for i in rng.integers(0, images, rows)])
    return dict(gt=gt, pred=pred, albox=albox, calib_albox=albox * 1.25, entropy=entropy, calib_entropy=entropy * 0.75,
                opt=0.7 * entropy + 0.4 * np.mean(albox, axis=1), ious=ious, tp=tp, names=names)


def host_heatmap(pred, value, mask_size, uncert=True):
    """`_heatmap_plot` (uncertainty_analysis.py:925-937) up to the array it hands to imshow."""
    mask = np.zeros(mask_size)
    normalizer = np.zeros(mask_size)
    i = 0
    for bb in pred:
        mask[int(bb[0]):int(bb[2]), int(bb[1]):int(bb[3])] += value[i]
        normalizer[int(bb[0]):int(bb[2]), int(bb[1]):int(bb[3])] += 1
        i += 1
    if uncert:
        with np.errstate(all="ignore"):
            mask = np.nan_to_num(mask / normalizer)
    return mask


def host_maps(d, filters, mask_size):
    gt, pred = d["gt"], d["pred"]
    out = {"gt_loc": host_heatmap(gt, np.mean(np.ones_like(gt), axis=1), mask_size, uncert=False)}
    for al, stem in ((d["albox"], "albox"), (d["calib_albox"], "calib_albox")):
        out["uncert_" + stem] = host_heatmap(pred, np.mean(al, axis=1), mask_size)
        out["rmse_" + stem] = host_heatmap(gt, np.sqrt(np.mean((np.abs(gt - pred) - al) ** 2, axis=-1)), mask_size)
    out["entropy"] = host_heatmap(pred, d["entropy"], mask_size)
    out["calib_entropy"] = host_heatmap(pred, d["calib_entropy"], mask_size)
    for f, key in zip(filters, ("opt_uncert_cr", "opt_uncert_fr", "opt_uncert_fk")):
        out[key] = host_heatmap(pred[f], d["opt"][f], mask_size)
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
    ap.add_argument("--images", type=int, default=7000)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device-only", action="store_true", help="time the device calls and the copies only (for a kernel trace)")
    a = ap.parse_args()
    import torch
    from uda_amd import capi
    from uda_amd import post_thresholding as pt
    from uda_amd import thresholding as th
    lib = capi.load()
    N, H, W, K = a.rows, a.height, a.width, len(DEFAULT6)
    d = synthetic(N, a.images, H, W)
    params = {"thr_cd": True, "thr_fpr_tpr": 0.95, "thr_iou_thrs": DEFAULT6}
    filters = th.collect_thresh_results(d["opt"], d["ious"], d["tp"], max(DEFAULT6), params=params)
    kw = dict(albox=d["albox"], calib_albox=d["calib_albox"], entropy=d["entropy"], calib_entropy=d["calib_entropy"],
              opt_uncert=d["opt"], pred_filters=filters)
    res = dict(rows=N, images=int(len(np.unique(d["names"]))), map=[H, W], maps=len(pt.HEAT_KEYS), thresholds=K,
               removed=[int(f.sum()) for f in filters[:3]])

    # the prepared arrays of the ten maps, captured from heat_maps' own call
    captured = {}

    def capture(*args, **kwargs):
        captured["args"] = pt.check_heat_problem(*args)
        return pt.heat_np(*args, **kwargs)

    maps = pt.heat_maps(d["gt"], d["pred"], (H, W), heat=capture, **kw)
    assert list(maps) == list(pt.HEAT_KEYS)
    if not a.device_only:
        t0 = time.perf_counter()
        want = host_maps(d, filters, (H, W))
        res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        for key in pt.HEAT_KEYS:
            assert np.array_equal(maps[key].view(np.uint64), want[key].view(np.uint64)), "map %s differs from the host loop's" % key
    rects, values, sel, m_rect, m_value, m_sel, m_mean, _, _ = captured["args"]
    M, V, Q, R = m_rect.size, values.shape[0], sel.shape[0], rects.shape[0]
    heat = np.zeros((M, H, W))
    p = lambda x: x.ctypes.data          # noqa: E731

    def heat_call():
        rc = lib.uda_heat_maps_np(0, p(rects), R, p(values), V, p(sel), Q, N, p(m_rect), p(m_value), p(m_sel), p(m_mean), M, H, W,
                                  p(heat), None)
        capi.check(lib, None, rc, "uda_heat_maps_np")

    thrs6 = np.ascontiguousarray(th.thr_report(d["opt"][None], d["ious"], d["tp"], DEFAULT6, True, 0.95).thr[0, 0])
    iou6, tp8 = np.asarray(DEFAULT6), np.ascontiguousarray(d["tp"].astype(np.uint8))
    ids = np.ascontiguousarray(np.unique(d["names"], return_inverse=True)[1].reshape(-1).astype(np.int32))
    n_img = int(ids.max()) + 1
    outs = [np.zeros((K, 2, 4), np.int64), np.zeros((K, 2)), np.zeros((n_img, 4), np.int32), np.zeros((n_img, 3), np.int32)]

    def post_call():
        rc = lib.uda_thr_post_np(0, p(d["opt"]), p(d["ious"]), p(tp8), p(ids), N, n_img, p(iou6), p(thrs6), K, K - 1,
                                 *[p(o) for o in outs])
        capi.check(lib, None, rc, "uda_thr_post_np")

    up, down = int(rects.nbytes + values.nbytes + sel.nbytes), int(heat.nbytes)
    h_up, h_down = torch.empty(up, dtype=torch.uint8), torch.empty(down, dtype=torch.uint8)
    d_up, d_down = torch.empty(up, dtype=torch.uint8, device="cuda"), torch.empty(down, dtype=torch.uint8, device="cuda")

    def copy_up():
        d_up.copy_(h_up)
        torch.cuda.synchronize()

    def copy_down():
        h_down.copy_(d_down)
        torch.cuda.synchronize()

    tiles = -(-H // pt.TILE_H) * -(-W // pt.TILE_W)
    res.update(bytes_up=up, bytes_down=down, blocks=tiles * M, table_bytes_read_by_all_blocks=int(tiles * M * N * 25),
               heat_device=timed(heat_call, a.steps, a.warmup), post_device=timed(post_call, a.steps, a.warmup),
               upload=timed(copy_up, a.steps, a.warmup), download=timed(copy_down, a.steps, a.warmup))
    res["rest_ms"] = round(res["heat_device"]["p50_ms"] - res["upload"]["p50_ms"] - res["download"]["p50_ms"], 3)
    if not a.device_only:
        res["heat_maps"] = timed(lambda: pt.heat_maps(d["gt"], d["pred"], (H, W), **kw), a.steps, a.warmup)
        res["spider"] = timed(lambda: pt.spider_metrics(d["opt"], d["ious"], d["tp"], params=params), a.steps, a.warmup)
        res["rank"] = timed(lambda: pt.rank_images(d["names"], d["opt"], d["ious"], d["tp"], max(DEFAULT6), params=params,
                                                   rng=random.Random(1)), a.steps, a.warmup)
        res["host_over_heat_maps"] = round(res["host_ms"] / res["heat_maps"]["p50_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
