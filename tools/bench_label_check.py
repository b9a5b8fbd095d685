#!/usr/bin/env python3
"""Cost of label correction (`ServingDriver.serve_label_check`, reference src/ssl_utils/glc.py) on the flagship workload: 32 images
1280 x 768, D0, full MC dropout (T = 10), loss attenuation, softmax, with the consistency check (4 x 32 images per run).

  serve_label_check   the consistency run, the ground-truth upload and the label check in one device pass; the host receives the
                      verdicts, and the run's box and class columns once when a missing label is flagged (the writer of
                      missing boxes reads them)
  verdicts_only       the same with missing_boxes=False: the verdicts and nothing else
  host_path           what a caller does without it: serve_consistency (every detection column of the 4 x 32 images, cons_iou and
                      cons_cls come to the host), the columns split as serve_unpacked splits them, and a vectorised numpy
                      stand-in of the three verdicts (per image one IoU matrix; the reference's own two Python loops are slower)
  step alone          on the resident run: label_check (upload of the ground truth, kernel, one copy of the verdicts, the
                      reference-shaped lists of `LabelCheck`) and its three library calls alone, against the numpy stand-in
                      on arrays that are already on the host (which builds no lists)

The ground truth is made from the run's own detections (G rows per image: jittered copies, exact copies, far-away boxes) and
min_score is the median score, so that about half of the rows are kept.  Device and stand-in must agree on every count before
their times mean anything.  Wall-clock p50 / mean over --steps calls after --warmup; bytes copied to the host per batch are
counted from the arrays each path brings over.  Prints ONE JSON line.

    python tools/bench_label_check.py [--batch 32] [--gt-rows 24] [--steps 5] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(p50_ms=round(float(np.median(t)), 3), mean_ms=round(float(np.mean(t)), 3))


def make_gt(boxes, scores, min_score, G, seed=3):
    rng = np.random.default_rng(seed)
    n = boxes.shape[0]
    gb, gc = np.full((n, G, 4), -1, np.float32), np.full((n, G), -1, np.float32)
    for i in range(n):
        kept = np.where(scores[i] > min_score)[0]
        for g in range(G - 2):
            kind = rng.random()
            if kind < 0.15 or not len(kept):
                gb[i, g] = [5000 + 100 * g, 5000, 5060 + 100 * g, 5080]
            else:
                src = boxes[i, kept[rng.integers(len(kept))], :4]
                gb[i, g] = src if kind < 0.3 else src + rng.normal(0, 3.0, 4).astype(np.float32)
            gc[i, g] = float(rng.integers(1, 8))
    return gb, gc


def numpy_verdicts(boxes, scores, cons, gb, gc, min_score, iou_consist, correct_max_inter, correct_score):
    """The three verdicts, vectorised per image (float32 differences, float64 products, as the handle computes them)."""
    n = scores.shape[0]
    counts = np.zeros((n, 5), np.int64)
    out = []
    for i in range(n):
        kept = np.where(scores[i] > np.float32(min_score))[0]
        rows = np.where(gc[i] > 0)[0]
        counts[i, :2] = len(kept), len(rows)
        if not len(kept) or not len(rows):
            counts[i, 4] = int((cons[i, kept] >= iou_consist).sum()) if len(kept) else 0
            out.append((np.zeros(0, np.int64), np.zeros(len(kept), bool), gb[i, rows]))
            continue
        p, g = boxes[i, kept, :4], gb[i, rows]
        yA, xA = np.maximum(g[:, None, 0], p[None, :, 0]), np.maximum(g[:, None, 1], p[None, :, 1])
        yB, xB = np.minimum(g[:, None, 2], p[None, :, 2]), np.minimum(g[:, None, 3], p[None, :, 3])
        inter = np.maximum(np.float32(0), xB - xA).astype(np.float64) * np.maximum(np.float32(0), yB - yA).astype(np.float64)
        area_g = np.abs(g[:, 3] - g[:, 1]).astype(np.float64) * np.abs(g[:, 2] - g[:, 0]).astype(np.float64)
        area_p = np.abs(p[:, 3] - p[:, 1]).astype(np.float64) * np.abs(p[:, 2] - p[:, 0]).astype(np.float64)
        union = (area_g[:, None] + area_p[None, :]) - inter
        ious = np.divide(inter, union, out=np.zeros_like(inter), where=union != 0)
        matched, iou_gt = np.argmax(ious, 1), np.max(ious, 1)
        wrong = np.where(iou_gt == 0)[0]
        extra = np.equal(np.max(ious, 0), 0) * np.greater_equal(cons[i, kept], iou_consist)
        cond = (cons[i, kept][matched] > iou_consist) * (iou_gt <= correct_max_inter) * (scores[i, kept][matched] >= np.float32(correct_score))
        corrected = g.copy()
        better = np.unique(matched[cond])
        for k in better:
            corrected[np.argmax(matched == k)] = p[k]
        counts[i, 2:] = len(wrong), len(better), int(extra.sum())
        out.append((wrong, extra, corrected))
    return counts, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--image-size", default="1280x768")
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--gt-rows", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    from uda_amd import hparams_config, weights as weights_mod
    from uda_amd.infer_lib import KerasDriver
    cfg = hparams_config.get_efficientdet_config("efficientdet-d0")
    cfg.override(dict(image_size=a.image_size, num_classes=7, mc_dropout=True, mc_dropoutrate=0.05, mc_dropoutsamp=a.samples,
                      loss_attenuation=True, enable_softmax=True, consistency_ssl=True))
    p = cfg.as_dict()
    p["is_training_bn"] = False
    d = KerasDriver("_", False, "efficientdet-d0", a.batch, False, p, weights=weights_mod.init_weights(p, seed=0, cls_spread=20.0))
    d.set_dropout_seed(5)
    W, H = (int(v) for v in a.image_size.split("x"))
    imgs = np.random.default_rng(2).integers(0, 256, (a.batch, H, W, 3), dtype=np.uint8)

    det, cons, agree = d.serve_consistency(imgs)
    min_score = float(np.median(det[1]))
    thr = dict(iou_consist=float(np.median(cons[det[1] > min_score])), correct_max_inter=1.0, correct_score=min_score)
    gb, gc = make_gt(det[0], det[1], min_score, a.gt_rows)

    def host_path():
        dt, ci, ag = d.serve_consistency(imgs)
        boxes, classes = dt[0][..., :4], (dt[2] if dt[2].ndim == 2 else dt[2][..., 0])
        return numpy_verdicts(boxes, dt[1], ci, gb, gc, min_score, **thr), (boxes, classes)

    chk = d.serve_label_check(imgs, gb, gc, min_score=min_score, md_max_inter=0, **thr)
    (want, _), _ = host_path()
    assert np.array_equal(chk.counts, want), "device and the numpy stand-in disagree"
    n, M, G = a.batch, d.M, a.gt_rows
    verdict_bytes = n * G * (8 + 4 + 1 + 16) + n * M * (8 + 1) + n * 20
    full = d._collect(4 * n)
    column_bytes = sum(x.nbytes for x in full)
    box_class_bytes = full[0].nbytes + full[2].nbytes          # what the flagged missing labels bring over: boxes and classes
    res = dict(config="D0 %s, %d images, full MC T=%d, loss attenuation, consistency run of %d images, G=%d rows, M=%d"
                      % (a.image_size, n, a.samples, 4 * n, G, M),
               totals=chk.totals(), min_score=round(min_score, 5),
               serve_label_check=timed(lambda: d.serve_label_check(imgs, gb, gc, min_score=min_score, **thr), a.steps, a.warmup),
               verdicts_only=timed(lambda: d.serve_label_check(imgs, gb, gc, min_score=min_score, missing_boxes=False, **thr), a.steps, a.warmup),
               host_path=timed(host_path, a.steps, a.warmup),
               serve_consistency=timed(lambda: d.serve_consistency(imgs), a.steps, a.warmup))
    d.serve_consistency(imgs)
    from uda_amd import label_correction as lc
    args = d._label_check_args(lc.METHODS, min_score, thr["iou_consist"], 0, "eq", thr["correct_max_inter"], thr["correct_score"])
    raw = lc.empty_result(n, M, G)

    def library_calls():
        d._ck(d._lib.uda_set_ground_truth(d._h, gb.ctypes.data, gc.ctypes.data, n, G), "uda_set_ground_truth")
        d._queue_label_check(args)
        d._ck(d._lib.uda_get_label_check(d._h, *[raw[k].ctypes.data for k in lc.RESULT_ORDER]), "uda_get_label_check")

    res["step_alone"] = dict(
        library_calls=timed(library_calls, 20, 3),
        label_check=timed(lambda: d.label_check(gb, gc, min_score=min_score, missing_boxes=False, **thr), 20, 3),
        numpy_stand_in=timed(lambda: numpy_verdicts(det[0][..., :4], det[1], cons, gb, gc, min_score, **thr), 20, 3))
    res["bytes_to_host"] = dict(verdicts_only=verdict_bytes, serve_label_check=verdict_bytes + box_class_bytes,
                                host_path=column_bytes + cons.nbytes + agree.size)
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
