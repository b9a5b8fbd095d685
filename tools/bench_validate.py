#!/usr/bin/env python3
"""Cost of the validate step (`ServingDriver.serve_validate`, reference validate_model.py:154-470) in the shipped inference
configuration: KITTI raw 1242 x 375 -> D0 1024 x 512, head-only MC dropout (T = 10, rates 0.05), loss attenuation, softmax;
ground truth padded to G = 100 rows with a dozen real ones, method IoU.

  host_loop        serve() + class_probs() + what the reference does next on the host: per kept GT row one numpy
                   gt_box_assigner call over the 100 detections, then the row of every column (what a caller without
                   serve_validate has to write)
  host_vectorized  the same with the G x M IoU matrix of an image built in one numpy expression
  serve_validate   one device pass: the assignment and the row gather run behind the post-process, the matched rows come
                   back as one table

Wall-clock per call (upload, download included), p50 and mean over --steps calls after --warmup, at batch 1 and at
--batch images.  Prints ONE JSON line.  For the new kernels' device times run it under
`rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_validate.py` and read assign_gt_kernel and
gather_assigned_kernel in the kernel statistics.

    python tools/bench_validate.py [--steps 50] [--warmup 5] [--batch 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def iou_np(gt, boxes):
    """utils_box.calc_iou_np (float32 differences, float64 products), broadcasting gt [..., 1, 4] against boxes [M, 4]."""
    yA, xA = np.maximum(gt[..., 0], boxes[..., 0]), np.maximum(gt[..., 1], boxes[..., 1])
    yB, xB = np.minimum(gt[..., 2], boxes[..., 2]), np.minimum(gt[..., 3], boxes[..., 3])
    inter = np.maximum(np.float32(0), xB - xA).astype(np.float64) * np.maximum(np.float32(0), yB - yA).astype(np.float64)
    a = np.abs(gt[..., 3] - gt[..., 1]).astype(np.float64) * np.abs(gt[..., 2] - gt[..., 0]).astype(np.float64)
    b = np.abs(boxes[..., 3] - boxes[..., 1]).astype(np.float64) * np.abs(boxes[..., 2] - boxes[..., 0]).astype(np.float64)
    union = (a + b) - inter
    return np.divide(inter, union, out=np.zeros_like(inter), where=union != 0)


def host_flow(d, imgs, gb, gc, vectorized):
    from uda_amd import postprocess as pp
    det = d.serve(imgs)
    n = det[0].shape[0]
    probab, entropy = d.class_probs(n)
    un = pp.unpack_detections(d.params, det, probab, entropy)
    im_idx, ks = [], []
    for i in range(n):
        rows = np.where(gc[i] > 0)[0]
        boxes = un["boxes"][i]
        if vectorized:
            k = np.argmax(iou_np(gb[i, rows][:, None, :], boxes[None]), axis=1)
        else:
            k = [int(np.argmax(iou_np(np.repeat(gb[i, r][None], len(boxes), 0), boxes))) for r in rows]
        im_idx += [i] * len(rows)
        ks += list(k)
    im_idx, ks = np.asarray(im_idx), np.asarray(ks)
    return {key: (None if un[key] is None else un[key][im_idx, ks])
            for key in ("scores", "boxes", "classes", "logits", "probab", "entropy", "mcclass", "mcbox", "albox")}


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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    from uda_amd import hparams_config, weights as weights_mod
    from uda_amd.infer_lib import KerasDriver
    cfg = hparams_config.get_efficientdet_config("efficientdet-d0")
    cfg.override(dict(image_size="1024x512", num_classes=7, mc_dropout=True, mc_boxheadrate=0.05, mc_classheadrate=0.05,
                      mc_dropoutsamp=10, loss_attenuation=True, enable_softmax=True))
    p = cfg.as_dict()
    p["is_training_bn"] = False
    w = weights_mod.init_weights(p, seed=0, cls_spread=20.0)
    res = dict(config="D0 1024x512, KITTI raw 1242x375, head-only MC T=10, loss attenuation, G=100 (12 real rows), IoU")
    for batch in (1, a.batch):
        d = KerasDriver("_", False, "efficientdet-d0", batch, False, p, weights=w)
        d.set_dropout_seed(5)
        rng = np.random.default_rng(3)
        imgs = rng.integers(0, 256, (batch, 375, 1242, 3), dtype=np.uint8)
        det = d.serve(imgs)
        gb = np.full((batch, 100, 4), -1, np.float32)
        gc = np.full((batch, 100), -1, np.float32)
        for i in range(batch):
            ks = rng.integers(0, max(int(det[3][i]), 1), 12)
            gb[i, :12] = det[0][i, ks, :4] + rng.normal(0, 2, (12, 4)).astype(np.float32)
            gc[i, :12] = rng.integers(1, 8, 12)
        got = d.serve_validate(imgs, gb, gc, method="IoU")[1]
        want = host_flow(d, imgs, gb, gc, False)
        for key, v in want.items():                       # the three flows must agree before their times mean anything
            assert (v is None and got[key] is None) or np.array_equal(v, got[key]), key
        assert all(np.array_equal(v, host_flow(d, imgs, gb, gc, True)[k]) for k, v in want.items() if v is not None)
        r = dict(serve_validate=timed(lambda: d.serve_validate(imgs, gb, gc, method="IoU"), a.steps, a.warmup),
                 host_loop=timed(lambda: host_flow(d, imgs, gb, gc, False), a.steps, a.warmup),
                 host_vectorized=timed(lambda: host_flow(d, imgs, gb, gc, True), a.steps, a.warmup),
                 serve_only=timed(lambda: d.serve(imgs), a.steps, a.warmup))
        r["speedup_vs_host_loop"] = round(r["host_loop"]["p50_ms"] / r["serve_validate"]["p50_ms"], 3)
        res["batch_%d" % batch] = r
        d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
