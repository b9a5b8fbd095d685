#!/usr/bin/env python3
"""Cost of the COCO evaluation (`coco_metric.EvaluationMetric`, `ServingDriver.serve_eval`; reference coco_metric.py:59-283,
custom_cocoeval.py:265-545).

  dataset   --images synthetic images x 100 detection rows, ground truth padded to G = 100 rows with a dozen real ones, 7 classes,
            the 10 standard thresholds:
              device_match + host_accumulate   `coco_metric.match_np` in batches of --batch images (upload, kernel, download), then
                                               `CocoAccumulator.accumulate` + `summarize`
              cpu_loops                        tests/coco_ref.py: evaluateImg / accumulate / summarize as the reference's Python
                                               loops, on this machine's CPU (run once)
            the two must give the same 12 stats bit for bit before their times mean anything
  serving   the shipped inference configuration (KITTI raw 1242 x 375 -> D0 1024 x 512, head-only MC dropout T = 10, loss
            attenuation) in per-class mode at --batch images: serve() against serve_eval(), and the match kernel's device time
            (profile kind 20) beside them

Wall-clock p50 / mean over --steps calls after --warmup.  Prints ONE JSON line.

    python tools/bench_eval.py [--images 256] [--batch 8] [--steps 30] [--warmup 5]
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


def synthetic(n, M=100, G=100, C=7, real=12, seed=3):
    rng = np.random.default_rng(seed)
    gt = np.zeros((n, G, 7), np.float32)
    gt[:, :, 6] = -1
    xy, wh = rng.integers(0, 900, (n, real, 2)), rng.integers(8, 200, (n, real, 2))
    gt[:, :real, 0], gt[:, :real, 1] = xy[..., 1], xy[..., 0]
    gt[:, :real, 2], gt[:, :real, 3] = xy[..., 1] + wh[..., 1], xy[..., 0] + wh[..., 0]
    gt[:, :real, 4] = rng.random((n, real)) < 0.05
    gt[:, :real, 6] = rng.integers(1, C + 1, (n, real))
    det = np.zeros((n, M, 7), np.float32)
    det[:, :, 0] = -1
    k = rng.integers(0, real, (n, M))
    i = np.arange(n)[:, None]
    det[:, :, 1] = gt[i, k, 1] + rng.integers(-8, 9, (n, M))
    det[:, :, 2] = gt[i, k, 0] + rng.integers(-8, 9, (n, M))
    det[:, :, 3] = np.maximum(wh[i, k, 0] + rng.integers(-6, 7, (n, M)), 1)
    det[:, :, 4] = np.maximum(wh[i, k, 1] + rng.integers(-6, 7, (n, M)), 1)
    det[:, :, 5] = np.round(rng.random((n, M)), 3)
    det[:, :, 6] = np.where(rng.random((n, M)) < 0.8, gt[i, k, 6], rng.integers(1, C + 1, (n, M)))
    return gt, det


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
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import coco_ref as R
    from uda_amd import capi, coco_metric as CM, hparams_config, weights as weights_mod
    from uda_amd.infer_lib import KerasDriver
    C = 7
    gt, det = synthetic(a.images, C=C)
    res = dict(dataset="%d images x 100 rows, G=100 (12 real), C=7, 10 thresholds" % a.images)

    def device_flow():
        m = CM.EvaluationMetric(apiou_curve=False, num_classes=C)
        for lo in range(0, a.images, a.batch):
            m.update_state(gt[lo:lo + a.batch], det[lo:lo + a.batch])
        return m

    def match_only():
        for lo in range(0, a.images, a.batch):
            CM.match_np(det[lo:lo + a.batch], gt[lo:lo + a.batch], C)

    t0 = time.perf_counter()
    rec, npig, used = R.match(det, gt, C, R.STD_THRS)
    t1 = time.perf_counter()
    ev = R.accumulate(R.image_ids_of(det), rec, npig, used, R.gt_class_counts(gt, C), list(range(10)))
    want = R.summarize(ev, R.STD_THRS)
    t2 = time.perf_counter()
    m = device_flow()
    assert np.array_equal(m.accumulator.summarize().view(np.uint64), want.view(np.uint64)), "device and CPU loops disagree"
    res["cpu_loops"] = dict(match_ms=round((t1 - t0) * 1e3, 1), accumulate_ms=round((t2 - t1) * 1e3, 1))
    res["device_match"] = timed(match_only, max(a.steps // 5, 2), 1)
    res["host_accumulate"] = timed(lambda: m.accumulator.summarize(), max(a.steps // 5, 2), 1)
    res["device_flow_total"] = timed(lambda: device_flow().result(), max(a.steps // 5, 2), 1)
    res["speedup_vs_cpu_loops"] = round((t2 - t0) * 1e3 / res["device_flow_total"]["p50_ms"], 1)

    cfg = hparams_config.get_efficientdet_config("efficientdet-d0")
    cfg.override(dict(image_size="1024x512", num_classes=C, mc_dropout=True, mc_boxheadrate=0.05, mc_classheadrate=0.05,
                      mc_dropoutsamp=10, loss_attenuation=True, enable_softmax=True))
    p = cfg.as_dict()
    p["is_training_bn"] = False
    d = KerasDriver("_", False, "efficientdet-d0", a.batch, False, p, weights=weights_mod.init_weights(p, seed=0, cls_spread=20.0))
    d.set_dropout_seed(5)
    imgs = np.random.default_rng(3).integers(0, 256, (a.batch, 375, 1242, 3), dtype=np.uint8)
    out = d.serve(imgs, post_mode="per_class")
    g = np.zeros((a.batch, 100, 7), np.float32)
    g[:, :, 6] = -1
    g[:, :12, :4] = out[0][:, :12, :4] + np.float32(2)
    g[:, :12, 6] = np.maximum(out[2][:, :12], 1)
    sink = CM.EvaluationMetric(apiou_curve=True, num_classes=C)

    def serve_eval():
        sink.reset_states()
        d.serve_eval(imgs, g, sink)

    d.profile_enable([capi.PROF_EVAL])
    r = dict(serve=timed(lambda: d.serve(imgs, post_mode="per_class"), a.steps, a.warmup), serve_eval=timed(serve_eval, a.steps, a.warmup))
    ms, launches = d.profile_read(capi.PROF_EVAL)
    r["match_kernel_ms"] = round(ms / max(launches, 1), 4)
    r["thresholds"] = int(sink.iou_thrs.size)
    res["serving_batch_%d_per_class" % a.batch] = r
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
