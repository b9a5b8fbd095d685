#!/usr/bin/env python3
"""Cost of the consistency check (`consistency_ssl`, reference infer_model.py:768-848) in the shipped inference configuration:
KITTI raw 1242 x 375 -> D0 1024 x 512, head-only MC dropout (T = 10, rates 0.05), loss attenuation, softmax
(configs/inference/inference_k.yaml -> allclasses_mcdropout_lossatt_head.yaml), one image per call as the reference serves.

  consistency   ServingDriver.serve_consistency(image): the image and its flip / blur / noise variants in one device run
  four_serves   what a caller does by hand: serve() of the original and of three host-built variants (flip, blur and a
                uint8-rounded noisy image - serve() takes uint8 only, so the float noise variant itself cannot be fed)
  one_serve     serve() of the image alone (the figure without the check)

Wall-clock per call (upload, download and the scores included), p50 and mean over --steps calls after --warmup.  The host
build of the three variants is timed apart (`host_variants_ms`).  Prints ONE JSON line.  For the new kernels' device times
run it under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/bench_consistency.py` and read
augment_u8_kernel, preprocess_kernel<true> and consistency_kernel in the kernel statistics.

    python tools/bench_consistency.py [--steps 50] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def blur_u8(im):
    """The device's fixed-point 9x9 Gaussian (csrc/kernels_post.hip augment_u8_kernel) in numpy, for the host-built variant."""
    taps = (4, 13, 30, 51, 60, 51, 30, 13, 4)
    h, w = im.shape[:2]
    ys = np.abs(np.arange(-4, h + 4))
    ys = np.where(ys >= h, 2 * h - 2 - ys, ys)
    xs = np.abs(np.arange(-4, w + 4))
    xs = np.where(xs >= w, 2 * w - 2 - xs, xs)
    pad = im[ys][:, xs].astype(np.int64)
    r = sum(c * pad[:, i:i + w] for i, c in enumerate(taps))
    s = sum(c * r[j:j + h] for j, c in enumerate(taps))
    return ((s + 32768) >> 16).astype(np.uint8)


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
    a = ap.parse_args()
    from uda_amd import hparams_config, weights as weights_mod
    from uda_amd.infer_lib import KerasDriver
    cfg = hparams_config.get_efficientdet_config("efficientdet-d0")
    cfg.override(dict(image_size="1024x512", num_classes=7, mc_dropout=True, mc_boxheadrate=0.05, mc_classheadrate=0.05,
                      mc_dropoutsamp=10, loss_attenuation=True, enable_softmax=True, consistency_ssl=True))
    p = cfg.as_dict()
    p["is_training_bn"] = False
    w = weights_mod.init_weights(p, seed=0, cls_spread=20.0)
    d = KerasDriver("_", False, "efficientdet-d0", 1, False, p, weights=w)
    d.set_dropout_seed(5)
    img = np.random.default_rng(3).integers(0, 256, (1, 375, 1242, 3), dtype=np.uint8)

    def host_variants():
        flip = np.ascontiguousarray(img[:, :, ::-1])
        blur = blur_u8(img[0])[None]
        noisy = np.clip(np.rint(img + np.random.default_rng(0).normal(0.0, np.sqrt(0.5), img.shape)), 0, 255).astype(np.uint8)
        return flip, blur, noisy
    variants = host_variants()

    def four_serves():
        d.serve(img)
        for v in variants:
            d.serve(v)

    res = dict(config="D0 1024x512, KITTI raw 1242x375, head-only MC T=10, loss attenuation, batch 1",
               consistency=timed(lambda: d.serve_consistency(img), a.steps, a.warmup),
               four_serves=timed(four_serves, a.steps, a.warmup),
               one_serve=timed(lambda: d.serve(img), a.steps, a.warmup),
               host_variants_ms=timed(host_variants, 5, 1)["p50_ms"])
    res["speedup_vs_four_serves"] = round(res["four_serves"]["p50_ms"] / res["consistency"]["p50_ms"], 2)
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
