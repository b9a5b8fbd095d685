#!/usr/bin/env python3
"""Cost of the active-learning scoring step (`ServingDriver.score_images`, reference active_learning_loop.py:528-765) in the
shipped inference configuration: KITTI raw 1242 x 375 -> D0 1024 x 512, head-only MC dropout (T = 10, rates 0.05), loss
attenuation, softmax.  A pool of --batches batches of --batch images is scored two ways with the strategy --strategy:

  file_route    the route without score_images: `writers.predict_to_file` (serve_stream + class_probs + unpack + one text
                line per detection above min_score), then what `ActiveLearning.score_image` does with the file - every line
                through ast.literal_eval, per detection np.mean(relativize_uncert(...)) / np.mean, per image mean or max
  score_images  `serve_stream(while_resident=score_images)` into `active_learning.ImageScores`
  serve_only    `serve_stream` with a while_resident that does nothing: the served step both routes contain

min_score is chosen on the first batch so that about --rows detections per image lie above it (the seeded weights give scores
of 0.01 to 0.02, where a trained model's 0.4 would keep nothing).  Wall-clock per image over --steps pools after --warmup;
the device time of the score kernel (with the softmax / entropy kernel when the strategy reads entropy) comes from HIP events
around it (profile kind 19), collected in a pass of its own.  Prints ONE JSON line.

    python tools/bench_score.py [--steps 10] [--warmup 2] [--batch 8] [--batches 6] [--strategy mean_alluncert] [--rows 12]
"""
import argparse
import ast
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_score_file(path, st):
    """score_image's walk over the file for the resolved strategy `st`: name -> per-image components."""
    per_image, order = {}, []
    with open(path) as f:
        for line in f:
            d = ast.literal_eval(line.replace("inf", "2e308"))
            vals = []
            for comp in st.components:
                v = 0.0
                for src, tr, w in comp:
                    if src == "entropy":
                        t = d["entropy"]
                    elif src == "det_score":
                        t = d["det_score"]
                    else:
                        u = np.asarray([d["uncalib_" + src]])
                        if tr == "rel_mean":
                            b = np.asarray([d["bbox"]])
                            hgt, wid = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
                            u = u / np.swapaxes([hgt, wid, hgt, wid], 0, 1)
                        t = np.mean(u)
                    v = v + w * t
                vals.append(v)
            if d["image_name"] not in per_image:
                per_image[d["image_name"]] = []
                order.append(d["image_name"])
            per_image[d["image_name"]].append(vals)
    red = np.mean if st.reduce_mean else np.max
    return order, np.asarray([[red([r[k] for r in per_image[name]]) for k in range(st.n_comp)] for name in order])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--strategy", default="mean_alluncert")
    ap.add_argument("--rows", type=int, default=12)
    a = ap.parse_args()
    from uda_amd import active_learning as AL, capi, hparams_config, weights as weights_mod, writers
    from uda_amd.infer_lib import KerasDriver
    cfg = hparams_config.get_efficientdet_config("efficientdet-d0")
    cfg.override(dict(image_size="1024x512", num_classes=7, mc_dropout=True, mc_boxheadrate=0.05, mc_classheadrate=0.05,
                      mc_dropoutsamp=10, loss_attenuation=True, enable_softmax=True))
    p = cfg.as_dict()
    p["is_training_bn"] = False
    w = weights_mod.init_weights(p, seed=0, cls_spread=20.0)
    d = KerasDriver("_", False, "efficientdet-d0", a.batch, False, p, weights=w)
    d.set_dropout_seed(5)
    rng = np.random.default_rng(3)
    pool = [rng.integers(0, 256, (a.batch, 375, 1242, 3), dtype=np.uint8) for _ in range(a.batches)]
    names = [["%06d" % (b * a.batch + i) for i in range(a.batch)] for b in range(a.batches)]
    n_images = a.batch * a.batches
    first = d.serve(pool[0])
    min_score = float(np.float32(np.median(np.sort(first[1], 1)[:, -a.rows - 1])))
    st = AL.resolve_strategy(a.strategy, p)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "prediction_data.txt")

    def file_route():
        if os.path.exists(path):
            os.remove(path)
        written = writers.predict_to_file(d, pool, names, path, min_score)
        order, comp = host_score_file(path, st)
        return order, AL.combine_components(comp, st.combine), written

    def device_route():
        acc = AL.ImageScores(st)
        state = {"b": 0}

        def per_batch(det):
            acc.add([nm + ".jpg" for nm in names[state["b"]]], d.score_images(st, min_score))
            state["b"] += 1
        for _ in d.serve_stream(pool, while_resident=per_batch):
            pass
        return acc.names, acc.scores(), int(acc.count.sum())

    def serve_only():
        for _ in d.serve_stream(pool, while_resident=lambda det: None):
            pass

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        t = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3 / n_images)
        return dict(p50_ms_per_image=round(float(np.median(t)), 4), mean_ms_per_image=round(float(np.mean(t)), 4))

    o1, s1, rows = file_route()
    o2, s2, kept = device_route()
    assert o1 == o2 and rows == kept, (len(o1), len(o2), rows, kept)       # the two routes score the same detections
    res = dict(config="D0 1024x512, KITTI raw 1242x375, head-only MC T=10, loss attenuation; %d batches of %d" % (a.batches, a.batch),
               strategy=a.strategy, min_score=min_score, detections_per_image=round(rows / n_images, 2),
               max_score_difference=float(np.abs(s1 - s2).max()),
               ranking_equal=bool(np.array_equal(np.argsort(s1), np.argsort(s2))))
    res["file_route"] = timed(file_route)
    res["score_images"] = timed(device_route)
    res["serve_only"] = timed(serve_only)
    d.profile_enable([capi.PROF_SCORE])
    device_route()
    ms, launches = d.profile_read(capi.PROF_SCORE)
    d.profile_enable([])
    res["score_kernel_device_us_per_batch"] = round(ms * 1e3 / max(launches, 1), 2)
    res["score_kernel_launches"] = int(launches)
    res["speedup_vs_file_route"] = round(res["file_route"]["p50_ms_per_image"] / res["score_images"]["p50_ms_per_image"], 3)
    d.close()
    os.remove(path)
    os.rmdir(tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
