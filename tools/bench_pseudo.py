#!/usr/bin/env python3
"""Cost of the teacher's pseudo-labelling step (`ServingDriver.pseudo_rows`, reference SSL_stac.py:302-642) on one batch of the
flagship workload: 32 images 1280 x 768, D0, MC dropout T = 10 (rate 0.05 everywhere), loss attenuation, softmax, 7 classes.
The batch is selected two ways with the strategy --strategy:

  pseudo_rows   `serve_resident` + `pseudo_rows` + `PseudoLabelSet.finalize`: the pack's head and the candidate records are all
                that reaches the host
  unpacked      a stand-in for the route without pseudo_rows, on the same run: `serve_unpacked` (the 100-row columns, logits,
                probabilities and entropy downloaded) plus the selection in VECTORISED numpy - the strategy's value for all M rows
                at once, the cap, the filters, nanmin / nanmax.  A caller without pseudo_rows would go through the text file or
                score row by row, both slower: the comparison is conservative
  serve_only    `serve_resident` + a synchronize: the served step both routes contain

min_score and tau are chosen on the first serve so that about --rows detections per image lie above min_score and half of them
above tau (the seeded weights give scores of 0.01 to 0.02, where the writer's 0.1 would keep nothing).  Wall-clock per batch
over --steps after --warmup.  Bytes to the host: for pseudo_rows what the library copies - the head (minmax, kept, cand, the
error flag: 24 n + 8 bytes) and the K used records (40 K), not the room for n x 99 records behind them; for unpacked the arrays
`serve_unpacked` returns, each of which is one download.  The device time
of the row and packing kernels (with the softmax / entropy kernel when the strategy reads entropy) comes from HIP events around
them (profile kind 21), collected in a pass of its own.  Prints ONE JSON line.

    python tools/bench_pseudo.py [--steps 10] [--warmup 2] [--batch 32] [--strategy alluncert] [--rows 40]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_select(un, sel, min_score, tau, max_rows):
    """The first half of score_image on unpacked columns, vectorised numpy (float64): -> per image (rows, v) of the
    candidates, and the batch's min / max."""
    scores = un["scores"]
    boxes = un["boxes"][..., :4].astype(np.float64)
    h, w = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
    side = np.stack([h, w, h, w], -1)

    def term(src, tr):
        if src == "entropy":
            return un["entropy"].astype(np.float64)
        if src == "det_score":
            return scores.astype(np.float64)
        a = un[src].astype(np.float64)
        with np.errstate(all="ignore"):
            return (a / side).mean(-1) if tr == "rel_mean" else a.mean(-1)

    comps = []
    for comp in sel.components:
        v = comp[0][2] * term(comp[0][0], comp[0][1])
        if len(comp) > 1:
            v = v + comp[1][2] * term(comp[1][0], comp[1][1])
        comps.append(v)
    with np.errstate(all="ignore"):
        v = 1.0 / np.mean(comps, axis=0) if sel.invert else comps[0]
    out, lo, hi = [], np.inf, -np.inf
    for i in range(scores.shape[0]):
        part = np.where(scores[i] > np.float32(min_score))[0][:max_rows]
        vi = v[i, part]
        if len(vi):
            lo, hi = min(lo, np.nanmin(vi)), max(hi, np.nanmax(vi))
        cand = (vi > tau) if sel.gate else (scores[i, part].astype(np.float64) > tau)
        out.append((part[cand], vi[cand]))
    return out, lo, hi


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--strategy", default="alluncert")
    ap.add_argument("--rows", type=int, default=40)
    a = ap.parse_args()
    from uda_amd import capi, hparams_config, pseudo_labels as PL, weights as weights_mod
    from uda_amd.infer_lib import KerasDriver
    cfg = hparams_config.get_efficientdet_config("efficientdet-d0")
    cfg.override(dict(image_size="1280x768", num_classes=7, mc_dropout=True, mc_dropoutrate=0.05, mc_dropoutsamp=10,
                      loss_attenuation=True, enable_softmax=True))
    p = cfg.as_dict()
    p["is_training_bn"] = False
    w = weights_mod.init_weights(p, seed=0, cls_spread=20.0)
    d = KerasDriver("_", False, "efficientdet-d0", a.batch, False, p, weights=w)
    d.set_dropout_seed(5)
    images = np.random.default_rng(3).integers(0, 256, (a.batch, 768, 1280, 3), dtype=np.uint8)
    names = ["%06d.png" % i for i in range(a.batch)]
    first = d.serve(images)
    ranked = np.sort(first[1], 1)
    min_score = float(np.float32(np.median(ranked[:, -a.rows - 1])))
    sel = PL.resolve_selection(a.strategy, p, (0.7, 1.3))
    tau = float(np.float32(np.median(ranked[:, -a.rows // 2 - 1])))
    opt_thrs = [0.5]
    moved = {}

    def device_route():
        d.serve_resident(images)
        got = d.pseudo_rows(sel, tau, min_score=min_score)
        moved["pseudo_rows"] = 24 * a.batch + 8 + PL.RECORD_DTYPE.itemsize * len(got[0])      # uda_pseudo_rows_shape + uda_get_pseudo_rows
        acc = PL.PseudoLabelSet(sel, tau, opt_thrs)
        acc.add(names, got)
        return acc.finalize(), int(got[3].sum())

    def host_route():
        un = d.serve_unpacked(images)
        moved["unpacked"] = sum(v.nbytes for v in un.values() if isinstance(v, np.ndarray))
        per_image, lo, hi = host_select(un, sel, min_score, tau, PL.MAX_ROWS)
        acc = PL.PseudoLabelSet(sel, tau, opt_thrs)
        rec = np.zeros((sum(len(r) for r, _ in per_image),), PL.RECORD_DTYPE)
        k = 0
        for i, (rows, v) in enumerate(per_image):
            s = slice(k, k + len(rows))
            rec["image"][s], rec["row"][s], rec["v"][s] = i, rows, v
            rec["box"][s], rec["cls"][s] = un["boxes"][i, rows, :4], un["classes"][i, rows]
            k += len(rows)
        cand = np.asarray([len(r) for r, _ in per_image], np.int32)
        acc.add(names, (rec, np.asarray([[lo, hi]] + [[np.inf, -np.inf]] * (a.batch - 1)), cand, cand))
        return acc.finalize(), int(cand.sum())

    def serve_only():
        d.serve_resident(images)
        d.synchronize()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        t = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return dict(p50_ms_per_batch=round(float(np.median(t)), 4), mean_ms_per_batch=round(float(np.mean(t)), 4))

    (sel1, k1), (sel2, k2) = device_route(), host_route()
    same = k1 == k2 and [str(x) for x in sel1[0]] == [str(x) for x in sel2[0]] and all(np.array_equal(x, y) for x, y in zip(sel1[1], sel2[1]))
    res = dict(config="D0 1280x768, MC T=10 rate 0.05, loss attenuation, softmax; one batch of %d" % a.batch, strategy=a.strategy,
               min_score=min_score, tau=tau, candidates_per_image=round(k1 / a.batch, 2), selections_equal=bool(same))
    res["pseudo_rows"] = timed(device_route)
    res["unpacked"] = timed(host_route)
    res["serve_only"] = timed(serve_only)
    res["bytes_to_host"] = dict(moved)
    d.profile_enable([capi.PROF_PSEUDO])
    device_route()
    ms, launches = d.profile_read(capi.PROF_PSEUDO)
    d.profile_enable([])
    res["pseudo_kernels_device_us_per_batch"] = round(ms * 1e3 / max(launches, 1), 2)
    res["speedup_vs_unpacked"] = round(res["unpacked"]["p50_ms_per_batch"] / res["pseudo_rows"]["p50_ms_per_batch"], 3)
    d.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
