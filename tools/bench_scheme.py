#!/usr/bin/env python3
"""Step time of the split schemes side by side: BASELINE configs[1] (D0, 32 x 1280x768, T = 10, full MC dropout) and the
head-only MC regime (mc_classheadrate = mc_boxheadrate = 0.05), served through ServingDriver.serve_stream for each scheme,
one child process per scheme (the scheme is fixed when a handle is created).  Prints ONE JSON line:

    {"f16x2": {"full": {...}, "head_only": {...}}, "f16": {...}, "bf16": {...}, "speedup": {"f16": {...}, "bf16": {...}}}

per regime: ms per step (a step = 32 images x T samples, network + post-process + detections on the host, pipelined),
images x samples per second, and the device time per kernel kind of one profiled step (profile_read).

    python tools/bench_scheme.py [--schemes f16x2,f16,bf16] [--steps 10] [--warmup 3]

The first scheme is the baseline of "speedup" (with two schemes: one ratio per regime, as before).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {1: "stem", 2: "pw", 3: "dw", 4: "se", 5: "fuse", 6: "pool", 7: "mbx", 8: "sep", 16: "aggregate", 17: "nms", 18: "preprocess"}
BATCH, T, SIZE = 32, 10, "1280x768"


def child(scheme, regime, steps, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    from uda_amd import hparams_config, weights as weights_mod
    from uda_amd.infer_lib import KerasDriver
    cfg = hparams_config.get_efficientdet_config("efficientdet-d0")
    over = dict(image_size=SIZE, num_classes=7, loss_attenuation=True, enable_softmax=True, mc_dropout=True, mc_dropoutsamp=T)
    over.update(dict(mc_dropoutrate=0.05) if regime == "full" else dict(mc_classheadrate=0.05, mc_boxheadrate=0.05))
    cfg.override(over)
    p = cfg.as_dict()
    p["is_training_bn"] = False
    p["uda_pw_scheme"] = scheme
    W_, H_ = [int(v) for v in SIZE.split("x")]
    images = np.random.default_rng(2).integers(0, 256, (BATCH, H_, W_, 3), dtype=np.uint8)
    w = weights_mod.init_weights(p, seed=0, cls_spread=1.0)
    d = KerasDriver("_", False, "efficientdet-d0", BATCH, False, p, weights=w, chunk_images=16)
    assert d.pw_scheme == scheme, (d.pw_scheme, scheme)
    d.set_dropout_seed(5)
    for _ in range(max(1, warmup)):
        d.serve(images)
    d.profile_enable(list(KINDS))
    d.serve(images)
    kinds = {KINDS[k]: round(d.profile_read(k)[0], 3) for k in KINDS}
    d.profile_enable([])
    d.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _ in d.serve_stream([images] * steps):
        n += 1
    d.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / n
    res = dict(ms_per_step=round(ms, 2), images_samples_per_s=round(BATCH * T * 1e3 / ms, 1), kernel_ms_by_kind=kinds,
               range_demotions=int(d.range_demotions()))
    d.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--schemes", default="f16x2,f16,bf16")
    ap.add_argument("--regimes", default="full,head_only")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", nargs=2, metavar=("SCHEME", "REGIME"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.steps, a.warmup)
    out = {}
    for scheme in a.schemes.split(","):
        out[scheme] = {}
        for regime in a.regimes.split(","):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", scheme, regime, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], cwd=ROOT, capture_output=True, text=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stderr[-3000:])
                sys.exit("bench_scheme: %s / %s failed (exit %d)" % (scheme, regime, r.returncode))
            out[scheme][regime] = json.loads(line[0][len("RESULT "):])
            sys.stderr.write("%s %s: %s ms/step\n" % (scheme, regime, out[scheme][regime]["ms_per_step"]))
    names = a.schemes.split(",")
    ratio = lambda new: {rg: round(out[names[0]][rg]["ms_per_step"] / out[new][rg]["ms_per_step"], 3) for rg in a.regimes.split(",")}
    if len(names) == 2:
        out["speedup"] = ratio(names[1])
    elif len(names) > 2:
        out["speedup"] = {new: ratio(new) for new in names[1:]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
