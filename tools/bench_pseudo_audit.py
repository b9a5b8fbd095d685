#!/usr/bin/env python3
"""Cost of the pseudo-label audit (`pseudo_audit.audit_np` -> `uda_pseudo_audit_np`; reference ssl_utils/parent.py:1648-1813) on two
seeded synthetic pools: `small`, about 7 000 images with 3-20 ground-truth rows and pseudo labels each, and `large`, about 70 000
images with 5-60 each.  The labels are jittered copies of rows, duplicates and random boxes on a 1/8 grid.

    device      the C entry point alone on prepared arrays: upload of boxes and offsets, one launch, one copy per output
                array out of the packed results; the host clock around the call, which ends in a device-to-host copy (a synchronise)
    upload /    copies of the same byte counts between pageable host memory and the device, timed apart with torch (the entry
    download    point uses plain hipMemcpy on pageable memory too); `rest` = device - upload - download is the allocations, the
                launch and the kernel together (a difference of medians, not a measurement of its own)
    audit_np    the Python call around it: flattening the per-image lists, the finite check, the output arrays
    end_to_end  audit_pseudo_labels: audit_np plus the per-image members of PseudoAudit (Python lists, as the reference keeps)
    mirror      tests/audit_ref.py, which is the reference's loop statement for statement (a stored matrix per image, np.argmax,
                the mutating while loop) on this machine's CPU, on the first --mirror-images images; `mirror_scaled_ms` scales its
                time to the pool by the image count

The script asserts that the device's arrays equal the mirror's on those images before it prints a time.  Wall-clock p50 / mean
over --steps runs after --warmup, each part in its own loop.  Prints ONE JSON line per pool.

    python tools/bench_pseudo_audit.py [--pools small,large] [--steps 5] [--warmup 1] [--mirror-images 2000] [--device-only]
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
POOLS = {"small": (7000, 3, 20), "large": (70000, 5, 60)}


def synthetic(images, lo, hi, seed=11):
    rng = np.random.default_rng([seed, images, lo, hi])
    gts, dets = [], []
    for _ in range(images):
        G, D = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        y, x = rng.integers(0, 3000, G) / 8.0, rng.integers(0, 9000, G) / 8.0
        gt = np.stack([y, x, y + rng.integers(80, 960, G) / 8.0, x + rng.integers(80, 960, G) / 8.0], 1)
        pick = rng.integers(0, G, D)
        det = gt[pick] + rng.integers(-40, 41, (D, 4)) / 8.0 * (rng.random((D, 1)) < 0.9)
        loose = rng.random(D) < 0.25
        yy, xx = rng.integers(0, 3000, D) / 8.0, rng.integers(0, 9000, D) / 8.0
        det[loose] = np.stack([yy, xx, yy + rng.integers(80, 960, D) / 8.0, xx + rng.integers(80, 960, D) / 8.0], 1)[loose]
        gts.append(gt)
        dets.append(det)
    return gts, dets


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
    ap.add_argument("--pools", default="small,large")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mirror-images", type=int, default=2000)
    ap.add_argument("--device-only", action="store_true", help="time the device call and the copies only (for a kernel trace)")
    a = ap.parse_args()
    import torch
    import audit_ref as R
    from uda_amd import capi
    from uda_amd import pseudo_audit as pa
    lib = capi.load()
    for pool in a.pools.split(","):
        images, lo, hi = POOLS[pool]
        gts, dets = synthetic(images, lo, hi)
        gt, gt_off = pa._flat(gts, "ground-truth")
        det, det_off = pa._flat(dets, "pseudo-label")
        keys = pa._ROW_KEYS + pa._DET_KEYS
        out = {k: np.zeros(len(gt) if (k, dt) in pa._ROW_KEYS else len(det), dt) for k, dt in keys}
        n_matches = np.zeros(images, np.int32)

        def device_call():
            rc = lib.uda_pseudo_audit_np(0, images, gt.ctypes.data, gt_off.ctypes.data, det.ctypes.data, det_off.ctypes.data, 0.5,
                                         *[out[k].ctypes.data for k, _ in keys], n_matches.ctypes.data)
            capi.check(lib, None, rc, "uda_pseudo_audit_np")

        m = min(a.mirror_images, images)
        t0 = time.perf_counter()
        want = R.audit(gts[:m], dets[:m], 0.5)
        mirror_ms = (time.perf_counter() - t0) * 1e3
        got = pa.audit_np(gts, dets, 0.5)
        for k, dt in keys:
            hi_ = int((gt_off if (k, dt) in pa._ROW_KEYS else det_off)[m])
            a_, b_ = got[k][:hi_], want[k]
            same = np.array_equal(a_.view(np.uint64), b_.astype(np.float64).view(np.uint64)) if dt == np.float64 else np.array_equal(a_, b_)
            assert same, "%s of the device differs from the mirror's" % k
        assert np.array_equal(got["n_matches"][:m], want["n_matches"])

        up = int(gt.nbytes + det.nbytes + gt_off.nbytes + det_off.nbytes)
        down = int(sum(v.nbytes for v in out.values()) + n_matches.nbytes)
        h_up, h_down = torch.empty(up, dtype=torch.uint8), torch.empty(down, dtype=torch.uint8)
        d_up, d_down = torch.empty(up, dtype=torch.uint8, device="cuda"), torch.empty(down, dtype=torch.uint8, device="cuda")

        def copy_up():
            d_up.copy_(h_up)
            torch.cuda.synchronize()

        def copy_down():
            h_down.copy_(d_down)
            torch.cuda.synchronize()

        classes = [(g, np.full(len(g), "a")) for g in gts], [(d, np.full(len(d), "a")) for d in dets]
        res = dict(pool=pool, images=images, rows=int(gt_off[-1]), labels=int(det_off[-1]), matches=int(got["n_matches"].sum()),
                   ious_matrix=int((np.diff(gt_off) * np.diff(det_off)).sum()), bytes_up=up, bytes_down=down,
                   device=timed(device_call, a.steps, a.warmup), upload=timed(copy_up, a.steps, a.warmup),
                   download=timed(copy_down, a.steps, a.warmup), mirror_images=m, mirror_ms=round(mirror_ms, 1),
                   mirror_scaled_ms=round(mirror_ms * images / m, 1))
        res["rest_ms"] = round(res["device"]["p50_ms"] - res["upload"]["p50_ms"] - res["download"]["p50_ms"], 3)
        res["mirror_over_device"] = round(res["mirror_scaled_ms"] / res["device"]["p50_ms"], 1)
        if not a.device_only:
            res["audit_np"] = timed(lambda: pa.audit_np(gts, dets, 0.5), a.steps, a.warmup)
            res["end_to_end"] = timed(lambda: pa.audit_pseudo_labels(classes[0], classes[1], ["a"], 0.5), max(1, a.steps // 2), a.warmup)
            res["mirror_over_end_to_end"] = round(res["mirror_scaled_ms"] / res["end_to_end"]["p50_ms"], 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
