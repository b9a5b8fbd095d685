#!/usr/bin/env python3
"""Cost of the pool's perceptual hashes (`dataset_pruning.phash_device` -> `uda_phash_np`; reference
active_learning_loop.py:215-224) on seeded synthetic frames: --images frames (default 2000), alternately 375 x 1242 (KITTI) and
720 x 1280 (BDD100K), each a coarse random colour field enlarged bilinearly plus +-20 noise, so that every image's low
frequencies lie well away from their median and none ties.

    host        the reference-shaped loop on this machine's CPU, once: `phash(Image.fromarray(frame).resize((512, 256)))` per
                frame - Pillow's bicubic resize, grey, Lanczos thumbnail, scipy's DCT.  No decode in it
    device      `phash_device(frames)`: packing the frames of a call into one array (a host copy), the C entry point - tables on
                the host, one upload of the pixels, the resample passes and the tail kernel, four downloads - and the host-side
                settling of ties (none here); as many calls as the byte cap asks for
    entry       the C entry point alone on pixels packed beforehand, the same calls
    upload /    copies of the same byte counts between pageable host memory and the device, timed apart with torch.  The kernels
    download    alone: run this script with --device-only under a kernel trace
    decode      PNG and JPEG decoding of --decode-sample frames of each size with Pillow, per image: the decode stays the
                caller's with or without a device and is not part of any figure above

The script asserts that EVERY device hash equals the host loop's before it prints a time.  Wall-clock p50 / mean over --steps
runs after --warmup.  Prints ONE JSON line.

    python tools/bench_phash.py [--images 2000] [--steps 3] [--warmup 1] [--device-only]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((1242, 375), (1280, 720))          # (w, h)


def synthetic(n, seed=29):
    from PIL import Image
    rng = np.random.default_rng([seed, n])
    noise = {s: [rng.integers(-20, 21, (s[1], s[0], 3)).astype(np.int16) for _ in range(4)] for s in SIZES}
    frames = []
    for k in range(n):
        w, h = SIZES[k % 2]
        coarse = rng.integers(0, 256, (5, 8, 3), dtype=np.uint8)
        field = np.asarray(Image.fromarray(coarse).resize((w, h), Image.BILINEAR)).astype(np.int16)
        frames.append(np.clip(field + noise[(w, h)][(k // 2) % 4], 0, 255).astype(np.uint8))
    return frames


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
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--decode-sample", type=int, default=16)
    ap.add_argument("--device-only", action="store_true", help="the device calls only, after a check of every 16th hash (for a kernel trace)")
    a = ap.parse_args()
    import torch                                # before the library: one HIP runtime in the process, torch's
    from PIL import Image
    from uda_amd import capi
    from uda_amd import dataset_pruning as DP
    frames = synthetic(a.images)
    n = len(frames)
    res = dict(images=n, sizes=["%dx%d" % (h, w) for w, h in SIZES], bytes_up=int(sum(f.nbytes for f in frames)))

    def host_word(f):
        return DP._bits_to_words(DP.phash(Image.fromarray(f).resize((512, 256))).reshape(1, -1))[0, 0]

    info = {}
    got = DP.phash_device(frames, info=info)[:, 0]
    res["ties"] = len(info["ties"])
    res["min_margin"] = round(float(info["margin"].min()), 4)
    if a.device_only:
        for k in range(0, n, 16):
            assert got[k] == host_word(frames[k]), "hash %d differs from the host loop's" % k
        res["device"] = timed(lambda: DP.phash_device(frames), a.steps, a.warmup)
        res["device_per_image_ms"] = round(res["device"]["p50_ms"] / n, 4)
        print(json.dumps(res), flush=True)
        return
    t0 = time.perf_counter()
    want = np.array([host_word(f) for f in frames], np.uint64)
    res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["host_per_image_ms"] = round(res["host_ms"] / n, 4)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "hashes %s differ from the host loop's" % bad[:10].tolist()
    res["all_hashes_equal_host"] = True
    res["distinct_hashes"] = int(np.unique(want).size)

    # the calls phash_device makes, packed beforehand
    lib = capi.load()
    calls, k0 = [], 0
    while k0 < n:
        k1, need = k0, 0
        while k1 < n and (k1 == k0 or need + DP._phash_call_bytes(frames[k1].shape[1], frames[k1].shape[0]) <= capi.PHASH_MAX_BYTES):
            need += DP._phash_call_bytes(frames[k1].shape[1], frames[k1].shape[0])
            k1 += 1
        wh = np.array([(f.shape[1], f.shape[0]) for f in frames[k0:k1]], np.int32)
        calls.append((k1 - k0, wh, np.concatenate([f.reshape(-1) for f in frames[k0:k1]])))
        k0 = k1
    res["calls"] = len(calls)
    words, margin, thumb = np.zeros(n, np.uint64), np.zeros(n), np.zeros((n, 32, 32), np.uint8)

    def entry():
        at = 0
        for m, wh, pix in calls:
            rc = lib.uda_phash_np(0, m, wh.ctypes.data, pix.ctypes.data, words[at:].ctypes.data, margin[at:].ctypes.data,
                                  thumb[at:].ctypes.data, None)
            capi.check(lib, None, rc, "uda_phash_np")
            at += m

    res["entry"] = timed(entry, a.steps, a.warmup)
    assert np.array_equal(words, want)
    res["device"] = timed(lambda: DP.phash_device(frames), a.steps, a.warmup)
    res["device_per_image_ms"] = round(res["device"]["p50_ms"] / n, 4)
    res["entry_per_image_ms"] = round(res["entry"]["p50_ms"] / n, 4)

    down = n * (8 + 8 + 1024)

    def copies_up():
        for _, _, pix in calls:
            d = torch.empty(pix.size, dtype=torch.uint8, device="cuda")
            d.copy_(torch.from_numpy(pix))
            torch.cuda.synchronize()

    h_down, d_down = torch.empty(down, dtype=torch.uint8), torch.empty(down, dtype=torch.uint8, device="cuda")

    def copy_down():
        h_down.copy_(d_down)
        torch.cuda.synchronize()

    res.update(bytes_down=down, upload=timed(copies_up, a.steps, a.warmup), download=timed(copy_down, a.steps, a.warmup))
    res["upload_per_image_ms"] = round(res["upload"]["p50_ms"] / n, 4)
    res["rest_per_image_ms"] = round((res["entry"]["p50_ms"] - res["upload"]["p50_ms"] - res["download"]["p50_ms"]) / n, 4)
    for fmt, key in (("PNG", "png_decode_per_image_ms"), ("JPEG", "jpeg_decode_per_image_ms")):
        per = {}
        for s, (w, h) in enumerate(SIZES):
            blobs = []
            for f in frames[s::2][:a.decode_sample]:
                b = io.BytesIO()
                Image.fromarray(f).save(b, format=fmt)
                blobs.append(b.getvalue())
            t0 = time.perf_counter()
            for b in blobs:
                np.asarray(Image.open(io.BytesIO(b)))
            per["%dx%d" % (h, w)] = round((time.perf_counter() - t0) * 1e3 / max(len(blobs), 1), 2)
        res[key] = per
    res["host_over_device"] = round(res["host_ms"] / res["device"]["p50_ms"], 2)
    res["host_over_entry"] = round(res["host_ms"] / res["entry"]["p50_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
