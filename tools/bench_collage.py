#!/usr/bin/env python3
"""Cost of the rare-class collage (`collage.crop_collage` -> `uda_resample_np`; reference ssl_utils/parent.py:317-686) on a seeded
synthetic labelled set: --images images of 720 x 1280 (default 700), about --crops boxes of the target class (default 3000) of 20
to 300 pixels a side among other boxes, default margins (0.5 .. 1.0), BDD100K-sized collages of 720 rows.

    plan        `plan_collage`: the reference's decisions from the image sizes (host, Python)
    cut         the crop pixels copied out of the images (host, numpy)
    device      `collage.resample_np` on the prepared crops: packing the crops into one array, the C entry point - coefficient
                tables on the host, upload of crops, tables and passes, zeroing, two launches a level, the download of the
                collages - and the host clock around it (the call ends in a device-to-host copy)
    upload /    copies of the same byte counts between pageable host memory and the device, timed apart with torch; `rest` =
    download    device - upload - download is the packing, the tables, the allocations, the memsets and the kernels together (a
                difference of medians, not a measurement of its own).  The kernels alone: run this script with --device-only
                under a kernel trace
    end_to_end  `crop_collage` on arrays: plan + cut + device, no encoding
    encode      PNG (KITTI writer) and JPEG (BDD100K writer) encoding of --encode-sample collages with Pillow, and the same scaled
                to all collages: it is not part of the service and it is not hidden
    host        the reference-shaped loop on this machine's CPU, once: per collage every `Image.resize(size, Image.LANCZOS)` and
                `paste` of the job list with Pillow (a resized crop that is read again is pasted into an Image.new first, which the
                reference does not need: one copy more a crop)

--augment turns `manual_augmentations` on (parent.py:261-315): every resized crop gets one of the reference's five random
augmentations before it is pasted, the call is `collage.collage_np` -> `uda_collage_np` (the noise planes are part of its
upload), and the host loop applies Image.transpose / ImageEnhance / ImageFilter.GaussianBlur / the numpy noise add as the
reference does.  `plan` then includes the reference's own draws (a noise plane a noisy crop).

The script asserts that EVERY collage of the device equals Pillow's before it prints a time.  Wall-clock p50 / mean over --steps
runs after --warmup.  Prints ONE JSON line.

    python tools/bench_collage.py [--images 700] [--crops 3000] [--scale] [--augment] [--steps 3] [--warmup 1] [--device-only]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W = 720, 1280


def synthetic(n_images, n_crops, seed=23):
    """A few distinct images (smooth ramps, noise, hard edges) handed out in turn, and per image its share of the target boxes
    plus as many other boxes.  Boxes are [y1, x1, y2, x2], as the BDD100K readers give them."""
    rng = np.random.default_rng([seed, n_images, n_crops])
    base = []
    for k in range(8):
        y, x = np.mgrid[0:H, 0:W]
        im = np.stack([(x * (k + 1)) % 256, (y * (k + 2)) % 256, ((x + y) // 2) % 256], -1) + rng.integers(-20, 21, (H, W, 3))
        im = np.clip(im, 0, 255).astype(np.uint8)
        im[100 * k % H:100 * k % H + 60, ::7] = 255
        base.append(im)
    images = [base[i % len(base)] for i in range(n_images)]
    share = np.bincount(rng.integers(0, n_images, n_crops), minlength=n_images)
    classes, boxes = [], []
    for i in range(n_images):
        c, b = [], []
        for j in range(2 * share[i]):
            h, w = rng.integers(20, 301, 2)
            y, x = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
            b.append([float(y), float(x), float(y + h), float(x + w)])
            c.append("rider" if j < share[i] else "car")
        classes.append(np.asarray(c))
        boxes.append(np.asarray(b, np.float64).reshape(-1, 4))
    return images, classes, boxes


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(p50_ms=round(float(np.median(t)), 3), mean_ms=round(float(np.mean(t)), 3))


def jobs_by_collage(plan):
    """The jobs of every collage, in level order: a temporary belongs to the collage its pixels end in.  A job is its 7 values and,
    from a plan with augmentations, op, arg and where its noise starts in plan.noise."""
    S, T = len(plan.crops), len(plan.tmp_wh)
    owner = {}
    for j in plan.jobs[::-1].tolist():
        owner[j[1]] = owner[j[2]] if j[2] < S + T else j[2] - S - T
    per = [[] for _ in range(plan.n)]
    at = 0
    for j in plan.jobs.tolist():
        if len(j) == 9:
            j.append(at)
            at += 3 * j[5] * j[6] if j[7] == 5 else 0
        per[owner[j[1]]].append(j)
    return per


def pillow_augment(image, op, value, noise):
    """parent.py:264-304 on a PIL image."""
    from PIL import Image, ImageEnhance, ImageFilter
    if op == 1:
        return image.transpose(Image.FLIP_LEFT_RIGHT)
    if op == 2:
        return ImageEnhance.Brightness(image).enhance(value)
    if op == 3:
        return ImageEnhance.Contrast(image).enhance(value)
    if op == 4:
        return image.filter(ImageFilter.GaussianBlur(radius=value))
    np_image = np.array(image)
    np_image = np_image + noise.reshape(np_image.shape)
    np_image = np.clip(np_image, 0, 255)
    return Image.fromarray(np_image.astype("uint8"))


def pillow_collage(jobs, crops, plan):
    """One collage the way the reference makes it: resize with Image.LANCZOS, paste."""
    from PIL import Image
    S, T = len(plan.crops), len(plan.tmp_wh)
    planes = {}
    for _, s, d, x, y, w, h, *aug in jobs:
        src = planes[s] if s in planes else Image.fromarray(crops[s])
        if d not in planes:
            planes[d] = Image.new("RGB", plan.tmp_wh[d - S] if d < S + T else (plan.width, plan.height))
        if aug and aug[0]:
            op, arg, at = aug
            new = pillow_augment(src, op, plan.params[arg] if op in (2, 3, 4) else None, plan.noise[at:at + 3 * w * h] if op == 5 else None)
        else:
            new = src.resize((w, h), Image.LANCZOS)
        planes[d].paste(new, (x, y))
        out = planes[d]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=700)
    ap.add_argument("--crops", type=int, default=3000)
    ap.add_argument("--scale", action="store_true", help="the four-scale variant (scale=True)")
    ap.add_argument("--augment", action="store_true", help="manual_augmentations=True: one of five augmentations a crop")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--encode-sample", type=int, default=16)
    ap.add_argument("--device-only", action="store_true", help="the device call only, after one check (for a kernel trace)")
    a = ap.parse_args()
    import torch
    from PIL import Image
    from uda_amd import collage
    images, classes, boxes = synthetic(a.images, a.crops)
    target = ["rider"]
    kw = dict(dataset="BDD100K", scale=a.scale, manual_augmentations=a.augment)
    t0 = time.perf_counter()
    plan = collage.plan_collage(images, classes, boxes, target, **kw)
    plan_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    crops = [images[i][y0:y1, x0:x1] for i, x0, y0, x1, y1 in plan.crops]
    packed = [np.ascontiguousarray(c) for c in crops]
    cut_ms = (time.perf_counter() - t0) * 1e3
    sides = np.asarray([(c.shape[1], c.shape[0]) for c in crops])
    res = dict(images=a.images, target_boxes=a.crops, crops=len(crops), crop_w_mean=round(float(sides[:, 0].mean()), 1),
               crop_h_mean=round(float(sides[:, 1].mean()), 1), collages=plan.n, temporaries=len(plan.tmp_wh), jobs=len(plan.jobs),
               levels=int(plan.jobs[:, 0].max()) + 1, scale=bool(a.scale), augment=bool(a.augment), plan_ms=round(plan_ms, 1),
               cut_ms=round(cut_ms, 1))
    if a.augment:
        res["kinds"] = {k: sum(1 for kind, _ in plan.augment if kind == k) for k in collage.AUGMENT_KINDS}
        res["noise_bytes"] = int(plan.noise.nbytes)

    def device_call():
        if a.augment:
            return collage.collage_np(packed, plan.tmp_wh, plan.n, plan.height, plan.width, plan.jobs, plan.params, plan.noise)
        return collage.resample_np(packed, plan.tmp_wh, plan.n, plan.height, plan.width, plan.jobs)

    out = device_call()
    if a.device_only:
        per = jobs_by_collage(plan)
        for n in range(0, plan.n, max(1, plan.n // 8)):
            assert np.array_equal(np.asarray(pillow_collage(per[n], crops, plan)), out[n]), "collage %d differs from Pillow's" % n
        res["device"] = timed(device_call, a.steps, a.warmup)
        print(json.dumps(res), flush=True)
        return
    per = jobs_by_collage(plan)
    host_s = 0.0
    for n in range(plan.n):
        t0 = time.perf_counter()
        ref = pillow_collage(per[n], crops, plan)
        host_s += time.perf_counter() - t0
        assert np.array_equal(np.asarray(ref), out[n]), "collage %d differs from Pillow's" % n
    res["all_collages_equal_pillow"] = True
    res["host_ms"] = round(host_s * 1e3, 1)

    up = int(sum(c.nbytes for c in packed)) + int(plan.noise.nbytes)
    down = int(out.nbytes)
    h_up, h_down = torch.empty(up, dtype=torch.uint8), torch.empty(down, dtype=torch.uint8)
    d_up, d_down = torch.empty(up, dtype=torch.uint8, device="cuda"), torch.empty(down, dtype=torch.uint8, device="cuda")

    def copy_up():
        d_up.copy_(h_up)
        torch.cuda.synchronize()

    def copy_down():
        h_down.copy_(d_down)
        torch.cuda.synchronize()

    res.update(bytes_up=up, bytes_down=down, upload=timed(copy_up, a.steps, a.warmup), download=timed(copy_down, a.steps, a.warmup))
    del h_up, h_down, d_up, d_down
    torch.cuda.empty_cache()
    res["device"] = timed(device_call, a.steps, a.warmup)
    res["rest_ms"] = round(res["device"]["p50_ms"] - res["upload"]["p50_ms"] - res["download"]["p50_ms"], 3)
    res["end_to_end"] = timed(lambda: collage.crop_collage(images, classes, boxes, target, **kw), a.steps, a.warmup)
    k = min(a.encode_sample, plan.n)
    for fmt, ext in (("PNG", "png_encode"), ("JPEG", "jpeg_encode")):
        t0 = time.perf_counter()
        for n in range(k):
            Image.fromarray(out[n]).save(io.BytesIO(), format=fmt)
        ms = (time.perf_counter() - t0) * 1e3
        res[ext] = dict(sample=k, per_collage_ms=round(ms / k, 2), all_collages_ms=round(ms / k * plan.n, 1))
    res["host_over_device"] = round(res["host_ms"] / res["device"]["p50_ms"], 2)
    res["host_over_end_to_end"] = round(res["host_ms"] / res["end_to_end"]["p50_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
