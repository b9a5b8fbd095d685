"""numpy mirror of the collage service: Pillow's 8-bit Lanczos resize (libImaging/Resample.c) restated from its description -
precompute_coeffs in double with math.sin (the C library's), 22-bit fixed-point coefficients, the horizontal pass rounded to
uint8 and then the vertical pass (the other way round where `Image.resize` itself does so: a plane more than 100 times as tall as
wide that gets shorter) - and the execution of a job list of `uda_resample_np` with it (`run_jobs` has the signature
of `collage.resample_np`, so `crop_collage(resample=run_jobs)` runs without a GPU).  `pack` is the reference's packing loop
(parent.py:505-597) on crop sizes alone, written as the loop the reference runs - Image objects replaced by their sizes - for
the planner's tests.  Slow and plain on purpose; nothing here is imported by the package."""
import functools
import math

import numpy as np

BITS = 22


def _lanczos(x):
    def sinc(v):
        if v == 0.0:
            return 1.0
        v = v * math.pi
        return math.sin(v) / v
    return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


@functools.lru_cache(maxsize=None)
def coeffs(in_size, out_size):
    """-> (ksize, bounds [out, 2] int32 (xmin, xmax), kk [out, ksize] int32)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[xx, x] = int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


def _pass(img, out_size, axis):
    """One pass along `axis` (1: horizontal, 0: vertical) of a uint8 array [h, w, 3]."""
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    _, bounds, kk = coeffs(img.shape[0], out_size)
    out = np.zeros((out_size,) + img.shape[1:], np.uint8)
    for xx in range(out_size):
        xmin, xmax = bounds[xx]
        acc = (1 << (BITS - 1)) + np.tensordot(kk[xx, :xmax].astype(np.int64), img[xmin:xmin + xmax], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31            # Pillow's int32 accumulator does not wrap
        out[xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, w, h):
    """Image.fromarray(img).resize((w, h), Image.LANCZOS) as an array."""
    img = np.ascontiguousarray(img, np.uint8)
    if w < 1 or h < 1:
        raise ValueError("height and width must be > 0")
    if img.shape[0] > img.shape[1] * 100 and h < img.shape[0]:      # Image.resize's own rule (PIL/Image.py): y first, then x
        img = _pass(img, h, 0)
    if img.shape[1] != w:
        img = _pass(img, w, 1)
    if img.shape[0] != h:
        img = _pass(img, h, 0)
    return img.copy()


def pillow_resize(img, w, h):
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(img, np.uint8)).resize((w, h), Image.LANCZOS))


def run_jobs(src_planes, tmp_wh, n, height, width, jobs, resize_fn=resize):
    """The job list of uda_resample_np (include/uda_hip.h), job after job in list order."""
    planes = [np.ascontiguousarray(p, np.uint8) for p in src_planes]
    planes += [np.zeros((h, w, 3), np.uint8) for w, h in tmp_wh]
    out = np.zeros((n, height, width, 3), np.uint8)
    planes += [out[i] for i in range(n)]
    for _, s, d, x, y, w, h in np.asarray(jobs).reshape(-1, 7).tolist():
        assert d >= len(src_planes)
        r = resize_fn(planes[s], w, h)
        dst = planes[d]
        ch, cw = min(h, dst.shape[0] - y), min(w, dst.shape[1] - x)
        dst[y:y + ch, x:x + cw] = r[:ch, :cw]
    return out


def run_jobs_pillow(src_planes, tmp_wh, n, height, width, jobs):
    return run_jobs(src_planes, tmp_wh, n, height, width, jobs, resize_fn=pillow_resize)


def pack(crop_sizes, crop_boxes, crop_classes, collage_width, collage_height, scale):
    """parent.py:505-597 on sizes: -> per collage (placements [(crop index, x_offset, [resize sizes in order], quadrants or None)],
    labels).  quadrants: [(x in part, y in part, w, h)]."""
    queue = list(range(len(crop_sizes)))
    collages = []
    while queue:
        x_offset, labels, box_count, placed = 0, [], 0, []
        while x_offset < collage_width and queue and box_count < 100:
            k = queue.pop(0)
            ow, oh = crop_sizes[k]
            new_width = collage_width - x_offset if len(queue) == 0 else int(ow * collage_height / oh)
            sizes = [(new_width, collage_height)]
            iw, ih = new_width, collage_height
            if x_offset + iw > collage_width:
                iw = collage_width - x_offset
                sizes.append((iw, ih))
            quads = None
            if scale:
                qs = np.asarray([(np.ceil(iw * 0.75), np.ceil(ih * 0.75)), (np.ceil(iw * 0.25), np.ceil(ih * 0.75)),
                                 (np.ceil(iw * 0.75), np.ceil(ih * 0.25)), (np.ceil(iw * 0.25), np.ceil(ih * 0.25))]).astype(int)
                xp, yp, quads, positions = 0, 0, [], []
                for j in range(4):
                    if j == 2:
                        yp, xp = qs[0][1], 0
                    quads.append((int(xp), int(yp), int(qs[j][0]), int(qs[j][1])))
                    positions.append((x_offset + xp, yp))
                    xp += qs[j][0]
                    if j == 1:
                        xp = 0
                for idx, pos in enumerate(positions):
                    sx, sy = qs[idx][0] / ow, qs[idx][1] / oh
                    for cls, b in zip(crop_classes[k], crop_boxes[k]):
                        labels.append([cls, [pos[0] + sx * b[0], pos[1] + sy * b[1], pos[0] + sx * b[2], pos[1] + sy * b[3]]])
                        box_count += 1
                        if box_count >= 100:
                            break
            else:
                sx, sy = iw / ow, ih / oh
                for cls, b in zip(crop_classes[k], crop_boxes[k]):
                    labels.append([cls, [x_offset + sx * b[0], sy * b[1], x_offset + sx * b[2], sy * b[3]]])
                    box_count += 1
                    if box_count >= 100:
                        break
            placed.append((k, x_offset, sizes, quads))
            x_offset += iw
        collages.append((placed, labels))
    return collages


def render(crops, collages, collage_width, collage_height, resize_fn=resize):
    """The pixels of `pack`'s collages from the crop arrays, the way the reference builds them (resize, part, paste)."""
    out = np.zeros((len(collages), collage_height, collage_width, 3), np.uint8)

    def paste(dst, src, x, y):
        h, w = min(src.shape[0], dst.shape[0] - y), min(src.shape[1], dst.shape[1] - x)
        if h > 0 and w > 0:
            dst[y:y + h, x:x + w] = src[:h, :w]
    for n, (placed, _) in enumerate(collages):
        for k, x_offset, sizes, quads in placed:
            img = crops[k]
            for w, h in sizes:
                img = resize_fn(img, w, h)
            if quads is not None:
                part = np.zeros_like(img)
                for x, y, w, h in quads:
                    paste(part, resize_fn(img, w, h), x, y)
                img = part
            paste(out[n], img, x_offset, 0)
    return out
