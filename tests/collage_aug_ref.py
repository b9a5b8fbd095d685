"""numpy mirror of RCC's manual augmentations (reference ssl_utils/parent.py:261-315) as `uda_collage_np` runs them: Pillow's
FLIP_LEFT_RIGHT, ImageEnhance.Brightness / Contrast (ImagingBlend on a degenerate image), ImageFilter.GaussianBlur (three box
blurs an axis, libImaging/BoxBlur.c) and the reference's wrapping noise add, restated from their description in integer and
float32 arithmetic - np.float32 scalars, every operation rounded on its own - and the execution of a [K, 9] job list with them
(`run_jobs` has the signature of `collage.collage_np`, so `crop_collage(manual_augmentations=True, resample=run_jobs)` runs
without a GPU).  The `pillow_*` twins do the same with live Pillow.  Slow and plain on purpose; nothing here is imported by the
package."""
import math

import numpy as np

import collage_ref as R

FLIP, BRIGHTNESS, CONTRAST, BLUR, NOISE = 1, 2, 3, 4, 5
KINDS = {"flip": FLIP, "brightness": BRIGHTNESS, "contrast": CONTRAST, "blur": BLUR, "noise": NOISE}
F = np.float32


def flip(img):
    return np.ascontiguousarray(img[:, ::-1])


def blend(img, deg, factor):
    """ImagingBlend(degenerate, image, factor): deg + a (px - deg) in float32, truncated; clipped only when a is outside [0, 1]."""
    a = F(factor)
    px = img.astype(np.float32)
    d = F(deg)
    t = d + a * (px - d)                                  # float32 arrays: the product and the sum each rounded to float32
    assert t.dtype == np.float32
    if F(0) <= a <= F(1):
        return t.astype(np.int32).astype(np.uint8)        # (truncation toward zero)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32)))
    return out.astype(np.uint8)


def luma_sum(img):
    img = img.astype(np.int64)
    return int(((img[..., 0] * 19595 + img[..., 1] * 38470 + img[..., 2] * 7471 + 0x8000) >> 16).sum())


def contrast_mean(img):
    return int(luma_sum(img) / (img.shape[0] * img.shape[1]) + 0.5)


def brightness(img, factor):
    return blend(img, 0, factor)


def contrast(img, factor):
    return blend(img, contrast_mean(img), factor)


def gauss_box(radius):
    """-> (fr float32, ww, fw): the box radius of ImagingGaussianBlur's three passes and the weights of one pass."""
    rad = F(radius)
    s2 = F(F(rad * rad) / F(3))
    L = F(math.sqrt(12.0 * float(s2) + 1.0))
    l = F(math.floor((float(L) - 1.0) / 2.0))
    a = F(F(F(2) * l + F(1)) * F(F(l * F(l + F(1))) - F(F(3) * s2)))
    a = F(a / F(F(6) * F(s2 - F(F(l + F(1)) * F(l + F(1))))))
    fr = F(l + a)
    r = int(fr)
    ww = int(F(F(1 << 24) / F(F(fr * F(2)) + F(1))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return fr, ww, fw


def box_pass(lines, fr, ww, fw):
    """One box blur pass along the last axis of an integer array [..., n]."""
    n, r = lines.shape[-1], int(fr)
    x = np.arange(n)
    c = lambda i: np.clip(i, 0, n - 1)                   # noqa: E731
    lines = lines.astype(np.int64)
    acc = np.zeros_like(lines)
    for d in range(-r, r + 1):
        acc += lines[..., c(x + d)]
    acc = ww * acc + fw * (lines[..., c(x - r - 1)] + lines[..., c(x + r + 1)]) + (1 << 23)
    assert acc.max() < 2 ** 32                            # Pillow's uint32 accumulator does not wrap
    return acc >> 24


def gaussian_blur(img, radius):
    fr, ww, fw = gauss_box(radius)
    img = np.ascontiguousarray(img, np.uint8)
    if fr == 0:
        return img.copy()
    for axis in (1, 0):
        lines = np.moveaxis(img, axis, -1)
        for _ in range(3):
            lines = box_pass(lines, fr, ww, fw)
        img = np.ascontiguousarray(np.moveaxis(lines, -1, axis)).astype(np.uint8)
    return img


def add_bytes(img, noise):
    return (img.astype(np.uint8) + np.asarray(noise, np.uint8).reshape(img.shape)).astype(np.uint8)      # wraps modulo 256


def augment(img, op, value=None, noise=None):
    img = np.ascontiguousarray(img, np.uint8)
    if op == FLIP:
        return flip(img)
    if op == BRIGHTNESS:
        return brightness(img, value)
    if op == CONTRAST:
        return contrast(img, value)
    if op == BLUR:
        return gaussian_blur(img, value)
    if op == NOISE:
        return add_bytes(img, noise)
    raise ValueError(op)


def pillow_augment(img, op, value=None, noise=None):
    """The reference's five augmentations (parent.py:264-304) with live Pillow."""
    from PIL import Image, ImageEnhance, ImageFilter
    image = Image.fromarray(np.ascontiguousarray(img, np.uint8))
    if op == FLIP:
        image = image.transpose(Image.FLIP_LEFT_RIGHT)
    elif op == BRIGHTNESS:
        image = ImageEnhance.Brightness(image).enhance(value)
    elif op == CONTRAST:
        image = ImageEnhance.Contrast(image).enhance(value)
    elif op == BLUR:
        image = image.filter(ImageFilter.GaussianBlur(radius=value))
    elif op == NOISE:
        np_image = np.array(image)
        np_image = np_image + np.asarray(noise, np.uint8).reshape(np_image.shape)
        np_image = np.clip(np_image, 0, 255)
        image = Image.fromarray(np_image.astype("uint8"))
    else:
        raise ValueError(op)
    return np.asarray(image)


def run_jobs(src_planes, tmp_wh, n, height, width, jobs, params=(), noise=None, resize_fn=R.resize, augment_fn=augment):
    """The job list of uda_collage_np (include/uda_hip.h), job after job in list order."""
    planes = [np.ascontiguousarray(p, np.uint8) for p in src_planes]
    planes += [np.zeros((h, w, 3), np.uint8) for w, h in tmp_wh]
    out = np.zeros((n, height, width, 3), np.uint8)
    planes += [out[i] for i in range(n)]
    noise = np.zeros(0, np.uint8) if noise is None else np.asarray(noise, np.uint8).reshape(-1)
    at = 0
    for _, s, d, x, y, w, h, op, arg in np.asarray(jobs).reshape(-1, 9).tolist():
        assert d >= len(src_planes)
        if op == 0:
            r = resize_fn(planes[s], w, h)
        else:
            assert planes[s].shape[:2] == (h, w)
            nz = None
            if op == NOISE:
                nz, at = noise[at:at + 3 * w * h].reshape(h, w, 3), at + 3 * w * h
            r = augment_fn(planes[s], op, params[arg] if op in (BRIGHTNESS, CONTRAST, BLUR) else None, nz)
        dst = planes[d]
        ch, cw = min(h, dst.shape[0] - y), min(w, dst.shape[1] - x)
        dst[y:y + ch, x:x + cw] = r[:ch, :cw]
    assert at == len(noise)
    return out


def run_jobs_pillow(src_planes, tmp_wh, n, height, width, jobs, params=(), noise=None):
    return run_jobs(src_planes, tmp_wh, n, height, width, jobs, params, noise, resize_fn=R.pillow_resize, augment_fn=pillow_augment)
