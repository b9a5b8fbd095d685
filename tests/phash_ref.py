"""numpy mirror of the device perceptual hash (uda_phash_np, include/uda_hip.h): Pillow's 8-bit resample applied as integer
arithmetic on the coefficient tables the library hands out (uda_resample_coeffs_filter_np), Pillow's grey formula, and the 8 x 8
low corner of the two-axis DCT as direct float64 sums against the table of uda_phash_table_np, added in the order the kernel adds
in - every product rounded, then every sum; numpy's elementwise `*` and `+` never fuse.  Also the structured test images.  Slow
and plain on purpose; nothing here is imported by the package."""
import ctypes as C
import functools

import numpy as np

from uda_amd import capi

BITS = 22
PRE_W, PRE_H, SIDE, LOW = 512, 256, 32, 8


@functools.lru_cache(maxsize=None)
def table(in_size, out_size, filt):
    """-> (ksize, bounds [out, 2], kk [out, ksize]) of the library, host only."""
    lib = capi.load()
    ks = C.c_int32()
    assert lib.uda_resample_coeffs_filter_np(in_size, out_size, filt, C.byref(ks), None, None, 0) == 0, lib.uda_last_error(None)
    bounds, kk = np.zeros((out_size, 2), np.int32), np.zeros((out_size, ks.value), np.int32)
    assert lib.uda_resample_coeffs_filter_np(in_size, out_size, filt, C.byref(ks), bounds.ctypes.data, kk.ctypes.data, kk.size) == 0
    return ks.value, bounds, kk


@functools.lru_cache(maxsize=None)
def dct_table():
    T = np.zeros((LOW, SIDE), np.float64)
    assert capi.load().uda_phash_table_np(T.ctypes.data) == 0
    return T


def _pass(img, out_size, axis, filt):
    """One pass along `axis` of a uint8 array [h, w] or [h, w, 3]: 2^21 + sum pixel * k, >> 22, clamped."""
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    _, bounds, kk = table(img.shape[0], out_size, filt)
    out = np.zeros((out_size,) + img.shape[1:], np.uint8)
    for xx in range(out_size):
        xmin, xmax = bounds[xx]
        acc = (1 << (BITS - 1)) + np.tensordot(kk[xx, :xmax].astype(np.int64), img[xmin:xmin + xmax], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31            # Pillow's int32 accumulator does not wrap
        out[xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, w, h, filt):
    """Image.fromarray(img).resize((w, h), filt) as an array, Image.resize's vertical-first rule included."""
    img = np.ascontiguousarray(img, np.uint8)
    if img.shape[0] > img.shape[1] * 100 and h < img.shape[0]:
        img = _pass(img, h, 0, filt)
    if img.shape[1] != w:
        img = _pass(img, w, 1, filt)
    if img.shape[0] != h:
        img = _pass(img, h, 0, filt)
    return img.copy()


def grey(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def thumbnail(img):
    """uint8 [h, w, 3] -> the 32 x 32 thumbnail the hash is made of."""
    pre = resize(img, PRE_W, PRE_H, capi.FILTER_BICUBIC)
    return resize(grey(pre), SIDE, SIDE, capi.FILTER_LANCZOS)


def low_of(thumb):
    """a[k][j] = sum_i T[k][i] x[i][j], i ascending from 0.0; low[k][l] = sum_j a[k][j] T[l][j], j ascending."""
    T, x = dct_table(), thumb.astype(np.float64)
    a = np.zeros((LOW, SIDE))
    for i in range(SIDE):
        a = a + T[:, i, None] * x[i][None, :]
    low = np.zeros((LOW, LOW))
    for j in range(SIDE):
        low = low + a[:, j, None] * T[None, :, j]
    return low


def tail(thumb):
    """-> (low [8, 8], med, bits bool [64], margin).  The median by rank, as the kernel finds it."""
    low = low_of(thumb)
    v = low.reshape(-1)
    order = np.argsort(v, kind="stable")              # ties by index
    med = (v[order[31]] + v[order[32]]) / 2.0
    assert med == np.median(v)
    return low, med, v > med, np.abs(v - med).min()


def word(bits):
    return np.uint64(int("".join("1" if b else "0" for b in np.asarray(bits).reshape(-1)), 2))


def mirror(img):
    """-> (word, margin, thumb, low) of one image, what uda_phash_np returns for it."""
    th = thumbnail(img)
    low, _, bits, margin = tail(th)
    return word(bits), margin, th, low.reshape(-1)


# ---- test images.  SIZES are (w, h); 3 x 400 takes Image.resize's vertical-first rule
SIZES = [(1, 1), (2, 3), (30, 40), (511, 255), (512, 256), (513, 257), (1242, 375), (3, 400)]


def noise_image(w, h, seed=0):
    return np.random.default_rng([w, h, seed]).integers(0, 256, (h, w, 3), dtype=np.uint8)


def structured_image(w, h, seed=0):
    """A coarse random colour field enlarged bilinearly, plus +-20 noise: low frequencies well away from their median."""
    rng = np.random.default_rng([w, h, seed, 7])
    coarse = rng.uniform(0, 255, (5, 6, 3))
    ys, xs = np.linspace(0, 4, h), np.linspace(0, 5, w)
    y0, x0 = np.minimum(ys.astype(int), 3), np.minimum(xs.astype(int), 4)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    f = ((1 - fy) * (1 - fx) * coarse[y0][:, x0] + (1 - fy) * fx * coarse[y0][:, x0 + 1]
         + fy * (1 - fx) * coarse[y0 + 1][:, x0] + fy * fx * coarse[y0 + 1][:, x0 + 1])
    return np.clip(f + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


def host_words(img):
    """The host recipe on one array: phash(Image.resize((512, 256))) packed as hash_files packs it."""
    from PIL import Image
    from uda_amd import dataset_pruning as DP
    return DP._bits_to_words(DP.phash(Image.fromarray(img).resize((PRE_W, PRE_H))).reshape(1, -1))[0, 0]
