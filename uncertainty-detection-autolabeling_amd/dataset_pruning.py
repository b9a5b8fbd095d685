"""The pruning step of the reference's active-learning loop (`ActiveLearning.extract_hash_matrix`,
src/active_learning_loop.py:198-316, called from :165-168 under the `prune` strategies) without its distance matrix.

The reference keeps one `imagehash` value per pool image, builds the N x N matrix of Hamming distances as Python objects, takes
the matrix maximum and lists, for every image, the images within `max_dist * prune_thr` of it; of every such list with more
than one entry it keeps one randomly drawn representative.  Here the quadratic part - maximum and lists - runs on the device
on packed 64-bit words (C entry point uda_hash_neighbors_np: tiled all-pairs popcount(xor), integer-exact, no matrix); the
draws, the removal and the budget stay on the host and consume numpy's legacy stream exactly as the reference does.

  pack_hashes         imagehash values / bool arrays / uint64 words -> uint64 [N, W]
  hamming_neighbours  max_dist and the CSR rows of near-duplicates, on the device
  duplicate_groups    the reference's `duplicates` list
  prune               `kept_inds` of the hash branch (:263-299)
  random_prune        `kept_inds` of the `rand` branch (:202-207)
  adjust_budget       the iteration budget after pruning (:306-314)
  prune_pool          the whole method by its substring tests
  phash, hash_files   imagehash's perceptual hash restated with PIL and scipy (:215-224); host code
  phash_device        the same recipe from the decoded pixels on - resize to (512, 256), grey, thumbnail, DCT, median, bits -
                      for a batch of RGB images on the device (C entry point uda_phash_np); hash_files(.., device=0) uses it

Two deviations: a pool without any group keeps every image, where the reference dies in `np.concatenate([])`; and the
reference's .npy caches next to the dataset (hashes, matrix, duplicates, kept_inds) are not written or read.
"""
import ctypes as C

import numpy as np

from . import capi

MAX_WORDS = capi.PRUNE_MAX_W
PHASH_TIE = 1e-6                     # see phash_device
HASH_CHUNK_BYTES = 1 << 28           # decoded pixels hash_files holds before it hands them to the device


def _bits_to_words(bits):
    """bool [N, B] -> uint64 [N, ceil(B / 64)]: bit k of a row goes to word k // 64 at bit 63 - k % 64 (the first bit is the most
    significant), so that for B = 64 the word is int(str(imagehash value), 16).  B that is no multiple of 64 is padded with zeros."""
    n, b = bits.shape
    if b < 1 or b > 64 * MAX_WORDS:
        raise ValueError("a hash of %d bits: 1..%d are taken" % (b, 64 * MAX_WORDS))
    w = (b + 63) // 64
    padded = np.zeros((n, w * 64), np.uint8)
    padded[:, :b] = bits
    by = np.packbits(padded, axis=1, bitorder="big").reshape(n, w, 8)
    return np.ascontiguousarray(by).view(">u8").reshape(n, w).astype(np.uint64)


def pack_hashes(h):
    """uint64 [N, W] from any of: uint64 [N] / [N, W] (taken as they are), a bool array [N, s, s] or [N, bits] (imagehash's `.hash`
    stacked), or a sequence / object array of values with a `.hash` bool array (imagehash.ImageHash itself).  Bits are taken
    row-major, 64 to a word, the first bit the most significant."""
    a = h if isinstance(h, np.ndarray) else None
    if a is None:
        seq = list(h)
        if seq and all(hasattr(v, "hash") for v in seq):
            a = np.stack([np.asarray(v.hash, bool).reshape(-1) for v in seq])
        else:
            a = np.asarray(seq)
    elif a.dtype == object:
        a = np.stack([np.asarray(v.hash, bool).reshape(-1) for v in a.reshape(-1)])
    if a.dtype == np.uint64:
        if a.ndim not in (1, 2):
            raise ValueError("packed hashes are uint64 [N] or [N, W], got shape %s" % (a.shape,))
        a = a.reshape(a.shape[0], -1)
        if not 1 <= a.shape[1] <= MAX_WORDS:
            raise ValueError("%d words per hash: 1..%d are taken" % (a.shape[1], MAX_WORDS))
        return np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        if a.ndim < 2:
            raise ValueError("hash bits are bool [N, bits] or [N, s, s], got shape %s" % (a.shape,))
        return _bits_to_words(a.reshape(a.shape[0], -1))
    raise ValueError("hashes must be uint64 words, bool bits or values with a .hash array, got dtype %s" % a.dtype)


def unpack_hashes(words, bits=None):
    """The inverse of `pack_hashes` on bits: uint64 [N, W] -> bool [N, bits] (bits defaults to 64 W)."""
    words = pack_hashes(words)
    n, w = words.shape
    by = words.astype(">u8").view(np.uint8).reshape(n, w * 8)
    out = np.unpackbits(by, axis=1, bitorder="big").astype(bool)
    return out[:, :w * 64 if bits is None else bits]


class Neighbours:
    """max_dist and the rows of near-duplicates in CSR form: row i is indices[row_offsets[i]:row_offsets[i + 1]], ascending, i
    itself included."""

    def __init__(self, max_dist, row_offsets, indices):
        self.max_dist, self.row_offsets, self.indices = int(max_dist), row_offsets, indices

    def __iter__(self):                      # max_dist, row_offsets, indices = hamming_neighbours(...)
        return iter((self.max_dist, self.row_offsets, self.indices))

    def __len__(self):
        return self.row_offsets.size - 1

    def row(self, i):
        return self.indices[self.row_offsets[i]:self.row_offsets[i + 1]]


def hamming_neighbours(hashes, prune_thr=None, max_distance=None, device=0, max_entries=1 << 26):
    """For every hash the hashes within the limit, on the device.  The limit is the reference's float64 product
    `max_dist * prune_thr` (inclusive), or `max_distance` bits when that is given.  One call with a guessed capacity, and one
    more with the exact one when the guess was short.  Raises ValueError when the rows hold more than max_entries entries: such a
    threshold keeps nearly every pair and the result would not be a list of near-duplicates."""
    words = pack_hashes(hashes)
    n, w = words.shape
    if (prune_thr is None) == (max_distance is None):
        raise ValueError("give exactly one of prune_thr and max_distance")
    if max_distance is not None:
        if int(max_distance) != max_distance or not 0 <= max_distance <= 0x7FFFFFFF:
            raise ValueError("max_distance %r is not a whole number of bits >= 0" % (max_distance,))
        thr, absolute = 0.0, int(max_distance)
    else:
        thr, absolute = float(prune_thr), -1
        if not (thr >= 0.0 and np.isfinite(thr)):
            raise ValueError("prune_thr %r is negative or not finite" % (prune_thr,))
    lib = capi.load()
    row_off = np.zeros(n + 1, np.int64)
    md, total = C.c_int32(), C.c_int64()
    cap = int(min(max_entries, max(8 * n, 1 << 12)))
    for _ in range(2):
        idx = np.zeros(cap, np.int32)
        rc = lib.uda_hash_neighbors_np(int(device), words.ctypes.data, n, w, thr, absolute, cap, C.byref(md), row_off.ctypes.data,
                                       idx.ctypes.data, C.byref(total))
        capi.check(lib, None, rc, "uda_hash_neighbors_np")
        if total.value > max_entries:
            raise ValueError("the neighbour rows of %d hashes hold %d entries, more than max_entries = %d: this threshold keeps "
                             "nearly every pair (max_dist %d)" % (n, total.value, max_entries, md.value))
        if total.value <= cap:
            return Neighbours(md.value, row_off, idx[:total.value])
        cap = int(total.value)
    raise RuntimeError("uda_hash_neighbors_np reported %d entries for a capacity of %d twice" % (total.value, cap))


def duplicate_groups(nb):
    """The reference's `duplicates` (:263-270): the rows with more than one entry, in row order, as int64 arrays."""
    _, off, idx = nb
    return [idx[off[i]:off[i + 1]].astype(np.int64) for i in np.flatnonzero(np.diff(off) > 1)]


def remove_duplicates(groups, n, rng=None):
    """`kept_inds` from the groups (:281-294): one `rng.choice(group)` per group in list order, everything else of every group
    removed, the ascending rest kept.  No group: every image is kept (the reference raises there)."""
    rng = np.random if rng is None else rng
    keep = [rng.choice(g) for g in groups]
    if not groups:
        return np.arange(n, dtype=np.int64)
    removed = np.unique(np.concatenate([g[g != k] for g, k in zip(groups, keep)]))
    mask = np.ones(n, bool)
    mask[removed] = False
    return np.flatnonzero(mask).astype(np.int64)


def prune(hashes, prune_thr, rng=None, device=0):
    """`kept_inds` of the hash branch: the pool indices that survive, ascending.  rng=None draws from numpy's global legacy
    stream (np.random), as the reference does; a np.random.RandomState may be passed instead."""
    words = pack_hashes(hashes)
    nb = hamming_neighbours(words, prune_thr=prune_thr, device=device)
    return remove_duplicates(duplicate_groups(nb), words.shape[0], rng)


def random_prune(n, prune_thr, rng=None):
    """`kept_inds` of the `rand` branch (:203-207): int((1 - prune_thr) * n) indices without replacement, in drawn order."""
    rng = np.random if rng is None else rng
    return rng.choice(np.arange(n), size=int((1 - prune_thr) * n), replace=False)


def adjust_budget(iteration_budget, n_before, n_after, full_prune=False):
    """The budget after pruning (:306-314): [100] under `full_prune`, else the percentages scaled by n_before / n_after and cut
    to the prefix whose running sum stays within 100."""
    if full_prune:
        return [100]
    new = np.asarray(iteration_budget) * n_before / n_after
    return new[new.cumsum() <= 100]


def prune_pool(strategy, hashes, available_indices, iteration_budget, prune_thr, rng=None, device=0):
    """`extract_hash_matrix` by its substring tests: `rand` in the strategy prunes at random (hashes are not read and may be
    None), anything else by hash; `full_prune` collapses the budget.  Returns (available_indices re-indexed by kept_inds, the new
    budget, kept_inds)."""
    n = len(available_indices)
    if "rand" in strategy:
        kept = random_prune(n, prune_thr, rng)
    else:
        words = pack_hashes(hashes)
        if words.shape[0] != n:
            raise ValueError("%d hashes for a pool of %d images" % (words.shape[0], n))
        kept = prune(words, prune_thr, rng, device)
    available = [available_indices[i] for i in kept]
    return available, adjust_budget(iteration_budget, n, len(available), "full_prune" in strategy), kept


def phash(image, hash_size=8, highfreq_factor=4):
    """imagehash.phash restated: grey (`L`), Lanczos resize to (hash_size * highfreq_factor) squared, scipy.fftpack.dct along axis
    0 and then axis 1, the top-left hash_size x hash_size block compared with its own median.  Returns bool [hash_size, hash_size].
    imagehash is not a dependency and was not available to compare with."""
    import scipy.fftpack
    from PIL import Image
    if not isinstance(image, Image.Image):
        image = Image.fromarray(np.asarray(image))
    size = hash_size * highfreq_factor
    pixels = np.asarray(image.convert("L").resize((size, size), Image.LANCZOS))
    dct = scipy.fftpack.dct(scipy.fftpack.dct(pixels, axis=0), axis=1)
    low = dct[:hash_size, :hash_size]
    return low > np.median(low)


def _phash_call_bytes(w, h):
    """The device bytes uda_phash_np counts for one image (include/uda_hip.h): its 512 x 256 plane, its source, and the first
    pass's result when both axes change."""
    pw, ph = capi.PHASH_PRE_W, capi.PHASH_PRE_H
    mid = 0 if w == pw or h == ph else (3 * w * ph if h > 100 * w and ph < h else 3 * pw * h)
    return 3 * pw * ph + 3 * w * h + mid


def phash_device(images, device=0, info=None):
    """`phash(image.resize((512, 256)))` of every image, on the device: uint64 [N, 1] as `hash_files` packs them.  images: uint8
    arrays [h, w, 3] or PIL images of mode RGB.  They go to uda_phash_np in as many calls as its byte cap asks for.

    The result equals the host recipe for every image.  Resize, grey and thumbnail are Pillow's bit for bit; the DCT is not
    scipy's: the device adds 32 products in a fixed order where scipy runs an FFT, and the two agree only to rounding, so a bit
    whose coefficient lies within rounding of the median is determined by neither.  Every call therefore fetches the margin - the
    smallest |low - median| of the image - and the 32 x 32 thumbnail (1 KB an image), and an image with margin <= PHASH_TIE gets
    its bits on the host, from the device's thumbnail with scipy.fftpack.dct as `phash` does.  info["ties"], when a dict is
    given, lists those images' indices; info["margin"] has every margin.

    PHASH_TIE = 1e-6: |low| <= 32 * 2 * 32 * 2 * 255 ~ 1.04e6, and two sequential sums of 32 rounded products at that magnitude
    carry at most about 64 * 2^-53 * 1.04e6 ~ 1e-8 of absolute error on the device side.  scipy's own error has no bound derived
    here; the largest |direct sum - scipy| measured over 24 images was 9.8e-11.  1e-6 leaves a factor of 100 over the first figure
    and 10^4 over the second.  Constant images always land here: their AC terms are exactly 0 with scipy and noise in a sum."""
    import scipy.fftpack
    planes = []
    for k, im in enumerate(images):
        if not isinstance(im, np.ndarray):
            if getattr(im, "mode", None) != "RGB":
                raise ValueError("image %d has mode %r: RGB PIL images or uint8 arrays [h, w, 3] are taken" % (k, getattr(im, "mode", None)))
            im = np.asarray(im)
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError("image %d is %s %s: uint8 [h, w, 3] with h, w >= 1 is taken" % (k, im.dtype, im.shape))
        if max(im.shape[:2]) > capi.RESAMPLE_MAX_SIDE:
            raise ValueError("image %d is %d x %d: a side above %d is not taken" % (k, im.shape[1], im.shape[0], capi.RESAMPLE_MAX_SIDE))
        planes.append(np.ascontiguousarray(im))
    n = len(planes)
    words, margin = np.zeros(n, np.uint64), np.zeros(n, np.float64)
    thumb = np.zeros((n, capi.PHASH_SIDE, capi.PHASH_SIDE), np.uint8)
    lib = capi.load() if n else None
    k0 = 0
    while k0 < n:
        k1, need = k0, 0
        while k1 < n and (k1 == k0 or need + _phash_call_bytes(planes[k1].shape[1], planes[k1].shape[0]) <= capi.PHASH_MAX_BYTES):
            need += _phash_call_bytes(planes[k1].shape[1], planes[k1].shape[0])
            k1 += 1
        wh = np.array([(p.shape[1], p.shape[0]) for p in planes[k0:k1]], np.int32)
        pix = np.concatenate([p.reshape(-1) for p in planes[k0:k1]])
        rc = lib.uda_phash_np(int(device), k1 - k0, wh.ctypes.data, pix.ctypes.data, words[k0:k1].ctypes.data,
                              margin[k0:k1].ctypes.data, thumb[k0:k1].ctypes.data, None)
        capi.check(lib, None, rc, "uda_phash_np")
        k0 = k1
    ties = np.flatnonzero(margin <= PHASH_TIE)
    for k in ties:
        dct = scipy.fftpack.dct(scipy.fftpack.dct(thumb[k], axis=0), axis=1)
        low = dct[:capi.PHASH_LOW, :capi.PHASH_LOW]
        words[k] = _bits_to_words((low > np.median(low)).reshape(1, -1))[0, 0]
    if info is not None:
        info["ties"], info["margin"] = ties.tolist(), margin
    return words.reshape(n, 1)


def hash_files(paths, method="p", device=None):
    """The hashes of the pool as the reference computes them (:215-224): every file opened, resized to (512, 256) with PIL's
    default filter, then the perceptual hash.  Returns uint64 [N, 1].  method "w" (imagehash.whash) needs a wavelet package
    (PyWavelets) this build does not depend on; the reference's own command line fixes the method to perceptual.

    device=None is the host loop.  With a device the files that open in mode RGB are decoded here and hashed by `phash_device`,
    HASH_CHUNK_BYTES of pixels at a time; a file of any other mode takes the host path.  The hashes are the same either way."""
    if method != "p":
        raise ValueError("hash method %r: only 'p' (perceptual) is built; 'w' needs the wavelet package PyWavelets (pywt)" % (method,))
    from PIL import Image
    if device is not None:
        paths = list(paths)
        words = np.zeros((len(paths), 1), np.uint64)
        held, where, held_bytes = [], [], 0

        def flush():
            if held:
                words[where] = phash_device(held, device)
            del held[:], where[:]
        for k, p in enumerate(paths):
            with Image.open(p) as im:
                if im.mode == "RGB":
                    held.append(np.asarray(im))
                    where.append(k)
                    held_bytes += held[-1].nbytes
                else:
                    words[k] = _bits_to_words(phash(im.resize((512, 256))).reshape(1, -1))
            if held_bytes >= HASH_CHUNK_BYTES:
                flush()
                held_bytes = 0
        flush()
        return words
    bits = []
    for p in paths:
        with Image.open(p) as im:
            bits.append(phash(im.resize((512, 256))).reshape(-1))
    return _bits_to_words(np.stack(bits)) if bits else np.zeros((0, 1), np.uint64)
