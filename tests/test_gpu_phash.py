"""The perceptual hash on the device (`dataset_pruning.phash_device` / `hash_files(.., device=0)` -> `uda_phash_np`; reference
active_learning_loop.py:215-224): the C entry point against live Pillow (the thumbnail, exactly), against the numpy mirror
(tests/phash_ref.py: low and margin, bit for bit) and against the host recipe `phash(im.resize((512, 256)))` (the words, for
every structured image - each of which is first shown on the host to lie at least 1e-3 from a tie, so none is left out); the
same outputs alone, in a batch and at another position; images that tie; refusals; and the package's file loop."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

import phash_ref as R
from uda_amd import capi
from uda_amd import dataset_pruning as DP

pytestmark = pytest.mark.gpu

SIZES = R.SIZES + [(1280, 720)]
SENT_W, SENT_F, SENT_B = np.uint64(0xA5A5A5A5A5A5A5A5), -123.5, 0x5A


def raw(images, want_thumb=True, want_low=True, device=0):
    """One call of the C entry point on sentinel-filled outputs: (rc, words, margin, thumb, low)."""
    lib = capi.load()
    n = len(images)
    wh = np.array([(im.shape[1], im.shape[0]) for im in images], np.int32).reshape(n, 2)
    pix = np.concatenate([im.reshape(-1) for im in images]) if n else np.zeros(1, np.uint8)
    words, margin = np.full(max(n, 1), SENT_W, np.uint64), np.full(max(n, 1), SENT_F)
    thumb, low = np.full((max(n, 1), 32, 32), SENT_B, np.uint8), np.full((max(n, 1), 64), SENT_F)
    rc = lib.uda_phash_np(device, n, wh.ctypes.data, pix.ctypes.data, words.ctypes.data, margin.ctypes.data,
                          thumb.ctypes.data if want_thumb else None, low.ctypes.data if want_low else None)
    return rc, words, margin, thumb, low


def untouched(words, margin, thumb, low):
    return (words == SENT_W).all() and (margin == SENT_F).all() and (thumb == SENT_B).all() and (low == SENT_F).all()


@pytest.fixture(scope="module")
def structured():
    """One structured image of every size with its mirror and its host word, computed once: {(w, h): (img, mirror, word)}."""
    out = {}
    for w, h in SIZES[1:]:
        img = R.structured_image(w, h)
        out[(w, h)] = (img, R.mirror(img), R.host_words(img))
    return out


def pillow_thumb(img):
    return np.asarray(Image.fromarray(img).resize((512, 256)).convert("L").resize((32, 32), Image.LANCZOS))


def assert_image(got, k, img, mirror, host_word=None):
    _, words, margin, thumb, low = got
    mw, mm, mt, ml = mirror
    assert np.array_equal(thumb[k], pillow_thumb(img)) and np.array_equal(thumb[k], mt)
    assert np.array_equal(low[k].view(np.uint64), ml.view(np.uint64))
    assert margin[k] == mm and words[k] == mw
    if host_word is not None:
        assert mm >= 1e-3                                      # the input's condition, from the mirror alone
        assert words[k] == host_word


@pytest.mark.parametrize("w,h", SIZES[1:])
def test_structured_image_alone(structured, w, h):
    img, mirror, hw = structured[(w, h)]
    got = raw([img])
    assert got[0] == 0, capi.load().uda_last_error(None).decode()
    print("%d x %d: margin %.6g" % (w, h, got[2][0]))
    assert_image(got, 0, img, mirror, hw)
    info = {}
    assert DP.phash_device([img], info=info)[0, 0] == hw and info["ties"] == [] and info["margin"][0] == mirror[1]
    assert DP.phash_device([Image.fromarray(img)])[0, 0] == hw


@pytest.mark.parametrize("w,h", SIZES)
def test_noise_image_equals_pillow_and_the_mirror(w, h):
    """Noise reaches every clamp of the two resamples; its low frequencies may tie, so the word is the mirror's, and the wrapper's
    is the host recipe's whichever way it was settled."""
    img = R.noise_image(w, h, seed=3)
    got = raw([img])
    assert got[0] == 0, capi.load().uda_last_error(None).decode()
    assert_image(got, 0, img, R.mirror(img))
    assert DP.phash_device([img])[0, 0] == R.host_words(img)


def test_mixed_batch_and_positions(structured):
    """Every size in one call, a constant image among them: each image's outputs are those it has alone, wherever it stands."""
    keys = list(structured)
    imgs = [structured[k][0] for k in keys]
    flat = np.full((100, 200, 3), 77, np.uint8)
    batch = imgs[:4] + [flat] + imgs[4:]
    got = raw(batch)
    assert got[0] == 0, capi.load().uda_last_error(None).decode()
    back = raw(batch[::-1])
    assert back[0] == 0
    n = len(batch)
    for i, k in enumerate(keys):
        pos = i if i < 4 else i + 1
        assert_image(got, pos, structured[k][0], structured[k][1], structured[k][2])
        alone = raw([structured[k][0]])
        for a, b, c in zip(got[1:], back[1:], alone[1:]):
            assert a[pos:pos + 1].tobytes() == c[:1].tobytes() and b[n - 1 - pos:n - pos].tobytes() == c[:1].tobytes()
    info = {}
    words = DP.phash_device(batch, info=info)
    assert info["ties"] == [4]
    assert words[:, 0].tolist() == [R.host_words(im) for im in batch]
    # NULL thumb and low: the same words and margins, the optional arrays left alone
    lean = raw(batch, want_thumb=False, want_low=False)
    assert lean[0] == 0 and np.array_equal(lean[1], got[1]) and np.array_equal(lean[2], got[2])
    assert (lean[3] == SENT_B).all() and (lean[4] == SENT_F).all()


@pytest.mark.parametrize("n", [1, 2, 65])
def test_many_small_images(n):
    """8 x 8 images, one block each: N = 65 is more blocks than a wave has lanes and leaves none to its neighbour's outputs."""
    imgs = [R.structured_image(8, 8, seed=s) for s in range(n)]
    got = raw(imgs)
    assert got[0] == 0, capi.load().uda_last_error(None).decode()
    for k in sorted({0, 1 % n, n // 2, n - 1}):
        assert_image(got, k, imgs[k], R.mirror(imgs[k]))
    want = np.array([R.host_words(im) for im in imgs], np.uint64)
    info = {}
    assert np.array_equal(DP.phash_device(imgs, info=info)[:, 0], want)
    clear = np.setdiff1d(np.arange(n), info["ties"])
    assert np.array_equal(got[1][clear], want[clear])
    assert len(set(want.tolist())) > n // 2                    # (the images do differ)


def test_images_that_tie_are_settled_on_the_host():
    """Constant images and a two-level one: with scipy their AC terms (for the two-level one, every term with a vertical
    frequency) are exactly 0 and so is the median; a direct sum leaves noise there.  The device reports a margin within
    PHASH_TIE, the wrapper lists them and gives the host recipe's hash."""
    one = np.full((1, 1, 3), 200, np.uint8)
    flat = np.full((100, 200, 3), 77, np.uint8)
    black = np.zeros((256, 512, 3), np.uint8)
    two = np.zeros((64, 96, 3), np.uint8)
    two[:, 48:] = 255
    clear = R.structured_image(30, 40)
    imgs = [one, clear, flat, two, black]
    for k in (0, 2, 3, 4):
        assert R.mirror(imgs[k])[1] <= DP.PHASH_TIE
    got = raw(imgs)
    assert got[0] == 0, capi.load().uda_last_error(None).decode()
    for k, im in enumerate(imgs):
        assert_image(got, k, im, R.mirror(im))
    info = {}
    words = DP.phash_device(imgs, info=info)
    assert info["ties"] == [0, 2, 3, 4]
    assert words[:, 0].tolist() == [R.host_words(im) for im in imgs]
    assert words[0, 0] == 1 << 63 and words[4, 0] == 0         # the DC term alone above the median; nothing above it


def test_refusals_leave_the_outputs_untouched():
    lib = capi.load()
    img = R.structured_image(8, 8)
    n = 2
    wh = np.array([(8, 8), (8, 8)], np.int32)
    pix = np.concatenate([img.reshape(-1)] * 2)
    words, margin = np.full(n, SENT_W, np.uint64), np.full(n, SENT_F)
    thumb, low = np.full((n, 32, 32), SENT_B, np.uint8), np.full((n, 64), SENT_F)
    p = lambda a: a.ctypes.data
    big = capi.RESAMPLE_MAX_SIDE + 1
    # 40 000 x 40 000: 4.8e9 bytes of source alone, above the cap (refused before a pixel is read)
    bad_wh = [np.array(v, np.int32) for v in ([(8, 8), (0, 8)], [(8, -1), (8, 8)], [(8, 8), (big, 1)], [(8, 8), (1, big)],
                                              [(8, 8), (40000, 40000)])]
    cases = [(-1, p(wh), p(pix), p(words), p(margin)),
             (n, None, p(pix), p(words), p(margin)),
             (n, p(wh), None, p(words), p(margin)),
             (n, p(wh), p(pix), None, p(margin)),
             (n, p(wh), p(pix), p(words), None)] + [(n, p(b), p(pix), p(words), p(margin)) for b in bad_wh]
    for args in cases:
        rc = lib.uda_phash_np(0, args[0], args[1], args[2], args[3], args[4], p(thumb), p(low))
        assert rc == 1, args
        assert lib.uda_last_error(None).decode().startswith("uda_phash_np: ")
        assert untouched(words, margin, thumb, low)
    assert "split the call" in lib.uda_last_error(None).decode()
    rc = lib.uda_phash_np(0, n, p(wh), p(pix), p(words), p(margin), p(thumb), p(low))
    assert rc == 0 and words[0] == words[1] == R.host_words(img)


def test_no_images():
    got = raw([])
    assert got[0] == 0 and untouched(*got[1:])
    assert capi.load().uda_phash_np(0, 0, None, None, None, None, None, None) == 0
    assert DP.phash_device([]).shape == (0, 1)


def test_hash_files_and_prune_pool_on_a_directory(tmp_path):
    """RGB and grey PNGs, near-duplicates among them: hash_files(.., device=0) equals the host loop file for file, and the pool
    pruned by either keeps the same indices."""
    base = [R.structured_image(96, 64, seed=s) for s in range(5)]
    arrays = []
    for s, b in enumerate(base):
        arrays.append(b)
        near = b.copy()
        near[:4, :4] ^= 1
        arrays.append(near)
    paths = []
    for k, a in enumerate(arrays):
        path = str(tmp_path / ("im%02d.png" % k))
        (Image.fromarray(a).convert("L") if k % 4 == 3 else Image.fromarray(a)).save(path)
        paths.append(path)
    host = DP.hash_files(paths)
    dev = DP.hash_files(paths, device=0)
    assert dev.dtype == np.uint64 and dev.shape == (10, 1) and np.array_equal(dev, host)
    old = DP.HASH_CHUNK_BYTES
    DP.HASH_CHUNK_BYTES = 2 * 96 * 64 * 3                       # several device calls
    try:
        assert np.array_equal(DP.hash_files(paths, device=0), host)
    finally:
        DP.HASH_CHUNK_BYTES = old
    kept = [DP.prune_pool("prune", h, list(range(10)), [10, 20, 30], 0.1, rng=np.random.RandomState(3))[2] for h in (host, dev)]
    assert np.array_equal(kept[0], kept[1]) and 0 < len(kept[0]) < 10
