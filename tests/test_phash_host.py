"""The host side of the device perceptual hash (uda_phash_np; reference active_learning_loop.py:215-224), without a GPU: the
bicubic coefficient table against live Pillow, the Lanczos table against the entry point it generalises, the DCT table against
numpy's cosine, the numpy mirror (tests/phash_ref.py) against scipy and against `dataset_pruning.phash`, and the wrapper's
refusals."""
import ctypes as C

import numpy as np
import pytest
import scipy.fftpack
from PIL import Image

import collage_ref
import phash_ref as R
from uda_amd import capi
from uda_amd import dataset_pruning as DP

STRUCTURED = [(w, h, s) for (w, h) in R.SIZES[1:] + [(1280, 720)] for s in range(3)]


@pytest.mark.parametrize("w,h", R.SIZES)
def test_bicubic_table_gives_pillows_default_resize(w, h):
    """The table of uda_resample_coeffs_filter_np(.., UDA_FILTER_BICUBIC, ..) in integer arithmetic, along x and then along y
    (3 x 400: along y first), equals Image.resize((512, 256)) of the installed Pillow exactly."""
    assert capi.FILTER_BICUBIC == Image.BICUBIC and capi.FILTER_LANCZOS == Image.LANCZOS
    for img in (R.noise_image(w, h), R.structured_image(w, h)):
        want = np.asarray(Image.fromarray(img).resize((R.PRE_W, R.PRE_H)))
        got = R.resize(img, R.PRE_W, R.PRE_H, capi.FILTER_BICUBIC)
        assert got.shape == want.shape == (256, 512, 3) and np.array_equal(got, want)
    if (w, h) == (3, 400):                                    # the rule matters: x first gives other pixels
        img = R.noise_image(w, h)
        assert not np.array_equal(R._pass(R._pass(img, 512, 1, capi.FILTER_BICUBIC), 256, 0, capi.FILTER_BICUBIC),
                                  np.asarray(Image.fromarray(img).resize((512, 256))))


@pytest.mark.parametrize("w,h", [(7, 5), (40, 30), (600, 300)])
def test_bicubic_table_enlarging_and_shrinking_to_other_sizes(w, h):
    img = R.noise_image(w, h)
    for tw, th in ((13, 17), (64, 3), (w, 2 * h)):
        want = np.asarray(Image.fromarray(img).resize((tw, th), Image.BICUBIC))
        assert np.array_equal(R.resize(img, tw, th, capi.FILTER_BICUBIC), want)


@pytest.mark.parametrize("n_in,n_out", [(512, 32), (256, 32), (1, 1), (3, 7), (1242, 512), (100, 100), (65536, 5)])
def test_lanczos_through_the_filter_entry_is_the_old_table(n_in, n_out):
    lib = capi.load()
    ks = C.c_int32()
    assert lib.uda_resample_coeffs_np(n_in, n_out, C.byref(ks), None, None, 0) == 0
    b, k = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ks.value), np.int32)
    assert lib.uda_resample_coeffs_np(n_in, n_out, C.byref(ks), b.ctypes.data, k.ctypes.data, k.size) == 0
    ks2, b2, k2 = R.table(n_in, n_out, capi.FILTER_LANCZOS)
    assert ks2 == ks.value and np.array_equal(b2, b) and np.array_equal(k2, k)
    if n_in * n_out <= 1 << 16:
        ks3, b3, k3 = collage_ref.coeffs(n_in, n_out)
        assert ks3 == ks2 and np.array_equal(b3, b2) and np.array_equal(k3, k2)


def test_filter_entry_contract_and_refusals():
    lib = capi.load()
    ks = C.c_int32(-1)
    assert lib.uda_resample_coeffs_filter_np(512, 32, capi.FILTER_LANCZOS, C.byref(ks), None, None, 0) == 0 and ks.value == 97
    assert lib.uda_resample_coeffs_filter_np(256, 32, capi.FILTER_LANCZOS, C.byref(ks), None, None, 0) == 0 and ks.value == 49
    assert lib.uda_resample_coeffs_filter_np(1242, 512, capi.FILTER_BICUBIC, C.byref(ks), None, None, 0) == 0 and ks.value == 11
    assert lib.uda_resample_coeffs_filter_np(30, 512, capi.FILTER_BICUBIC, C.byref(ks), None, None, 0) == 0 and ks.value == 5
    b, k = np.full((512, 2), -7, np.int32), np.full((512, 5), -7, np.int32)
    for args in ((30, 512, 2, C.byref(ks), b.ctypes.data, k.ctypes.data, k.size),            # Image.BILINEAR: not built
                 (30, 512, 0, C.byref(ks), b.ctypes.data, k.ctypes.data, k.size),
                 (0, 512, capi.FILTER_BICUBIC, C.byref(ks), b.ctypes.data, k.ctypes.data, k.size),
                 (30, capi.RESAMPLE_MAX_SIDE + 1, capi.FILTER_BICUBIC, C.byref(ks), b.ctypes.data, k.ctypes.data, k.size),
                 (30, 512, capi.FILTER_BICUBIC, None, b.ctypes.data, k.ctypes.data, k.size),
                 (30, 512, capi.FILTER_BICUBIC, C.byref(ks), None, k.ctypes.data, k.size),
                 (30, 512, capi.FILTER_BICUBIC, C.byref(ks), b.ctypes.data, k.ctypes.data, k.size - 1)):
        assert lib.uda_resample_coeffs_filter_np(*args) == 1
        assert lib.uda_last_error(None).decode().startswith("uda_resample_coeffs_filter_np: ")
        assert (b == -7).all() and (k == -7).all()
    # rows sum to 2^22 up to the rounding of their entries; zeros past xmax
    _, b, k = R.table(1242, 512, capi.FILTER_BICUBIC)
    assert (np.abs(k.sum(1) - (1 << 22)) <= 11).all()
    assert all((k[i, b[i, 1]:] == 0).all() for i in range(512))


def test_dct_table_is_numpys_cosine_to_one_ulp():
    T = R.dct_table()
    k, i = np.arange(8)[:, None], np.arange(32)[None, :]
    want = 2.0 * np.cos(np.pi * k * (2 * i + 1) / 64.0)
    assert (np.abs(T - want) <= np.spacing(np.abs(want))).all()
    assert (T[0] == 2.0).all()
    assert capi.load().uda_phash_table_np(None) == 1
    assert capi.load().uda_last_error(None).decode().startswith("uda_phash_table_np: ")


@pytest.fixture(scope="module")
def structured():
    """[(image, thumb, (low, med, bits, margin))] of every structured image."""
    out = []
    for w, h, s in STRUCTURED:
        img = R.structured_image(w, h, s)
        th = R.thumbnail(img)
        out.append((img, th, R.tail(th)))
    return out


def test_mirror_thumbnail_is_pillows(structured):
    for img, th, _ in structured:
        want = np.asarray(Image.fromarray(img).resize((512, 256)).convert("L").resize((32, 32), Image.LANCZOS))
        assert np.array_equal(th, want)


def test_mirror_low_is_scipys_to_1e_8_and_bits_are_phashs(structured):
    worst, smallest = 0.0, np.inf
    for img, th, (low, med, bits, margin) in structured:
        want = scipy.fftpack.dct(scipy.fftpack.dct(th, axis=0), axis=1)[:8, :8]
        worst, smallest = max(worst, np.abs(low - want).max()), min(smallest, margin)
        assert np.abs(low - want).max() <= 1e-8
        assert margin >= 1e-3                                 # the condition the GPU test states for these inputs
        assert np.array_equal(bits.reshape(8, 8), DP.phash(Image.fromarray(img).resize((512, 256))))
        assert R.word(bits) == R.host_words(img)
    print("largest |direct sum - scipy| %.3g, smallest margin %.3g over %d images" % (worst, smallest, len(structured)))


def test_constant_images_tie_in_the_mirror():
    """A flat image: scipy's AC terms are exactly 0, the direct sum's are rounding noise - the margin is far below PHASH_TIE."""
    for img in (np.full((1, 1, 3), 200, np.uint8), np.full((100, 200, 3), 77, np.uint8)):
        th = R.thumbnail(img)
        assert (th == th[0, 0]).all()
        low, med, bits, margin = R.tail(th)
        assert margin <= DP.PHASH_TIE
        want = scipy.fftpack.dct(scipy.fftpack.dct(th, axis=0), axis=1)[:8, :8]
        assert (want.reshape(-1)[1:] == 0).all() and np.abs(low - want).max() <= 1e-8


def test_wrapper_refuses_wrong_dtypes_and_shapes():
    ok = np.zeros((4, 5, 3), np.uint8)
    for bad in (ok.astype(np.float32), ok[..., :1], ok[..., 0], np.zeros((0, 5, 3), np.uint8), np.zeros((4, 5, 4), np.uint8),
                Image.fromarray(ok).convert("L"), Image.fromarray(ok).convert("RGBA")):
        with pytest.raises(ValueError, match="image 1"):
            DP.phash_device([ok, bad])
    assert DP.phash_device([]).shape == (0, 1) and DP.phash_device([]).dtype == np.uint64
    with pytest.raises(ValueError, match="only 'p'"):
        DP.hash_files([], method="w", device=0)
    assert DP.hash_files([], device=0).shape == (0, 1)


def test_call_bytes_follow_the_header():
    assert DP._phash_call_bytes(512, 256) == 2 * 393216
    assert DP._phash_call_bytes(512, 100) == 393216 + 3 * 512 * 100
    assert DP._phash_call_bytes(1242, 375) == 393216 + 3 * 1242 * 375 + 3 * 512 * 375
    assert DP._phash_call_bytes(3, 400) == 393216 + 3 * 3 * 400 + 3 * 3 * 256
    assert capi.PHASH_MAX_BYTES == 1 << 32 and DP.PHASH_TIE == 1e-6
