"""Consistency check on the device (`ServingDriver.serve_consistency`, reference infer_model.py:768-848): the originals'
detections bit-identical to serve(), the device-built flip / blur images and the noise variant's preprocessed tensor
against their numpy restatements, the variants' detections against serve() of host-built variants, and the scores
against consistency_ref applied to the four detection sets the device produced."""
import numpy as np
import pytest

import consistency_ref as R
from common import FULL_MC, HEAD_MC, LOSS_ATT, make_images, make_params, make_weights

pytestmark = pytest.mark.gpu

SIZE = "256x128"                 # model input 128 x 256
RAW = (140, 260)                 # resized by 0.914
SEED = 23


def _ragged():
    rng = np.random.default_rng(9)
    return [rng.integers(0, 256, (140, 260, 3), dtype=np.uint8), rng.integers(0, 256, (136, 250, 3), dtype=np.uint8)]


def _driver(cfg, batch=2, **over):
    from uda_amd.infer_lib import KerasDriver
    p = make_params(image_size=SIZE, consistency_ssl=True, **dict(cfg, **over))
    d = KerasDriver("_", False, p["name"], batch, False, p, weights=make_weights(p, seed=12, cls_spread=20.0))
    d.set_dropout_seed(SEED)
    return d


@pytest.fixture(scope="module", params=["full", "head"])
def mc_driver(request):
    d = _driver(FULL_MC if request.param == "full" else HEAD_MC)
    yield d
    d.close()


def _check_scores(d, imgs, det, iou, agree):
    v = d.last_consistency_variants()
    cls = lambda t: t[2] if t[2].ndim == 2 else t[2][..., 0]
    widths = [np.shape(x)[1] for x in imgs]
    want_iou, want_agree = R.consistency_scores(det[0], [(v[k][0], cls(v[k])) for k in ("flip", "blur", "noise")], widths)
    np.testing.assert_allclose(iou, want_iou, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(agree, want_agree)


@pytest.mark.parametrize("post_mode", ["global", "per_class"])
def test_originals_bit_identical_to_serve(mc_driver, post_mode):
    d = mc_driver
    for imgs in (make_images(2, *RAW, seed=3), _ragged()):
        det, iou, agree = d.serve_consistency(imgs, post_mode=post_mode)
        assert iou.shape == agree.shape == (2, d.M) and iou.dtype == np.float64 and agree.dtype == bool
        _check_scores(d, imgs, det, iou, agree)
        want = d.serve(imgs, post_mode=post_mode)
        assert len(det) == len(want)
        for g, w in zip(det, want):
            assert g.shape == w.shape and g.dtype == w.dtype
            np.testing.assert_array_equal(g, w)
    assert det[3].max() > 0            # (the weights give detections: the scores are not judged on empty sets only)


def test_flip_and_blur_images_exact(mc_driver):
    d = mc_driver
    for imgs in (make_images(2, *RAW, seed=4), _ragged()):
        d.serve_consistency(imgs)
        flips, blurs = d.consistency_images(imgs)
        for im, f, b in zip(imgs, flips, blurs):
            np.testing.assert_array_equal(f, np.fliplr(im))
            np.testing.assert_array_equal(b, R.blur_u8(im))
        x, scales = d.preprocessed()
        assert x.shape[0] == 8 and scales.shape == (8,)
        np.testing.assert_array_equal(scales[2:4], scales[:2])
        np.testing.assert_array_equal(scales[6:8], scales[:2])


def test_noise_variant_preprocessed():
    from oracle import preprocess_ref as PP
    d = _driver(HEAD_MC)
    try:
        imgs = make_images(2, 128, 256, seed=5)          # raw = model size: no resize
        d.serve_consistency(imgs)
        x, _ = d.preprocessed()
        x = x.copy()
        p = d.params
        clean, _ = PP.preprocess(imgs, d.image_size, p["mean_rgb"], p["stddev_rgb"])
        np.testing.assert_array_equal(x[:2], clean)
        want, _ = PP.preprocess(R.noisy_images(imgs, SEED), d.image_size, p["mean_rgb"], p["stddev_rgb"])
        np.testing.assert_allclose(x[6:8], want, rtol=0, atol=1e-5)
        d.serve_consistency(imgs)
        again, _ = d.preprocessed()
        np.testing.assert_array_equal(again, x)                                     # same seed, same draws
        noise = ((x[6:8] - clean) * np.asarray(p["stddev_rgb"], np.float32)).astype(np.float64).ravel()
        k = noise.size
        assert abs(noise.mean()) < 4 * np.sqrt(0.5 / k)
        assert abs(noise.var() - 0.5) < 4 * np.sqrt(2 * 0.5 ** 2 / (k - 1))
    finally:
        d.close()


def test_variant_detections_match_serve_of_host_variants():
    d = _driver(LOSS_ATT)                                # no MC dropout: the variants' masks play no part
    try:
        for imgs in (make_images(2, *RAW, seed=6), _ragged()):
            det, iou, agree = d.serve_consistency(imgs)
            _check_scores(d, imgs, det, iou, agree)
            v = d.last_consistency_variants()
            for name, host in (("flip", [np.ascontiguousarray(np.fliplr(x)) for x in imgs]), ("blur", [R.blur_u8(x) for x in imgs])):
                want = d.serve(host)
                for g, w in zip(v[name], want):
                    np.testing.assert_array_equal(g, w, err_msg=name)
    finally:
        d.close()


def test_refusals(mc_driver):
    from uda_amd.infer_lib import KerasDriver
    with pytest.raises(ValueError, match="exceeds batch_size"):
        mc_driver.serve_consistency(make_images(3, *RAW))
    p = make_params(image_size=SIZE, **LOSS_ATT)
    d = KerasDriver("_", False, p["name"], 1, False, p, weights=make_weights(p, seed=12))
    try:
        with pytest.raises(ValueError, match="consistency_ssl"):
            d.serve_consistency(make_images(1, *RAW))
    finally:
        d.close()
