"""Consistency check (`consistency_ssl`, reference infer_model.py:768-848) on the CPU: the numpy restatement the GPU tests
judge the device by, the record columns, and the config / planner handling of the key."""
import numpy as np
import pytest

import consistency_ref as R
from common import make_params, make_weights


def test_blur_taps_follow_opencv_rule():
    taps = R.fixed_point_taps(9, 0.0)
    assert taps == R.BLUR_TAPS
    assert sum(taps) == 256 and taps == taps[::-1]
    assert R.fixed_point_taps(9, 1.7) == taps          # sigma 0 means 0.3 ((9 - 1) / 2 - 1) + 0.8 = 1.7


def test_reflect101_edges():
    assert [R.reflect101(p, 6) for p in range(-4, 0)] == [4, 3, 2, 1]
    assert [R.reflect101(p, 6) for p in range(6, 10)] == [4, 3, 2, 1]
    assert [R.reflect101(p, 2) for p in range(-4, 6)] == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]      # iterated on tiny images
    assert R.reflect101(-3, 1) == 0 and R.reflect101(5, 1) == 0


@pytest.mark.parametrize("hw", [(7, 11), (3, 2), (1, 5)])
def test_blur_reflects_at_all_four_edges(hw):
    h, w = hw
    im = np.random.default_rng(h * 31 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = R.blur_u8(im)
    c = R.BLUR_TAPS
    for y in range(h):
        for x in range(w):
            s = np.zeros(3, np.int64)
            for j in range(9):
                for i in range(9):
                    s += c[j] * c[i] * im[R.reflect101(y + j - 4, h), R.reflect101(x + i - 4, w)].astype(np.int64)
            np.testing.assert_array_equal(got[y, x], ((s + 32768) >> 16).astype(np.uint8), err_msg=str((y, x)))


def test_blur_of_constant_image_is_constant():
    for v in (0, 1, 127, 255):
        im = np.full((9, 13, 3), v, np.uint8)
        np.testing.assert_array_equal(R.blur_u8(im), im)


def test_iou_hand_cases():
    a = np.array([[10, 20, 50, 80]], np.float32)
    assert R.calc_iou_np(a, a)[0] == 1.0
    assert R.calc_iou_np(a, np.array([[60, 20, 90, 80]], np.float32))[0] == 0.0          # disjoint
    assert R.calc_iou_np(a, np.array([[50, 20, 90, 80]], np.float32))[0] == 0.0          # touching
    z = np.zeros((1, 4), np.float32)
    assert R.calc_iou_np(z, z)[0] == 0.0                                                 # zero union
    half = R.calc_iou_np(a, np.array([[10, 20, 30, 80]], np.float32))[0]
    assert half == 0.5


def test_unflip():
    b = np.array([[1, 2, 3, 7], [0, 0, 0, 0]], np.float32)
    np.testing.assert_array_equal(R.unflip(b, 10), [[1, 3, 3, 8], [0, 10, 0, 10]])
    assert R.unflip(b, 10).dtype == np.float32


def _synthetic(rng, N, M, valid):
    y1 = rng.uniform(0, 100, (N, M)).astype(np.float32)
    x1 = rng.uniform(0, 200, (N, M)).astype(np.float32)
    hh = rng.uniform(1, 40, (N, M)).astype(np.float32)
    ww = rng.uniform(1, 60, (N, M)).astype(np.float32)
    b = np.round(np.stack([y1, x1, y1 + hh, x1 + ww], -1) * 4).astype(np.float32) / 4      # (quarters: W - x is exact)
    b[:, valid:] = 0                                                                      # padded rows
    return b


def test_scores_identical_variants_give_one_and_pad_rows_zero():
    rng = np.random.default_rng(3)
    N, M, W = 2, 10, 250
    boxes = _synthetic(rng, N, M, 7)
    cls = rng.integers(0, 5, (N, M)).astype(np.float32)
    flipped = np.stack([R.unflip(boxes[i], W) for i in range(N)])                        # flipping twice = identity
    iou, agree = R.consistency_scores(boxes, [(flipped, cls), (boxes, cls), (boxes, cls)], [W, W])
    np.testing.assert_array_equal(iou[:, :7], 1.0)
    np.testing.assert_array_equal(iou[:, 7:], 0.0)                                       # zero boxes: zero unions
    np.testing.assert_array_equal(agree, True)                                           # 3 x the same id: divisible by 3


def test_scores_disjoint_variants_give_zero():
    rng = np.random.default_rng(4)
    boxes = _synthetic(rng, 1, 6, 6)
    far = boxes + np.float32(1000)
    cls = np.zeros((1, 6), np.float32)
    iou, _ = R.consistency_scores(boxes, [(far, cls), (far, cls), (far, cls)], [5000])
    np.testing.assert_array_equal(iou, 0.0)


def test_scores_mean_of_three_maxima():
    a = np.array([[[0, 0, 10, 10], [0, 0, 0, 0]]], np.float32)
    half = np.array([[[0, 0, 10, 5], [0, 0, 0, 0]]], np.float32)
    cls = np.zeros((1, 2), np.float32)
    flip_of_a = R.unflip(a[0], 10)[None]
    iou, _ = R.consistency_scores(a, [(flip_of_a, cls), (half, cls), (a, cls)], [10])
    assert iou[0, 0] == (1.0 + 0.5 + 1.0) / 3.0
    assert iou.dtype == np.float64


def test_class_agreement_is_rankwise_divisibility():
    rng = np.random.default_rng(5)
    N, M = 3, 40
    boxes = _synthetic(rng, N, M, M)
    cls = [rng.integers(0, 9, (N, M)).astype(np.float32) for _ in range(3)]
    _, agree = R.consistency_scores(boxes, [(boxes, c) for c in cls], [300] * N)
    want = ((cls[0] + cls[1] + cls[2]).astype(np.int64) % 3) == 0
    np.testing.assert_array_equal(agree, want)
    assert agree.any() and not agree.all()


def test_records_carry_consistency_columns_in_reference_position():
    from uda_amd import writers
    M, C = 4, 3
    un = dict(boxes=np.arange(M * 4, dtype=np.float32).reshape(1, M, 4), scores=np.array([[0.9, 0.5, 0.2, 0.0]], np.float32),
              classes=np.array([[1, 2, 1, 0]], np.float32), logits=np.zeros((1, M, C), np.float32),
              entropy=np.zeros((1, M), np.float32), probab=np.full((1, M, C), 1 / 3, np.float32))
    iou = np.array([[2 / 3, 0.25, 0.0, 0.0]], np.float64)
    agree = np.array([[True, False, True, True]])
    recs = writers.prediction_records(un, ["img"], 0.3, consistency=(iou, agree))
    assert len(recs) == 2
    keys = list(recs[0])
    assert keys[keys.index("class") + 1:keys.index("class") + 4] == ["cons_iou", "cons_cls", "logits"]
    assert recs[0]["cons_iou"] == 2 / 3 and type(recs[0]["cons_iou"]) is float
    assert recs[0]["cons_cls"] is True and recs[1]["cons_cls"] is False
    line = str(recs[0])
    assert "'class': 1.0, 'cons_iou': 0.6666666666666666, 'cons_cls': True, 'logits': " in line
    plain = writers.prediction_records(un, ["img"], 0.3)
    assert all("cons_iou" not in r and "cons_cls" not in r for r in plain)


def test_consistency_ssl_is_a_default_key_with_a_stated_handling():
    from uda_amd import hparams_config as hp, plan as plan_mod
    assert hp.default_detection_configs().as_dict()["consistency_ssl"] is False
    assert plan_mod.MODEL_PARAM_HANDLING["consistency_ssl"].startswith("consumed")
    p = make_params(consistency_ssl=True)
    pl = plan_mod.Plan(p, make_weights(p), chunk_images=1, max_images=4)
    assert "consistency_ssl" not in pl.unknown_keys


def test_other_drivers_refuse_consistency():
    from uda_amd import dist, infer_lib
    for cls in (infer_lib.EnsembleDriver, dist.SampleShardedDriver):
        obj = cls.__new__(cls)
        with pytest.raises(NotImplementedError):
            obj.serve_consistency(np.zeros((1, 8, 8, 3), np.uint8))
