"""COCO matching on the device (`uda_eval_match_np`, `ServingDriver.eval_match` / `serve_eval`, `coco_metric.EvaluationMetric`;
reference coco_metric.py:59-283, custom_cocoeval.py:265-545): the kernel against what the reference's own evaluateImg produced
(tests/golden/coco_eval_golden.npz) bit for bit, the metric end to end against the reference's evaluate(), the resident layout
against the legacy-row layout on the detections of the same run, and the refusals."""
import os

import numpy as np
import pytest

from common import PLAIN, make_images, make_params, make_weights

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_eval_golden.npz"))
SIZE = "192x128"
RAW = (100, 180)
# the seeded weights score every anchor between 0.009 and 0.02: this threshold ends the lists early, so images carry padded rows
NMS = dict(nms_configs=dict(method="gaussian", iou_thresh=None, score_thresh=0.0125, sigma=None, pyfunc=False,
                            max_nms_inputs=0, max_output_size=100))


def g(ds, key):
    return GOLD["%s_%s" % (ds, key)]


def assert_records_equal(got, want, where=None):
    for f in ("score", "cls", "rank"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    for f in ("matched", "ignored"):
        a, b = (got[f], want[f]) if where is None else (got[f][where], want[f][where])
        np.testing.assert_array_equal(a, b, err_msg=f)


# ------------------------------------------------------------------ the kernel against the reference's own results
@pytest.mark.parametrize("ds", ["a", "b"])
@pytest.mark.parametrize("tag", ["all", "std"])
def test_match_np_equals_reference_records(ds, tag):
    from uda_amd import coco_metric as CM
    rec, npig, used = CM.match_np(g(ds, "det"), g(ds, "gt"), int(g(ds, "num_classes")), g(ds, "iou_thrs_" + tag))
    want = g(ds, "rec_" + tag)
    np.testing.assert_array_equal(used, g(ds, "used"))
    assert_records_equal(rec, want, g(ds, "evaluated"))
    ev = used > 0
    np.testing.assert_array_equal(npig[ev], g(ds, "npig_" + tag)[ev])
    assert (rec["rank"] >= 100).any() == (ds == "b")
    big = rec["rank"] >= 100
    assert (rec["matched"][big] == 0).all() and (rec["ignored"][big] == 0).all()


def test_match_np_one_pass_of_29_thresholds():
    from uda_amd import coco_metric as CM
    ds = "b"
    thr = np.concatenate([CM.ALL_IOU_THRS, CM.STD_IOU_THRS])
    rec, npig, used = CM.match_np(g(ds, "det"), g(ds, "gt"), int(g(ds, "num_classes")), thr)
    ev = g(ds, "evaluated")
    for f in ("matched", "ignored"):
        want = g(ds, "rec_all")[f] | (g(ds, "rec_std")[f] << np.uint32(19))
        np.testing.assert_array_equal(rec[f][ev], want[ev], err_msg=f)


@pytest.mark.parametrize("ds", ["a", "b"])
def test_evaluation_metric_equals_reference(ds):
    from uda_amd import coco_metric as CM
    C = int(g(ds, "num_classes"))
    m = CM.EvaluationMetric(label_map={k: "class%d" % k for k in range(1, C + 1)}, apiou_curve=True)
    for lo, hi in g(ds, "batches"):
        m.update_state(g(ds, "gt")[lo:hi], g(ds, "det")[lo:hi])
    metrics, precision_all = m.result()
    assert metrics.dtype == np.float32
    np.testing.assert_array_equal(metrics, g(ds, "metrics"))
    assert np.array_equal(np.ascontiguousarray(precision_all).view(np.uint64), g(ds, "curve_precision").view(np.uint64))
    assert m.result()[0] is metrics
    plain = CM.EvaluationMetric(apiou_curve=False, num_classes=C)
    plain.update_state(g(ds, "gt"), g(ds, "det"))
    np.testing.assert_array_equal(plain.result(), g(ds, "stats_std").astype(np.float32))


# ------------------------------------------------------------------ the served flow
@pytest.fixture(scope="module")
def driver():
    from uda_amd.infer_lib import KerasDriver
    p = make_params(image_size=SIZE, **dict(PLAIN, **NMS))
    d = KerasDriver("_", False, p["name"], 2, False, p, weights=make_weights(p, seed=12, cls_spread=20.0))
    yield d
    d.close()


def ground_truth_from(det, G=12):
    """Ground truth taken from the run's own detections (boxes y1 x1 y2 x2, classes): some copied, some shifted by a few pixels, one
    crowd, one box far from everything; padded with class -1."""
    boxes, scores, classes, valid = det[:4]
    n = boxes.shape[0]
    gt = np.zeros((n, G, 7), np.float32)
    gt[:, :, 6] = -1
    for i in range(n):
        k = min(int(valid[i]), G - 2)
        assert k >= 4
        rows = np.arange(k) * max(int(valid[i]) // k, 1)
        gt[i, :k, :4] = boxes[i, rows, :4]
        gt[i, :k, 6] = classes[i, rows]
        gt[i, 1:k:2, :4] += np.float32(3.0)                  # every other one shifted
        gt[i, 2, 4] = 1                                      # a crowd
        gt[i, k, :4] = (5000, 5000, 5040, 5040)              # nobody finds this one
        gt[i, k, 6] = gt[i, 0, 6]
    assert (gt[:, :, 6] != 0).all()
    return gt


@pytest.mark.parametrize("mode", ["per_class", "global"])
def test_serve_eval_equals_match_np_on_the_same_detections(driver, mode):
    from uda_amd import coco_metric as CM
    from uda_amd import postprocess as pp
    d = driver
    imgs = make_images(2, *RAW, seed=4)
    det = d.serve(imgs, post_mode=mode)
    assert 0 < det[3].min() and (det[1] > 0).any()
    gt = ground_truth_from(det)
    ev = CM.EvaluationMetric(apiou_curve=True, num_classes=d.num_classes)
    rows = d.serve_eval(imgs, gt, ev, image_ids=[11, 4], post_mode=mode)
    again = d._collect(2, d._mode(mode))
    for a, b in zip(det, again):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(rows, d.legacy_rows(det, [11, 4]))
    assert rows.shape == (2, d.M, 7) and (rows[:, :, 0] == np.asarray([[11], [4]])).all()
    rec, npig, used = d.eval_match(gt, ev.iou_thrs)
    want = CM.match_np(pp.transform_detections(rows), gt, d.num_classes, ev.iou_thrs)
    assert_records_equal(rec, want[0])
    np.testing.assert_array_equal(npig, want[1])
    np.testing.assert_array_equal(used, want[2])
    ranked = rec[rec["rank"] >= 0]
    assert (ranked["matched"][:, 0] != 0).any(), "no match"
    assert (ranked["matched"][:, 0] == 0).any(), "no miss"
    assert sorted(ev.accumulator.images) == [4, 11]
    for iid, i in ((11, 0), (4, 1)):
        kept = rec[i][(rec[i]["rank"] >= 0) & (rec[i]["rank"] < 100)]
        assert ev.accumulator.images[iid][0].tobytes() == kept.tobytes()
    metrics, _ = ev.result()
    assert metrics.shape == (12,) and 0 < metrics[8] < 1        # ARmax100: some found, the far box never


def test_serve_stream_with_eval_match_while_resident(driver):
    from uda_amd import coco_metric as CM
    d = driver
    batches = [make_images(2, *RAW, seed=s) for s in (4, 6)]
    gts = [ground_truth_from(d.serve(b, post_mode="per_class")) for b in batches]
    ev = CM.EvaluationMetric(apiou_curve=False, num_classes=d.num_classes)
    it = iter(gts)

    def hook(det):
        gt = next(it)
        ev.add_records(None, *d.eval_match(gt, ev.iou_thrs), groundtruth_data=gt)
        return det
    out = list(d.serve_stream(batches, post_mode="per_class", while_resident=hook))
    assert len(out) == 2 and sorted(ev.accumulator.images) == [1, 2, 3, 4]
    one = CM.EvaluationMetric(apiou_curve=False, num_classes=d.num_classes)
    for b, gt in zip(batches, gts):
        d.serve_eval(b, gt, one)
    np.testing.assert_array_equal(ev.result(), one.result())


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable():
    from uda_amd import capi
    from uda_amd import coco_metric as CM
    from uda_amd.infer_lib import KerasDriver, _ptr
    p = make_params(image_size=SIZE, **dict(PLAIN, **NMS))
    d = KerasDriver("_", False, p["name"], 2, False, p, weights=make_weights(p, seed=12, cls_spread=20.0))
    lib, h = d._lib, d._h
    thr = np.ascontiguousarray(CM.STD_IOU_THRS)
    imgs = make_images(2, *RAW, seed=4)

    def refused(rc, text):
        assert rc != 0
        msg = lib.uda_last_error(h).decode()
        assert text in msg, msg

    gt = np.zeros((2, 4, 7), np.float32)
    gt[:, :, 6] = -1
    refused(lib.uda_eval_match(h, _ptr(thr), 10), "no ground truth is set")
    refused(lib.uda_get_eval_records(h, None, None, None), "no match")
    assert lib.uda_set_eval_ground_truth(h, _ptr(gt), 2, 4) == 0
    refused(lib.uda_eval_match(h, _ptr(thr), 10), "no post-process has run yet")
    det = d.serve(imgs, post_mode="per_class")
    refused(lib.uda_eval_match(h, _ptr(thr), 0), "T outside 1..32")
    refused(lib.uda_eval_match(h, _ptr(thr), 33), "T outside 1..32")
    refused(lib.uda_eval_match(h, None, 10), "NULL thresholds")
    assert lib.uda_set_eval_ground_truth(h, _ptr(gt), 1, 4) == 0
    refused(lib.uda_eval_match(h, _ptr(thr), 10), "ground truth of 1 images, the last post-process holds 2")
    big = np.zeros((2, capi.EVAL_MAX_GT + 1, 7), np.float32)
    refused(lib.uda_set_eval_ground_truth(h, _ptr(big), 2, capi.EVAL_MAX_GT + 1), "at most %d" % capi.EVAL_MAX_GT)
    refused(lib.uda_set_eval_ground_truth(h, _ptr(gt), 3, 4), "the handle holds 1..2")
    assert lib.uda_set_eval_ground_truth(h, _ptr(gt), 2, 4) == 0
    d.stage_images(imgs)
    t = d.run_async("per_class")
    refused(lib.uda_eval_match(h, _ptr(thr), 10), "in flight")
    d.collect(t)
    # the handle-free entry point
    rows = np.zeros((1, 8, 7), np.float32)
    out = np.zeros((1, 8), CM.RECORD_DTYPE)
    for args, text in (((1, 8, capi.EVAL_MAX_GT + 1, 3, _ptr(thr), 10), "at most %d" % capi.EVAL_MAX_GT),
                       ((1, 8, 4, 3, _ptr(thr), 33), "T outside 1..32"), ((1, 4097, 4, 3, _ptr(thr), 10), "at most 4096"),
                       ((1, 8, 4, 0, _ptr(thr), 10), "bad argument")):
        assert lib.uda_eval_match_np(0, _ptr(rows), _ptr(big), *args, _ptr(out), None, None) != 0
        assert text in lib.uda_last_error(None).decode()
    with pytest.raises(ValueError, match="at most"):
        d.eval_match(big)
    # and the handle serves and matches as before
    again = d.serve(imgs, post_mode="per_class")
    for a, b in zip(det, again):
        np.testing.assert_array_equal(a, b)
    rec, npig, used = d.eval_match(ground_truth_from(again))
    assert (rec["rank"] >= 0).any() and (used > 0).all() and npig.sum() > 0
    d.close()
