"""Ground-truth assignment on the device (`ServingDriver.serve_validate` / `assign_ground_truth`, `utils_extra.assign_gt_boxes`;
reference utils_extra.py:44-64, validate_model.py:314-470, calibrate_model.py:133-211): the kernel against what the
reference's own functions returned (tests/golden/gt_assign_golden.npz), the served flow against validate_ref applied to the
detections the device produced, the refusals, and the two writer flows against the same flows run on the host."""
import filecmp
import os

import numpy as np
import pytest

import validate_ref as V
from common import FULL_MC, HEAD_MC, LOSS_ATT, PLAIN, make_images, make_params, make_weights

pytestmark = pytest.mark.gpu

SIZE = "256x128"                 # model input 128 x 256
RAW = (140, 260)
SEED = 23
CFGS = {"full_mc": FULL_MC, "head_mc": HEAD_MC, "loss_att": LOSS_ATT, "plain": PLAIN}
# The seeded weights give every image 100 detections with scores between 0.009 and 0.02 (soft-NMS never drops a box at the
# default score_thresh 0): this threshold ends the list early, so that the images carry padded slots (0 < valid_len < M)
NMS = dict(nms_configs=dict(method="gaussian", iou_thresh=None, score_thresh=0.0125, sigma=None, pyfunc=False,
                            max_nms_inputs=0, max_output_size=100))
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_assign_golden.npz"))


def _ragged(seed=9):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (140, 260, 3), dtype=np.uint8), rng.integers(0, 256, (136, 250, 3), dtype=np.uint8)]


def _driver(cfg, batch=2, **over):
    from uda_amd.infer_lib import KerasDriver
    p = make_params(image_size=SIZE, **dict(cfg, **dict(NMS, **over)))
    d = KerasDriver("_", False, p["name"], batch, False, p, weights=make_weights(p, seed=12, cls_spread=20.0))
    d.set_dropout_seed(SEED)
    return d


@pytest.fixture(scope="module", params=list(CFGS))
def driver(request):
    d = _driver(CFGS[request.param])
    yield d
    d.close()


@pytest.fixture(scope="module")
def plain_driver():
    d = _driver(PLAIN)
    yield d
    d.close()


def make_gt(det, G, seed, extra=0):
    """GT from the run's own detections: jittered copies of detections (the last valid one among them), an exact copy of row
    0 (ties with every padded slot), a far-away box, a class-0 row (kept by calibrate only), -1 padding."""
    rng = np.random.default_rng(seed)
    boxes, valid = det[0][..., :4], det[3]
    n = len(valid)
    gb = np.full((n, G, 4), -1, np.float32)
    gc = np.full((n, G), -1, np.float32)
    for i in range(n):
        v = max(int(valid[i]), 1)
        ranks = [v - 1, v // 2, min(3, v - 1)] + list(rng.integers(0, v, extra))
        rows = [boxes[i, k] + rng.normal(0, 0.5, 4).astype(np.float32) for k in ranks]
        rows.insert(2, boxes[i, 0].copy())
        rows.insert(3, np.array([5000, 5000, 5100, 5200], np.float32))
        cls = [float(c) for c in rng.integers(1, 8, len(rows))]
        cls[4] = 0.0
        gb[i, :len(rows)], gc[i, :len(rows)] = np.stack(rows), cls
    return gb, gc


def check_assignment(d, det, asg, gb, gc, method, keep="validate"):
    probab = entropy = None
    if d.params["enable_softmax"]:
        probab, entropy = d.class_probs(det[0].shape[0])
    idx, iou, count = V.assign(method, gb, gc, det[0], keep)
    np.testing.assert_array_equal(asg["det_index"], idx)
    np.testing.assert_array_equal(asg["count"], count)
    assert asg["iou"].dtype == np.float64
    np.testing.assert_allclose(asg["iou"], iou, rtol=0, atol=1e-12)
    want = V.gather(d.params, det, idx, gb, gc, probab, entropy, keep)
    for k in V.COLUMNS + ("gt_boxes", "gt_classes", "image", "gt_row"):
        if want[k] is None:
            assert asg[k] is None, k
        else:
            assert asg[k].shape == want[k].shape and asg[k].dtype == want[k].dtype, k
            np.testing.assert_array_equal(asg[k], want[k], err_msg=k)
    return idx


# ------------------------------------------------------------------ the kernel against the reference's own results
@pytest.mark.parametrize("keep", ["validate", "calibrate"])
@pytest.mark.parametrize("method", V.METHODS)
def test_golden_through_device(method, keep):
    from uda_amd import utils_extra as U
    bit_identical, rows = True, 0
    for ci in range(int(GOLD["n_cases"][0])):
        dets, gtb, gtc = GOLD["c%d_dets" % ci], GOLD["c%d_gt_boxes" % ci], GOLD["c%d_gt_classes" % ci]
        tag = "c%d_%s_%s" % (ci, method, keep)
        if not int(GOLD[tag + "_ok"][0]):
            with pytest.raises(ValueError):
                U.assign_gt_boxes(method, gtb, gtc, dets, keep=keep)
            continue
        idx, iou, count = U.assign_gt_boxes(method, gtb, gtc, dets, keep=keep)
        np.testing.assert_array_equal(idx, GOLD[tag + "_idx"])
        np.testing.assert_array_equal(count, (GOLD[tag + "_idx"] >= 0).sum(1))
        np.testing.assert_allclose(iou, GOLD[tag + "_iou"], rtol=0, atol=1e-12)
        bit_identical &= np.array_equal(iou.view(np.uint64), GOLD[tag + "_iou"].view(np.uint64))
        rows += int(count.sum())
    assert rows > 100
    print("golden %s/%s: %d rows, IoU bit-identical to the reference: %s" % (method, keep, rows, bit_identical))


def test_gt_box_assigner_call_shape():
    from uda_amd import utils_extra as U
    dets, gtb = GOLD["c0_dets"][1], GOLD["c0_gt_boxes"][1]
    for method in V.METHODS:
        want = GOLD["c0_%s_validate_idx" % method][1]
        for i in np.nonzero(want >= 0)[0][:6]:
            assert U.gt_box_assigner(method, gtb, dets, int(i)) == want[i]


# ------------------------------------------------------------------ the served flow
def test_serve_validate(driver):
    from uda_amd import utils_extra as U
    d = driver
    partial = nonzero = False
    for call, (imgs, G, method, keep) in enumerate([(make_images(2, *RAW, seed=3), 12, "IoU", "validate"),
                                                    (_ragged(), 20, "MSE", "validate"),
                                                    (make_images(2, *RAW, seed=5), 7, "IoU", "calibrate"),
                                                    (make_images(1, *RAW, seed=6), 9, "rank", "validate")]):
        want = d.serve(imgs)
        gb, gc = make_gt(want, G, seed=call, extra=G - 7 if G > 7 else 0)
        det, asg = d.serve_validate(imgs, gb, gc, method=method, keep=keep)
        assert len(det) == len(want)
        for g, w in zip(det, want):
            assert g.shape == w.shape and g.dtype == w.dtype
            np.testing.assert_array_equal(g, w)
        idx = check_assignment(d, det, asg, gb, gc, method, keep)
        # the handle path and the handle-free entry point run the same kernel
        i2, u2, c2 = U.assign_gt_boxes(method, gb, gc, det[0], keep=keep)
        np.testing.assert_array_equal(i2, asg["det_index"])
        np.testing.assert_array_equal(c2, asg["count"])
        assert np.array_equal(u2.view(np.uint64), asg["iou"].view(np.uint64))
        # assign_ground_truth on the resident run gives the same again
        again = d.assign_ground_truth(gb, gc, method=method, keep=keep)
        np.testing.assert_array_equal(again["det_index"], asg["det_index"])
        np.testing.assert_array_equal(again["boxes"], asg["boxes"])
        print("valid_len", det[3].tolist(), "matched ranks", idx[idx >= 0].tolist())
        partial |= bool(((det[3] > 0) & (det[3] < d.M)).any())
        nonzero |= bool((idx > 0).any())
        if method == "IoU":
            assert (asg["iou"][:, 3] == 0).all() and (asg["det_index"][:, 3] == 0).all()    # the far-away box: IoU 0, rank 0
            assert (asg["det_index"][:, 2] == 0).all()                                      # the copy of row 0 beats its padded twins
    assert partial, "no image with 0 < valid_len < M: the padded-slot ties were not exercised"
    assert nonzero, "every matched rank is 0"


def test_default_method_is_model_params(plain_driver):
    d = plain_driver
    imgs = make_images(2, *RAW, seed=3)
    det = d.serve(imgs)
    gb, gc = make_gt(det, 8, seed=1)
    assert d.params["assign_gt_box"] == "IoU"
    np.testing.assert_array_equal(d.assign_ground_truth(gb, gc)["det_index"], V.assign("IoU", gb, gc, det[0])[0])
    with pytest.raises(ValueError, match="finite"):
        d.assign_ground_truth(np.where(gb == gb[0, 0, 0], np.nan, gb), gc)
    with pytest.raises(ValueError, match="beyond"):
        d.assign_ground_truth(np.zeros((2, d.M + 1, 4), np.float32), np.ones((2, d.M + 1), np.float32), method="rank")


def test_after_resident_stream_and_consistency(plain_driver):
    d = plain_driver
    imgs = make_images(2, *RAW, seed=7)
    want = d.serve(imgs)
    gb, gc = make_gt(want, 10, seed=2, extra=3)
    ref = V.assign("IoU", gb, gc, want[0])
    assert d.serve_resident(imgs) == 2                     # the 100-row tuple is never downloaded
    asg = d.assign_ground_truth(gb, gc)
    np.testing.assert_array_equal(asg["det_index"], ref[0])
    im, row = np.nonzero(ref[0] >= 0)
    np.testing.assert_array_equal(asg["boxes"], want[0][im, ref[0][im, row], :4])
    seen = []
    for out in d.serve_stream([imgs, imgs[:1]], while_resident=lambda det: (det, d.assign_ground_truth(gb[:det[0].shape[0]], gc[:det[0].shape[0]]))):
        det, a = out
        check_assignment(d, det, a, gb[:det[0].shape[0]], gc[:det[0].shape[0]], "IoU")
        seen.append(int(a["count"].sum()))
    assert len(seen) == 2 and min(seen) > 0
    c = _driver(HEAD_MC, consistency_ssl=True)
    try:
        det, _, _ = c.serve_consistency(imgs)
        gb2, gc2 = make_gt(det, 9, seed=4, extra=2)
        a = c.assign_ground_truth(gb2, gc2, method="MSE")                  # the originals' rows of the 4n resident images
        idx = V.assign("MSE", gb2, gc2, det[0])[0]
        np.testing.assert_array_equal(a["det_index"], idx)
        im, row = np.nonzero(idx >= 0)
        np.testing.assert_array_equal(a["boxes"], det[0][im, idx[im, row], :4])
        np.testing.assert_array_equal(a["logits"], det[4][im, idx[im, row]])
    finally:
        c.close()


def test_ensemble_assigns_in_its_aggregating_handle():
    from uda_amd.infer_lib import EnsembleDriver
    p = make_params(image_size=SIZE, **dict(LOSS_ATT, **NMS))
    ens = EnsembleDriver([make_weights(p, seed=40 + m, cls_spread=20.0) for m in range(2)], p["name"], batch_size=2, model_params=p)
    try:
        imgs = make_images(2, *RAW, seed=14)
        want = ens.serve(imgs)
        gb, gc = make_gt(want, 9, seed=6, extra=2)
        det, asg = ens.serve_validate(imgs, gb, gc, method="MSE")
        for g, w in zip(det, want):
            np.testing.assert_array_equal(g, w)
        idx = check_assignment(ens.post, det, asg, gb, gc, "MSE")
        assert (idx > 0).any()
    finally:
        ens.close()


def test_refusals(plain_driver):
    from uda_amd import capi
    from uda_amd.infer_lib import KerasDriver
    d = plain_driver
    imgs = make_images(2, *RAW, seed=8)
    det = d.serve(imgs)
    gb, gc = make_gt(det, 8, seed=3)
    with pytest.raises(capi.UdaError, match="ground truth of 1 images"):
        d.assign_ground_truth(gb[:1], gc[:1])
    with pytest.raises(ValueError, match="batch of 2"):
        d.serve_validate(imgs, gb[:1], gc[:1])
    d.serve(imgs, post_mode="per_class")
    with pytest.raises(capi.UdaError, match="per class"):
        d.assign_ground_truth(gb, gc)
    d.stage_images(imgs)
    t = d.run_async()
    with pytest.raises(capi.UdaError, match="in flight"):
        d.assign_ground_truth(gb, gc)
    got = d.collect(t)
    np.testing.assert_array_equal(got[0], det[0])
    np.testing.assert_array_equal(d.assign_ground_truth(gb, gc)["det_index"], V.assign("IoU", gb, gc, det[0])[0])   # after uda_collect
    p = d.params
    fresh = KerasDriver("_", False, p["name"], 2, False, p, weights=d.weights)
    try:
        with pytest.raises(capi.UdaError, match="no global post-process"):
            fresh.assign_ground_truth(gb, gc)
    finally:
        fresh.close()


# ------------------------------------------------------------------ the writer flows against the same flows on the host
@pytest.mark.parametrize("name", ["plain", "full_mc"])
def test_validate_to_file_and_gather_detections(tmp_path, name):
    from uda_amd import calibration, writers
    d = _driver(CFGS[name])
    try:
        batches = [make_images(2, *RAW, seed=11), _ragged(12), make_images(1, *RAW, seed=13)]
        dets = [d.serve(b) for b in batches]
        gts = [make_gt(det, G, seed=20 + i, extra=2) for i, (det, G) in enumerate(zip(dets, (9, 14, 8)))]
        names = [["a.png", "b.png"], ["c.png", "d.png"], ["e.png"]]
        occl = [np.arange(g[1].size).reshape(g[1].shape) % 3 for g in gts]
        trunc = [(np.arange(g[1].size).reshape(g[1].shape) % 5).astype(np.float32) / 4 for g in gts]
        box_cal = cls_cal = None
        if name == "full_mc":
            box_cal = calibration.BoxCalibrator(d, {"ts_all": 2.0, "ts_percoo": [1.0, 2.0, 3.0, 4.0]})
            cls_cal = calibration.ClassCalibrator(d, {"ts_all": 1.5}, seed=3)
        host = V.RefDriver(d.params, d.serve, d.class_probs)
        out = {}
        for tag, drv in (("device", d), ("host", host)):
            out[tag] = str(tmp_path / tag)
            f = writers.validate_to_file(drv, batches, gts, names, out[tag], box_calibrator=box_cal, class_calibrator=cls_cal,
                                         occlusions=occl, truncations=trunc)
            assert len(f["names"]) == sum(int((g[1] > 0).sum()) for g in gts)
        files = sorted(os.listdir(out["device"]))
        assert files == sorted(os.listdir(out["host"]))
        assert ("model_performance.txt" in files) == (name == "plain")
        for fn in files:
            if fn != "validationstep_runtime.txt":                      # wall-clock times
                assert filecmp.cmp(os.path.join(out["device"], fn), os.path.join(out["host"], fn), shallow=False), fn
        assert len(open(os.path.join(out["device"], "validate_results.txt")).readlines()) > 10
        got = calibration.gather_detections(d, batches, gts)
        want = calibration.gather_detections(host, batches, gts)
        assert set(got) == set(want) and len(got["iou"]) > 5
        for k in want:
            if want[k] is None:
                assert got[k] is None, k
            else:
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    finally:
        d.close()
