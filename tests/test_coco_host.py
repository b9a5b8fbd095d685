"""The host half of the COCO metric (`uda_amd.coco_metric`: CocoAccumulator, EvaluationMetric; reference coco_metric.py:59-283,
custom_cocoeval.py:351-545) without a GPU: fed the records the reference's own matching produced (tests/golden/coco_eval_golden.npz)
the accumulator reproduces the reference's precision / recall / scores / stats / per-class AP bit for bit; merging is independent of
batching and arrival order; the loop-level restatement tests/coco_ref.py is pinned to the same fixture (matching included) and
then serves as the reference on random data; the refusals; header = binding = library for the new symbols."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import coco_ref as R
from common import ROOT
from uda_amd import capi
from uda_amd import coco_metric as CM

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_eval_golden.npz"))
DATASETS = ("a", "b")
SETS = ("all", "std")
NEW_SYMBOLS = ("uda_set_eval_ground_truth", "uda_eval_match", "uda_get_eval_records", "uda_eval_match_np")


def g(ds, key):
    return GOLD["%s_%s" % (ds, key)]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def accumulator(ds, tag, order=None, parts=1):
    """The fixture's reference records in `parts` accumulators, images arriving in `order`."""
    C = int(g(ds, "num_classes"))
    n = g(ds, "det").shape[0]
    order = list(range(n)) if order is None else list(order)
    gc = R.gt_class_counts(g(ds, "gt"), C)
    accs = []
    for chunk in np.array_split(np.asarray(order), parts):
        acc = CM.CocoAccumulator(C, g(ds, "iou_thrs_" + tag))
        acc.add(g(ds, "image_ids")[chunk], g(ds, "rec_" + tag)[chunk], g(ds, "npig_" + tag)[chunk], g(ds, "used")[chunk], gc[chunk])
        accs.append(acc)
    return accs


def test_constants_match_the_restatement():
    assert CM.RECORD_DTYPE == R.RECORD_DTYPE and CM.RECORD_DTYPE.itemsize == 44
    assert np.array_equal(CM.STD_IOU_THRS, g("a", "iou_thrs_std")) and np.array_equal(CM.ALL_IOU_THRS, g("a", "iou_thrs_all"))
    assert np.array_equal(CM.REC_THRS, R.REC_THRS) and list(CM.MAX_DETS) == R.MAX_DETS


@pytest.mark.parametrize("ds", DATASETS)
@pytest.mark.parametrize("tag", SETS)
def test_accumulator_reproduces_reference_exactly(ds, tag):
    acc, = accumulator(ds, tag)
    ev = acc.accumulate()
    np.testing.assert_array_equal(ev["category_ids"], g(ds, "category_ids"))
    for key in ("precision", "recall", "scores"):
        want = g(ds, "%s_%s" % (key, tag))
        assert ev[key].shape == want.shape
        assert np.array_equal(bits(ev[key]), bits(want)), key
    assert np.array_equal(bits(acc.summarize(ev)), bits(g(ds, "stats_" + tag)))
    assert (ev["precision"] > -1).any()
    if ds == "b":                      # a cell without a single non-ignored ground-truth row stays -1
        assert (ev["precision"] == -1).any()


@pytest.mark.parametrize("ds", DATASETS)
def test_per_class_ap_and_metric_vector(ds):
    C = int(g(ds, "num_classes"))
    acc, = accumulator(ds, "std")
    ap = acc.per_class_ap({k: "class%d" % k for k in range(1, C + 1)})
    metrics = np.array(np.concatenate((acc.summarize(), ap)), dtype=np.float32)
    np.testing.assert_array_equal(metrics, g(ds, "metrics"))
    np.testing.assert_array_equal(metrics[12:], g(ds, "per_class_ap"))
    if ds == "b":                      # classes nobody labelled stay 0, as in the reference
        assert all(metrics[12 + k - 1] == 0 for k in (4, 6, 8, 9, 10))
        assert metrics[12 + 7 - 1] == -1        # every ground-truth row of class 7 is a crowd: a category, but nothing to find


@pytest.mark.parametrize("ds", DATASETS)
def test_merge_is_independent_of_batching_and_order(ds):
    whole, = accumulator(ds, "all")
    want = whole.accumulate()
    n = g(ds, "det").shape[0]
    order = np.random.default_rng(5).permutation(n)
    first, second, third = accumulator(ds, "all", order, parts=3)
    merged = pickle.loads(pickle.dumps(second)).merge(third).merge(pickle.loads(pickle.dumps(first)))
    got = merged.accumulate()
    for key in ("precision", "recall", "scores"):
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    with pytest.raises(ValueError, match="image ids in both"):
        merged.merge(first)
    with pytest.raises(ValueError, match="added before"):
        merged.add(g(ds, "image_ids"), g(ds, "rec_all"), g(ds, "npig_all"), g(ds, "used"))
    with pytest.raises(ValueError, match="different class counts or thresholds"):
        merged.merge(CM.CocoAccumulator(int(g(ds, "num_classes")), CM.STD_IOU_THRS))


def test_one_pass_of_29_thresholds_splits_into_both_sets():
    """EvaluationMetric matches COCOeval_all's 19 thresholds and the 10 standard ones as bits 0..18 and 19..28 of one record."""
    ds = "a"
    C = int(g(ds, "num_classes"))
    rec = g(ds, "rec_all").copy()
    for f in ("matched", "ignored"):
        rec[f] |= g(ds, "rec_std")[f] << np.uint32(19)
    acc = CM.CocoAccumulator(C, np.concatenate([CM.ALL_IOU_THRS, CM.STD_IOU_THRS]))
    acc.add(g(ds, "image_ids"), rec, g(ds, "npig_all"), g(ds, "used"), R.gt_class_counts(g(ds, "gt"), C))
    assert np.array_equal(bits(acc.accumulate(np.arange(19))["precision"]), bits(g(ds, "precision_all")))
    ev = acc.accumulate(np.arange(19, 29))
    assert np.array_equal(bits(ev["precision"]), bits(g(ds, "precision_std")))
    assert np.array_equal(bits(acc.summarize(ev)), bits(g(ds, "stats_std")))


# ------------------------------------------------------------------ the restatement, pinned to the reference
@pytest.mark.parametrize("ds", DATASETS)
@pytest.mark.parametrize("tag", SETS)
def test_restatement_matches_reference_records(ds, tag):
    C = int(g(ds, "num_classes"))
    rec, npig, used = R.match(g(ds, "det"), g(ds, "gt"), C, g(ds, "iou_thrs_" + tag))
    want, ev = g(ds, "rec_" + tag), g(ds, "evaluated")
    np.testing.assert_array_equal(used, g(ds, "used"))
    np.testing.assert_array_equal(rec["rank"], want["rank"])
    np.testing.assert_array_equal(rec["cls"], want["cls"])
    np.testing.assert_array_equal(rec["score"], want["score"])
    for f in ("matched", "ignored"):
        np.testing.assert_array_equal(rec[f][ev], want[f][ev])
    np.testing.assert_array_equal(npig[used > 0], g(ds, "npig_" + tag)[used > 0])
    np.testing.assert_array_equal(R.image_ids_of(g(ds, "det"))[used > 0], g(ds, "image_ids")[used > 0]) if ds == "b" else None


def test_restatement_accumulate_matches_reference():
    ds, tag = "a", "std"
    C = int(g(ds, "num_classes"))
    ev = R.accumulate(g(ds, "image_ids"), g(ds, "rec_" + tag), g(ds, "npig_" + tag), g(ds, "used"), R.gt_class_counts(g(ds, "gt"), C),
                      list(range(10)))
    for key in ("precision", "recall", "scores"):
        assert np.array_equal(bits(ev[key]), bits(g(ds, "%s_%s" % (key, tag)))), key
    assert np.array_equal(bits(R.summarize(ev, g(ds, "iou_thrs_std"))), bits(g(ds, "stats_std")))


def random_batch(seed, n=5, M=40, G=12, C=4):
    rng = np.random.default_rng(seed)
    gt = np.zeros((n, G, 7), np.float32)
    gt[:, :, 6] = -1
    det = np.zeros((n, M, 7), np.float32)
    det[:, :, 6] = -1
    for i in range(n):
        ng, nd = int(rng.integers(0, G + 1)), int(rng.integers(0, M + 1))
        xy, wh = rng.integers(0, 200, (ng, 2)), rng.integers(4, 120, (ng, 2))
        gt[i, :ng, 0], gt[i, :ng, 1], gt[i, :ng, 2], gt[i, :ng, 3] = xy[:, 1], xy[:, 0], xy[:, 1] + wh[:, 1], xy[:, 0] + wh[:, 0]
        gt[i, :ng, 4] = rng.random(ng) < 0.15
        gt[i, :ng, 6] = rng.integers(1, C + 1, ng)
        for r in range(nd):
            if ng and rng.random() < 0.7:
                k = int(rng.integers(0, ng))
                box = [gt[i, k, 1] + rng.integers(-5, 6), gt[i, k, 0] + rng.integers(-5, 6), wh[k, 0] + rng.integers(-3, 4), wh[k, 1] + rng.integers(-3, 4)]
                cls = gt[i, k, 6]
            else:
                box = [*rng.integers(0, 200, 2), *rng.integers(4, 120, 2)]
                cls = rng.integers(0, C + 2)
            det[i, r] = [-1, *box, np.round(rng.random(), 1), cls]
    return gt, det


@pytest.mark.parametrize("seed", [1, 2])
def test_accumulator_equals_restatement_on_random_data(seed):
    C = 4
    gt, det = random_batch(seed, C=C)
    thrs = CM.STD_IOU_THRS
    rec, npig, used = R.match(det, gt, C, thrs)
    ids = R.image_ids_of(det)
    gc = R.gt_class_counts(gt, C)
    acc = CM.CocoAccumulator(C, thrs)
    acc.add(ids, rec, npig, used, gc)
    got, want = acc.accumulate(), R.accumulate(ids, rec, npig, used, gc, list(range(10)))
    np.testing.assert_array_equal(got["category_ids"], want["category_ids"])
    for key in ("precision", "recall", "scores"):
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    assert np.array_equal(bits(acc.summarize(got)), bits(R.summarize(want, thrs)))
    np.testing.assert_array_equal(CM.gt_class_counts(gt, C), gc)


@pytest.mark.parametrize("ds", DATASETS)
def test_evaluation_metric_end_to_end_with_the_restatement_as_matcher(ds, monkeypatch):
    """update_state -> result() with tests/coco_ref.match standing in for the device match: image ids, the running counter, the
    29-threshold pass, ground-truth class counts and the returned pair equal what the reference's evaluate() returned."""
    monkeypatch.setattr(CM, "match_np", lambda det, gt, C, thrs=None, device=0: R.match(det, gt, C, thrs))
    C = int(g(ds, "num_classes"))
    m = CM.EvaluationMetric(label_map={k: "class%d" % k for k in range(1, C + 1)}, apiou_curve=True)
    for lo, hi in g(ds, "batches"):
        m.update_state(g(ds, "gt")[lo:hi], g(ds, "det")[lo:hi])
    assert sorted(m.accumulator.images) == sorted(int(v) for v in g(ds, "image_ids")[g(ds, "used") > 0])
    metrics, precision_all = m.result()
    assert metrics.dtype == np.float32
    np.testing.assert_array_equal(metrics, g(ds, "metrics"))
    assert np.array_equal(bits(precision_all), bits(g(ds, "curve_precision")))
    assert m.result()[0] is metrics
    m.reset_states()
    assert not m.accumulator.images and m.image_id == 1


# ------------------------------------------------------------------ refusals
def test_evaluation_metric_refusals():
    with pytest.raises(ValueError, match="COCO JSON"):
        CM.EvaluationMetric(filename="instances_val2017.json")
    with pytest.raises(ValueError, match="test-dev"):
        CM.EvaluationMetric(testdev_dir="testdev")
    with pytest.raises(ValueError, match="label_map"):
        CM.EvaluationMetric(label_map="kitti")
    m = CM.EvaluationMetric(label_map={1: "car", 2: "van", 3: "truck"})
    assert m.num_classes == 3 and m.iou_thrs.size == 29 and m.metric_names == CM.METRIC_NAMES
    assert CM.EvaluationMetric(apiou_curve=False).iou_thrs.size == 10
    with pytest.raises(ValueError, match="no image"):
        m.evaluate()
    gt, det = random_batch(3, C=3)
    bad = gt.copy(); bad[0, 0, 6] = 4
    with pytest.raises(ValueError, match="whole numbers in 1..3"):
        m.update_state(bad, det)
    bad = gt.copy(); bad[0, 0, 6] = 0
    with pytest.raises(ValueError, match="whole numbers in 1..3"):
        m.update_state(bad, det)
    bad = gt.copy(); bad[0, 0, 6] = 1.5
    with pytest.raises(ValueError, match="whole numbers"):
        m.update_state(bad, det)
    bad = gt.copy(); bad[0, 0, 6] = 1; bad[0, 0, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        m.update_state(bad, det)
    with pytest.raises(ValueError, match="at most %d" % capi.EVAL_MAX_GT):
        m.update_state(np.zeros((1, capi.EVAL_MAX_GT + 1, 7), np.float32), det[:1])
    with pytest.raises(ValueError, match=r"\[n, G, 7\]"):
        m.update_state(gt[:, :, :6], det)
    with pytest.raises(ValueError, match=r"\[n, M, 7\]"):
        m.update_state(gt, det[:, :, :6])
    with pytest.raises(ValueError, match="thresholds"):
        CM.check_iou_thrs(np.linspace(0, 1, 33))


def test_header_binding_and_library_have_the_new_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uda_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(uda_[a-z0-9_]+)\s*\(", src))
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    assert "#define UDA_EVAL_MAX_GT %d" % capi.EVAL_MAX_GT in src and "#define UDA_EVAL_MAX_THRS %d" % capi.EVAL_MAX_THRS in src
    assert capi.EVAL_MAX_GT >= 100
