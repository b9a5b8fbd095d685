"""The services on resident detections when their buffers grow, are reused and are read twice (`uda_set_ground_truth`,
`uda_set_eval_ground_truth`, the result packs and their first-reader fetch in csrc/uda_services.hip): ground truth of 1, then 6
(the buffers grow), then 2 rows per image (the larger buffers are reused) through `assign_ground_truth`, `label_check` and
`eval_match`, each step bit for bit against the handle-free twin on the downloaded detections; and every raw getter read twice
on the same handle, then once more after the service was queued again with other arguments."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_glc as TG
import test_gpu_validate as TV
from common import PLAIN, make_images

pytestmark = pytest.mark.gpu

GS = (1, 6, 2)                   # rows per image: the first allocation, growth, reuse of the larger buffers
METHODS = ("md", "mistakes", "noisy")


@pytest.fixture(scope="module")
def plain():
    d = TV._driver(PLAIN)
    det = d.serve(make_images(2, *TV.RAW, seed=3))
    yield d, det
    d.close()


@pytest.fixture(scope="module")
def cons():
    d = TG._driver(consistency_ssl=True)
    det, iou, _ = d.serve_consistency(make_images(2, *TG.RAW, seed=3))
    yield d, det, iou
    d.close()


def class_ids(det):
    return det[2] if det[2].ndim == 2 else det[2][..., 0]


def ground_truth(det, G, seed):
    """[n, G, 4] / [n, G] from the run's own detections: jittered copies with the detections' classes, from three rows on a box
    far from everything, and above one row a last row of padding."""
    rng = np.random.default_rng(seed)
    boxes, valid, cls = det[0][..., :4], det[3], class_ids(det)
    n = len(valid)
    gb, gc = np.full((n, G, 4), -1, np.float32), np.full((n, G), -1, np.float32)
    k = max(G - 1, 1)
    for i in range(n):
        ranks = rng.integers(0, max(int(valid[i]), 1), k)
        gb[i, :k] = boxes[i, ranks] + rng.normal(0, 0.5, (k, 4)).astype(np.float32)
        gc[i, :k] = np.maximum(cls[i, ranks], 1)
        if k >= 3:
            gb[i, 2] = (5000, 5000, 5100, 5200)
    return gb, gc


def eval_ground_truth(gb, gc):
    gt = np.zeros(gc.shape + (7,), np.float32)
    gt[..., :4], gt[..., 6] = gb, gc
    return gt


def same_bits(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        assert a.tobytes() == b.tobytes(), (what, k)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ the raw getters, as the wrappers call them
def raw_assignment(d, n, G):
    idx, iou, count = np.full((n, G), -1, np.int32), np.zeros((n, G), np.float64), np.zeros((n,), np.int32)
    d._ck(d._lib.uda_get_assignment(d._h, ptr(idx), ptr(iou), ptr(count)), "uda_get_assignment")
    cols = C.c_int32()
    d._ck(d._lib.uda_assigned_row_cols(d._h, C.byref(cols)), "uda_assigned_row_cols")
    table = np.empty((int(count.sum()), cols.value), np.float32)
    d._ck(d._lib.uda_get_assigned_rows(d._h, ptr(table), table.size), "uda_get_assigned_rows")
    return idx, iou, count, table


def raw_label_check(d, n, G):
    from uda_amd import label_correction as lc
    res = lc.empty_result(n, d.M, G)
    d._ck(d._lib.uda_get_label_check(d._h, *[ptr(res[k]) for k in lc.RESULT_ORDER]), "uda_get_label_check")
    return tuple(res[k] for k in lc.RESULT_ORDER)


def raw_eval(d, n):
    from uda_amd import coco_metric as cm
    rec, npig, used = np.zeros((n, d.M), cm.RECORD_DTYPE), np.zeros((n, d.num_classes, 4), np.int32), np.zeros((n,), np.int32)
    d._ck(d._lib.uda_get_eval_records(d._h, ptr(rec), ptr(npig), ptr(used)), "uda_get_eval_records")
    return rec, npig, used


def raw_scores(d, n, n_comp):
    comp, count, cls = np.zeros((n, n_comp), np.float64), np.zeros((n,), np.int32), np.zeros((n, d.num_classes), np.int32)
    d._ck(d._lib.uda_get_image_scores(d._h, ptr(comp), ptr(count), ptr(cls)), "uda_get_image_scores")
    return comp, count, cls


def raw_pseudo(d, n, K):
    from uda_amd import pseudo_labels as pl
    rec, minmax = np.zeros((K,), pl.RECORD_DTYPE), np.zeros((n, 2), np.float64)
    kept, cand = np.zeros((n,), np.int32), np.zeros((n,), np.int32)
    d._ck(d._lib.uda_get_pseudo_rows(d._h, ptr(rec), K, ptr(minmax), ptr(kept), ptr(cand)), "uda_get_pseudo_rows")
    return rec, minmax, kept, cand


# ------------------------------------------------------------------ the twins on the downloaded detections
def check_assign(d, det, gb, gc, method, keep="validate"):
    from uda_amd import utils_extra as U
    asg = d.assign_ground_truth(gb, gc, method=method, keep=keep)
    idx, iou, count = U.assign_gt_boxes(method, gb, gc, det[0], keep=keep)
    same_bits((asg["det_index"], asg["iou"], asg["count"]), (idx, iou, count), "assign G %d" % gc.shape[1])
    im, row = np.nonzero(idx >= 0)
    np.testing.assert_array_equal(asg["boxes"], det[0][im, idx[im, row], :4])
    np.testing.assert_array_equal(asg["scores"], det[1][im, idx[im, row]])
    return asg


def check_label(d, det, cons_iou, gb, gc, methods, min_score, **thr):
    from uda_amd import label_correction as lc
    chk = d.label_check(gb, gc, methods=methods, min_score=min_score, **thr)
    want = lc.check_labels(det[0][..., :4], det[1], cons_iou, gb, gc, classes=class_ids(det), methods=methods, min_score=min_score,
                           as_float32=True, **thr)
    np.testing.assert_array_equal(chk.counts, want.counts)
    for k in ("wrong_gt", "extra_correct_dets", "matched_det", "noisy_rows", "replaced", "pred_ranks"):
        for a, b in zip(getattr(chk, k), getattr(want, k)):
            np.testing.assert_array_equal(a, b, err_msg=k)
    for a, b in zip(chk.ious_gt + chk.det_max_iou, want.ious_gt + want.det_max_iou):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert chk.corrected_gt_boxes == want.corrected_gt_boxes
    raw = lc.label_check_np(det[0][..., :4], det[1], cons_iou, gb, gc, min_score, methods=methods, as_float32=True, **thr)
    same_bits(raw_label_check(d, *gc.shape), tuple(raw[k] for k in lc.RESULT_ORDER), "label check G %d" % gc.shape[1])
    return chk


def check_eval(d, det, gt, thrs=None):
    from uda_amd import coco_metric as cm, postprocess as pp
    got = d.eval_match(gt, thrs)
    want = cm.match_np(pp.transform_detections(d.legacy_rows(det)), gt, d.num_classes, thrs)
    same_bits(got, want, "eval G %d" % gt.shape[1])
    return got


# ------------------------------------------------------------------ growth and reuse
def test_plain_driver_grows_and_reuses(plain):
    d, det = plain
    min_score = float(np.median(det[1][det[1] > 0]))       # (padded slots score 0)
    matched = mistakes = hits = 0
    for step, G in enumerate(GS):
        gb, gc = ground_truth(det, G, seed=step)
        matched += int(check_assign(d, det, gb, gc, ("IoU", "MSE", "rank")[step])["count"].sum())
        mistakes += int(check_label(d, det, None, gb, gc, ("mistakes",), min_score).counts[:, 2].sum())
        rec = check_eval(d, det, eval_ground_truth(gb, gc))[0]
        hits += int((rec["matched"][rec["rank"] >= 0][:, 0] != 0).sum())
    assert matched >= 2 * sum(max(G - 1, 1) for G in GS) and mistakes > 0 and hits > 0


def test_consistency_driver_grows_and_reuses(cons):
    d, det, cons_iou = cons
    min_score = float(np.median(det[1]))
    thr = dict(iou_consist=float(np.median(cons_iou[det[1] > min_score])), correct_score=min_score)
    seen = np.zeros(5, np.int64)
    for step, G in enumerate(GS):
        gb, gc = ground_truth(det, G, seed=10 + step)
        # the label check first: here IT is the call that makes uda_set_ground_truth grow the buffers of the assignment
        seen += check_label(d, det, cons_iou, gb, gc, METHODS, min_score, **thr).counts.sum(0)
        check_assign(d, det, gb, gc, ("MSE", "IoU", "IoU")[step], keep=("validate", "calibrate", "validate")[step])
    assert seen[0] > 0 and seen[1] == 2 * sum(max(G - 1, 1) for G in GS)


def test_growth_behind_an_assignment_retires_it(plain):
    """Ground truth with more rows than the buffers hold frees the pack the last assignment lies in: nothing is left to read."""
    d, det = plain
    gb, gc = ground_truth(det, 3, seed=5)
    check_assign(d, det, gb, gc, "IoU")
    gb, gc = ground_truth(det, 9, seed=6)
    check_label(d, det, None, gb, gc, ("mistakes",), float(np.median(det[1][det[1] > 0])))
    idx, iou, count = np.zeros((2, 9), np.int32), np.zeros((2, 9), np.float64), np.zeros((2,), np.int32)
    assert d._lib.uda_get_assignment(d._h, ptr(idx), ptr(iou), ptr(count)) == 1
    assert b"no assignment" in d._lib.uda_last_error(d._h)
    check_assign(d, det, gb, gc, "MSE")


# ------------------------------------------------------------------ reading twice, and again after another queue
def test_getters_read_twice_and_follow_a_new_queue(plain):
    from uda_amd import active_learning as AL, pseudo_labels as PL
    d, det = plain
    n = det[0].shape[0]
    cols = dict(boxes=det[0][..., :4], scores=det[1], classes=class_ids(det))
    lo, hi = (float(np.quantile(det[1][det[1] > 0], q)) for q in (0.25, 0.75))      # (padded slots score 0)
    gts = [ground_truth(det, 4, seed=20), ground_truth(det, 3, seed=21)]

    asg = check_assign(d, det, *gts[0], "IoU")
    first = raw_assignment(d, n, 4)
    same_bits(first[:3], (asg["det_index"], asg["iou"], asg["count"]), "assignment")
    same_bits(raw_assignment(d, n, 4), first, "assignment, second read")
    asg = check_assign(d, det, *gts[1], "MSE")
    same_bits(raw_assignment(d, n, 3)[:3], (asg["det_index"], asg["iou"], asg["count"]), "assignment, queued again")

    for m, (gb, gc) in zip((lo, hi), gts):                  # (check_label reads the raw getter against the twin itself)
        check_label(d, det, None, gb, gc, ("mistakes",), m)
        first = raw_label_check(d, *gc.shape)
        same_bits(raw_label_check(d, *gc.shape), first, "label check, second read")

    for thrs, (gb, gc) in zip((None, [0.3, 0.6]), gts):
        got = check_eval(d, det, eval_ground_truth(gb, gc), thrs)
        same_bits(raw_eval(d, n), got, "eval records")
        same_bits(raw_eval(d, n), got, "eval records, second read")

    st = AL.resolve_strategy("foo", d.params)              # (a key no prediction line holds: the reference's fallback, det_score)
    kept = []
    for m in (lo, hi):
        got = d.score_images(st, m)
        same_bits(got, AL.score_detections(cols, st, m, num_classes=d.num_classes, as_float32=True), "scores")
        same_bits(raw_scores(d, n, st.n_comp), got, "scores, first raw read")
        same_bits(raw_scores(d, n, st.n_comp), got, "scores, second read")
        kept.append(int(got[1].sum()))
    assert kept[0] > kept[1] > 0

    sel = PL.resolve_selection("score", d.params)
    cand = []
    for m, tau in ((lo, lo), (lo, hi)):
        got = d.pseudo_rows(sel, tau, min_score=m)
        same_bits(got, PL.select_detections(cols, sel, tau, m, num_classes=d.num_classes, as_float32=True), "pseudo rows")
        same_bits(raw_pseudo(d, n, len(got[0])), got, "pseudo rows, first raw read")
        same_bits(raw_pseudo(d, n, len(got[0])), got, "pseudo rows, second read")
        cand.append(len(got[0]))
    assert cand[0] > cand[1] > 0
