"""The pseudo-label audit on the device (`uda_pseudo_audit_np`, csrc/kernels_audit.hip; `pseudo_audit.audit_np` /
`audit_pseudo_labels`; reference src/ssl_utils/parent.py:1567-1813): the C entry point against the numpy mirror
(tests/audit_ref.py: a stored matrix, the reference's mutating loop) at every wave and block boundary, with planted reductions, a
chain of dependent allocations, ragged batches with empty images, the caps and the refusals, and the reference's own members and
files (tests/golden/audit_golden.npz).  Every output is exact: there is no tolerance anywhere."""
import json
import os

import numpy as np
import pytest

import audit_ref as R
import test_audit_host as H
from uda_amd import capi, pseudo_audit as pa, writers

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257]
OUT = (("gt_max_iou", np.float64, "g"), ("gt_best_det", np.int32, "g"), ("gt_alloc_det", np.int32, "g"), ("gt_flags", np.uint8, "g"),
       ("det_max_iou", np.float64, "d"), ("det_best_gt", np.int32, "d"), ("det_alloc_gt", np.int32, "d"), ("det_alloc_miou", np.float64, "d"),
       ("det_alloc_pair_iou", np.float64, "d"), ("det_flags", np.uint8, "d"), ("n_matches", np.int32, "b"))
SENTINEL = 77


def buffers(ng, nd, B):
    n = {"g": ng, "d": nd, "b": B}
    return {k: np.full(n[w] + 1, SENTINEL, dt) for k, dt, w in OUT}


def call(gt, det, gt_off, det_off, thr, out, B=None):
    lib = capi.load()
    gt_off, det_off = np.asarray(gt_off, np.int64), np.asarray(det_off, np.int64)
    rc = lib.uda_pseudo_audit_np(0, len(gt_off) - 1 if B is None else B, gt.ctypes.data, gt_off.ctypes.data, det.ctypes.data, det_off.ctypes.data,
                                 thr, *[out[k].ctypes.data for k, _, _ in OUT])
    return rc, lib.uda_last_error(None).decode()


def raw(gts, dets, thr=0.5):
    """One call of the C entry point on lists of per-image boxes -> the mirror's dict.  Every output buffer is one element longer
    than asked for and must keep its sentinel there."""
    gts = [np.asarray(g, np.float64).reshape(-1, 4) for g in gts]
    dets = [np.asarray(d, np.float64).reshape(-1, 4) for d in dets]
    gt_off = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int64)
    det_off = np.concatenate([[0], np.cumsum([len(d) for d in dets])]).astype(np.int64)
    gt, det = np.ascontiguousarray(np.concatenate(gts)), np.ascontiguousarray(np.concatenate(dets))
    out = buffers(len(gt), len(det), len(gts))
    rc, msg = call(gt, det, gt_off, det_off, thr, out)
    assert rc == 0, msg
    for k, _, _ in OUT:
        assert out[k][-1] == SENTINEL, k
    res = {k: out[k][:-1] for k, _, _ in OUT}
    res["gt_off"], res["det_off"] = gt_off, det_off
    return res


def same(got, want):
    for k, dt, _ in OUT:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, k
        if dt == np.float64:
            a, b = a.view(np.uint64), b.astype(np.float64).view(np.uint64)
        bad = np.where(a != b)[0]
        assert len(bad) == 0, (k, bad[:8], np.asarray(got[k])[bad[:8]], np.asarray(want[k])[bad[:8]])


def boxes(G, D, *seed):
    """Ground truth and labels on a 1/8 grid.  Even G + D: the coarse grid of 8-pixel steps, where equal IoUs, duplicates and
    predictions that take rows which did not choose them are frequent; odd: spread boxes, the labels jittered copies (some exact,
    some duplicated) and random ones."""
    rng = np.random.default_rng([G, D, *seed])
    if (G + D) % 2 == 0:
        def coarse(n):
            y, x = rng.integers(0, 6, n) * 8.0, rng.integers(0, 6, n) * 8.0
            return np.stack([y, x, y + rng.integers(1, 5, n) * 8.0, x + rng.integers(1, 5, n) * 8.0], 1)
        return coarse(G), coarse(D)
    y, x = rng.integers(0, 16000, G) / 8.0, rng.integers(0, 16000, G) / 8.0
    gt = np.stack([y, x, y + rng.integers(80, 480, G) / 8.0, x + rng.integers(80, 480, G) / 8.0], 1)
    det = np.zeros((D, 4))
    for d in range(D):
        u = rng.random()
        if u < 0.6:
            det[d] = gt[rng.integers(0, G)] + rng.integers(-16, 17, 4) / 8.0 * (rng.random() < 0.8)
        elif u < 0.7 and d > 0:
            det[d] = det[rng.integers(0, d)]
        else:
            yy, xx = rng.integers(0, 16000, 2) / 8.0
            det[d] = [yy, xx, yy + rng.integers(80, 480) / 8.0, xx + rng.integers(80, 480) / 8.0]
    return gt, det


@pytest.mark.parametrize("G", SIZES)
def test_wave_and_block_boundaries(G):
    """G rows against every D of the sweep, one image each in one call; a second call gives the same bits."""
    gts, dets = zip(*[boxes(G, D) for D in SIZES])
    want = R.audit(gts, dets, 0.5)
    got = raw(gts, dets)
    same(got, want)
    same(raw(gts, dets), got)
    assert want["n_matches"].sum() > 0


FAR = np.array([5000.0, 5000.0, 5010.0, 5010.0])
A = np.array([100.0, 100.0, 140.0, 164.0])


def far(n):
    return FAR + 20.0 * np.arange(n)[:, None]


@pytest.mark.parametrize("at", [(0,), (63,), (64,), (199,), (70, 5), (67, 3), (11, 10), (130, 70, 5), (199, 0)])
def test_planted_best_label_and_best_row(at):
    """The best sits at the first lane, the last lane, the first of the second sweep and the end; equal maxima sit in different
    lanes and different sweeps, and the lower index wins - for the labels of a row (phase 1) and for the rows of a label (phases 2
    and 3: the label takes the lowest of its equal rows)."""
    n = 200
    many = far(n)
    many[list(at)] = A
    one = A[None, :] + np.array([0.0, 0.0, 0.0, 0.125])
    first = min(at)
    res = raw([one], [many])                                          # one row, 200 labels
    same(res, R.audit([one], [many]))
    assert res["gt_best_det"][0] == first and list(np.where(res["det_alloc_gt"] >= 0)[0]) == [first]
    assert list(np.where(res["det_flags"] == 0)[0]) == sorted(at)    # the duplicates of the allocated label are not extra
    res = raw([many], [one])                                          # 200 rows, one label
    same(res, R.audit([many], [one]))
    assert res["det_best_gt"][0] == first and res["det_alloc_gt"][0] == first and res["n_matches"][0] == 1
    assert list(np.where(res["gt_flags"] == 0)[0]) == sorted(at)


def test_planted_second_choice_among_equal_rows():
    """Rows 5 and 70 are the same box and choose label 0; label 1, a near copy, has them as its two equal best rows.  Label 0 takes
    row 5, label 1 finds it taken and takes row 70 - which did not choose it - although row 100 did."""
    rows = far(131)
    rows[[5, 70]] = A
    a2 = A + np.array([0.0, 0.125, 0.0, 0.125])
    rows[100] = a2 + np.array([0.0, 8.0, 0.0, 8.0])
    labels = np.stack([A, a2])
    res = raw([rows], [labels])
    same(res, R.audit([rows], [labels]))
    assert list(res["gt_best_det"][[5, 70, 100]]) == [0, 0, 1] and list(res["det_alloc_gt"]) == [5, 70]
    assert res["gt_alloc_det"][100] == -1 and res["gt_flags"][100] == R.GT_NOMATCH


def chain(K):
    """K + 1 labels that all become matched predictions, each taking the row the next one has as its best: label 0 covers row 0
    and row K + 1 equally (0.5) and takes row 0; label j is row j - 1 moved by one pixel, finds rows j - 1 and j - 2 taken and ahead
    of its third choice, row j."""
    w, s = 64.0, 16.0
    rows = [[0.0, k * s, 8.0, k * s + w] for k in range(K + 1)] + [[8.0, 0.0, 16.0, w]]
    labels = [[0.0, 0.0, 16.0, w]] + [[0.0, (j - 1) * s - 1.0, 8.0, (j - 1) * s - 1.0 + w] for j in range(1, K + 1)]
    return np.asarray(rows), np.asarray(labels)


def test_chain_of_dependent_allocations():
    K = 64
    rows, labels = chain(K)
    res = raw([rows], [labels])
    same(res, R.audit([rows], [labels]))
    assert res["n_matches"][0] == K + 1 and list(res["det_alloc_gt"]) == list(range(K + 1))
    assert list(res["gt_best_det"][:K]) == list(range(1, K + 1))     # no row but the last chose the label that took it
    taken = res["det_alloc_gt"]
    assert (res["det_alloc_miou"][:K] < res["gt_max_iou"][taken[:K]]).all()     # the entries of later labels were invalidated


def test_ragged_batch_with_empty_images():
    D, G = 130, 70
    g_full, d_full = boxes(G, D, 7)
    g2, d2 = boxes(64, 64, 8)
    none = np.zeros((0, 4))
    gts = [g_full, g_full[:1], g_full[:1], none, g_full, g2, none, g2]
    dets = [d_full, g_full[:1] + 0.125, d_full, d_full, d_full[:1], none, none, d2]
    got = raw(gts, dets)
    same(got, R.audit(gts, dets))
    for b, (g, d) in enumerate(zip(gts, dets)):                       # the images audited one call each
        alone = raw([g], [d])
        for k, _, w in OUT:
            lo, hi = (b, b + 1) if w == "b" else (got["gt_off" if w == "g" else "det_off"][b], got["gt_off" if w == "g" else "det_off"][b + 1])
            np.testing.assert_array_equal(got[k][lo:hi], alone[k], err_msg="%s of image %d" % (k, b))
    o = got["det_off"]
    assert (got["det_flags"][o[3]:o[4]] == R.DET_EXTRA).all() and (got["det_best_gt"][o[3]:o[4]] == -1).all() and got["n_matches"][3] == 0
    o = got["gt_off"]
    assert (got["gt_flags"][o[5]:o[6]] == R.GT_NOMATCH).all() and (got["gt_best_det"][o[5]:o[6]] == -1).all() and got["n_matches"][5] == 0


def test_image_at_the_caps():
    G = D = capi.AUDIT_MAX_G
    rng = np.random.default_rng(1024)
    y, x = rng.integers(0, 32000, G) / 8.0, rng.integers(0, 32000, G) / 8.0
    gt = np.stack([y, x, y + rng.integers(80, 480, G) / 8.0, x + rng.integers(80, 480, G) / 8.0], 1)
    det = gt[rng.permutation(G)] + rng.integers(-16, 17, (G, 4)) / 8.0
    det[700:] = gt[rng.integers(0, G, D - 700)] + rng.integers(-64, 65, (D - 700, 4)) / 8.0
    res = raw([gt], [det])
    same(res, R.audit([gt], [det]))
    assert res["n_matches"][0] > 500


def test_refusals_leave_the_outputs_untouched():
    box = np.tile(A, (capi.AUDIT_MAX_G + 1, 1))
    cases = [
        (box, box[:1], [0, capi.AUDIT_MAX_G + 1], [0, 1], 0.5, None, "at most"),
        (box[:1], box, [0, 1], [0, capi.AUDIT_MAX_D + 1], 0.5, None, "at most"),
        (box[:4], box[:4], [0, 3, 2, 4], [0, 1, 2, 4], 0.5, None, "do not ascend"),
        (box[:4], box[:4], [0, 2, 4], [0, 3, 2], 0.5, None, "do not ascend"),
        (box[:4], box[:4], [1, 4], [0, 4], 0.5, None, "not at 0"),
        (box[:4], box[:4], [0, 4], [0, 4], float("nan"), None, "not finite"),
        (box[:4], box[:4], [0, 4], [0, 4], float("inf"), None, "not finite"),
        (box[:4], box[:4], [0, 4], [0, 4], 0.5, 0, "0 images"),
    ]
    for gt, det, gt_off, det_off, thr, B, words in cases:
        out = buffers(len(gt), len(det), len(gt_off) - 1)
        rc, msg = call(np.ascontiguousarray(gt), np.ascontiguousarray(det), gt_off, det_off, thr, out, B)
        assert rc == 1 and msg.startswith("uda_pseudo_audit_np: ") and words in msg, msg
        for k, _, _ in OUT:
            assert (out[k] == SENTINEL).all(), (k, words)
    res = raw([box[:capi.AUDIT_MAX_G]], [box[:1]])                    # exactly the cap passes
    assert res["n_matches"][0] == 1
    with pytest.raises(ValueError, match="not finite"):
        pa.audit_np([A[None]], [np.array([[0.0, np.inf, 1.0, 1.0]])])


def test_null_outputs_are_skipped():
    g, d = boxes(20, 30)
    want = raw([g], [d])
    lib = capi.load()
    off_g, off_d = np.array([0, 20], np.int64), np.array([0, 30], np.int64)
    n = np.full(2, SENTINEL, np.int32)
    rc = lib.uda_pseudo_audit_np(0, 1, np.ascontiguousarray(g).ctypes.data, off_g.ctypes.data, np.ascontiguousarray(d).ctypes.data,
                                 off_d.ctypes.data, 0.5, *([None] * 10), n.ctypes.data)
    assert rc == 0 and n[0] == want["n_matches"][0] and n[1] == SENTINEL


@pytest.mark.parametrize("dataset", ["kitti", "bdd"])
def test_golden_through_the_device(dataset):
    names, gt, dets, cls = H.fixture(dataset)
    res = pa.audit_np([g[0] for g in gt], [d[0] for d in dets], H.THR)
    same(res, R.audit([g[0] for g in gt], [d[0] for d in dets], H.THR))
    k = dataset + "_"
    assert np.array_equal(H.bits(res["gt_max_iou"]), H.bits(H.GOLD[k + "gt_max_iou"]))
    assert np.array_equal(H.bits(res["det_max_iou"]), H.bits(H.GOLD[k + "det_max_iou"]))
    np.testing.assert_array_equal(res["gt_best_det"], H.GOLD[k + "gt_best_det"])
    np.testing.assert_array_equal(res["det_best_gt"], H.GOLD[k + "det_best_gt"])
    np.testing.assert_array_equal(res["n_matches"], H.GOLD[k + "n_gt_matches"])
    au = pa.audit_pseudo_labels(gt, dets, cls, H.THR, names=names)
    assert H.numbers(au.summary()) == H.numbers(str(H.GOLD[k + "print_data"][0]))
    np.testing.assert_array_equal(np.concatenate(au.matched_preds), H.GOLD[k + "matched_preds"])
    got_box = np.asarray([b for im in au.allocated_dets["gt"]["box"] for b in im], np.float64).reshape(-1, 4)
    np.testing.assert_array_equal(got_box, H.GOLD[k + "alloc_gt_box"])


def test_end_to_end_files_on_the_device_path(tmp_path):
    """audit_pseudo_labels on the device, corrected_pseudo and both writers: the bytes of the reference's files, all six methods."""
    names, det_dir, gt_dir = H._write_kitti_inputs(tmp_path)
    _, gt, dets, cls = H.fixture("kitti")
    au = pa.audit_pseudo_labels(gt, dets, cls, H.THR, names=names)
    _, gt_b, dets_b, cls_b = H.fixture("bdd")
    names_b = H.fixture("bdd")[0]
    au_b = pa.audit_pseudo_labels(gt_b, dets_b, cls_b, H.THR, names=names_b)
    pred, gtj = json.loads(str(H.GOLD["bdd_det_json"][0])), json.loads(str(H.GOLD["bdd_gt_json"][0]))
    for method in H.METHODS:
        out = tmp_path / ("k_" + method)
        writers.write_kitti_corrected_pseudo(det_dir, gt_dir, str(out), cls, au, pa.corrected_pseudo(au, method))
        files = sorted(os.listdir(out))
        assert files == [str(f) for f in H.GOLD["kitti_%s_files" % method]]
        for f, want in zip(files, H.GOLD["kitti_%s_texts" % method]):
            assert (out / f).read_text() == str(want), (method, f)
        out = tmp_path / ("b_" + method)
        cor = pa.corrected_pseudo(au_b, method)
        writers.write_bdd_corrected_pseudo(pred, gtj, str(out), cls_b, au_b, cor)
        assert (out / "pseudo_labels.json").read_text() == str(H.GOLD["bdd_%s_text" % method][0]), method
        nm2, gt2, dets2 = pa.corrected_arrays(au_b, cor, "BDD100K")
        again = pa.audit_pseudo_labels(gt2, dets2, cls_b, H.THR, names=nm2)
        assert H.numbers(again.summary()) == H.numbers(str(H.GOLD["bdd_%s_output" % method][0]).split("new data: ")[1])
