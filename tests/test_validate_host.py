"""Ground-truth assignment, host side: the numpy restatement (validate_ref) against what the reference's own
`gt_box_assigner` / `calc_iou_np` returned (tests/golden/gt_assign_golden.npz), the keep rules, the argument checks, the split
of the matched-rows table (with an injected NaN: the host does the reference's nan_to_num), and `writers.validate_to_file` /
`calibration.gather_detections` end to end over a driver stand-in."""
import ast
import os

import numpy as np
import pytest

import validate_ref as V
from common import FULL_MC, LOSS_ATT, PLAIN, make_params

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gt_assign_golden.npz")


def golden_cases():
    g = np.load(GOLDEN)
    for ci in range(int(g["n_cases"][0])):
        yield ci, g, g["c%d_dets" % ci], g["c%d_gt_boxes" % ci], g["c%d_gt_classes" % ci]


@pytest.mark.parametrize("keep", ["validate", "calibrate"])
@pytest.mark.parametrize("method", V.METHODS)
def test_restatement_equals_reference(method, keep):
    seen = 0
    for ci, g, dets, gtb, gtc in golden_cases():
        tag = "c%d_%s_%s" % (ci, method, keep)
        if not int(g[tag + "_ok"][0]):
            with pytest.raises(ValueError):
                V.assign(method, gtb, gtc, dets, keep)
            continue
        idx, iou, count = V.assign(method, gtb, gtc, dets, keep)
        np.testing.assert_array_equal(idx, g[tag + "_idx"])
        assert iou.dtype == np.float64 and np.array_equal(iou.view(np.uint64), g[tag + "_iou"].view(np.uint64))   # bit for bit
        np.testing.assert_array_equal(count, (g[tag + "_idx"] >= 0).sum(1))
        seen += int(count.sum())
    assert seen > 100


def test_golden_has_the_cases_it_is_for():
    nonzero = ties = far = flat = 0
    for ci, g, dets, gtb, gtc in golden_cases():
        assert dets.shape[1:] == (100, 4) and dets.dtype == gtb.dtype == gtc.dtype == np.float32
        vl = g["c%d_valid_len" % ci]
        for im, v in enumerate(vl):
            assert np.all(dets[im, v:] == dets[im, 0] if v else dets[im] == 0)       # padded rows carry row 0's box
        idx = g["c%d_IoU_validate_idx" % ci]
        nonzero += int((idx > 0).sum())
        ties += int(((idx == 0) & (gtc > 0)).sum())
        assert (gtc == -1).any() and (gtc == 0).any()             # padding rows; class-0 rows (kept by calibrate only)
        far += int(((gtb[..., 0] > 1600) & (gtc > 0)).sum())
        flat += int(((gtb[..., 0] == gtb[..., 2]) & (gtc > 0)).sum())
    assert nonzero > 50 and ties > 20 and far > 10 and flat > 10
    # the MSE order matters: the other association of the four squares moves at least one float32 key of the fixture
    _, g, dets, gtb, _ = next(golden_cases())
    d = gtb[0, :, None, :] - dets[0][None]
    s = d * d
    seq = ((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3]
    alt = s[..., 0] + ((s[..., 1] + s[..., 2]) + s[..., 3])
    assert (seq != alt).any()


def test_keep_rules():
    cls = np.array([[3, 0, -1, 2, 1, -1]], np.float32)
    boxes = np.zeros((1, 4, 4), np.float32)
    assert V.kept_rows(cls[0], 4, "validate").tolist() == [0, 3, 4]
    assert V.kept_rows(cls[0], 4, "calibrate").tolist() == [0, 1, 3]            # rows < min(G, M), class >= 0
    assert V.kept_rows(cls[0], 100, "calibrate").tolist() == [0, 1, 3, 4]
    gtb = np.zeros((1, 6, 4), np.float32)
    with pytest.raises(ValueError):
        V.assign("rank", gtb, cls, boxes, "validate")                             # kept row 4 >= M = 4
    idx, _, count = V.assign("rank", gtb, cls, boxes, "calibrate")
    assert idx.tolist() == [[0, 1, -1, 3, -1, -1]] and count.tolist() == [3]
    idx, iou, _ = V.assign("IoU", gtb, cls, boxes, "validate")                    # IoU 0 everywhere: rank 0
    assert idx.tolist() == [[0, -1, -1, 0, 0, -1]] and not iou.any()


def test_argument_checks():
    from uda_amd import dist, utils_extra as U
    gb, gc = np.zeros((2, 5, 4)), np.zeros((2, 5), np.int64)
    b, c = U.check_ground_truth(gb, gc)
    assert b.dtype == c.dtype == np.float32 and b.flags.c_contiguous
    for bad_b, bad_c in ((np.zeros((2, 5, 3)), gc), (gb, np.zeros((2, 4))), (np.zeros((5, 4)), np.zeros(5)),
                         (np.zeros((0, 5, 4)), np.zeros((0, 5)))):
        with pytest.raises(ValueError):
            U.check_ground_truth(bad_b, bad_c)
    for v in (np.nan, np.inf, -np.inf):
        x = gb.copy(); x[1, 2, 3] = v
        with pytest.raises(ValueError, match="finite"):
            U.check_ground_truth(x, gc)
        y = gc.astype(np.float64); y[0, 1] = v
        with pytest.raises(ValueError, match="finite"):
            U.check_ground_truth(gb, y)
    with pytest.raises(ValueError):
        U.keep_code("all")
    assert [U.assign_method_code(m) for m in ("IoU", "MSE", "rank", None, "iou")] == [0, 1, 2, 2, 2]
    cls = np.array([[1, 1, 1, -1]], np.float32)
    U.check_rank_rows("rank", cls, 3, "validate")
    U.check_rank_rows("IoU", cls, 2, "validate")
    U.check_rank_rows("rank", cls, 2, "calibrate")
    with pytest.raises(ValueError, match="beyond"):
        U.check_rank_rows("rank", cls, 2, "validate")
    # a sample-sharded serve leaves no handle with the whole batch: it says so instead of assigning a shard
    d = object.__new__(dist.SampleShardedDriver)
    with pytest.raises(ValueError, match="assign_gt_boxes"):
        d.assign_ground_truth(gb, gc)
    with pytest.raises(ValueError, match="assign_gt_boxes"):
        d.serve_validate(None, gb, gc)


def fake_detections(rng, params, n, M=100, valid=None):
    C = int(params["num_classes"])
    mc = bool(params.get("mc_dropout")) and bool(params.get("mc_dropoutrate"))
    la = bool(params.get("loss_attenuation"))
    bc, cc = 4 + 4 * la + 4 * mc, 1 + C * mc
    c = rng.uniform(30, 300, (n, M, 2)); hw = rng.uniform(5, 60, (n, M, 2))
    boxes = np.concatenate([c - hw / 2, c + hw / 2, rng.uniform(0, 3, (n, M, bc - 4))], -1).astype(np.float32)
    scores = np.sort(rng.uniform(0, 1, (n, M)).astype(np.float32))[:, ::-1].copy()
    classes = rng.integers(1, C + 1, (n, M, 1)).astype(np.float32)
    if cc > 1:
        classes = np.concatenate([classes, rng.uniform(0, 1, (n, M, C)).astype(np.float32)], -1)
    else:
        classes = classes[..., 0]
    valid = np.asarray(valid if valid is not None else [M] * n, np.int32)
    logits = rng.normal(0, 2, (n, M, C)).astype(np.float32)
    for a in (boxes, scores, classes, logits):
        for i, v in enumerate(valid):
            a[i, v:] = a[i, 0]
    det = (boxes, scores, classes, valid) + ((logits,) if params["enable_softmax"] else ())
    return det


def softmax_entropy(logits):
    z = logits - logits.max(-1, keepdims=True)
    p = (np.exp(z) / np.exp(z).sum(-1, keepdims=True)).astype(np.float32)
    return p, (-(p * np.log2(np.maximum(p, 1e-7))).sum(-1)).astype(np.float32)


def gt_from(rng, det, G, rows):
    n = det[0].shape[0]
    gb = np.full((n, G, 4), -1, np.float32)
    gc = np.full((n, G), -1, np.float32)
    for i in range(n):
        ks = rng.integers(0, max(int(det[3][i]), 1), rows)
        gb[i, :rows] = det[0][i, ks, :4] + rng.normal(0, 1.5, (rows, 4)).astype(np.float32)
        gc[i, :rows] = det[2][i, ks] if det[2].ndim == 2 else det[2][i, ks, 0]
        gc[i, 0] = 0                                            # kept by calibrate only
        gb[i, 1] = [900, 900, 950, 950]                         # overlaps nothing
    return gb, gc


@pytest.mark.parametrize("cfg", [FULL_MC, LOSS_ATT, PLAIN, dict(PLAIN, enable_softmax=False)], ids=["full_mc", "loss_att", "plain", "no_softmax"])
def test_split_assigned_rows_with_injected_nan(cfg):
    """The device copies matched rows unchanged; infer_lib.split_assigned_rows (host) applies the reference's nan_to_num to
    the uncertainty columns and nothing else."""
    from uda_amd.infer_lib import split_assigned_rows
    p = make_params(**cfg)
    rng = np.random.default_rng(3)
    det = fake_detections(rng, p, 2, valid=[100, 17])
    bc, cc, C = det[0].shape[-1], (det[2].shape[-1] if det[2].ndim == 3 else 1), p["num_classes"]
    if bc > 4:
        det[0][0, 5, 4] = np.nan
        det[0][1, 3, bc - 1] = np.inf
    if cc > 1:
        det[2][0, 7, 2] = np.nan
    probab = entropy = None
    if p["enable_softmax"]:
        probab, entropy = softmax_entropy(det[4])
    gb, gc = gt_from(rng, det, 9, 6)
    gb[0, 2], gb[0, 3], gb[1, 2] = det[0][0, 5, :4], det[0][0, 7, :4], det[0][1, 3, :4]      # the rows that hold the NaNs are matched
    idx, iou, count = V.assign("IoU", gb, gc, det[0])
    assert idx[0, 2] == 5 and idx[0, 3] == 7 and idx[1, 2] == 3
    want = V.gather(p, det, idx, gb, gc, probab, entropy)
    im, row = np.nonzero(idx >= 0)
    k = idx[im, row]
    cls = det[2][im, k].reshape(len(k), -1)
    parts = [det[0][im, k], det[1][im, k][:, None], cls]
    if p["enable_softmax"]:
        parts += [det[4][im, k], probab[im, k], entropy[im, k][:, None]]
    table = np.concatenate(parts, 1).astype(np.float32)
    assert np.isnan(table).any() == (bc > 4 or cc > 1)
    got = split_assigned_rows(p, table, bc, cc, C)
    for key in V.COLUMNS:
        if want[key] is None:
            assert got[key] is None, key
        else:
            np.testing.assert_array_equal(got[key], want[key], err_msg=key)
            assert np.isfinite(got[key]).all()
    with pytest.raises(ValueError):
        split_assigned_rows(p, table[:, :-1], bc, cc, C)


class StubBoxCal:
    models = {"ts_all": 2.0, "iso_all": None}

    def __init__(self, drv):
        self.drv = drv

    def calibrate_boxuncert(self, n, which, method):
        b = self.drv._det[0]
        col0 = 4 if which == "albox" or b.shape[-1] == 8 else 8
        return b[:n, :, col0:col0 + 4] / (2.0 if method == "ts_all" else 3.0)


class StubClassCal:
    models = {"ts_all": 1.5}

    def __init__(self, drv, with_unc):
        self.drv, self.with_unc = drv, with_unc

    def perform_class_calib(self, n, method):
        p, e = softmax_entropy(self.drv._det[4][:n] / 1.5)
        return (e, p, p * 0.1) if self.with_unc else (e, p)


def _flow(tmp_path, cfg, method="IoU"):
    from uda_amd import writers
    p = make_params(assign_gt_box=method, **cfg)
    rng = np.random.default_rng(11)
    dets = [fake_detections(rng, p, 2, valid=[100, 40]), fake_detections(rng, p, 1, valid=[3])]
    batches = [np.zeros((d[0].shape[0], 8, 8, 3), np.uint8) for d in dets]
    gts = [gt_from(rng, dets[0], 12, 7), gt_from(rng, dets[1], 5, 4)]
    names = [["a.png", "b.png"], ["c.png"]]
    occl = [rng.integers(0, 3, g[1].shape) for g in gts]
    trunc = [rng.uniform(0, 1, g[1].shape).astype(np.float32) for g in gts]
    it = iter(dets)
    drv = V.RefDriver(p, lambda b: next(it), lambda n: softmax_entropy(drv._det[4][:n]))
    out = str(tmp_path / "val")
    filtered = writers.validate_to_file(drv, batches, gts, names, out, box_calibrator=StubBoxCal(drv),
                                        class_calibrator=StubClassCal(drv, dets[0][2].ndim == 3) if p["enable_softmax"] else None,
                                        occlusions=occl, truncations=trunc)
    return p, dets, gts, filtered, out


@pytest.mark.parametrize("cfg", [FULL_MC, LOSS_ATT, PLAIN, dict(PLAIN, enable_softmax=False)], ids=["full_mc", "loss_att", "plain", "no_softmax"])
def test_validate_to_file_end_to_end(tmp_path, cfg):
    p, dets, gts, filtered, out = _flow(tmp_path, cfg)
    K = sum(int((g[1] > 0).sum()) for g in gts)
    lines = open(os.path.join(out, "validate_results.txt")).read().splitlines()
    assert len(lines) == K == len(filtered["names"]) > 10
    recs = [ast.literal_eval(l.replace("inf", "2e308")) for l in lines]
    want_keys = ["image_name", "score", "bbox", "gt_bbox", "gt_occl", "gt_trunc", "class", "gt_class"]
    mc, la = bool(p.get("mc_dropoutrate")), bool(p.get("loss_attenuation"))
    if p["enable_softmax"]:
        want_keys += ["logits", "probab", "entropy", "ts_all_probab", "ts_all_entropy"]
    if mc:
        want_keys += ["uncalib_mcclass", "ts_all_mcclass", "uncalib_mcbox", "iso_all_mcbox", "ts_all_mcbox"]
    if la:
        want_keys += ["uncalib_albox", "iso_all_albox", "ts_all_albox"]
    assert list(recs[0]) == want_keys
    assert [r["image_name"] for r in recs] == ["a.png"] * int((gts[0][1][0] > 0).sum()) + ["b.png"] * int((gts[0][1][1] > 0).sum()) + \
        ["c.png"] * int((gts[1][1][0] > 0).sum())
    # record 0 is image 0's first kept GT row, matched by IoU
    idx, iou, _ = V.assign("IoU", gts[0][0], gts[0][1], dets[0][0])
    r0 = int(np.nonzero(gts[0][1][0] > 0)[0][0])
    k0 = idx[0, r0]
    assert recs[0]["bbox"] == [float(str(v)) for v in dets[0][0][0, k0, :4]]
    assert recs[0]["gt_bbox"] == [float(str(v)) for v in gts[0][0][0, r0]]
    assert recs[0]["score"] == float(str(dets[0][1][0, k0])) and recs[0]["gt_class"] == float(gts[0][1][0, r0])
    assert float(open(os.path.join(out, "average_score.txt")).read()) == float(np.mean(filtered["scores"].astype(np.float64)))
    rt = open(os.path.join(out, "validationstep_runtime.txt")).read().splitlines()
    assert [l.split(":")[0] for l in rt] == ["Mean time in ms", "STD time in ms", "Median time in ms"]
    perf = os.path.join(out, "model_performance.txt")
    assert os.path.exists(perf) == (not mc and not la)            # the reference writes it without box uncertainty only
    if os.path.exists(perf):
        mis, miou, rmse = V.model_performance(filtered["gt_classes"], filtered["classes"], filtered["gt_boxes"], filtered["boxes"])
        assert open(perf).read() == "Misclassification rate: {}\nmIoU: {}\nRMSE: {}\n".format(mis, miou, rmse)
        assert 0 < miou < 1 and rmse > 0


def test_validate_to_file_follows_assign_gt_box(tmp_path):
    """model_params["assign_gt_box"] picks the method: the rank branch pairs GT row i with detection i."""
    p, dets, gts, filtered, out = _flow(tmp_path, PLAIN, method="none")
    im, row = np.nonzero(gts[0][1] > 0)
    np.testing.assert_array_equal(filtered["boxes"][:len(im)], dets[0][0][im, row, :4])


def test_gather_detections_filter():
    from uda_amd import calibration
    p = make_params(**FULL_MC)
    rng = np.random.default_rng(5)
    dets = [fake_detections(rng, p, 2, valid=[100, 9]), fake_detections(rng, p, 2, valid=[50, 0])]
    gts = [gt_from(rng, d, 8, 6) for d in dets]
    it = iter(dets)
    drv = V.RefDriver(p, lambda b: next(it), lambda n: softmax_entropy(drv._det[4][:n]))
    got = calibration.gather_detections(drv, [None, None], gts)
    want = {k: [] for k in ("gt_classes", "logits", "mcclass", "gt_boxes", "boxes", "albox", "mcbox")}
    for d, (gb, gc) in zip(dets, gts):
        idx, iou, _ = V.assign("IoU", gb, gc, d[0], "calibrate")
        pr, en = softmax_entropy(d[4])
        g = V.gather(p, d, idx, gb, gc, pr, en, "calibrate")
        sel = iou[g["image"], g["gt_row"]] > 0
        for k in want:
            want[k].append(g[k][sel])
    for k in want:
        np.testing.assert_array_equal(got[k], np.concatenate(want[k]), err_msg=k)
    assert (got["iou"] > 0).all() and 0 < len(got["iou"]) < sum(int((gc >= 0).sum()) for _, gc in gts)   # the far-away boxes left
    assert got["gt_classes"].min() == -1.0                        # class 0 rows are kept and reported as class - 1


def test_model_param_entry():
    from uda_amd import plan
    assert plan.MODEL_PARAM_HANDLING["assign_gt_box"].startswith("consumed")
