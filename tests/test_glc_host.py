"""Label correction on the host (`label_correction`, `writers.write_*_corrected_gt`; reference src/ssl_utils/glc.py): the numpy
mirror of the contract (tests/glc_ref.py) against what the reference's own methods returned (tests/golden/glc_golden.npz, maker
beside it), `LabelCheck` and both writers on mirror output against the reference's returns and the bytes of its files, the
refusals of the Python layer, the resolution of min_score and the binding of the new symbols.  Everything is exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import glc_ref as R
from common import make_params
from uda_amd import capi, label_correction as lc, writers

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glc_golden.npz"))
CASES = [tuple(c) for c in GOLD["cases"]]
MIN_SCORE = float(GOLD["min_score"][0])
COLS = tuple(GOLD[k] for k in ("boxes", "scores", "cons_iou", "gt_boxes", "gt_classes"))


def mirror(ci, md_rule="eq", f32=False, methods=lc.METHODS):
    ic, md, cmi, cs = CASES[ci]
    return R.check(*COLS, MIN_SCORE, ic, md, md_rule, cmi, cs, methods, f32=f32)


def as_check(res, dt=np.float64):
    return lc.LabelCheck.from_arrays(res, GOLD["boxes"].astype(dt), GOLD["gt_boxes"].astype(dt), GOLD["gt_classes"], GOLD["classes"],
                                     names=list(GOLD["names"]))


def check_against_golden(chk, ci, md_rule="eq"):
    """A LabelCheck (every image of the golden has kept detections and counted rows) against the reference's returns."""
    np.testing.assert_array_equal(np.concatenate(chk.matched_det), GOLD["k%d_matched" % ci])
    got_iou = np.concatenate(chk.ious_gt)
    assert np.array_equal(got_iou.view(np.uint64), GOLD["k%d_iou" % ci].view(np.uint64))            # bit for bit
    np.testing.assert_array_equal(np.concatenate([np.full(len(w), i) for i, w in enumerate(chk.wrong_gt)]), GOLD["k%d_wrong_image" % ci])
    np.testing.assert_array_equal(np.concatenate(chk.wrong_gt), GOLD["k%d_wrong_row" % ci])
    np.testing.assert_array_equal(np.concatenate(chk.extra_correct_dets), GOLD["k%d_extra%s" % (ci, "_le" if md_rule == "le" else "")])
    np.testing.assert_array_equal(np.concatenate([np.asarray(c).reshape(-1, 4) for c in chk.corrected_gt_boxes]), GOLD["k%d_corrected" % ci])


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("md_rule", ["eq", "le"])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_mirror_reproduces_the_reference(ci, md_rule, f32):
    """Both arithmetic variants: the coordinates are multiples of 1/8 below 2^11, so float32 differences are exact."""
    res = mirror(ci, md_rule, f32)
    check_against_golden(as_check(res, np.float32 if f32 else np.float64), ci, md_rule)
    n = len(GOLD["names"])
    np.testing.assert_array_equal(res["counts"][:, 0], (GOLD["scores"] > MIN_SCORE).sum(1))
    np.testing.assert_array_equal(res["counts"][:, 1], (GOLD["gt_classes"] > 0).sum(1))
    assert res["counts"][:, 2].sum() == len(GOLD["k%d_wrong_row" % ci]) and res["counts"].shape == (n, 5)


def test_planted_cases_are_in_the_golden():
    res = mirror(1)
    F = res["gt_flags"]
    # image 0: the first of two rows matched to rank 0 fails the noisy conditions, the second meets them; the FIRST is replaced
    assert F[0, 0] == R.GT_REPLACED and F[0, 1] == R.GT_NOISY and list(res["det_rank"][0, :2]) == [0, 0]
    # image 1: three rows on rank 1 (the lower of two duplicate boxes); the third qualifies, the first is replaced
    assert list(res["det_rank"][1, :3]) == [1, 1, 1] and F[1, 0] == R.GT_REPLACED and F[1, 1] == 0 and F[1, 2] == R.GT_NOISY
    # image 2: rank 0 is not kept; the mistake row is matched to rank 1, the first kept, and takes its box
    assert res["det_rank"][2, 0] == 1 and F[2, 0] & R.GT_MISTAKE and F[2, 0] & R.GT_REPLACED and res["iou"][2, 0] == 0
    np.testing.assert_array_equal(res["gt_boxes_out"][2, 0], GOLD["boxes"][2, 1].astype(np.float32))
    # image 4: the maximum IoU is exactly 0.25
    assert res["det_max_iou"][4, 0] == 0.25 and res["det_flags"][4, 0] == R.DET_KEPT | R.DET_MISSING and res["det_flags"][4, 1] == R.DET_KEPT
    # image 3 under the defaults: cons_iou == iou_consist is a missing label (>=) and not a better box (strict); score == correct_score is
    r0 = mirror(0)
    assert r0["det_flags"][3, 0] & R.DET_MISSING and not r0["gt_flags"][3, 0] & R.GT_NOISY and r0["gt_flags"][3, 1] & R.GT_NOISY
    assert r0["iou"][3, 1] == 1.0 and not r0["det_flags"][3, 3]              # (score == min_score: not kept, between kept rows)


def test_mirror_defined_cases():
    """No kept detection: det_rank -1, IoU 0, no flag.  No counted row: the md rule on a maximum of 0."""
    b, s, c, gb, gc = (a[:2].copy() for a in COLS)
    s[0] = 0.05
    gc[1] = -1
    res = R.check(b, s, c, gb, gc, MIN_SCORE)
    assert (res["det_rank"][0] == -1).all() and not res["gt_flags"][0].any() and not res["det_flags"][0].any()
    assert list(res["counts"][0]) == [0, int((COLS[4][0] > 0).sum()), 0, 0, 0]
    kept = s[1] > MIN_SCORE
    np.testing.assert_array_equal((res["det_flags"][1] & R.DET_MISSING) != 0, kept & (c[1] >= 0.9))
    assert res["counts"][1, 1] == 0 and (res["det_rank"][1] == -1).all()
    chk = lc.LabelCheck.from_arrays(res, b, gb, gc, GOLD["classes"][:2])
    assert len(chk.wrong_gt[0]) == 0 and len(chk.extra_correct_dets[0]) == 0 and chk.corrected_gt_boxes[1] == []
    assert (chk.matched_det[0] == -1).all() and len(chk.corrected_gt_boxes[0]) == res["counts"][0, 1]


def test_label_check_shapes_and_merge():
    res = mirror(0)
    chk = as_check(res)
    n = len(GOLD["names"])
    assert len(chk) == n and chk.counts.shape == (n, 5) and chk.counts.dtype == np.int32 and chk.methods == lc.METHODS
    for i in range(n):
        K, rows = int(res["counts"][i, 0]), int(res["counts"][i, 1])
        assert chk.extra_correct_dets[i].dtype == bool and chk.extra_correct_dets[i].shape == (K,)
        assert len(chk.corrected_gt_boxes[i]) == rows and all(len(b) == 4 and type(b[0]) is float for b in chk.corrected_gt_boxes[i])
        assert len(chk.pred_boxes[i]) == K and len(chk.pred_classes[i]) == K and chk.ious_gt[i].shape == (rows,)
        assert len(chk.wrong_gt[i]) == res["counts"][i, 2] and len(chk.replaced[i]) == res["counts"][i, 3]
        assert chk.extra_correct_dets[i].sum() == res["counts"][i, 4]
    t = chk.totals()
    assert t["mistakes"] == len(GOLD["k0_wrong_row"]) and t["missing"] == int(GOLD["k0_extra"].sum()) and t["kept"] == int((GOLD["scores"] > MIN_SCORE).sum())
    # two batches merged are the whole
    cut = 3
    parts = []
    for sl in (slice(0, cut), slice(cut, n)):
        sub = {k: v[sl] for k, v in res.items()}
        parts.append(lc.LabelCheck.from_arrays(sub, GOLD["boxes"][sl], GOLD["gt_boxes"][sl], GOLD["gt_classes"][sl], GOLD["classes"][sl],
                                               names=list(GOLD["names"][sl])))
    merged = parts[0].merge(parts[1])
    assert merged is parts[0] and len(merged) == n and merged.names == list(GOLD["names"])
    check_against_golden(merged, 0)
    np.testing.assert_array_equal(merged.counts, chk.counts)
    with pytest.raises(ValueError, match="different methods"):
        merged.merge(lc.LabelCheck(("mistakes",)))
    # a float32 detection box is held as its shortest decimal
    b32 = GOLD["boxes"].astype(np.float32)
    b32[0, 0] = np.float32([10.1, 10.2, 50.3, 50.4])
    c32 = lc.LabelCheck.from_arrays(res, b32, GOLD["gt_boxes"], GOLD["gt_classes"], GOLD["classes"])
    assert c32.corrected_gt_boxes[0][0] == [10.1, 10.2, 50.3, 50.4] and c32.pred_boxes[0][0] == [10.1, 10.2, 50.3, 50.4]


def _kitti_inputs(tmp_path):
    src = tmp_path / "label_2"
    src.mkdir()
    files = [nm + ".txt" for nm in GOLD["names"]]
    for f, text in zip(files, GOLD["kitti_label_texts"]):
        (src / f).write_text(str(text))
    return str(src), files


MODES = {"remove": dict(remove_mistakes=True), "add": dict(add_missingboxes=True), "correct": dict(correct_boxes=True)}


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_kitti_writer_reproduces_the_reference_bytes(ci, tmp_path):
    chk = as_check(mirror(ci))
    src, files = _kitti_inputs(tmp_path)
    for tag, kw in MODES.items():
        out = tmp_path / ("out_" + tag)
        lines = writers.write_kitti_corrected_gt(src, str(out), files, list(GOLD["kitti_classes"]), check=chk, **kw)
        assert sorted(os.listdir(out)) == list(GOLD["k%d_kitti_%s_files" % (ci, tag)])
        texts = [open(out / f, newline="").read() for f in GOLD["k%d_kitti_%s_files" % (ci, tag)]]
        assert texts == [str(t) for t in GOLD["k%d_kitti_%s_texts" % (ci, tag)]], tag
        assert lines == sum(t.count("\n") for t in texts)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_bdd_writer_reproduces_the_reference_bytes(ci, tmp_path):
    chk = as_check(mirror(ci))
    data = json.loads(str(GOLD["bdd_json"][0]))
    before = json.dumps(data)
    names = [nm + ".jpg" for nm in GOLD["names"]]
    for tag, kw in MODES.items():
        out = tmp_path / ("out_" + tag)
        writers.write_bdd_corrected_gt(data, str(out), names, list(GOLD["bdd_classes"]), check=chk, **kw)
        assert list(GOLD["k%d_bdd_%s_files" % (ci, tag)]) == ["bdd100k_labels_images_train.json"] == os.listdir(out)
        assert open(out / "bdd100k_labels_images_train.json", newline="").read() == str(GOLD["k%d_bdd_%s_texts" % (ci, tag)][0]), tag
    assert json.dumps(data) == before                       # the input is not modified (the reference writes into it)
    with pytest.raises(ValueError, match="order image_names like the json"):
        writers.write_bdd_corrected_gt(data, str(tmp_path / "x"), names[::-1], list(GOLD["bdd_classes"]), check=chk, remove_mistakes=True)
    with pytest.raises(ValueError, match="needs wrong_gt"):
        writers.write_bdd_corrected_gt(data, str(tmp_path / "x"), names, list(GOLD["bdd_classes"]), remove_mistakes=True)


def test_python_layer_refusals():
    b, s, c, gb, gc = COLS
    with pytest.raises(ValueError, match="unknown method 'mds'"):
        lc.check_labels(b, s, c, gb, gc, methods=("mds",))
    with pytest.raises(ValueError, match="no method given"):
        lc.check_labels(b, s, c, gb, gc, methods=())
    with pytest.raises(ValueError, match="md_rule 'lt'"):
        lc.check_labels(b, s, c, gb, gc, md_rule="lt")
    with pytest.raises(ValueError, match="iou_consist must be finite"):
        lc.check_labels(b, s, c, gb, gc, iou_consist=float("nan"))
    with pytest.raises(ValueError, match="min_score must be finite"):
        lc.check_labels(b, s, c, gb, gc, min_score=float("inf"))
    with pytest.raises(ValueError, match="read cons_iou"):
        lc.check_labels(b, s, None, gb, gc, methods=("md",))
    with pytest.raises(ValueError, match="cons_iou must be"):
        lc.check_labels(b, s, c[:, :5], gb, gc)
    with pytest.raises(ValueError, match=r"gt_boxes must be \[10, G, 4\]"):
        lc.check_labels(b, s, c, gb[:3], gc[:3])
    bad = gb.copy()
    bad[1, 0, 2] = np.nan
    with pytest.raises(ValueError, match="gt_boxes holds non-finite"):
        lc.check_labels(b, s, c, bad, gc)
    with pytest.raises(ValueError, match="no image given"):
        lc.check_labels(b[:0], s[:0], c[:0], gb[:0], gc[:0])
    with pytest.raises(ValueError, match="4097 detection rows per image, at most 4096"):
        lc.check_labels(np.zeros((1, 4097, 4)), np.zeros((1, 4097)), np.zeros((1, 4097)), gb[:1], gc[:1])
    with pytest.raises(ValueError, match="16385 ground-truth rows per image, at most 16384"):
        lc.check_labels(b[:1], s[:1], c[:1], np.zeros((1, 16385, 4)), np.ones((1, 16385)))
    with pytest.raises(ValueError, match="lists differ in length"):
        lc.check_labels([[[0, 0, 1, 1]]], [[0.5]], [[0.9]], [[], []])
    assert lc.method_mask("mistakes") == capi.LC_MISTAKES and lc.method_mask(lc.METHODS) == 7


def test_min_score_resolution():
    """infer_model.py:568-573: 0.1 for a model served from an SSL folder (GLC's own run), else score_thresh or the average score
    or 0.4."""
    p = make_params()
    assert lc.resolve_min_score(p) == 0.1
    assert lc.resolve_min_score(p, 0.25) == 0.25
    p["nms_configs"]["score_thresh"] = 0.0
    assert lc.resolve_min_score(p, ssl=False) == 0.4 and lc.resolve_min_score(p, average_score=0.3, ssl=False) == 0.3
    p["nms_configs"]["score_thresh"] = 0.2
    assert lc.resolve_min_score(p, ssl=False) == 0.2 and lc.resolve_min_score(p) == 0.1
    assert lc.DEFAULTS == dict(iou_consist=0.90, md_max_inter=0, md_rule="eq", correct_max_inter=1.0, correct_score=0.40)


def test_new_symbols_are_bound():
    for name in ("uda_label_check", "uda_get_label_check", "uda_label_check_np", "uda_label_check_np_f32"):
        assert name in capi.EXPORTS
    res, args = capi._SIGNATURES["uda_label_check"]
    assert res is C.c_int and args == [C.c_void_p, C.c_float, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_float, C.c_int32]
    assert len(capi._SIGNATURES["uda_get_label_check"][1]) == 8
    for name, scalar in (("uda_label_check_np", C.c_double), ("uda_label_check_np_f32", C.c_float)):
        args = capi._SIGNATURES[name][1]
        assert len(args) == 23 and args[9] is scalar and args[14] is scalar and args[10] is C.c_double
    assert (capi.LC_MD, capi.LC_MISTAKES, capi.LC_NOISY) == (R.MD, R.MISTAKES, R.NOISY)
    assert (capi.LC_GT_MISTAKE, capi.LC_GT_NOISY, capi.LC_GT_REPLACED, capi.LC_DET_KEPT, capi.LC_DET_MISSING) == (1, 2, 4, 1, 2)
    header = open(capi.HEADER).read()
    for name, val in (("UDA_LC_MD", 1), ("UDA_LC_MISTAKES", 2), ("UDA_LC_NOISY", 4), ("UDA_LC_MD_LE", 1), ("UDA_LC_GT_REPLACED", 4),
                      ("UDA_LC_DET_MISSING", 2)):
        assert "#define %s %d" % (name, val) in header
