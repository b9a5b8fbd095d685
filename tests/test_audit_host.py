"""The pseudo-label audit on the host (`pseudo_audit`, `writers.write_*_corrected_pseudo`; reference src/ssl_utils/parent.py:1567-1813,
3d.py:80-255, pls.py:102-282) without a GPU: the numpy mirror of the contract (tests/audit_ref.py) against what the reference's own
methods left (tests/golden/audit_golden.npz, maker beside it), then `PseudoAudit`, `corrected_pseudo`, both writers and the PLS
numbers on mirror output (`audit=`) against the reference's members, the bytes of its files and its saved arrays.  Everything
is exact."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import audit_ref as R
from common import ROOT
from uda_amd import capi, pseudo_audit as pa, writers

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audit_golden.npz"))
THR = float(GOLD["gt_iou_thr"][0])
STEMS = [str(s) for s in GOLD["stems"]]
KITTI, BDD = [str(c) for c in GOLD["kitti_classes"]], [str(c) for c in GOLD["bdd_classes"]]
METHODS = [str(m) for m in GOLD["methods"]]
N = len(STEMS)


def _images(side, class_names):
    off = np.concatenate([[0], np.cumsum(GOLD[side + "_n"])])
    return [([[float(v) for v in b] for b in GOLD[side + "_boxes"][off[i]:off[i + 1]]],
             np.asarray([class_names[c - 1] for c in GOLD[side + "_classes"][off[i]:off[i + 1]]])) for i in range(N)]


def fixture(dataset):
    """-> names, gt, dets (as (boxes, classes) pairs), used classes, in the order the reference audited them."""
    if dataset == "kitti":
        order = [STEMS.index(str(nm)[:-4]) for nm in GOLD["kitti_images_data"]]
        names, cls = [STEMS[i] + ".txt" for i in order], KITTI
    else:
        order, names, cls = list(range(N)), [s + ".jpg" for s in STEMS], BDD
    gt, dets = _images("gt", cls), _images("det", cls)
    return names, [gt[i] for i in order], [dets[i] for i in order], cls


def audited(dataset):
    names, gt, dets, cls = fixture(dataset)
    return pa.audit_pseudo_labels(gt, dets, cls, THR, names=names, audit=R.audit)


def numbers(text):
    """The numbers of a print_data text, as strings, whatever numpy's repr of a scalar is."""
    text = re.sub(r"np\.(float64|int64)\(([^)]*)\)", r"\2", text)
    return re.findall(r"nan|-?\d+\.?\d*", text)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("dataset", ["kitti", "bdd"])
def test_mirror_reproduces_the_reference_members(dataset):
    names, gt, dets, cls = fixture(dataset)
    res = R.audit([g[0] for g in gt], [d[0] for d in dets], THR)
    k = dataset + "_"
    assert np.array_equal(bits(res["gt_max_iou"]), bits(GOLD[k + "gt_max_iou"]))
    assert np.array_equal(bits(res["det_max_iou"]), bits(GOLD[k + "det_max_iou"]))
    np.testing.assert_array_equal(res["gt_best_det"], GOLD[k + "gt_best_det"])
    np.testing.assert_array_equal(res["det_best_gt"], GOLD[k + "det_best_gt"])
    np.testing.assert_array_equal(res["n_matches"], GOLD[k + "n_gt_matches"])
    np.testing.assert_array_equal(np.diff(res["gt_off"]), GOLD[k + "n_gts_perim"])
    np.testing.assert_array_equal(np.diff(res["det_off"]), GOLD[k + "n_pred_perim"])
    matched = [np.where(res["det_alloc_gt"][a:b] >= 0)[0] for a, b in zip(res["det_off"][:-1], res["det_off"][1:])]
    np.testing.assert_array_equal(np.concatenate(matched), GOLD[k + "matched_preds"])
    alloc_gt = np.concatenate([np.asarray(g[0])[res["det_alloc_gt"][a:b][m]].reshape(-1, 4)
                               for g, a, b, m in zip(gt, res["det_off"][:-1], res["det_off"][1:], matched)])
    np.testing.assert_array_equal(alloc_gt, GOLD[k + "alloc_gt_box"])


@pytest.mark.parametrize("dataset", ["kitti", "bdd"])
def test_pseudo_audit_members_totals_and_summary(dataset):
    au = audited(dataset)
    k = dataset + "_"
    for member in ("n_gts_perim", "n_pred_perim", "n_gt_matches", "n_extra_detections"):
        np.testing.assert_array_equal(np.asarray(getattr(au, member)), GOLD[k + member])
    assert np.array_equal(bits(au.n_missing_dets), bits(GOLD[k + "n_missing_dets"]))
    np.testing.assert_array_equal(np.concatenate(au.matched_preds), GOLD[k + "matched_preds"])
    np.testing.assert_array_equal(np.concatenate(au.nomatch_preds), GOLD[k + "nomatch_preds"])
    assert np.array_equal(bits(np.concatenate(au.gt_max_iou)), bits(GOLD[k + "gt_max_iou"]))
    np.testing.assert_array_equal(np.concatenate(au.gt_best_det), GOLD[k + "gt_best_det"])
    for side in ("gt", "pseudo"):
        got_cls = [str(c) for im in au.allocated_dets[side]["class"] for c in im]
        assert got_cls == [str(c) for c in GOLD[k + "alloc_%s_class" % side]]
        got_box = np.asarray([b for im in au.allocated_dets[side]["box"] for b in im], np.float64).reshape(-1, 4)
        np.testing.assert_array_equal(got_box, GOLD[k + "alloc_%s_box" % side])
    text = str(GOLD[k + "print_data"][0])
    assert numbers(au.summary()) == numbers(text)
    assert "nan" in numbers(text)                                     # a class without a matched row
    if int(np.__version__.split(".")[0]) == int(GOLD["numpy_major"][0]):
        assert au.summary() == text
    t, p = au.totals(), au.percls()
    assert int(t["n_gts"]) == int(GOLD[k + "n_gts_perim"].sum()) and int(t["found_gts"]) == int(GOLD[k + "n_gt_matches"].sum())
    assert np.isnan(p["miou"][au.used_classes[6]]) and np.isnan(p["acc"][au.used_classes[6]])


def test_planted_cases():
    names, gt, dets, cls = fixture("bdd")                            # the fixture's own order: images 0..3 are the designed ones
    res = R.audit([g[0] for g in gt], [d[0] for d in dets], THR)
    g, d = res["gt_off"], res["det_off"]
    # image 0: label 0 takes row 0, which chose label 1; row 0's mIoU (0.5) is below its maximum (0.8); row 2 is missing
    assert list(res["gt_best_det"][g[0]:g[1]]) == [1, 1, 0] and list(res["det_alloc_gt"][d[0]:d[1]]) == [0, 1]
    assert res["det_alloc_miou"][d[0]] == 0.5 and res["gt_max_iou"][g[0]] == 0.8 and res["det_alloc_pair_iou"][d[0]] == 0.5
    assert list(res["gt_alloc_det"][g[0]:g[1]]) == [0, 1, -1] and list(res["gt_flags"][g[0]:g[1]]) == [0, 0, R.GT_NOMATCH]
    # image 1: duplicate labels, the first wins and the second is not extra; the duplicate of an allocated row is not unmatched
    assert list(res["gt_best_det"][g[1]:g[2]]) == [0, 0, 2] and list(res["det_flags"][d[1]:d[2]]) == [0, 0, 0]
    assert list(res["gt_alloc_det"][g[1]:g[2]]) == [0, -1, 2] and list(res["gt_flags"][g[1]:g[2]]) == [0, 0, 0]
    # image 2: exactly 0.5, 0.75, 0.9, nothing missing
    assert list(res["gt_max_iou"][g[2]:g[3]]) == [0.5, 0.75, 0.9] and res["n_matches"][2] == 3
    # image 3: a row that touches nothing; an extra label
    assert res["gt_max_iou"][g[3]] == 0.0 and res["gt_best_det"][g[3]] == 0 and res["det_flags"][d[3] + 2] == R.DET_EXTRA
    assert (res["det_alloc_miou"] < res["gt_max_iou"][np.maximum(res["det_alloc_gt"], 0) + np.repeat(g[:-1], np.diff(d))])[res["det_alloc_gt"] >= 0].any()


def _write_kitti_inputs(tmp_path):
    names, _, _, _ = fixture("kitti")
    det_dir, gt_dir = tmp_path / "det", tmp_path / "gt"
    det_dir.mkdir(), gt_dir.mkdir()
    for i, stem in enumerate(STEMS):
        (det_dir / (stem + ".txt")).write_text(str(GOLD["kitti_det_texts"][i]))
        (gt_dir / (stem + ".txt")).write_text(str(GOLD["kitti_gt_texts"][i]))
    return names, str(det_dir), str(gt_dir)


def test_readers(tmp_path):
    names, det_dir, gt_dir = _write_kitti_inputs(tmp_path)
    _, gt, dets, _ = fixture("kitti")
    for nm, g, d in zip(names, gt, dets):
        for folder, want in ((gt_dir, g), (det_dir, d)):
            objs = pa.read_kitti_annotations(os.path.join(folder, nm), KITTI)
            assert [o["bbox"] for o in objs] == want[0] and [o["class"] for o in objs] == list(want[1])
    items = json.loads(str(GOLD["bdd_gt_json"][0]))
    names, gt, _, _ = fixture("bdd")
    for nm, g in zip(names, gt):
        objs = pa.read_bdd_annotations(items, nm, BDD)
        assert [o["bbox"] for o in objs] == g[0] and [o["class"] for o in objs] == list(g[1])
    with pytest.raises(ValueError, match="not among"):
        pa.read_bdd_annotations(items, "nowhere.jpg", BDD)


@pytest.mark.parametrize("method", METHODS)
def test_kitti_writer_bytes_and_second_audit(tmp_path, method):
    names, det_dir, gt_dir = _write_kitti_inputs(tmp_path)
    au = audited("kitti")
    cor = pa.corrected_pseudo(au, method)
    out = tmp_path / "out"
    written = writers.write_kitti_corrected_pseudo(det_dir, gt_dir, str(out), KITTI, au, cor)
    files = sorted(os.listdir(out))
    assert files == [str(f) for f in GOLD["kitti_%s_files" % method]] and written == len(files)
    for f, want in zip(files, GOLD["kitti_%s_texts" % method]):
        assert (out / f).read_text() == str(want), f
    new_data = str(GOLD["kitti_%s_output" % method][0]).split("new data: ")[1]
    if method == "nonoise":                                           # the 83-character cut runs lines together: audit the files
        again = pa.audit_pseudo_labels([pa.read_kitti_annotations(os.path.join(gt_dir, f), KITTI) for f in files],
                                       [pa.read_kitti_annotations(str(out / f), KITTI) for f in files], KITTI, THR, names=files, audit=R.audit)
        assert any(len(line) > 83 for t in GOLD["kitti_det_texts"] for line in str(t).splitlines(True))
        assert all(len(seg) <= 83 for f in files for seg in re.findall(r"[A-Z][a-z_]+ [^A-Z]*", (out / f).read_text()))
    else:
        nm2, gt2, dets2 = pa.corrected_arrays(au, cor, "KITTI")
        assert sorted(nm2) == files
        again = pa.audit_pseudo_labels(gt2, dets2, KITTI, THR, names=nm2, audit=R.audit)
    assert numbers(again.summary()) == numbers(new_data)


@pytest.mark.parametrize("method", METHODS)
def test_bdd_writer_bytes_and_second_audit(tmp_path, method):
    au = audited("bdd")
    cor = pa.corrected_pseudo(au, **pa.METHODS[method])
    pred, gtj = json.loads(str(GOLD["bdd_det_json"][0])), json.loads(str(GOLD["bdd_gt_json"][0]))
    before = json.dumps(pred)
    n = writers.write_bdd_corrected_pseudo(pred, gtj, str(tmp_path), BDD, au, cor)
    text = (tmp_path / "pseudo_labels.json").read_text()
    assert text == str(GOLD["bdd_%s_text" % method][0]) and n == len(json.loads(text))
    assert json.dumps(pred) == before                                 # the input is not modified
    nm2, gt2, dets2 = pa.corrected_arrays(au, cor, "BDD100K")
    assert nm2 == [it["name"] for it in json.loads(text)]
    again = pa.audit_pseudo_labels(gt2, dets2, BDD, THR, names=nm2, audit=R.audit)
    new_data = str(GOLD["bdd_%s_output" % method][0]).split("new data: ")[1]
    assert numbers(again.summary()) == numbers(new_data)
    if method == "highprec":                                          # image 0 reaches 0.8 at most: its selector is empty, it stays
        assert len(cor.selector[0]) == 0 and json.loads(text)[0] == pred[0]


def test_corrected_pseudo_decisions_and_refusals(tmp_path):
    au = audited("bdd")
    noise = pa.corrected_pseudo(au, "nonoise")
    assert noise.iou_thr == 0.75 and pa.corrected_pseudo(au, "highprec").iou_thr == 0.9 and pa.corrected_pseudo(au, "nofd").iou_thr == 0.5
    # image 3: label 0 (IoU 0.675) is below 0.75 and stays; label 1 (40 / 41) is replaced by row 2
    assert noise.replacements[3].tolist() == [[1, 2]] and list(noise.kept[3]) == [0, 1, 2]
    both = pa.corrected_pseudo(au, remove_noise=True, remove_fds=True)           # remove_fds overrides the replacement
    assert both.replacements[3].shape == (0, 2) and list(both.kept[3]) == [1]
    fix = pa.corrected_pseudo(au, "fixmd")
    assert list(fix.appended[0]) == [] and list(fix.appended[3]) == [0] and not any(fix.dropped)
    nomd = pa.corrected_pseudo(au, "nomd")
    assert nomd.dropped[0] and not nomd.dropped[2]
    with pytest.raises(ValueError, match="unknown method"):
        pa.corrected_pseudo(au, "nomds")
    with pytest.raises(ValueError, match="unknown flag"):
        pa.corrected_pseudo(au, remove_md=True)
    with pytest.raises(ValueError, match="not both"):
        pa.corrected_pseudo(au, "nomd", add_mds=True)
    # a pseudo label outside the used classes: the reference's indices would disagree silently
    pred, gtj = json.loads(str(GOLD["bdd_det_json"][0])), json.loads(str(GOLD["bdd_gt_json"][0]))
    pred[2]["labels"].insert(1, {"category": "lane", "attributes": {}, "poly2d": [], "id": 7})
    with pytest.raises(ValueError, match="not of a used class"):
        writers.write_bdd_corrected_pseudo(pred, gtj, str(tmp_path), BDD, au, fix)
    pred = json.loads(str(GOLD["bdd_det_json"][0]))
    with pytest.raises(ValueError, match="in its order"):
        writers.write_bdd_corrected_pseudo(pred[::-1], gtj, str(tmp_path), BDD, au, fix)
    names, det_dir, gt_dir = _write_kitti_inputs(tmp_path)
    ak = audited("kitti")
    with open(os.path.join(det_dir, names[0]), "a") as f:
        f.write("DontCare -1 -1 -10 5.00 6.00 7.00 8.00 -1 -1 -1 -1000 -1000 -1000 -10\n")
    with pytest.raises(ValueError, match="not of a used class"):
        writers.write_kitti_corrected_pseudo(det_dir, gt_dir, str(tmp_path / "o"), KITTI, ak, pa.corrected_pseudo(ak, "fixmd"))


def test_pls_scores_and_selection():
    order = [STEMS.index(str(nm)[:-4]) for nm in GOLD["pls_images_data"]]
    gt, dets = _images("gt", KITTI), _images("det", KITTI)
    names = [STEMS[i] + ".txt" for i in order]
    au = pa.audit_pseudo_labels([gt[i] for i in order], [dets[i] for i in order], KITTI, THR, names=names, audit=R.audit)
    off = np.concatenate([[0], np.cumsum(GOLD["scores_n"])])
    scores = [GOLD["scores"][off[i]:off[i + 1]] for i in order]
    beta, top_k, seed = (float(v) for v in GOLD["beta_topk_seed"])
    s = pa.pls_scores(au, scores, int(GOLD["delta_s"][0]), beta)
    for key, f in (("s_i", "score_si"), ("c_i", "score_ci"), ("max_drop", "max_drop"), ("mean_drop", "mean_drop"), ("avg_score", "avg_score"),
                   ("std_drop", "std_drop"), ("md", "md")):
        assert np.array_equal(bits(s[key]), bits(GOLD["pls_" + f])), key
    np.testing.assert_array_equal(np.asarray(s["n_det"]), GOLD["pls_n_det"])
    assert np.array_equal(bits(s["d_i"]), bits((1 - beta) * GOLD["pls_score_si"] + GOLD["pls_score_ci"] * beta))
    assert np.array_equal(bits(pa.pls_scores(au, scores, 0.4, beta)["s_i"]), bits(s["s_i"]))
    top, bot, rand = pa.pls_select(s["d_i"], top_k, np.random.RandomState(int(seed)))
    for sel, tag in ((top, "top"), (bot, "bot"), (rand, "rand")):
        assert sorted(names[i] for i in sel) == [str(f) for f in GOLD["pls_%s_files" % tag]], tag
    with pytest.raises(ValueError, match="scores of"):
        pa.pls_scores(au, scores[:-1], 4, beta)


def test_merge_of_two_halves_is_the_whole():
    names, gt, dets, cls = fixture("kitti")
    whole = audited("kitti")
    h = N // 2
    a = pa.audit_pseudo_labels(gt[:h], dets[:h], cls, THR, names=names[:h], audit=R.audit)
    b = pa.audit_pseudo_labels(gt[h:], dets[h:], cls, THR, names=names[h:], audit=R.audit)
    assert a.merge(b) is a and len(a) == N and a.names == whole.names
    assert a.summary() == whole.summary() and a.n_gt_matches == whole.n_gt_matches
    assert [list(m) for m in a.matched_preds] == [list(m) for m in whole.matched_preds] and a.matched_gt == whole.matched_gt
    assert a.allocated_dets["gt"]["box"] == whole.allocated_dets["gt"]["box"]
    with pytest.raises(ValueError, match="different classes"):
        a.merge(audited("bdd"))


def test_allow_empty_raises_or_defines():
    names, gt, dets, cls = fixture("kitti")
    gt, dets = list(gt[:3]), list(dets[:3])
    gt[1] = ([], np.zeros(0, "<U1"))
    with pytest.raises(ValueError, match=re.escape(repr(names[1]))):
        pa.audit_pseudo_labels(gt, dets, cls, THR, names=names[:3], audit=R.audit)
    au = pa.audit_pseudo_labels(gt, dets, cls, THR, names=names[:3], allow_empty=True, audit=R.audit)
    assert au.n_gt_matches[1] == 0 and au.extra_dets[1] == list(range(len(dets[1][0]))) and list(au.matched_preds[1]) == []
    dets[2] = []
    with pytest.raises(ValueError, match="0 pseudo labels"):
        pa.audit_pseudo_labels(gt[2:], dets[2:], cls, THR, audit=R.audit)
    au = pa.audit_pseudo_labels(gt[2:], dets[2:], cls, THR, allow_empty=True, audit=R.audit)
    assert au.nomatch_gts[0] == list(range(au.n_gts_perim[0])) and au.n_missing_dets[0] == 1.0


def test_audit_np_refuses_bad_values_before_the_library():
    box = [[0.0, 0.0, 1.0, 1.0]]
    with pytest.raises(ValueError, match="pseudo-label boxes of image 1"):
        pa.audit_np([box, box], [box, [[0.0, np.nan, 1.0, 1.0]]])
    with pytest.raises(ValueError, match="gt_iou_thr"):
        pa.audit_np([box], [box], gt_iou_thr=float("nan"))
    with pytest.raises(ValueError, match="ground truth of 2 images"):
        pa.audit_np([box, box], [box])
    with pytest.raises(ValueError, match="0 images"):
        pa.audit_np([], [])


def test_binding_and_limits_match_the_header():
    text = open(capi.HEADER).read()
    for name, value in (("UDA_AUDIT_MAX_G", capi.AUDIT_MAX_G), ("UDA_AUDIT_MAX_D", capi.AUDIT_MAX_D), ("UDA_AUDIT_MAX_B", capi.AUDIT_MAX_B),
                        ("UDA_AUDIT_DET_EXTRA", capi.AUDIT_DET_EXTRA), ("UDA_AUDIT_GT_NOMATCH", capi.AUDIT_GT_NOMATCH)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value
    assert "uda_pseudo_audit_np" in capi.EXPORTS and len(capi._SIGNATURES["uda_pseudo_audit_np"][1]) == 18


def test_entry_point_fails_loudly_without_gpu():
    """Without a HIP device the entry point returns 1 and says who failed, in HIP's words; a refusal comes before the device."""
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from uda_amd import capi\n"
            "lib = capi.load()\n"
            "b = np.array([[0., 0., 1., 1.]]); off = np.array([0, 1], np.int64); bad = np.array([0, -1], np.int64)\n"
            "def call(go, thr):\n"
            "    return lib.uda_pseudo_audit_np(0, 1, b.ctypes.data, go.ctypes.data, b.ctypes.data, off.ctypes.data, thr,\n"
            "                                   *([None] * 11))\n"
            "for go, thr in ((off, 0.5), (bad, 0.5), (off, float('nan'))):\n"
            "    print('%%d|%%s' %% (call(go, thr), lib.uda_last_error(None).decode()))\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [line.split("|", 1) for line in out.stdout.splitlines() if "|" in line]
    assert len(rows) == 3 and all(rc == "1" and msg.startswith("uda_pseudo_audit_np: ") for rc, msg in rows), out.stdout
    assert "do not ascend" in rows[1][1] and "not finite" in rows[2][1] and "ascend" not in rows[0][1] and len(rows[0][1]) > 25
