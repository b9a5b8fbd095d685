"""Generates tests/golden/glc_golden.npz by running the REAL reference methods `AdvancedLabels.mds`, `.mistakes`, `.noisy_boxes`
and `.corrected_gt` (src/ssl_utils/glc.py) and `Parent_SSL.read_predictions` (src/ssl_utils/parent.py) on a prediction file and
label files written here.  Run once where a checkout of the reference exists; the .npz (data only) is committed and is what
the tests read.

    python tests/golden/make_glc_golden.py <src directory of the reference's checkout>

How the class is reached: the heavy imports (tensorflow and friends, cv2, seaborn, ijson, skimage, aug, the TFRecord creators) are stubbed;
`ssl_utils.parent` is imported and `Parent_SSL.__init__` replaced by a function that raises a private exception; glc.py is then
executed through importlib - its module-level `AdvancedLabels(...)` call stops at `super().__init__` before it touches any file,
and the class is left in the module's namespace.  An object made with `__new__` gets what `AdvancedLabels.__init__` would have
given it: pred_box / score_perim / ciou_perim / pred_cls from the reference's own `read_predictions` on the file written here,
gt_box / gt_cls from its own `_read_kitti_annotations`, the four thresholds, and ious / matched_det / ious_gt by the statements of
glc.py:182-187 with the reference's `calc_iou_np`.  `corrected_gt` runs in a temporary directory with the TFRecord creators and
`generate_commands_and_create_dirs` stubbed.

The fixture holds the detections as dense float64 arrays [n, M, ...] (rows at or below min_score are NOT in the file; some lie
between kept rows), the ground truth padded with class -1, and per case (a set of thresholds) the reference's returns and the
bytes of the files it wrote.  The `le` rule of the synthetic branch (:468-472) cannot be driven without its random drops: its
expected flags are the reference's statement evaluated here on the reference's own `ious`.  All coordinates are multiples of
1/8, so float32 and its shortest decimal agree.

Planted (asserted below): rows matched to one detection whose first row does not meet the noisy conditions while a later one
does (two rows: image 0, three rows: image 1); a mistake row whose first-kept match is in `better` (image 2, where rank 0 is
not kept); duplicate detection boxes (image 1); every threshold hit exactly (image 3: cons_iou == iou_consist, iou_gt ==
correct_max_inter, score == correct_score); a detection of maximum IoU exactly 0.25 under md_max_inter 0.25 (image 4)."""
import copy
import importlib.util
import json
import os
import sys
import tempfile
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_glc_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
for name in ("tensorflow", "tensorflow_probability", "uncertainty_toolbox", "uncertainty_toolbox.viz", "cv2", "seaborn", "ijson", "skimage", "aug", "aug.autoaugment", "datasets", "datasets.BDD100K",
             "datasets.BDD100K.bdd_tf_creator", "datasets.KITTI", "datasets.KITTI.kitti_tf_creator"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
import numpy as np                       # noqa: E402
import ssl_utils.parent as P             # noqa: E402  (the reference module)
from utils_box import calc_iou_np        # noqa: E402


class _Stop(Exception):
    pass


def _stop(self, *a, **k):
    raise _Stop()


P.Parent_SSL.__init__ = _stop
_spec = importlib.util.spec_from_file_location("glc_reference", os.path.join(REF_SRC, "ssl_utils", "glc.py"))
GLC = importlib.util.module_from_spec(_spec)
try:
    _spec.loader.exec_module(GLC)
    raise SystemExit("glc.py ran through: its module-level call was expected to stop in Parent_SSL.__init__")
except _Stop:
    pass
AdvancedLabels = GLC.AdvancedLabels
GLC.generate_commands_and_create_dirs = lambda *a, **k: None

M, G = 12, 8
MIN_SCORE = 0.1
KITTI = ["Car", "Van", "Truck", "Pedestrian", "Person_sitting", "Cyclist", "Tram"]
BDD = ["pedestrian", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle", "traffic light", "traffic sign"]
# iou_consist, md_max_inter, correct_max_inter, correct_score
CASES = [(0.90, 0, 1.0, 0.40), (0.90, 0.25, 0.75, 0.40), (0.90, 0, 0.5, 0.0)]
FAR = [900.0, 900.0, 950.0, 990.0]


def designed():
    """-> per image (detections [(box, score, cons_iou, class)], ground truth [(box, class)])."""
    im = []
    # 0: two rows matched to rank 0; row 0 (IoU 1600 / 1680 > 0.75) fails case 1's correct_max_inter, row 1 (IoU 0.5) meets it
    im.append(([([10, 10, 50, 50], 0.9, 0.95, 1), ([200, 200, 240, 260], 0.7, 0.5, 2)],
               [([10, 10, 50, 52], 1), ([10, 10, 50, 90], 1), ([200, 200, 240, 250], 2)]))
    # 1: duplicate boxes at ranks 1 and 2 (tie to rank 1); three rows matched to rank 1, the first two above 0.75, the third at 0.5;
    #    rank 0 touches no ground truth and is consistent: a missing label
    im.append(([([400, 400, 440.5, 440.5], 0.95, 0.99, 3), ([20, 20, 60, 60], 0.85, 0.92, 1), ([20, 20, 60, 60], 0.8, 0.99, 1),
                ([300, 20, 330, 50], 0.05, 0.99, 4)],
               [([20, 20, 60, 61], 1), ([20, 20, 61, 60], 1), ([20, 20, 60, 100], 6), ([300, 20, 330, 50], 4)]))
    # 2: rank 0 is not kept; row 0 touches nothing and is matched to the first kept detection (rank 1), which row 1 puts in `better`
    im.append(([([100, 100, 150, 150], 0.05, 0.99, 1), ([100, 100, 150, 150.5], 0.8, 0.95, 2), ([0.125, 0.25, 30.5, 40.75], 0.6, 0.2, 5)],
               [(FAR, 7), ([100, 100, 150, 151], 2), ([0, 0, 30, 40], 5)]))
    # 3: the thresholds hit exactly.  rank 0: cons_iou == 0.90, touches nothing -> md yes (>=); rank 1: cons_iou == 0.90 -> noisy no
    #    (strict); rank 2: score == 0.40 and an identical ground-truth box (IoU == 1.0 == correct_max_inter of case 0) -> noisy yes;
    #    rank 3: IoU exactly 0.5 (== correct_max_inter of case 2) with a low-score row in between
    im.append(([([500, 500, 540, 540], 0.9, 0.90, 1), ([10, 10, 30, 30], 0.9, 0.90, 1), ([100, 10, 130, 30], 0.40, 0.95, 2),
                ([700, 700, 710, 710], 0.1, 0.99, 1), ([0, 100, 2, 102], 0.5, 0.97, 3)],
               [([10, 10, 30, 31], 1), ([100, 10, 130, 30], 2), ([0, 100, 2, 104], 3)]))
    # 4: maximum IoU exactly 0.25 ([0,0,2,2] in [0,0,2,8]); rank 1 touches nothing (0 <= 0.25 under the `le` rule only)
    im.append(([([0, 0, 2, 2], 0.9, 0.95, 1), ([50, 50, 60, 60], 0.8, 0.95, 2), ([80, 80, 90, 90.5], 0.7, 0.95, 2)],
               [([0, 0, 2, 8], 1), ([80, 80, 90, 92], 2)]))
    return im


def random_images(rng, count):
    im = []
    for _ in range(count):
        k = int(rng.integers(4, M + 1))
        g = int(rng.integers(2, G + 1))
        gts = []
        for _ in range(g):
            y, x = rng.integers(0, 1600, 2) / 8.0
            h, w = rng.integers(80, 480, 2) / 8.0
            gts.append(([y, x, y + h, x + w], int(rng.integers(1, 8))))
        dets = []
        for r in range(k):
            if r < g and rng.random() < 0.8:                    # a jittered copy of a ground-truth box
                b = np.asarray(gts[r][0]) + rng.integers(-24, 25, 4) / 8.0
            else:
                y, x = rng.integers(0, 1600, 2) / 8.0
                b = np.asarray([y, x, y + rng.integers(80, 480) / 8.0, x + rng.integers(80, 480) / 8.0])
            dets.append((list(b), float(np.round(rng.uniform(0.02, 0.99), 4)), float(np.round(rng.uniform(0.3, 1.0), 4)),
                         int(rng.integers(1, 8))))
        dets.sort(key=lambda d: -d[1])
        im.append((dets, gts))
    return im


def dense(images):
    n = len(images)
    boxes, scores, cons, classes = np.zeros((n, M, 4)), np.zeros((n, M)), np.zeros((n, M)), np.zeros((n, M))
    gtb, gtc = np.zeros((n, G, 4)), np.full((n, G), -1.0)
    for i, (dets, gts) in enumerate(images):
        for k, (b, s, c, cl) in enumerate(dets):
            boxes[i, k], scores[i, k], cons[i, k], classes[i, k] = b, s, c, cl
        for g, (b, cl) in enumerate(gts):
            gtb[i, g], gtc[i, g] = b, cl
    assert (boxes * 8 == np.round(boxes * 8)).all() and (gtb * 8 == np.round(gtb * 8)).all()
    return boxes, scores, cons, classes, gtb, gtc


def write_predictions(path, names, boxes, scores, cons, classes):
    with open(path, "w") as f:
        for i, name in enumerate(names):
            for r in np.where(scores[i] > MIN_SCORE)[0]:
                d = {"image_name": name + ".jpg", "score_thresh": MIN_SCORE, "det_score": float(scores[i, r]),
                     "bbox": [float(v) for v in boxes[i, r]], "class": float(classes[i, r]), "cons_iou": float(cons[i, r]),
                     "cons_cls": True}
                f.write(str(d) + "\n")


def write_kitti_labels(folder, names, gtb, gtc):
    os.makedirs(folder)
    texts = []
    for i, name in enumerate(names):
        lines = []
        for g in np.where(gtc[i] > 0)[0]:
            y1, x1, y2, x2 = gtb[i, g]
            lines.append("%s 0.00 %d -1.57 %s %s %s %s 1.50 1.60 3.90 1.00 1.50 20.00 -1.50"
                         % (KITTI[int(gtc[i, g]) - 1], g % 3, repr(float(x1)), "%.3f" % y1, "%.3f" % x2, repr(float(y2))))
            if g == 0:
                lines.append("DontCare -1 -1 -10 5.00 6.00 7.00 8.00 -1 -1 -1 -1000 -1000 -1000 -10")
        text = "\n".join(lines) + "\n"
        texts.append(text)
        with open(os.path.join(folder, name + ".txt"), "w") as f:
            f.write(text)
    return texts


def bdd_labels(names, gtb, gtc):
    data = [{"name": "zzz_unlabelled.jpg", "attributes": {"weather": "clear"}, "timestamp": 10000}]
    for i, name in enumerate(names):
        labels = []
        for g in np.where(gtc[i] > 0)[0]:
            y1, x1, y2, x2 = (float(v) for v in gtb[i, g])
            labels.append({"category": BDD[int(gtc[i, g]) - 1], "attributes": {"occluded": bool(g % 2), "truncated": False,
                                                                               "trafficLightColor": "none"},
                           "manualShape": True, "box2d": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}, "id": 10 * i + int(g)})
            if g == 1:
                labels.append({"category": "lane", "attributes": {}, "poly2d": [], "id": 999})
        data.append({"name": name + ".jpg", "attributes": {"weather": "overcast"}, "timestamp": 10000, "labels": labels})
        if i == 1:
            data.append({"name": "not_predicted.jpg", "attributes": {}, "timestamp": 10000,
                         "labels": [{"category": "car", "attributes": {}, "box2d": {"x1": 1.0, "y1": 2.0, "x2": 3.0, "y2": 4.0}, "id": 5}]})
    return data


def make_object(pred, gt_box, gt_cls, case):
    o = AdvancedLabels.__new__(AdvancedLabels)
    _, o.score_perim, o.pred_cls, o.pred_box, o.ciou_perim, _ = pred
    o.gt_box, o.gt_cls = gt_box, gt_cls
    o.consist_intersection, o.md_max_inter, o.correct_max_inter, o.correct_score = case
    o.ious = [[calc_iou_np([gt], o.pred_box[i]) for gt in o.gt_box[i]] for i in range(len(o.gt_box))]      # glc.py:182-187
    o.matched_det = [np.argmax(iou, axis=-1) for iou in o.ious]
    o.ious_gt = [np.max(iou, axis=-1) for iou in o.ious]
    return o


def read_tree(folder):
    files = sorted(os.listdir(folder))
    return files, [open(os.path.join(folder, f)).read() for f in files]


def main():
    rng = np.random.default_rng(20241019)
    images = designed() + random_images(rng, 5)
    n = len(images)
    names = ["%06d" % (5 * i + 2) for i in range(n)]
    boxes, scores, cons, classes, gtb, gtc = dense(images)
    assert ((scores > MIN_SCORE).sum(1) > 0).all() and ((gtc > 0).sum(1) > 0).all()
    out = {"names": np.array(names), "min_score": np.array([MIN_SCORE]), "cases": np.array(CASES, np.float64), "boxes": boxes,
           "scores": scores, "cons_iou": cons, "classes": classes, "gt_boxes": gtb, "gt_classes": gtc,
           "kitti_classes": np.array(KITTI), "bdd_classes": np.array(BDD)}
    with tempfile.TemporaryDirectory() as td:
        pred_path = os.path.join(td, "prediction_data.txt")
        write_predictions(pred_path, names, boxes, scores, cons, classes)
        pred = P.Parent_SSL.read_predictions(pred_path, "score", True)
        assert list(pred[0]) == [nm + ".jpg" for nm in names] and len(pred) == 6
        for i in range(n):                                        # the parsed literals are the dense arrays' kept rows
            kept = np.where(scores[i] > MIN_SCORE)[0]
            assert np.array_equal(np.asarray(pred[3][i]), boxes[i, kept]) and np.array_equal(np.asarray(pred[1][i]), scores[i, kept])
            assert np.array_equal(np.asarray(pred[4][i]), cons[i, kept]) and np.array_equal(np.asarray(pred[2][i]), classes[i, kept])
        general = os.path.join(td, "general")
        label_dir = os.path.join(general, "datasets", "KITTI", "training", "label_2")
        out["kitti_label_texts"] = np.array(write_kitti_labels(label_dir, names, gtb, gtc))
        with open(os.path.join(general, "datasets", "KITTI", "vaL_index_list.txt"), "w") as f:
            f.write("0\n")
        kitti_objs = [P.Parent_SSL._read_kitti_annotations(os.path.join(label_dir, nm + ".txt"), KITTI) for nm in names]
        gt_box = [[[b["bbox"][1], b["bbox"][0], b["bbox"][3], b["bbox"][2]] for b in im] for im in kitti_objs]   # glc.py:174-177
        gt_cls = [[b["class"] for b in im] for im in kitti_objs]
        for i in range(n):
            assert np.array_equal(np.asarray(gt_box[i]), gtb[i, gtc[i] > 0])
        bdd = bdd_labels(names, gtb, gtc)
        out["bdd_json"] = np.array([json.dumps(bdd)])
        for ci, case in enumerate(CASES):
            o = make_object(pred, gt_box, gt_cls, case)
            extra = o.mds(False, False)
            wrong = o.mistakes(False, False)
            corrected = o.noisy_boxes(False, False)
            le = [np.less_equal(np.max(giou, axis=0), o.md_max_inter) * np.greater_equal(ciou, o.consist_intersection)
                  for ciou, giou in zip(o.ciou_perim, o.ious)]                                            # glc.py:468-472
            out["k%d_matched" % ci] = np.concatenate(o.matched_det)
            out["k%d_iou" % ci] = np.concatenate(o.ious_gt)
            out["k%d_wrong_image" % ci] = np.concatenate([np.full(len(w), i) for i, w in enumerate(wrong)]).astype(np.int64)
            out["k%d_wrong_row" % ci] = np.concatenate(wrong).astype(np.int64)
            out["k%d_extra" % ci] = np.concatenate(extra).astype(bool)
            out["k%d_extra_le" % ci] = np.concatenate(le).astype(bool)
            out["k%d_corrected" % ci] = np.concatenate([np.asarray(c, np.float64).reshape(-1, 4) for c in corrected])
            changed = [(i, g) for i in range(n) for g in range(len(gt_box[i])) if list(corrected[i][g]) != list(gt_box[i][g])]
            print("case", case, "mistakes", len(out["k%d_wrong_row" % ci]), "md", int(out["k%d_extra" % ci].sum()), "md(le)",
                  int(out["k%d_extra_le" % ci].sum()), "replaced", changed)
            if ci == 0:
                assert (0, 0) in changed and (1, 0) in changed and (2, 0) in changed and 0 in wrong[2]
                assert (3, 1) not in changed and (3, 0) not in changed      # identical box replaced by itself; cons_iou == 0.90 is not > 0.90
                assert extra[3][0] and extra[1][0] and not extra[4][0]
                assert o.matched_det[1][0] == 1 and o.matched_det[1][2] == 1 and o.matched_det[2][0] == 0
            if ci == 1:
                # the first rows fail correct_max_inter 0.75, a later row meets it, and the FIRST row is replaced
                assert o.ious_gt[0][0] > 0.75 and o.ious_gt[0][1] == 0.5 and (0, 0) in changed and (0, 1) not in changed
                assert min(o.ious_gt[1][0], o.ious_gt[1][1]) > 0.75 and o.ious_gt[1][2] == 0.5 and (1, 0) in changed
                assert (1, 1) not in changed and (1, 2) not in changed
                assert extra[4][0] and not extra[4][1] and le[4][0] and le[4][1] and np.max(o.ious[4], axis=0)[0] == 0.25
            if ci == 2:
                assert o.ious_gt[3][2] == 0.5 and (3, 2) in changed
            # the files: KITTI, then BDD (each mode into a folder of its own, as mds / mistakes / noisy_boxes call it)
            for ds in ("KITTI", "BDD100K"):
                o.dataset, o.general_path, o.added_name = ds, general, "glc"
                o.dataset_path = os.path.join(general, "datasets", ds) + "/"
                o.labeled_indices, o.labeled_portion, o.num_labeled = [0], 0, 0
                if ds == "KITTI":
                    o.used_classes, o.gt_labels_folder = KITTI, label_dir
                    o.clean_perd_im_names = np.asarray([nm + ".txt" for nm in names])
                else:
                    o.used_classes = BDD
                    o.clean_perd_im_names = np.asarray([nm + ".jpg" for nm in names])
                modes = (("remove", dict(remove_mistakes=True, wrong_gt=wrong)),
                         ("add", dict(add_missingboxes=True, missing_gt_boxes=extra)),
                         ("correct", dict(correct_boxes=True, corrected_gt_boxes=corrected)))
                for tag, kw in modes:
                    o.bdd_data = copy.deepcopy(bdd)               # (corrected_gt writes into the loaded json's objects)
                    o.corrected_gt(folder_name="/%s/" % tag, **kw)
                    files, texts = read_tree(o.dataset_path + "/pseudo_labels/glc/%s/" % tag)
                    key = "k%d_%s_%s" % (ci, "kitti" if ds == "KITTI" else "bdd", tag)
                    out[key + "_files"], out[key + "_texts"] = np.array(files), np.array(texts)
    dst = os.path.join(HERE, "glc_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 100000


if __name__ == "__main__":
    main()
