"""Generates tests/golden/audit_golden.npz by running the REAL reference methods `Parent_SSL.extract_pseudo_gt_data` (with
`_percls_analysis`, src/ssl_utils/parent.py:1567-1813), `ThreeDproblem.corrected_pseudo` (src/ssl_utils/3d.py:80-255; all six
methods, KITTI and BDD100K) and `Advanced_Pseudo_Labels._pls` (src/ssl_utils/pls.py:102-282; KITTI) on label files written here.
Run once where a checkout of the reference exists; the .npz (data only) is committed and is what the tests read.

    python tests/golden/make_audit_golden.py <src directory of the reference's checkout>

How the classes are reached: the heavy imports (tensorflow and friends, cv2, seaborn, ijson, skimage, sklearn, aug, the
TFRecord creators) are stubbed; `ssl_utils.parent` is imported and `Parent_SSL.__init__` replaced by a function that raises a
private exception; 3d.py and pls.py are executed through importlib - their module-level calls stop at `super().__init__` before
they touch any file, and the classes are left in the modules' namespaces.  Objects made with `__new__` get the attributes the
constructors would have given them.  `ijson.items` (a json.load), `roc_curve`, `auc` and `plt` are stubbed in the modules'
namespaces and np.random.seed is fixed before `_pls`.

Recorded: the inputs (boxes, classes, the label files' texts, both jsons, the scores `_pls` reads), the members of the audit,
`print_data`, numpy's major version, per method the bytes of every written file and the `new data` text of its output.txt, the
.npy files `_pls` saves with its three selections, and `images_data` in the order os.listdir gave.  All coordinates are multiples
of 1/8.  What is planted is asserted in main()."""
import copy
import importlib.util
import json
import os
import sys
import tempfile
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_audit_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
for name in ("tensorflow", "tensorflow_probability", "uncertainty_toolbox", "uncertainty_toolbox.viz", "cv2", "seaborn", "ijson", "skimage", "aug",
             "aug.autoaugment", "datasets", "datasets.BDD100K", "datasets.BDD100K.bdd_tf_creator", "datasets.KITTI",
             "datasets.KITTI.kitti_tf_creator", "sklearn", "sklearn.metrics"):
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


def load_stopped(fname, modname):
    spec = importlib.util.spec_from_file_location(modname, os.path.join(REF_SRC, "ssl_utils", fname))
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
        raise SystemExit("%s ran through: its module-level call was expected to stop in Parent_SSL.__init__" % fname)
    except _Stop:
        pass
    return mod


TD = load_stopped("3d.py", "threed_reference")
PLS = load_stopped("pls.py", "pls_reference")
TD.ijson = mock.MagicMock()
TD.ijson.items = lambda f, prefix: json.load(f)
PLS.plt = mock.MagicMock()
PLS.roc_curve = lambda *a, **k: (np.array([0.0, 1.0]), np.array([0.0, 1.0]), np.array([1.0, 0.0]))
PLS.auc = lambda *a, **k: 0.5

KITTI = ["Car", "Van", "Truck", "Pedestrian", "Person_sitting", "Cyclist", "Tram"]
BDD = ["pedestrian", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle", "traffic light", "traffic sign"]
METHODS = ["nomd", "nofd", "nomdfd", "fixmd", "highprec", "nonoise"]
FOLDERS = {"nomd": "_nomd_", "nofd": "_nofd_", "nomdfd": "_nofdnomd_", "fixmd": "_addmd_", "highprec": "_highprec_", "nonoise": "_nonoise_"}
FLAGS = {"nomd": dict(remove_imgs_with_mds=True), "nofd": dict(remove_fds=True), "nomdfd": dict(remove_imgs_with_mds=True, remove_fds=True),
         "fixmd": dict(add_mds=True), "highprec": dict(high_precision=True), "nonoise": dict(remove_noise=True)}
GT_IOU_THR = 0.5
BETA, TOP_K, SEED = 0.1, 0.6, 20241020
FAR = [900.0, 900.0, 950.0, 990.0]
# The classes of the random images.  Person_sitting (5) makes a KITTI line longer than 83 characters, and the reference's `nonoise`
# branch then cuts the line's end off, so that the next line runs into it and is lost to the audit that follows; an image left
# without any match makes the reference's own _percls_analysis raise under numpy 2.  Only designed image 3 carries the class.
SHORT = [1, 2, 3, 4, 6]


def designed():
    """-> per image (pseudo labels [(box, class)], ground truth [(box, class)]); classes are 1-based indices."""
    im = []
    # 0: a strip of height 8, so an IoU is the overlap of two intervals over their union.  Rows 0 and 1 choose label 1 (0.8, 0.75),
    #    row 2 chooses label 0 at exactly 0.5.  Label 0's column holds 0.5 at rows 0 and 2: the tie goes to row 0, so label 0 TAKES
    #    row 0, which did not choose it; label 1 then finds row 0 taken, the entry is invalidated, and it takes row 1.  Row 0's
    #    mIoU is 0.5, below its plain maximum 0.8; row 2 is missing.
    im.append(([([0, 0, 8, 40], 1), ([0, 10, 8, 50], 1)],
               [([0, 10, 8, 60], 1), ([0, 20, 8, 50], 2), ([0, 0, 8, 20], 1)]))
    # 1: duplicate labels 0 and 1 (the tie goes to 0); rows 0 and 1 are duplicates too and both choose label 0: row 1 is not
    #    allocated but equals an allocated row's box, so it is not in the no-match list; label 1 is not extra
    im.append(([([10, 10, 50, 50], 1), ([10, 10, 50, 50], 1), ([200, 200, 240, 260], 2)],
               [([10, 10, 50, 52], 1), ([10, 10, 50, 52], 1), ([200, 200, 240, 250], 3)]))
    # 2: maxima of exactly 0.5, 0.75 and 0.9; nothing is missing
    im.append(([([0, 0, 2, 2], 4), ([100, 0, 102, 3], 4), ([200, 0, 202, 9], 6)],
               [([0, 0, 2, 4], 4), ([100, 0, 102, 4], 4), ([200, 0, 202, 10], 6)]))
    # 3: a row that touches nothing (the only Tram: a class without a matched row), a long class name (lines above 83 characters)
    #    with an IoU between 0.5 and 0.75 (replaced under nonoise), and an extra label
    im.append(([([300, 300, 340, 340.5], 5), ([20, 20, 60, 60], 1), ([500, 100, 530.125, 150.25], 5)],
               [(FAR, 7), ([300, 300, 340, 360], 5), ([20, 20, 60, 61], 1)]))
    return im


def random_images(rng, count):
    """The 8-pixel grid of small boxes on which ties, steals and invalidations are frequent, then jittered copies."""
    im = []
    for k in range(count):
        g, d = int(rng.integers(2, 8)), int(rng.integers(2, 8))
        if k % 2 == 0:
            def boxes(n):
                y, x = rng.integers(0, 6, n) * 8.0, rng.integers(0, 6, n) * 8.0
                return [([a, b, a + h, b + w], SHORT[int(rng.integers(0, 5))]) for a, b, h, w in
                        zip(y, x, rng.integers(1, 5, n) * 8.0, rng.integers(1, 5, n) * 8.0)]
            gts, dets = boxes(g), boxes(d)
        else:
            gts = []
            for _ in range(g):
                y, x = rng.integers(0, 1600, 2) / 8.0
                h, w = rng.integers(80, 480, 2) / 8.0
                gts.append(([y, x, y + h, x + w], SHORT[int(rng.integers(0, 5))]))
            dets = []
            for r in range(d):
                if r < g and rng.random() < 0.8:
                    b = np.asarray(gts[r][0]) + rng.integers(-24, 25, 4) / 8.0
                    cl = gts[r][1] if rng.random() < 0.8 else SHORT[int(rng.integers(0, 5))]
                else:
                    y, x = rng.integers(0, 1600, 2) / 8.0
                    b = np.asarray([y, x, y + rng.integers(80, 480) / 8.0, x + rng.integers(80, 480) / 8.0])
                    cl = SHORT[int(rng.integers(0, 5))]
                dets.append(([float(v) for v in b], cl))
        im.append((dets, gts))
    return im


def has_match(dets, gts):
    ious = np.asarray([calc_iou_np([g[0]], [d[0] for d in dets]) for g in gts])
    return bool((ious.max(-1) >= GT_IOU_THR).any())


def kitti_line(cls, box, k):
    # reader order: columns 4..7 are the box as it is.  Lines stay within 83 characters, except Person_sitting's (see SHORT)
    tail = "1.50 1.60 3.90 1.00 1.50 20.00 -1.50" if cls == 5 else "1 1 3 1 1 20 -1"
    line = "%s 0.0 %d -1.5 %s %s %s %s %s" % (KITTI[cls - 1], k % 3, repr(float(box[0])), "%.3f" % box[1], "%.3f" % box[2], repr(float(box[3])), tail)
    assert (len(line) + 1 > 83) == (cls == 5)
    return line


def write_kitti(folder, names, per_image, gt):
    os.makedirs(folder)
    texts = []
    for name, objs in zip(names, per_image):
        lines = []
        for k, (box, cls) in enumerate(objs):
            lines.append(kitti_line(cls, box, k))
            if gt and k == 0:
                lines.append("DontCare -1 -1 -10 5.00 6.00 7.00 8.00 -1 -1 -1 -1000 -1000 -1000 -10")
        text = "\n".join(lines) + "\n"
        texts.append(text)
        with open(os.path.join(folder, name), "w") as f:
            f.write(text)
    return texts


def bdd_items(names, per_image, gt):
    data = []
    for i, (name, objs) in enumerate(zip(names, per_image)):
        labels = []
        for k, (box, cls) in enumerate(objs):
            y1, x1, y2, x2 = (float(v) for v in box)         # reader order: y1 x1 y2 x2
            o = {"category": BDD[cls - 1], "attributes": {"occluded": bool(k % 2), "truncated": False, "trafficLightColor": "none"},
                 "box2d": {"x1": x1, "y1": y1, "x2": x2, "y2": y2}, "id": 100 * i + k}
            if not gt:
                o["score"] = 0.5 + k / 64.0
            labels.append(o)
            if gt and k == 1:
                labels.append({"category": "lane", "attributes": {}, "poly2d": [], "id": 999})
        data.append({"name": name, "attributes": {"weather": "overcast"}, "timestamp": 10000, "labels": labels})
        if gt and i == 1:
            data.append({"name": "not_predicted.jpg", "attributes": {}, "timestamp": 10000,
                         "labels": [{"category": "car", "attributes": {}, "box2d": {"x1": 1.0, "y1": 2.0, "x2": 3.0, "y2": 4.0}, "id": 5}]})
    return data


def read_tree(folder):
    files = sorted(os.listdir(folder))
    return files, [open(os.path.join(folder, f)).read() for f in files]


def record_members(out, key, o):
    """The members of extract_pseudo_gt_data, flattened in the order of o.images_data."""
    cat = lambda lists, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in lists] + [np.zeros(0, dt)])
    out[key + "n_gts_perim"], out[key + "n_pred_perim"] = np.asarray(o.n_gts_perim), np.asarray(o.n_pred_perim)
    out[key + "n_gt_matches"], out[key + "n_extra_detections"] = np.asarray(o.n_gt_matches), np.asarray(o.n_extra_detections)
    out[key + "n_missing_dets"] = np.asarray(o.n_missing_dets)
    out[key + "matched_preds"], out[key + "nomatch_preds"] = cat(o.matched_preds, np.int64), cat(o.nomatch_preds, np.int64)
    out[key + "gt_max_iou"] = cat([np.max(p, axis=-1) for p in o.perim_ious], np.float64)
    out[key + "gt_best_det"] = cat([np.argmax(p, axis=-1) for p in o.perim_ious], np.int64)
    out[key + "det_max_iou"] = cat([np.max(np.asarray(p).T, axis=-1) for p in o.perim_ious], np.float64)
    out[key + "det_best_gt"] = cat([np.argmax(np.asarray(p).T, axis=-1) for p in o.perim_ious], np.int64)
    for side in ("gt", "pseudo"):
        out[key + "alloc_%s_class" % side] = np.asarray([c for im in o.allocated_dets[side]["class"] for c in im], dtype=str)
        out[key + "alloc_%s_box" % side] = cat(o.allocated_dets[side]["box"], np.float64).reshape(-1, 4)
    out[key + "print_data"] = np.array([o.print_data])


def main():
    rng = np.random.default_rng(20241020)
    images = designed() + [im for im in random_images(rng, 40) if has_match(*im)][:10]
    n = len(images)
    stems = ["%06d" % (7 * i + 3) for i in range(n)]
    dets_all, gts_all = [im[0] for im in images], [im[1] for im in images]
    for objs in dets_all + gts_all:
        for box, _ in objs:
            assert (np.asarray(box) * 8 == np.round(np.asarray(box) * 8)).all()
    scores = [[float(np.round(rng.uniform(0.05, 0.99), 4)) for _ in range(len(d) + int(rng.integers(0, 5)))] for d in dets_all]
    out = {"numpy_major": np.array([int(np.__version__.split(".")[0])]), "gt_iou_thr": np.array([GT_IOU_THR]), "stems": np.array(stems),
           "kitti_classes": np.array(KITTI), "bdd_classes": np.array(BDD), "methods": np.array(METHODS),
           "beta_topk_seed": np.array([BETA, TOP_K, SEED]), "delta_s": np.array([4]),
           "scores": np.concatenate([np.asarray(s) for s in scores]), "scores_n": np.asarray([len(s) for s in scores]),
           "det_boxes": np.concatenate([np.asarray([b for b, _ in d], np.float64).reshape(-1, 4) for d in dets_all]),
           "det_classes": np.concatenate([np.asarray([c for _, c in d], np.int64) for d in dets_all]),
           "det_n": np.asarray([len(d) for d in dets_all]),
           "gt_boxes": np.concatenate([np.asarray([b for b, _ in g], np.float64).reshape(-1, 4) for g in gts_all]),
           "gt_classes": np.concatenate([np.asarray([c for _, c in g], np.int64) for g in gts_all]),
           "gt_n": np.asarray([len(g) for g in gts_all])}
    with tempfile.TemporaryDirectory(prefix="audit_") as td:
        assert not any(w in td for w in ("json", "score", "thr", "rand", "_V"))
        general = os.path.join(td, "general")
        # ---------------------------------------------------------------- KITTI
        ds_path = os.path.join(general, "datasets", "KITTI")
        names = [s + ".txt" for s in stems]
        gt_dir = os.path.join(ds_path, "training", "label_2")
        det_dir = os.path.join(ds_path, "pseudo_labels", "num_labeled_10", "score_thr_04_V0")
        out["kitti_gt_texts"] = np.array(write_kitti(gt_dir, names, gts_all, True))
        out["kitti_det_texts"] = np.array(write_kitti(det_dir, names, dets_all, False))
        assert max(len(l) for t in out["kitti_det_texts"] for l in str(t).splitlines(True)) > 83
        o = TD.ThreeDproblem.__new__(TD.ThreeDproblem)
        o.dataset, o.used_classes, o.gt_iou_thr, o.general_path = "KITTI", KITTI, GT_IOU_THR, general
        o.dataset_path, o.added_name, o.gt_labels_folder, o.det_folder = ds_path, "num_labeled_10", gt_dir, det_dir
        o.added_pseudo_name, o.delta_s, o.labeled_portion, o.v_number = "3d_problem", 0.4, 0, 0
        o.images_data = o.read_pred_folder()
        out["kitti_images_data"] = np.array(o.images_data)
        o.extract_pseudo_gt_data()
        record_members(out, "kitti_", o)
        order = [names.index(nm) for nm in o.images_data]
        # what is planted (indices are images in the fixture's own order)
        P_ = {i: o for i, o in zip(order, range(n))}
        ious = {i: np.asarray([calc_iou_np([g[0]], [d[0] for d in dets_all[i]]) for g in gts_all[i]]) for i in range(n)}
        mg0 = [int(np.where((np.asarray([b for b, _ in gts_all[0]]) == np.asarray(bx)).all(-1))[0][0]) for bx in o.allocated_dets["gt"]["box"][P_[0]]]
        assert list(o.matched_preds[P_[0]]) == [0, 1] and mg0 == [0, 1], (o.matched_preds[P_[0]], mg0)
        assert int(np.argmax(ious[0][0])) == 1 and ious[0][0].max() == 0.8 and ious[0][2].max() == 0.5            # the steal, and exactly 0.5
        assert o.n_gt_matches[P_[0]] == 2 and o.n_gts_perim[P_[0]] == 3                                              # one row is missing
        assert list(o.matched_preds[P_[1]]) == [0, 2] and o.n_gt_matches[P_[1]] == 2                                 # duplicates: the first wins
        assert [float(v) for v in ious[2].max(-1)] == [0.5, 0.75, 0.9] and o.n_missing_dets[P_[2]] == 0
        assert ious[3][0].max() == 0.0 and 0.5 <= ious[3][1].max() < 0.75
        assert "nan" in o.print_data.split("Acc:")[0], o.print_data       # a class without a matched row
        print(o.print_data)
        for m in METHODS:
            o.corrected_pseudo(folder_name="/3d_problem" + FOLDERS[m], **FLAGS[m])
            base = ds_path + "/pseudo_labels/num_labeled_10/3d_problem" + FOLDERS[m]
            files, texts = read_tree(base + "score_thr_04_V0")
            out["kitti_%s_files" % m], out["kitti_%s_texts" % m] = np.array(files), np.array(texts)
            out["kitti_%s_output" % m] = np.array([open(base + "data_score_thr_04_V0/output.txt").read()])
            print("KITTI", m, len(files), "files")
        assert len(out["kitti_nomd_files"]) < n
        k3 = list(out["kitti_nonoise_files"]).index(names[3])
        assert str(out["kitti_nonoise_texts"][k3]).count("\n") < 3          # a line cut to 83 characters lost its line end
        assert any(len(seg) > 83 for t in out["kitti_nofd_texts"] for seg in str(t).split("\n"))
        assert all(len(seg) <= 83 * 2 for t in out["kitti_nonoise_texts"] for seg in str(t).split("\n"))
        # ---------------------------------------------------------------- PLS (KITTI)
        q = PLS.Advanced_Pseudo_Labels.__new__(PLS.Advanced_Pseudo_Labels)
        q.dataset, q.used_classes, q.gt_iou_thr, q.general_path = "KITTI", KITTI, GT_IOU_THR, general
        q.dataset_path, q.added_name, q.gt_labels_folder, q.det_folder = ds_path, "num_labeled_10", gt_dir, det_dir + "/"
        q.beta, q.top_k, q.added_pseudo_name = BETA, TOP_K, "pls"
        q.inference_path = os.path.join(td, "prediction_data.txt")
        with open(q.inference_path, "w") as f:
            for i in range(n):       # ascending names: read_predictions pairs np.unique(names), which sorts, with scores in file order
                for s in scores[i]:
                    f.write(str({"image_name": stems[i] + ".jpg", "det_score": s, "bbox": [0.0, 0.0, 1.0, 1.0], "class": 1.0}) + "\n")
        q.images_data = q.read_pred_folder()
        assert sorted(q.images_data) == sorted(names)
        out["pls_images_data"] = np.array(q.images_data)
        q.extract_pseudo_gt_data()
        np.random.seed(SEED)
        q._pls()
        parent = ds_path + "/pseudo_labels/num_labeled_10/"
        for tag in ("top", "bot", "rand"):
            out["pls_%s_files" % tag] = np.array(sorted(os.listdir(parent + "pls_%s_score_thr_04_V0" % tag)))
        plots = parent + "pls_plots_score_thr_04_V0/"
        for f in ("score_si", "score_ci", "max_drop", "mean_drop", "avg_score", "std_drop", "n_det", "md"):
            out["pls_" + f] = np.load(plots + f + ".npy")
        out["pls_output"] = np.array([open(plots + "output.txt").read()])
        print("PLS top", len(out["pls_top_files"]), "bot", len(out["pls_bot_files"]), "rand", len(out["pls_rand_files"]))
        # ---------------------------------------------------------------- BDD100K
        ds_path = os.path.join(general, "datasets", "BDD100K")
        jnames = [s + ".jpg" for s in stems]
        gt_json, det_json = bdd_items(jnames, gts_all, True), bdd_items(jnames, dets_all, False)
        out["bdd_gt_json"], out["bdd_det_json"] = np.array([json.dumps(gt_json)]), np.array([json.dumps(det_json)])
        det_dir = os.path.join(ds_path, "pseudo_labels", "num_labeled_1", "score_thr_04_V0")
        os.makedirs(det_dir)
        with open(os.path.join(det_dir, "pseudo_labels.json"), "w") as f:
            json.dump(det_json, f)
        o = TD.ThreeDproblem.__new__(TD.ThreeDproblem)
        o.dataset, o.used_classes, o.gt_iou_thr, o.general_path = "BDD100K", BDD, GT_IOU_THR, general
        o.dataset_path, o.added_name, o.det_folder = ds_path, "num_labeled_1", det_dir
        o.gt_labels_folder = os.path.join(ds_path, "labels", "det_train.json")
        o.added_pseudo_name, o.delta_s, o.labeled_portion, o.v_number = "3d_problem", 0.4, 0, 0
        o.bdd_data, o.bdd_pseudo_data = copy.deepcopy(gt_json), None
        o.images_data = o.read_pred_folder()
        o.extract_pseudo_gt_data()
        assert o.images_data == jnames
        record_members(out, "bdd_", o)
        for m in METHODS:
            o.bdd_data = copy.deepcopy(gt_json)
            o.corrected_pseudo(folder_name="/3d_problem" + FOLDERS[m], **FLAGS[m])
            base = ds_path + "/pseudo_labels/num_labeled_1/3d_problem" + FOLDERS[m]
            out["bdd_%s_text" % m] = np.array([open(base + "score_thr_04_V0/pseudo_labels.json").read()])
            out["bdd_%s_output" % m] = np.array([open(base + "data_score_thr_04_V0/output.txt").read()])
            print("BDD", m, len(json.loads(str(out["bdd_%s_text" % m][0]))), "items")
        highprec = {it["name"]: it for it in json.loads(str(out["bdd_highprec_text"][0]))}
        assert any(len(highprec[nm]["labels"]) == len(d) and ious[i].max() < 0.9 for i, (nm, d) in enumerate(zip(jnames, dets_all))), \
            "no image with an empty selector under highprec (left unchanged, 3d.py:189)"
    dst = os.path.join(HERE, "audit_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 200000


if __name__ == "__main__":
    main()
