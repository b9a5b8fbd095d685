"""Generates tests/golden/coco_eval_golden.npz by running the REAL reference code: `coco_metric.EvaluationMetric.update_state /
evaluate` (src/coco_metric.py:113-283) and `custom_cocoeval.COCOeval_all.evaluate / accumulate / summarize`
(src/custom_cocoeval.py:139-545).  Run once where a checkout of the reference exists; the .npz (data only) is committed and is what
the tests read.

    python tests/golden/make_coco_eval_golden.py <src directory of the reference's checkout>

pycocotools is not installed, so three of its pieces are stated here from public knowledge of that package:
  * `pycocotools.mask.iou` for boxes = bbIou: float64 on [x, y, w, h]; iw = min(dx + dw, gx + gw) - max(dx, gx), ih likewise, 0 when
    either is <= 0, else i / (crowd ? da : da + ga - i); an empty side gives [];
  * `pycocotools.coco.COCO` as the small container the evaluation reads: createIndex, getImgIds, getCatIds, getAnnIds, loadAnns and
    loadRes on a float32 array (fields are float32 scalars, ids start at 1, area = bbox[2] * bbox[3], iscrowd = 0);
  * `pycocotools.cocoeval.COCOeval` = the reference's COCOeval_all (its modified copy) with params.iouThrs = linspace(0.5, 0.95, 10).
TensorFlow, absl and label_util are stubbed: update_state and evaluate are numpy only.

Two datasets: "a" (C = 3, M = 100, G = 24, explicit image ids, fed in two update_state calls) and "b" (C = 10, M = 128, G = 256, image
id -1 = the running counter).  Per dataset the fixture holds the inputs, the reference's per-(image, category, area) results packed
as the match kernel's records (rank, bit t of matched / ignored per area) for the 19 thresholds of COCOeval_all and for the 10
standard ones, gtIgnore, precision / recall / scores of both, stats, what evaluate() returned (`metrics`, `curve_precision` = its precision_all), and the per-class APs.  Rows the
reference never evaluates (images without a used row, categories absent from the evaluated ground truth) are marked in `evaluated`.

The branches the tests rely on are asserted below, or the fixture would have pinned nothing."""
import copy
import itertools
import os
import sys
import types
from collections import defaultdict

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_coco_eval_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
import numpy as np                       # noqa: E402

RECORD_DTYPE = np.dtype([("score", "<f4"), ("cls", "<i4"), ("rank", "<i4"), ("matched", "<u4", (4,)), ("ignored", "<u4", (4,))])
STD_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
G_CAP = 256


def bb_iou_matrix(dt, gt, iscrowd):
    if len(dt) == 0 or len(gt) == 0:
        return []
    d = np.asarray(dt, np.float64).reshape(-1, 4)
    g = np.asarray(gt, np.float64).reshape(-1, 4)
    out = np.zeros((len(d), len(g)), np.float64)
    for j in range(len(g)):
        ga = g[j, 2] * g[j, 3]
        for i in range(len(d)):
            da = d[i, 2] * d[i, 3]
            w = min(d[i, 2] + d[i, 0], g[j, 2] + g[j, 0]) - max(d[i, 0], g[j, 0])
            if w <= 0:
                continue
            h = min(d[i, 3] + d[i, 1], g[j, 3] + g[j, 1]) - max(d[i, 1], g[j, 1])
            if h <= 0:
                continue
            inter = w * h
            u = da if iscrowd[j] else da + ga - inter
            out[i, j] = inter / u
    return out


class MiniCOCO:
    def __init__(self, annotation_file=None):
        assert annotation_file is None
        self.dataset, self.anns, self.imgs, self.cats = {}, {}, {}, {}
        self.imgToAnns = defaultdict(list)

    def createIndex(self):
        self.anns = {a["id"]: a for a in self.dataset.get("annotations", [])}
        self.imgToAnns = defaultdict(list)
        for a in self.dataset.get("annotations", []):
            self.imgToAnns[a["image_id"]].append(a)
        self.imgs = {im["id"]: im for im in self.dataset.get("images", [])}
        self.cats = {c["id"]: c for c in self.dataset.get("categories", [])}

    def getImgIds(self):
        return list(self.imgs.keys())

    def getCatIds(self):
        return [c["id"] for c in self.dataset["categories"]]

    def getAnnIds(self, imgIds=[], catIds=[]):
        if len(imgIds) == 0 and len(catIds) == 0:
            anns = self.dataset["annotations"]
        else:
            if len(imgIds) > 0:
                anns = list(itertools.chain.from_iterable(self.imgToAnns[i] for i in imgIds if i in self.imgToAnns))
            else:
                anns = self.dataset["annotations"]
            anns = anns if len(catIds) == 0 else [a for a in anns if a["category_id"] in catIds]
        return [a["id"] for a in anns]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]

    def loadRes(self, data):
        assert isinstance(data, np.ndarray) and data.dtype == np.float32 and data.shape[1] == 7
        res = MiniCOCO()
        res.dataset["images"] = [im for im in self.dataset["images"]]
        anns = [{"image_id": int(data[i, 0]), "bbox": [data[i, 1], data[i, 2], data[i, 3], data[i, 4]], "score": data[i, 5],
                 "category_id": int(data[i, 6])} for i in range(data.shape[0])]
        assert set(a["image_id"] for a in anns) == (set(a["image_id"] for a in anns) & set(self.getImgIds()))
        res.dataset["categories"] = copy.deepcopy(self.dataset["categories"])
        for k, ann in enumerate(anns):
            bb = ann["bbox"]
            ann["area"] = bb[2] * bb[3]
            assert ann["area"].dtype == np.float32
            ann["id"] = k + 1
            ann["iscrowd"] = 0
        res.dataset["annotations"] = anns
        res.createIndex()
        return res


def _module(name, **members):
    m = types.ModuleType(name)
    m.__dict__.update(members)
    sys.modules[name] = m
    return m


_logger = types.SimpleNamespace(getEffectiveLevel=lambda: 0)
_module("tensorflow", get_logger=lambda: _logger,
        compat=types.SimpleNamespace(v1=types.SimpleNamespace(logging=types.SimpleNamespace(INFO=20))))
_module("absl", logging=types.SimpleNamespace(info=lambda *a, **k: None))
_module("absl.logging", info=lambda *a, **k: None)
_module("label_util")
_module("pycocotools")
_module("pycocotools.mask", iou=bb_iou_matrix)
_module("pycocotools.coco", COCO=MiniCOCO)
sys.path.insert(0, REF_SRC)
import custom_cocoeval as CE             # noqa: E402  (the reference module)

EVALS = []


class StdCOCOeval(CE.COCOeval_all):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.params.iouThrs = STD_THRS.copy()
        EVALS.append(self)


class AllCOCOeval(CE.COCOeval_all):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        EVALS.append(self)


_module("pycocotools.cocoeval", COCOeval=StdCOCOeval)
CE_all = CE.COCOeval_all
import coco_metric as CM                 # noqa: E402  (the reference module)
CM.COCOeval_all = AllCOCOeval


# ------------------------------------------------------------------------------------------------ data
def gt_row(x, y, w, h, cls, crowd=0):
    return [y, x, y + h, x + w, crowd, -7.0, cls]          # the area column is not read: a value nothing could use


def pad_rows(rows, count, width=7, fill=-1.0):
    out = np.full((count, width), fill, np.float32)
    if width == 7 and fill == -1.0:
        out[:, :6] = 0.0
    assert len(rows) <= count, (len(rows), count)
    if rows:
        out[:len(rows)] = np.asarray(rows, np.float32)
    return out


def random_image(rng, classes, n_gt, n_det, M, G, image_id, det_only=()):
    gts, dets = [], []
    for _ in range(n_gt):
        w, h = rng.integers(6, 140, 2)
        x, y = rng.integers(0, 500, 2)
        gts.append(gt_row(x, y, w, h, int(rng.choice(classes)), crowd=int(rng.random() < 0.1)))
    for k in range(n_det):
        if gts and rng.random() < 0.7:
            g = gts[int(rng.integers(0, len(gts)))]
            x, y, w, h = g[1] + rng.integers(-6, 7), g[0] + rng.integers(-6, 7), g[3] - g[1] + rng.integers(-4, 5), g[2] - g[0] + rng.integers(-4, 5)
            cls = g[6] if rng.random() < 0.85 else int(rng.choice(classes))
        else:
            w, h = rng.integers(4, 150, 2)
            x, y = rng.integers(0, 500, 2)
            cls = int(rng.choice(list(classes) + list(det_only)))
        if rng.random() < 0.3:                                   # non-integer corners too
            x, y = x + rng.random(), y + rng.random()
        dets.append([image_id, x, y, max(w, 1), max(h, 1), np.round(rng.random(), 2), cls])
    det = pad_rows(dets, M)
    det[len(dets):, 0] = image_id
    return pad_rows(gts, G), det


def dataset_a(rng):
    C, M, G = 3, 100, 24
    ids = [7, 3, 12, 5, 9, 1, 20, 15]
    gts, dets = [], []
    # image 0 (id 7): the crafted branches
    g = [gt_row(0, 0, 10, 20, 1),                 # det 10x10 inside: IoU exactly 0.5
         gt_row(100, 0, 10, 10, 1), [-1, -1, -1, -1, 0, 0, -1],   # (a padding row in the middle is skipped, not the end)
         gt_row(110, 0, 10, 10, 1),               # the det between the two: IoU 1/3 with each, the later row wins
         gt_row(200, 0, 50, 50, 2, crowd=1),      # a crowd matched by two detections
         gt_row(300, 0, 32, 32, 3),               # area exactly 1024: small AND medium
         gt_row(300, 100, 96, 96, 3),             # area exactly 9216: medium AND large
         gt_row(0, 200, 20, 20, 2)]               # small: ignored in the medium / large ranges
    d = [[7, 0, 0, 10, 10, 0.9, 1], [7, 105, 0, 10, 10, 0.5, 1], [7, 400, 400, 8, 8, 0.5, 1],      # equal scores in one class
         [7, 200, 0, 20, 20, 0.8, 2], [7, 225, 25, 20, 20, 0.7, 2], [7, 300, 0, 32, 32, 0.6, 3], [7, 300, 100, 96, 96, 0.6, 3],
         [7, 1, 201, 20, 20, 0.4, 2], [7, 450, 450, 5, 5, 0.3, 3], [7, 10, 300, 200, 200, 0.2, 0]]
    det = pad_rows(d, M); det[len(d):, 0] = 7
    gts.append(pad_rows(g, G)); dets.append(det)
    # image 1 (id 3): detections, no ground truth; a score equal to one of image 0's in class 1
    _, det = random_image(rng, [1, 2, 3], 0, 12, M, G, 3)
    det[0, 5:7] = (0.5, 1)
    gts.append(pad_rows([], G)); dets.append(det)
    # image 2 (id 12): ground truth, and only class-0 and class -1 rows: evaluated, every ground-truth row is missed
    gt, _ = random_image(rng, [1, 2], 5, 0, M, G, 12)
    d = [[12, 20 * k, 10, 30, 30, 0.5, 0] for k in range(6)]
    det = pad_rows(d, M); det[len(d):, 0] = 12
    gts.append(gt); dets.append(det)
    # image 3 (id 5): every row unused: the image is not evaluated, its ground truth does not count
    gt, _ = random_image(rng, [1, 2, 3], 6, 0, M, G, 5)
    det = pad_rows([], M); det[:, 0] = 5
    gts.append(gt); dets.append(det)
    for iid, (ng, nd) in zip(ids[4:], [(8, 40), (15, 100), (3, 9), (24, 70)]):
        gt, det = random_image(rng, [1, 2, 3], ng, nd, M, G, iid)
        gts.append(gt); dets.append(det)
    return dict(C=C, gt=np.stack(gts), det=np.stack(dets), batches=[(0, 3), (3, 8)])


def dataset_b(rng):
    C, M, G = 10, 128, G_CAP
    present = [1, 2, 3, 5, 7]
    gts, dets = [], []
    # image 0: 112 rows of class 1 (only the best 100 take part), with ties
    gt, det = random_image(rng, [1], 20, 112, M, G, -1)
    det[:112, 6] = 1
    extra = [[-1, 5 * k, 5 * k, 40, 40, 0.35, 2 + (k % 2)] for k in range(16)]
    det[112:128] = np.asarray(extra, np.float32)
    gts.append(gt); dets.append(det)
    # image 1: at the ground-truth cap
    gt, det = random_image(rng, present, G, 128, M, G, -1, det_only=[4, 9])
    gts.append(gt); dets.append(det)
    for ng, nd in [(10, 60), (0, 20), (30, 128), (5, 3)]:
        gt, det = random_image(rng, present, ng, nd, M, G, -1, det_only=[4, 9])       # classes 4 and 9: in detections only
        gts.append(gt); dets.append(det)
    gt = np.stack(gts)
    gt[gt[:, :, 6] == 7, 4] = 1           # every row of class 7 is a crowd: a category with ground truth and npig == 0
    return dict(C=C, gt=gt, det=np.stack(dets), batches=[(0, 6)])


# ------------------------------------------------------------------------------------------------ the reference at work
def run_reference(ds):
    C, gt, det = ds["C"], ds["gt"], ds["det"]
    n, M = det.shape[:2]
    metric = CM.EvaluationMetric(label_map={k: "class%d" % k for k in range(1, C + 1)}, apiou_curve=True)
    for lo, hi in ds["batches"]:
        metric.update_state(gt[lo:hi].copy(), det[lo:hi].copy())
    where = [(i, r) for i in range(n) for r in range(M) if det[i, r, 6] > -1]        # annotation id - 1 -> (image, row)
    assert len(where) == len(metric.detections)
    image_ids = np.zeros((n,), np.int64)
    evaluated_imgs = [i for i in range(n) if (det[i, :, 6] > -1).any()]
    for i, im in zip(evaluated_imgs, metric.dataset["images"]):
        image_ids[i] = im["id"]
    del EVALS[:]
    metrics, precision_all = metric.evaluate()
    ev_all, ev_std = EVALS
    assert len(ev_all.params.iouThrs) == 19 and len(ev_std.params.iouThrs) == 10
    ev_all.summarize()
    img_index = {int(image_ids[i]): i for i in evaluated_imgs}
    out = dict(num_classes=np.int64(C), gt=gt, det=det, image_ids=image_ids, metrics=metrics, curve_precision=precision_all,
               batches=np.asarray(ds["batches"], np.int64))
    assert np.array_equal(precision_all, ev_all.eval["precision"][:, :, :, 0, -1])
    assert np.array_equal(metrics[:12], ev_std.stats.astype(np.float32))
    cats = [int(c) for c in ev_std.params.catIds]
    used = np.asarray([(det[i, :, 6] > -1).sum() for i in range(n)], np.int32)
    G = gt.shape[1]
    for tag, ev in (("all", ev_all), ("std", ev_std)):
        T = len(ev.params.iouThrs)
        rec = np.zeros((n, M), RECORD_DTYPE)
        rec["score"] = det[:, :, 5]
        rec["rank"] = -1
        rec["cls"] = np.where(det[:, :, 6] > -1, det[:, :, 6].astype(np.int32), -1)
        evaluated = np.zeros((n, M), bool)
        npig = np.zeros((n, C, 4), np.int32)
        gt_ignore = np.full((n, C, 4, G), -1, np.int8)
        for i in range(n):                                   # ranks: the reference's own sort call (custom_cocoeval.py:289)
            for c in range(1, C + 1):
                rows = [r for r in range(M) if det[i, r, 6] > -1 and int(det[i, r, 6]) == c]
                for rank, j in enumerate(np.argsort([-det[i, r, 5] for r in rows], kind="mergesort") if rows else []):
                    rec[i, rows[j]]["rank"] = rank
                if i in evaluated_imgs and c in cats:
                    evaluated[i, rows] = True
        for e in ev.evalImgs:
            if e is None:
                continue
            i, c = img_index[int(e["image_id"])], int(e["category_id"])
            a = [list(r) for r in ev.params.areaRng].index(list(e["aRng"]))
            gi = np.asarray(e["gtIgnore"]).astype(np.int8)
            npig[i, c - 1, a] = int((gi == 0).sum())
            gt_ignore[i, c - 1, a, :gi.size] = gi
            for j, did in enumerate(e["dtIds"]):
                ii, r = where[did - 1]
                assert ii == i and rec[i, r]["rank"] == j and rec[i, r]["cls"] == c
                for t in range(T):
                    if e["dtMatches"][t, j] != 0:
                        rec[i, r]["matched"][a] |= np.uint32(1 << t)
                    if e["dtIgnore"][t, j]:
                        rec[i, r]["ignored"][a] |= np.uint32(1 << t)
        out.update({"rec_" + tag: rec, "npig_" + tag: npig, "evaluated": evaluated, "gt_ignore": gt_ignore, "used": used,
                    "iou_thrs_" + tag: np.asarray(ev.params.iouThrs, np.float64), "precision_" + tag: ev.eval["precision"],
                    "recall_" + tag: ev.eval["recall"], "scores_" + tag: ev.eval["scores"], "stats_" + tag: np.asarray(ev.stats, np.float64)})
    out["category_ids"] = np.asarray(cats, np.int64)
    out["per_class_ap"] = np.asarray(metrics[12:], np.float32)
    return out, ev_all, ev_std, where


def iou1(d, g, crowd=0):
    return bb_iou_matrix([list(d)], [list(g)], [crowd])[0, 0]


def check_branches(a, b, ev_a):
    det, gt = a["det"], a["gt"]
    xywh = lambda g: [g[1], g[0], g[3] - g[1], g[2] - g[0]]          # noqa: E731
    # an IoU exactly equal to a threshold: matched at 0.5, not at 0.55
    assert iou1(det[0, 0, 1:5], xywh(gt[0, 0])) == 0.5 and STD_THRS[0] == 0.5
    assert a["rec_std"][0, 0]["matched"][0] & 1 and not a["rec_std"][0, 0]["matched"][0] & 2
    # two ground-truth rows with equal IoU: the later one is taken
    v1, v2 = iou1(det[0, 1, 1:5], xywh(gt[0, 1])), iou1(det[0, 1, 1:5], xywh(gt[0, 3]))
    assert v1 == v2 and v1 > 0.3
    e = [e for e in ev_a.evalImgs if e is not None and e["image_id"] == 7 and e["category_id"] == 1 and list(e["aRng"]) == [0, 1e10]][0]
    j = [k for k, s in enumerate(e["dtScores"]) if s == np.float32(0.5)][0]
    later = e["gtIds"][2]
    assert e["dtMatches"][0, j] == later == 3, (e["dtMatches"][0], e["gtIds"])
    # equal scores inside one (image, class) and across images
    assert det[0, 1, 5] == det[0, 2, 5] and det[0, 1, 6] == det[0, 2, 6] and det[1, 0, 5] == det[0, 1, 5] and det[1, 0, 6] == det[0, 1, 6]
    # a crowd matched twice
    e = [e for e in ev_a.evalImgs if e is not None and e["image_id"] == 7 and e["category_id"] == 2 and list(e["aRng"]) == [0, 1e10]][0]
    crowd_id = [gid for gid, ig in zip(e["gtIds"], e["gtIgnore"]) if ig][0]
    assert (e["dtMatches"][0] == crowd_id).sum() == 2
    for ds in (a, b):
        for tag in ("all", "std"):
            r = ds["rec_" + tag][ds["evaluated"]]
            assert ((r["matched"] & r["ignored"]) != 0).any()            # a detection matched to an ignored row
            assert ((~r["matched"] & r["ignored"]) != 0).any()           # an unmatched detection outside the area range
            assert (r["matched"] != 0).any() and (r["rank"] >= 0).all()
    areas = (gt[0, :, 3] - gt[0, :, 1]) * (gt[0, :, 2] - gt[0, :, 0])
    assert 1024 in areas and 9216 in areas
    gi = a["gt_ignore"][0, 2]                                            # class 3 of image 0: [1024, 9216] in the four ranges
    assert sorted(gi[1, :2]) == [0, 1] and sorted(gi[2, :2]) == [0, 0] and sorted(gi[3, :2]) == [0, 1]
    assert gt[0, 2, 6] == -1 and gt[0, 3, 6] == 1                        # the padding row in the middle
    assert (gt[1, :, 6] == -1).all() and a["used"][1] > 0                # an image with no ground truth
    assert (gt[2, :, 6] > 0).any() and a["used"][2] > 0 and (det[2, :, 6] <= 0).all() and (det[2, :, 6] == 0).any()
    assert (gt[3, :, 6] > 0).any() and a["used"][3] == 0                 # every row unused
    assert a["num_classes"] == 3 and b["num_classes"] == 10
    db, gb = b["det"], b["gt"]
    assert set(b["category_ids"]) == {1, 2, 3, 5, 7} and (db[:, :, 6] == 4).any() and (db[:, :, 6] == 9).any()
    assert db.shape[1] == 128 and (db[0, :, 6] == 1).sum() > 100 and b["rec_all"][0]["rank"].max() >= 100
    assert gb.shape[1] == G_CAP and (gb[1, :, 6] > 0).all()             # an image at the ground-truth cap
    assert (b["image_ids"] == np.arange(1, 7)).all()                     # the running counter
    k7 = list(b["category_ids"]).index(7)                                # npig == 0 leaves -1; its per-class AP is -1, not 0
    assert (b["precision_std"][:, :, k7] == -1).all() and (b["npig_std"][:, 6] == 0).all() and b["per_class_ap"][6] == -1
    assert (b["per_class_ap"][[3, 5, 7, 8, 9]] == 0).all() and (b["per_class_ap"][[0, 1, 2, 4]] > 0).all()


def main():
    rng = np.random.default_rng(20240607)
    a, ev_a, _, _ = run_reference(dataset_a(rng))
    b, _, _, _ = run_reference(dataset_b(rng))
    check_branches(a, b, ev_a)
    out = {}
    for name, ds in (("a", a), ("b", b)):
        out.update({"%s_%s" % (name, k): v for k, v in ds.items()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "coco_eval_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
