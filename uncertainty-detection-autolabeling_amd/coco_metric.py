"""COCO detection metrics on records matched on the device (reference src/coco_metric.py:59-283, which runs pycocotools'
COCOeval and src/custom_cocoeval.py COCOeval_all:265-545).

The per-image half - `evaluateImg`, the greedy matching of every (image, category, area range, IoU threshold) - runs in
`coco_match_kernel` (csrc/kernels_post.hip) and returns one 44-byte record per detection row (`RECORD_DTYPE`).  The
dataset-wide half lives here: `CocoAccumulator` keeps the records of the evaluated images, `accumulate` restates
COCOeval_all.accumulate (:351-465) as vectorised float64 numpy in the reference's operation order, `summarize` the 12 stats
(:467-545).  `EvaluationMetric` has the reference's members on top of it.

Neither pycocotools nor a COCO JSON is needed: ground truth comes from the dataloader's `groundtruth_data`, as in the reference
when `filename` is None."""
import numpy as np

from . import capi

RECORD_DTYPE = np.dtype([("score", "<f4"), ("cls", "<i4"), ("rank", "<i4"), ("matched", "<u4", (4,)), ("ignored", "<u4", (4,))])
assert RECORD_DTYPE.itemsize == 44
STD_IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)      # pycocotools COCOeval
ALL_IOU_THRS = np.linspace(0.05, 0.95, int(np.round((0.95 - 0.05) / 0.05)) + 1, endpoint=True)    # custom_cocoeval.py:560-562
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
MAX_DETS = (1, 10, 100)
AREA_LABELS = ("all", "small", "medium", "large")
METRIC_NAMES = ["AP", "AP50", "AP75", "APs", "APm", "APl", "ARmax1", "ARmax10", "ARmax100", "ARs", "ARm", "ARl"]
MAX_ROWS = 4096


def _ptr(a):
    return None if a is None else a.ctypes.data_as(capi.C.c_void_p)


def check_iou_thrs(iou_thrs):
    t = np.ascontiguousarray(STD_IOU_THRS if iou_thrs is None else iou_thrs, dtype=np.float64).reshape(-1)
    if not 1 <= t.size <= capi.EVAL_MAX_THRS:
        raise ValueError("1..%d IoU thresholds in one pass, got %d" % (capi.EVAL_MAX_THRS, t.size))
    if not np.isfinite(t).all():
        raise ValueError("IoU thresholds must be finite")
    return t


def check_groundtruth(groundtruth_data, num_classes):
    """[n, G, 7] float32 rows y1, x1, y2, x2, is_crowd, area, class (coco_metric.py:228-229).  Rows with class <= -1 are padding
    (the reference keeps rows with class > -1, :256); every other row must carry a whole class id in 1..num_classes and finite
    values.  G above the kernel's cap is refused, never truncated."""
    gt = np.ascontiguousarray(groundtruth_data, dtype=np.float32)
    if gt.ndim != 3 or gt.shape[2] != 7:
        raise ValueError("groundtruth_data must be [n, G, 7], got %s" % (gt.shape,))
    if gt.shape[1] > capi.EVAL_MAX_GT:
        raise ValueError("%d ground-truth rows per image, the match kernel holds at most %d" % (gt.shape[1], capi.EVAL_MAX_GT))
    cls = gt[:, :, 6]
    real = cls > -1
    if not np.isfinite(gt[real]).all():
        raise ValueError("ground-truth rows must be finite")
    k = cls[real]
    if k.size and (np.any(k != np.floor(k)) or k.min() < 1 or k.max() > num_classes):
        raise ValueError("ground-truth classes must be whole numbers in 1..%d (padding rows: -1)" % num_classes)
    return gt


def check_detections(detections):
    """[n, M, 7] float32 rows image_id, x, y, w, h, score, class (coco_metric.py:230-231); finite."""
    det = np.ascontiguousarray(detections, dtype=np.float32)
    if det.ndim != 3 or det.shape[2] != 7:
        raise ValueError("detections must be [n, M, 7], got %s" % (det.shape,))
    if det.shape[1] > MAX_ROWS:
        raise ValueError("%d detection rows per image, at most %d" % (det.shape[1], MAX_ROWS))
    if not np.isfinite(det).all():
        raise ValueError("detection rows must be finite")
    return det


def gt_class_counts(gt, num_classes):
    """[n, C] ground-truth rows per class id 1..C, crowds and every area included: which categories an image's ground truth names."""
    n = gt.shape[0]
    out = np.zeros((n, num_classes), np.int32)
    img, row = np.nonzero(gt[:, :, 6] > -1)
    np.add.at(out, (img, gt[img, row, 6].astype(np.int64) - 1), 1)
    return out


def match_np(detections, groundtruth_data, num_classes, iou_thrs=None, device=0):
    """`evaluateImg` for host arrays through `uda_eval_match_np` (the match kernel in its legacy-row layout): detections
    [n, M, 7] as `postprocess.transform_detections` returns them, groundtruth_data [n, G, 7].
    Returns (records [n, M] RECORD_DTYPE, npig [n, C, 4] int32, used [n] int32)."""
    num_classes = int(num_classes)
    det = check_detections(detections)
    gt = check_groundtruth(groundtruth_data, num_classes)
    thr = check_iou_thrs(iou_thrs)
    n, M = det.shape[:2]
    if gt.shape[0] != n:
        raise ValueError("ground truth of %d images for detections of %d" % (gt.shape[0], n))
    rec = np.zeros((n, M), RECORD_DTYPE)
    npig = np.zeros((n, num_classes, 4), np.int32)
    used = np.zeros((n,), np.int32)
    lib = capi.load()
    rc = lib.uda_eval_match_np(int(device), _ptr(det), _ptr(gt), n, M, gt.shape[1], num_classes, _ptr(thr), thr.size,
                               _ptr(rec), _ptr(npig), _ptr(used))
    capi.check(lib, None, rc, "uda_eval_match_np")
    return rec, npig, used


class CocoAccumulator:
    """The records and ground-truth counts of the evaluated images, keyed by image id.  An image without a single used
    detection row is not evaluated and its ground truth does not count (coco_metric.py:237-238, :168).  Plain numpy members:
    picklable, so the ranks of a multi-GPU evaluation can gather their accumulators and `merge` them."""

    def __init__(self, num_classes, iou_thrs=None):
        self.num_classes = int(num_classes)
        self.iou_thrs = check_iou_thrs(iou_thrs)
        self.images = {}          # image id -> (records with 0 <= rank < 100, npig [C, 4], gt_count [C])

    def add(self, image_ids, records, npig, used, gt_count=None):
        """One batch: image_ids [n], records [n, M] RECORD_DTYPE, npig [n, C, 4], used [n] as the match returns them.
        gt_count [n, C] (`gt_class_counts`) names the categories of each image's ground truth; without it they are the
        classes with a non-ignored row (npig of the "all" range), which differs only for a category whose every row is a crowd."""
        records = np.asarray(records)
        npig = np.asarray(npig, np.int32)
        n = records.shape[0]
        if records.dtype != RECORD_DTYPE or npig.shape != (n, self.num_classes, 4) or len(image_ids) != n or len(used) != n:
            raise ValueError("records [n, M] of RECORD_DTYPE, npig [n, %d, 4], image_ids [n], used [n]" % self.num_classes)
        gt_count = npig[:, :, 0] if gt_count is None else np.asarray(gt_count, np.int32)
        if gt_count.shape != (n, self.num_classes):
            raise ValueError("gt_count must be [n, %d]" % self.num_classes)
        new = {}
        for i in range(n):
            if used[i] <= 0:
                continue
            iid = int(image_ids[i])
            if iid in self.images or iid in new:
                raise ValueError("image id %d was added before" % iid)
            r = records[i]
            new[iid] = (r[(r["rank"] >= 0) & (r["rank"] < MAX_DETS[-1])].copy(), npig[i].copy(), gt_count[i].copy())
        self.images.update(new)

    def merge(self, other):
        if other.num_classes != self.num_classes or not np.array_equal(other.iou_thrs, self.iou_thrs):
            raise ValueError("accumulators of different class counts or thresholds")
        both = set(self.images) & set(other.images)
        if both:
            raise ValueError("image ids in both accumulators: %s" % sorted(both)[:8])
        self.images.update(other.images)
        return self

    def _thr_index(self, thr_index):
        return np.arange(self.iou_thrs.size) if thr_index is None else np.asarray(thr_index, np.int64).reshape(-1)

    def accumulate(self, thr_index=None):
        """COCOeval_all.accumulate (custom_cocoeval.py:351-465) over the thresholds `thr_index` selects (all by default).
        Returns dict(precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M], category_ids [K], iou_thrs [T]);
        images concatenate in ascending id (np.unique order, :156), whatever order they arrived in."""
        ti = self._thr_index(thr_index)
        T, R, A, Mx = ti.size, REC_THRS.size, 4, len(MAX_DETS)
        ids = sorted(self.images)
        C = self.num_classes
        gt_count = np.zeros((C,), np.int64)
        npig_all = np.zeros((C, 4), np.int64)
        parts, img_of = [], []
        for o, iid in enumerate(ids):
            r, npig, gc = self.images[iid]
            gt_count += gc
            npig_all += npig
            parts.append(r)
            img_of.append(np.full((r.size,), o, np.int64))
        cats = [k + 1 for k in range(C) if gt_count[k] > 0]
        K = len(cats)
        precision = -np.ones((T, R, K, A, Mx))
        recall = -np.ones((T, K, A, Mx))
        scores = -np.ones((T, R, K, A, Mx))
        rec = np.concatenate(parts) if parts else np.zeros((0,), RECORD_DTYPE)
        img = np.concatenate(img_of) if img_of else np.zeros((0,), np.int64)
        shifts = ti.astype(np.uint32)[:, None]
        for k, cat in enumerate(cats):
            sel = np.nonzero(rec["cls"] == cat)[0]
            sel = sel[np.lexsort((rec["rank"][sel], img[sel]))]          # image by image, each in rank order
            rk = rec[sel]
            for a in range(A):
                npig = int(npig_all[cat - 1, a])
                if npig == 0:
                    continue
                for m, max_det in enumerate(MAX_DETS):
                    e = rk[rk["rank"] < max_det]
                    dt_scores = e["score"]
                    inds = np.argsort(-dt_scores, kind="mergesort")
                    dt_sorted = dt_scores[inds]
                    dtm = ((e["matched"][inds, a][None, :] >> shifts) & 1).astype(bool)
                    dt_ig = ((e["ignored"][inds, a][None, :] >> shifts) & 1).astype(bool)
                    tps = np.logical_and(dtm, np.logical_not(dt_ig))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                    tp = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp = np.cumsum(fps, axis=1).astype(dtype=float)
                    nd = tp.shape[1]
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[:, k, a, m] = rc[:, -1] if nd else 0
                    pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]
                    q = np.zeros((T, R))
                    ss = np.zeros((T, R))
                    for t in range(T):
                        pos = np.searchsorted(rc[t], REC_THRS, side="left")
                        ok = pos < nd                                     # entries past the end stay 0 (:448-453)
                        q[t, ok] = pr[t, pos[ok]]
                        ss[t, ok] = dt_sorted[pos[ok]]
                    precision[:, :, k, a, m] = q
                    scores[:, :, k, a, m] = ss
        return dict(precision=precision, recall=recall, scores=scores, category_ids=np.asarray(cats, np.int64),
                    iou_thrs=self.iou_thrs[ti])

    @staticmethod
    def _summarize(ev, ap, iou_thr=None, area="all", max_dets=100):
        aind = [i for i, lbl in enumerate(AREA_LABELS) if lbl == area]
        mind = [i for i, md in enumerate(MAX_DETS) if md == max_dets]
        s = ev["precision"] if ap == 1 else ev["recall"]
        if iou_thr is not None:
            s = s[np.where(iou_thr == ev["iou_thrs"])[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    def summarize(self, ev=None, thr_index=None):
        """The 12 stats of COCOeval.summarize (custom_cocoeval.py:508-522), float64."""
        ev = self.accumulate(thr_index) if ev is None else ev
        z = self._summarize
        stats = np.zeros((12,))
        stats[0] = z(ev, 1)
        stats[1] = z(ev, 1, iou_thr=0.5, max_dets=MAX_DETS[2])
        stats[2] = z(ev, 1, iou_thr=0.75, max_dets=MAX_DETS[2])
        stats[3] = z(ev, 1, area="small", max_dets=MAX_DETS[2])
        stats[4] = z(ev, 1, area="medium", max_dets=MAX_DETS[2])
        stats[5] = z(ev, 1, area="large", max_dets=MAX_DETS[2])
        stats[6] = z(ev, 0, max_dets=MAX_DETS[0])
        stats[7] = z(ev, 0, max_dets=MAX_DETS[1])
        stats[8] = z(ev, 0, max_dets=MAX_DETS[2])
        stats[9] = z(ev, 0, area="small", max_dets=MAX_DETS[2])
        stats[10] = z(ev, 0, area="medium", max_dets=MAX_DETS[2])
        stats[11] = z(ev, 0, area="large", max_dets=MAX_DETS[2])
        return stats

    def per_class_ap(self, label_map, ev=None, thr_index=None):
        """coco_metric.py:186-201: the mean of precision[:, :, k, 0, -1] > -1 at index category_id - 1; a list as long as
        max(K, len(label_map)), 0 where the evaluated ground truth has no such category, -1.0 where nothing is valid."""
        ev = self.accumulate(thr_index) if ev is None else ev
        precision = ev["precision"][:, :, :, 0, -1]
        ap = [0] * max(precision.shape[-1], len(label_map))
        for c in range(precision.shape[-1]):
            p = precision[:, :, c]
            p = p[p > -1]
            ap[int(ev["category_ids"][c]) - 1] = np.mean(p) if p.size else -1.0
        return ap


class EvaluationMetric:
    """The reference's `coco_metric.EvaluationMetric` (coco_metric.py:59-283) without pycocotools: `update_state` matches each
    batch on the device (`uda_eval_match_np`), `evaluate` accumulates on the host.  With `apiou_curve` the 19 thresholds of
    COCOeval_all and the 10 standard ones are matched in one pass (29 <= 32 bits per record).

    num_classes bounds the class ids; by default the largest id of `label_map`, else 90 (hparams_config's default).  Ground
    truth from a COCO JSON (`filename`) and the test-dev export (`testdev_dir`) are not built: both raise ValueError."""

    def __init__(self, filename=None, testdev_dir=None, label_map=None, apiou_curve=True, num_classes=None, device=0):
        if filename:
            raise ValueError("filename=%r: ground truth from a COCO JSON file is not built; pass groundtruth_data to update_state" % (filename,))
        if testdev_dir:
            raise ValueError("testdev_dir=%r: the test-dev export (detections_test-dev2017_test_results.json) is not built" % (testdev_dir,))
        if label_map is not None and not isinstance(label_map, dict):
            raise ValueError("label_map must be a dict from class id to name (or None)")
        self.label_map = label_map
        self.filename = filename
        self.testdev_dir = testdev_dir
        self.metric_names = list(METRIC_NAMES)
        self.apiou_curve = apiou_curve
        if num_classes is None:
            num_classes = max(int(k) for k in label_map) if label_map else 90
        self.num_classes = int(num_classes)
        self.device = int(device)
        self.iou_thrs = np.concatenate([ALL_IOU_THRS, STD_IOU_THRS]) if apiou_curve else STD_IOU_THRS.copy()
        self._all_index = np.arange(ALL_IOU_THRS.size) if apiou_curve else None
        self._std_index = np.arange(STD_IOU_THRS.size) + (ALL_IOU_THRS.size if apiou_curve else 0)
        self.reset_states()

    def reset_states(self):
        self.accumulator = CocoAccumulator(self.num_classes, self.iou_thrs)
        self.image_id = 1
        self.metric_values = None
        self.precision_all = None

    def _image_ids(self, first_ids, used):
        """coco_metric.py:241-244, :277: an evaluated image whose id is -1 gets the running counter; the counter advances with
        every evaluated image."""
        ids = np.zeros((len(used),), np.int64)
        for i in range(len(used)):
            if used[i] <= 0:
                continue
            ids[i] = self.image_id if first_ids[i] == -1 else int(first_ids[i])
            self.image_id += 1
        return ids

    def add_records(self, image_ids, records, npig, used, groundtruth_data=None):
        """Records matched elsewhere (`ServingDriver.eval_match` / `serve_eval`) with the thresholds `self.iou_thrs`.
        image_ids [n] (None or -1: the running counter)."""
        first = np.full((len(used),), -1, np.int64) if image_ids is None else np.asarray(image_ids).astype(np.int64)
        gc = None if groundtruth_data is None else gt_class_counts(check_groundtruth(groundtruth_data, self.num_classes), self.num_classes)
        self.accumulator.add(self._image_ids(first, used), records, npig, used, gc)
        self.metric_values = None

    def update_state(self, groundtruth_data, detections):
        """groundtruth_data [n, G, 7] rows y1, x1, y2, x2, is_crowd, area, class; detections [n, M, 7] rows image_id, x, y, w, h,
        score, class.  The image id is that of the image's first used row (coco_metric.py:241)."""
        det = check_detections(detections)
        gt = check_groundtruth(groundtruth_data, self.num_classes)
        rec, npig, used = match_np(det, gt, self.num_classes, self.iou_thrs, self.device)
        first = np.full((det.shape[0],), -1, np.int64)
        for i in range(det.shape[0]):
            rows = np.nonzero(det[i, :, 6] > -1)[0]
            if rows.size:
                first[i] = int(det[i, rows[0], 0])
        self.accumulator.add(self._image_ids(first, used), rec, npig, used, gt_class_counts(gt, self.num_classes))
        self.metric_values = None

    def evaluate(self, log_level=None):
        """float32 [12 (+ per-class AP when label_map is set)]; with apiou_curve the pair (metrics, precision_all) where
        precision_all = COCOeval_all's precision[:, :, :, 0, -1] over its 19 thresholds (coco_metric.py:171-207)."""
        if not self.accumulator.images:
            raise ValueError("no image with a used detection row has been added")
        precision_all = None
        if self.apiou_curve:
            precision_all = self.accumulator.accumulate(self._all_index)["precision"][:, :, :, 0, -1]
        ev = self.accumulator.accumulate(self._std_index)
        metrics = self.accumulator.summarize(ev)
        if self.label_map:
            metrics = np.concatenate((metrics, self.accumulator.per_class_ap(self.label_map, ev)))
        metrics = np.array(metrics, dtype=np.float32)
        return (metrics, precision_all) if self.apiou_curve else metrics

    def result(self, log_level=None):
        if self.metric_values is None:
            if self.apiou_curve:
                self.metric_values, self.precision_all = self.evaluate(log_level)
            else:
                self.metric_values = self.evaluate(log_level)
        return (self.metric_values, self.precision_all) if self.apiou_curve else self.metric_values
