"""Ground-truth label correction (GLC): the reference's `AdvancedLabels` (src/ssl_utils/glc.py) on the device.

The reference decides, from the detections of the labelled images, their `cons_iou` (the consistency check) and the ground
truth, which ground-truth boxes are *mistakes* (they touch no detection, :551), which detections are *missing labels* (`md`:
consistent detections that touch no ground truth, :432-436) and which *noisy* ground-truth boxes are replaced by the detection
matched to them (:813-834).  It gets there through an `inspector --mode 6` run, a re-parse of prediction_data.txt and two
Python loops; here the verdicts come from one kernel (`uda_label_check`, csrc/kernels_glc.hip; the contract is in
include/uda_hip.h and DESIGN 17):

  ServingDriver.serve_label_check / label_check   on the detections resident in a handle after `serve_consistency`
  check_labels                                    on host arrays, or the lists `read_predictions` returns (`uda_label_check_np`)
  LabelCheck                                      the result: the reference's return shapes, `merge` for batches
  writers.write_kitti_corrected_gt / write_bdd_corrected_gt   the label files of `corrected_gt` (:231-406)

The synthetic generators of the reference (dropped ground truth, random mistake boxes, box deviations) are experiments on top
of the same verdicts: a caller runs them by passing a modified ground truth, with md_rule="le" where the reference uses <=.
"""
import ctypes as C

import numpy as np

from . import capi

METHODS = ("md", "mistakes", "noisy")
_METHOD_BITS = {"md": capi.LC_MD, "mistakes": capi.LC_MISTAKES, "noisy": capi.LC_NOISY}
_MD_RULES = {"eq": capi.LC_MD_EQ, "le": capi.LC_MD_LE}
# AdvancedLabels' constructor defaults (glc.py:25-45)
DEFAULTS = dict(iou_consist=0.90, md_max_inter=0, md_rule="eq", correct_max_inter=1.0, correct_score=0.40)


def method_mask(methods):
    """("md", "mistakes", "noisy") or a subset -> the bit set of the C ABI; a single name is taken as one method."""
    if isinstance(methods, str):
        methods = (methods,)
    methods = tuple(methods)
    if not methods:
        raise ValueError("label check: no method given, choose among %s" % (METHODS,))
    unknown = [m for m in methods if m not in _METHOD_BITS]
    if unknown:
        raise ValueError("label check: unknown method %r, choose among %s" % (unknown[0], METHODS))
    mask = 0
    for m in methods:
        mask |= _METHOD_BITS[m]
    return mask


def md_rule_code(md_rule):
    if md_rule not in _MD_RULES:
        raise ValueError("label check: md_rule %r is neither 'eq' (np.equal, glc.py:433) nor 'le' (the synthetic branch, :469)" % (md_rule,))
    return _MD_RULES[md_rule]


def check_thresholds(iou_consist, md_max_inter, correct_max_inter, correct_score):
    vals = dict(iou_consist=iou_consist, md_max_inter=md_max_inter, correct_max_inter=correct_max_inter, correct_score=correct_score)
    for k, v in vals.items():
        if not np.isfinite(float(v)):
            raise ValueError("label check: %s must be finite, got %r" % (k, v))
    return tuple(float(v) for v in vals.values())


def resolve_min_score(params, min_score=None, average_score=0, ssl=True):
    """The threshold of the rows the check reads.  None: what `Infer.iterate_infer` writes its file with (infer_model.py:568-573)
    - 0.1 for a model served from an SSL folder, which is where GLC's own inference run takes its model (glc.py:132-134; ssl=True),
    else nms_configs.score_thresh, or the validation's average score, or 0.4."""
    if min_score is None:
        from . import active_learning as al
        min_score = al.default_min_score(params, average_score=average_score, ssl=ssl)
    min_score = float(min_score)
    if not np.isfinite(min_score):
        raise ValueError("label check: min_score must be finite, got %r" % (min_score,))
    return min_score


def _plain(a, f32):
    """The python floats the reference holds for the array a, as nested lists: read back from its file, a float32 value is its
    shortest decimal (numpy prints float32 as such; the strings are made and parsed array-wise)."""
    a = np.asarray(a)
    return (a.astype(np.float32).astype(str).astype(np.float64) if f32 else a.astype(np.float64)).tolist()


class LabelCheck:
    """The verdicts for a list of images, in the reference's shapes.  Indices are the reference's: ground-truth rows count over
    the image's COUNTED rows (class > 0: the boxes of the used classes), detections over its KEPT rows (score > min_score: the
    rows of prediction_data.txt).  An image without a kept detection is present with empty verdicts (the reference's file has
    no such image).

      wrong_gt             per image, the indices of the mistake rows (`mistakes`, glc.py:551)
      extra_correct_dets   per image, a bool array over the kept detections (`mds`, :432-436)
      corrected_gt_boxes   per image, the list of boxes [y1, x1, y2, x2] (`noisy_boxes`, :827-833): a replaced row carries its
                           detection's box as the number the reference reads back from its file
      matched_det, ious_gt per image (:186-187); counts [n, 5] int32 kept detections, counted rows, mistakes, replaced rows,
                           missing labels; pred_boxes / pred_classes / pred_ranks of the kept detections; replaced, noisy_rows
    """

    def __init__(self, methods=METHODS, names=None):
        self.methods = tuple(METHODS[i] for i in range(3) if method_mask(methods) & (1 << i))
        self.names = [] if names is None else list(names)
        self.wrong_gt, self.extra_correct_dets, self.corrected_gt_boxes = [], [], []
        self.matched_det, self.ious_gt, self.det_max_iou = [], [], []
        self.noisy_rows, self.replaced = [], []
        self.pred_boxes, self.pred_classes, self.pred_ranks = [], [], []
        self.counts = np.zeros((0, 5), np.int32)

    @classmethod
    def from_arrays(cls, res, boxes, gt_boxes, gt_classes, classes=None, methods=METHODS, names=None):
        """res: the dict of arrays of `uda_get_label_check` (det_rank, iou, gt_flags, det_flags, det_max_iou, counts); boxes
        [n, M, >= 4] and gt_boxes [n, G, 4] in the caller's own type (float32 values become their shortest decimals, float64
        stay as they are); classes [n, M] the detections' class ids (for the writer of missing boxes).  boxes None (the handle
        did not bring the detection columns over): a replaced row takes its box from the float32 gt_boxes_out, and pred_boxes /
        pred_classes hold None per image."""
        self = cls(methods, names)
        gt_boxes, gt_classes = np.asarray(gt_boxes), np.asarray(gt_classes)
        with_boxes = boxes is not None
        boxes = np.asarray(boxes) if with_boxes else None
        n, M = res["det_flags"].shape
        if names is not None and len(self.names) != n:
            raise ValueError("label check: %d names for %d images" % (len(self.names), n))
        f32_det, f32_gt = (not with_boxes) or boxes.dtype == np.float32, gt_boxes.dtype == np.float32
        for i in range(n):
            rows = np.where(gt_classes[i] > 0)[0]
            kept = np.where(res["det_flags"][i] & capi.LC_DET_KEPT)[0]
            packed = np.full((M + 1,), -1, np.int64)           # rank -> index among the kept (-1 stays -1)
            packed[kept] = np.arange(len(kept))
            flags = res["gt_flags"][i, rows]
            self.wrong_gt.append(np.where(flags & capi.LC_GT_MISTAKE)[0])
            self.noisy_rows.append(np.where(flags & capi.LC_GT_NOISY)[0])
            self.replaced.append(np.where(flags & capi.LC_GT_REPLACED)[0])
            self.extra_correct_dets.append((res["det_flags"][i, kept] & capi.LC_DET_MISSING) != 0)
            self.matched_det.append(packed[res["det_rank"][i, rows]])
            self.ious_gt.append(res["iou"][i, rows].astype(np.float64))
            self.det_max_iou.append(res["det_max_iou"][i, kept].astype(np.float64))
            out = _plain(gt_boxes[i, rows], f32_gt)
            hit = np.where(flags & capi.LC_GT_REPLACED)[0]
            if len(hit):
                src = boxes[i, res["det_rank"][i, rows[hit]], :4] if with_boxes else res["gt_boxes_out"][i, rows[hit]]
                for j, box in zip(hit, _plain(src, f32_det)):
                    out[j] = box
            self.corrected_gt_boxes.append(out)
            self.pred_ranks.append(kept)
            self.pred_boxes.append(_plain(boxes[i, kept, :4], f32_det) if with_boxes else None)
            cl = None if classes is None else np.asarray(classes)[i]
            self.pred_classes.append(None if cl is None else _plain((cl[:, 0] if cl.ndim == 2 else cl)[kept], False))
        self.counts = np.asarray(res["counts"], np.int32).reshape(n, 5).copy()
        return self

    def __len__(self):
        return len(self.wrong_gt)

    _LISTS = ("wrong_gt", "extra_correct_dets", "corrected_gt_boxes", "matched_det", "ious_gt", "det_max_iou", "noisy_rows",
              "replaced", "pred_boxes", "pred_classes", "pred_ranks")

    def merge(self, other):
        """Append the images of another batch (checked with the same methods)."""
        if other.methods != self.methods:
            raise ValueError("merge: the checks were run with different methods (%s, %s)" % (self.methods, other.methods))
        if bool(self.names) != bool(other.names) and len(self) and len(other):
            raise ValueError("merge: one check carries image names and the other does not")
        for k in self._LISTS:
            setattr(self, k, getattr(self, k) + getattr(other, k))
        self.names = self.names + other.names
        self.counts = np.concatenate([self.counts, other.counts])
        return self

    def totals(self):
        """{kept, gt_rows, mistakes, replaced, missing}: the sums of `counts` over the images."""
        s = self.counts.sum(0) if len(self) else np.zeros(5, np.int64)
        return dict(zip(("kept", "gt_rows", "mistakes", "replaced", "missing"), (int(v) for v in s)))


def _dense(boxes, scores, cons_iou, gt_boxes, gt_classes, classes, min_score, dt):
    """Arrays, or per-image lists as `read_predictions` returns them (ragged), -> dense arrays.  Padded detections score below
    min_score, padded ground-truth rows carry class -1; gt_classes None: every given row counts."""
    ragged = isinstance(scores, (list, tuple))
    if ragged:
        n = len(scores)
        if not (len(boxes) == n and len(gt_boxes) == n and (cons_iou is None or len(cons_iou) == n)):
            raise ValueError("label check: the per-image lists differ in length")
        M = max([len(s) for s in scores] + [1])
        G = max([len(g) for g in gt_boxes] + [1])
        b, s, c = np.zeros((n, M, 4), dt), np.full((n, M), min(min_score, 0.0) - 1.0, dt), np.zeros((n, M), np.float64)
        cl = None if classes is None else np.zeros((n, M), np.float64)
        gb, gc = np.zeros((n, G, 4), dt), np.full((n, G), -1.0, dt)
        for i in range(n):
            k, g = len(scores[i]), len(gt_boxes[i])
            if k:
                b[i, :k], s[i, :k] = np.asarray(boxes[i], dt).reshape(k, 4), np.asarray(scores[i], dt)
                if cons_iou is not None:
                    c[i, :k] = np.asarray(cons_iou[i], np.float64)
                if cl is not None:
                    cl[i, :k] = np.asarray(classes[i], np.float64)
            if g:
                gb[i, :g] = np.asarray(gt_boxes[i], dt).reshape(g, 4)
                gc[i, :g] = 1.0 if gt_classes is None else np.asarray(gt_classes[i], dt)
        return b, s, (None if cons_iou is None else c), gb, gc, cl
    s = np.ascontiguousarray(scores, dt)
    if s.ndim != 2:
        raise ValueError("scores must be [n, M], got %s" % (s.shape,))
    n, M = s.shape
    b = np.ascontiguousarray(np.asarray(boxes)[..., :4], dt)
    gb = np.ascontiguousarray(gt_boxes, dt)
    if gb.ndim != 3 or gb.shape[0] != n or gb.shape[2] != 4:
        raise ValueError("gt_boxes must be [%d, G, 4], got %s" % (n, gb.shape))
    gc = np.ones(gb.shape[:2], dt) if gt_classes is None else np.ascontiguousarray(gt_classes, dt)
    c = None if cons_iou is None else np.ascontiguousarray(cons_iou, np.float64)
    cl = None if classes is None else np.asarray(classes, np.float64)
    if cl is not None and cl.ndim == 3:
        cl = cl[..., 0]
    for name, a, shape in (("boxes", b, (n, M, 4)), ("cons_iou", c, (n, M)), ("gt_classes", gc, gb.shape[:2]), ("classes", cl, (n, M))):
        if a is not None and a.shape != shape:
            raise ValueError("%s must be %s, got %s" % (name, list(shape), a.shape))
    return b, s, c, gb, gc, cl


def check_inputs(b, s, c, gb, gc, mask):
    """What the C ABI refuses or leaves to the caller: the limits, cons_iou where md or noisy read it, finite values."""
    n, M = s.shape
    G = gc.shape[1]
    if n < 1:
        raise ValueError("label check: no image given")
    if M > capi.LC_MAX_M:
        raise ValueError("label check: %d detection rows per image, at most %d" % (M, capi.LC_MAX_M))
    if G > capi.LC_MAX_G:
        raise ValueError("label check: %d ground-truth rows per image, at most %d" % (G, capi.LC_MAX_G))
    if (mask & (capi.LC_MD | capi.LC_NOISY)) and c is None:
        raise ValueError("label check: md and noisy read cons_iou (serve_consistency), which is not given")
    for name, a in (("boxes", b), ("scores", s), ("cons_iou", c), ("gt_boxes", gb), ("gt_classes", gc)):
        if a is not None and not np.isfinite(a).all():
            raise ValueError("label check: %s holds non-finite values" % name)


def empty_result(n, M, G):
    return dict(det_rank=np.full((n, G), -1, np.int32), iou=np.zeros((n, G), np.float64), gt_flags=np.zeros((n, G), np.uint8),
                gt_boxes_out=np.zeros((n, G, 4), np.float32), det_flags=np.zeros((n, M), np.uint8),
                det_max_iou=np.zeros((n, M), np.float64), counts=np.zeros((n, 5), np.int32))


RESULT_ORDER = ("det_rank", "iou", "gt_flags", "gt_boxes_out", "det_flags", "det_max_iou", "counts")


def label_check_np(boxes, scores, cons_iou, gt_boxes, gt_classes, min_score, iou_consist=0.90, md_max_inter=0, md_rule="eq",
                   correct_max_inter=1.0, correct_score=0.40, methods=METHODS, as_float32=False, device=0):
    """The raw arrays of `uda_label_check_np` (float64) / `_np_f32` for dense arrays -> dict (RESULT_ORDER)."""
    dt = np.float32 if as_float32 else np.float64
    mask, rule = method_mask(methods), md_rule_code(md_rule)
    thr = check_thresholds(iou_consist, md_max_inter, correct_max_inter, correct_score)
    min_score = resolve_min_score(None, min_score)
    b, s, c, gb, gc, _ = _dense(boxes, scores, cons_iou, gt_boxes, gt_classes, None, min_score, dt)
    check_inputs(b, s, c, gb, gc, mask)
    n, M = s.shape
    res = empty_result(n, M, gc.shape[1])
    lib = capi.load()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    fn, what = (lib.uda_label_check_np_f32, "uda_label_check_np_f32") if as_float32 else (lib.uda_label_check_np, "uda_label_check_np")
    rc = fn(int(device), p(b), p(s), p(c), p(gb), p(gc), n, M, gc.shape[1], min_score, thr[0], thr[1], rule, thr[2], thr[3], mask,
            *[p(res[k]) for k in RESULT_ORDER])
    if rc != 0:
        raise capi.UdaError("%s failed: %s" % (what, lib.uda_last_error(None).decode()))
    return res


def check_labels(boxes, scores, cons_iou, gt_boxes, gt_classes=None, classes=None, methods=METHODS, min_score=0.1, iou_consist=0.90,
                 md_max_inter=0, md_rule="eq", correct_max_inter=1.0, correct_score=0.40, names=None, as_float32=False, device=0):
    """The label check on host arrays - boxes [n, M, 4], scores [n, M], cons_iou [n, M], gt_boxes [n, G, 4], gt_classes [n, G]
    (rows with class <= 0 are padding; None: every row counts) - or on per-image lists as `read_predictions(path, "score",
    True)` returns them (then every listed detection above min_score is kept, and the ground truth is a list of box lists).
    Through `uda_label_check_np`: float64, the reference's arithmetic bit for bit on the values read back from a
    prediction_data.txt; as_float32=True: the arithmetic of the handle.  -> `LabelCheck`."""
    dt = np.float32 if as_float32 else np.float64
    min_score = resolve_min_score(None, min_score)
    b, s, c, gb, gc, cl = _dense(boxes, scores, cons_iou, gt_boxes, gt_classes, classes, min_score, dt)
    res = label_check_np(b, s, c, gb, gc, min_score, iou_consist, md_max_inter, md_rule, correct_max_inter, correct_score, methods,
                         as_float32, device)
    return LabelCheck.from_arrays(res, b, gb, gc, cl, methods, names)
